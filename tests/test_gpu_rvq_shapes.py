"""GPU: the residual-VQ search (adk_rvq_encode) at every kind of shape it accepts, on every kernel it dispatches to, and on non-finite rows.

The cases and what makes them sharp are in tests/rvq_cases.py (checked on the CPU by tests/test_rvq_shapes.py).

  * exact cases: integer operands, one right answer -- indices equal the int64 arg-min with the lowest index on ties, zq equals the sum of the
    chosen codes and lookup() of the indices, bit for bit.  Every shape but 64 x 1024 runs on the general kernel rvq_encode_kernel<4>, with
    1, 3, 4, 1 and 1 live rows in the last workgroup; 64 x 1024 runs on v3, v4<2>, v4<4> and (above 256 rows with "rvq_rows" 0) the general
    kernel, at the row counts where the grid of helper blocks, "rvq_v4_min" and the 2 -> 4 rows-per-workgroup switch change;
  * real-valued cases against the oracle under the rules of the existing RVQ tests, and twice for identical bytes;
  * non-finite rows: a row with a NaN component takes code 0 of every stage on every kernel (what `(-dist).max(1)` gives the reference), a row
    with an infinite component takes SOME code of each stage (docs/design/rvq.md: the one place where kernels and reference may differ), and
    no other row changes by a bit.

Every call goes through layers.ResidualVQ (flatten_idx both ways) and once more through the C entry point with idx and zq pre-filled, so that an
element the kernel does not write shows."""
import ctypes as C

import numpy as np
import pytest
import torch

import rvq_cases as RC

pytestmark = pytest.mark.gpu

FAST_ROWS = (1, 7, 8, 9, 64, 65, 191, 192, 193, 512, 513)
# "rvq_rows", "rvq_v4_min", the row counts that reach the kernel named
VARIANTS = {"v3": (0, 192, [n for n in FAST_ROWS if n <= 256]),
            "v4_2": (2, 1, FAST_ROWS),
            "v4_4": (4, 1, FAST_ROWS),
            "default": (1, 192, FAST_ROWS),                   # v3 below 192 rows, v4<2> to 512, v4<4> above
            "general": (0, 192, (300, 512, 513))}
_cache = {}


def exact(shape, rows=RC.POOL):
    key = ("exact", shape, rows)
    if key not in _cache:
        _cache[key] = RC.exact_case(shape, rows)
    return _cache[key]


def real(shape):
    key = ("real", shape)
    if key not in _cache:
        _cache[key] = RC.real_case(shape)
    return _cache[key]


@pytest.fixture
def options(gpu):
    from audiodec_amd import native
    yield native.set_option
    native.set_option("rvq_rows", 1)
    native.set_option("rvq_v4_min", 192)


def same(a, b):
    """Bit-equal where neither is NaN, NaN in the same places."""
    a, b = a.cpu(), b.cpu()
    return a.shape == b.shape and torch.equal(a.isnan(), b.isnan()) and torch.equal(torch.where(a.isnan(), torch.zeros_like(a), a),
                                                                                    torch.where(b.isnan(), torch.zeros_like(b), b))


def encode(rvq, x):
    """x (n, dim) -> (zq (n, dim), idx (n_q, n) within the stage) on the host: forward_index with flatten_idx both ways and the entry point
    itself on pre-filled outputs, which must all agree."""
    from audiodec_amd import native
    n, n_q = x.shape[0], rvq.n_q
    zq_f, idx_f = rvq.forward_index(x[None], flatten_idx=True)
    zq_u, idx_u = rvq.forward_index(x[None], flatten_idx=False)
    assert zq_f.shape == (1, n, rvq.dim) and idx_f.shape == idx_u.shape == (n_q, n) and idx_f.dtype == torch.int64
    offsets = (torch.arange(n_q) * rvq.codebook_size).view(-1, 1)
    assert torch.equal(idx_f.cpu() - offsets, idx_u.cpu()) and same(zq_f, zq_u)
    xt = x.to(rvq.dev).contiguous()
    idx_r = torch.full((n_q, n), -1, dtype=torch.int64, device=rvq.dev)
    zq_r = torch.full((n, rvq.dim), float("nan"), device=rvq.dev)
    native.check(native.lib().adk_rvq_encode(
        C.c_void_p(xt.data_ptr()), C.c_void_p(rvq.embed.data_ptr()), C.c_void_p(rvq.enorm.data_ptr()), C.c_void_p(idx_r.data_ptr()),
        C.c_void_p(zq_r.data_ptr()), n, n_q, rvq.dim, rvq.codebook_size, native.current_stream(rvq.dev)), "adk_rvq_encode")
    assert torch.equal(idx_r, idx_f) and same(zq_r, zq_f[0])
    return zq_f[0].cpu(), idx_u.cpu()


def lookup(rvq, idx):
    """lookup() of in-stage indices (n_q, n) -> (n, dim) on the host; the float4 kernel refuses dim % 4 != 0, which is then what is checked."""
    flat = idx + (torch.arange(rvq.n_q) * rvq.codebook_size).view(-1, 1)
    if rvq.dim % 4:
        with pytest.raises(ValueError, match="adk_rvq_lookup"):
            rvq.lookup(flat)
        return None
    out = rvq.lookup(flat)
    assert out.shape == (1, idx.shape[1], rvq.dim)
    return out[0].cpu()


def check_exact(rvq, case, n, what):
    zq, idx = encode(rvq, case.x[:n])
    assert torch.equal(idx, case.idx[:, :n]), (what, n, np.argwhere((idx != case.idx[:, :n]).numpy())[:5])
    assert torch.equal(zq, case.zq[:n]), (what, n)
    back = lookup(rvq, idx)
    assert back is None or torch.equal(back, zq), (what, n)


@pytest.mark.parametrize("shape", RC.EXACT_SHAPES, ids=RC.case_id)
def test_exact_cases_at_every_shape(gpu, options, shape):
    """(64 x 1024 at these row counts is v3's; the general kernel at that shape is in test_fast_kernels_exact.)"""
    from audiodec_amd import layers, native
    case = exact(shape)
    rvq = layers.ResidualVQ(case.embeds, device=gpu)
    rvq.initial()
    for n in RC.ROWS:
        check_exact(rvq, case, n, RC.case_id(shape))
    assert native.device_flags() == 0


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_fast_kernels_exact(gpu, options, variant):
    """All variants equal the exact answer, hence each other, bit for bit."""
    from audiodec_amd import layers, native
    rows_opt, v4_min, counts = VARIANTS[variant]
    case = exact((64, 1024, 8), max(FAST_ROWS))
    rvq = layers.ResidualVQ(case.embeds, device=gpu)
    rvq.initial()
    options("rvq_rows", rows_opt)
    options("rvq_v4_min", v4_min)
    for n in counts:
        check_exact(rvq, case, n, variant)
    assert native.device_flags() == 0


@pytest.mark.parametrize("shape", RC.REAL_SHAPES, ids=RC.case_id)
def test_real_cases_against_the_oracle_and_twice(gpu, options, shape):
    from audiodec_amd import layers, native
    case = real(shape)
    rvq = layers.ResidualVQ(case.embeds, device=gpu)
    rvq.initial()
    zq, idx = encode(rvq, case.x[0])
    excused = RC.check_real(case, zq[None], idx, RC.case_id(shape))
    print(f"{RC.case_id(shape)}: excused share {excused:.5f} (excusable {case.excusable_share:.5f})")
    zq2, idx2 = encode(rvq, case.x[0])
    assert torch.equal(idx2, idx) and zq2.numpy().tobytes() == zq.numpy().tobytes()
    back = lookup(rvq, idx)
    if back is not None:
        # lookup adds the n_q codes exactly as stored, one after the other in f32: n_q - 1 roundings of partial sums below sum |code|
        codes = torch.stack([case.embeds[st].double()[:, idx[st]].T for st in range(case.n_q)])
        tol = (case.n_q - 1) * 2.0 ** -24 * codes.abs().sum(0)
        assert bool(((back.double() - codes.sum(0)).abs() <= tol).all())
    assert native.device_flags() == 0


NONFINITE = {"v3": ((64, 1024, 8), 9, 0, 192), "v4_2": ((64, 1024, 8), 9, 2, 1), "v4_4": ((64, 1024, 8), 9, 4, 1),
             "general_64x1024": ((64, 1024, 8), 300, 0, 192), "general_40x100": ((40, 100, 5), 9, 1, 192),
             "general_100x2049": ((100, 2049, 2), 9, 1, 192)}


@pytest.mark.parametrize("target", list(NONFINITE))
def test_nonfinite_rows(gpu, options, target):
    from audiodec_amd import layers, native
    shape, rows, rows_opt, v4_min = NONFINITE[target]
    dim, size, n_q = shape
    case = exact(shape, rows)
    rvq = layers.ResidualVQ(case.embeds, device=gpu)
    rvq.initial()
    options("rvq_rows", rows_opt)
    options("rvq_v4_min", v4_min)
    zq0, idx0 = encode(rvq, case.x)
    assert torch.equal(idx0, case.idx) and torch.equal(zq0, case.zq)
    comp, inf_row = 2 * dim // 3, rows // 2               # (100 dimensions: component 66, in the `lane + 64` half of |r|^2)
    x = case.x.clone()
    x[1, comp] = float("nan")
    x[rows - 1] = float("nan")
    x[inf_row, 1] = float("inf")
    zq, idx = encode(rvq, x)
    # a NaN row: code 0 of every stage; q' = r + (q - r) is the code itself on the finite components and NaN on the others
    code0 = torch.stack([e[:, 0] for e in case.embeds]).sum(0)
    assert not idx[:, 1].any() and not idx[:, rows - 1].any(), (idx[:, 1], idx[:, rows - 1])
    assert bool(zq[rows - 1].isnan().all())
    assert bool(zq[1, comp].isnan()) and int(zq[1].isnan().sum()) == 1 and torch.equal(zq[1][~zq[1].isnan()], code0[~zq[1].isnan()])
    # the inf row: some code of each stage
    assert int(idx[:, inf_row].min()) >= 0 and int(idx[:, inf_row].max()) < size, idx[:, inf_row]
    clean = torch.ones(rows, dtype=torch.bool)
    clean[[1, rows - 1, inf_row]] = False
    assert torch.equal(idx[:, clean], idx0[:, clean]) and zq[clean].numpy().tobytes() == zq0[clean].numpy().tobytes()
    back = lookup(rvq, idx)                               # raises nothing, flags nothing: every emitted index is a code of its stage
    assert torch.equal(back[clean], zq0[clean])
    assert native.device_flags() == 0
