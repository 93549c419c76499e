"""GPU: the residual-VQ EMA codebook update (adk_rvq_ema_update) and the calls built on it.

  * the reference's training-mode ResidualVQ.forward (tests/golden/vq_ema*.npz, made by make_vq_ema_golden.py) and the fp64
    restatement (tests/golden/vq_ema_oracle.py) over the reference's codes;
  * shapes at which the kernels can go wrong, against the restatement over codes drawn here;
  * bitwise reproducibility, also across different chunkings of the launch;
  * an index outside its stage: IndexError at the next flag check, the row contributes nothing at that stage, nothing read beyond;
  * layers.ResidualVQ.train(), CodebookEMA.update / install / state_dict, quantizer_forward(ema=...), an update across a guard repair.

Bounds against the restatement (u = 2^-24; the per-code sums are f64 on the device, so n_k does not enter):
  embed_avg'     one rounding of the f64 sum, the cast of 1 - decay, two products, one add: 5 u A
  cluster_size'  4 u (decay cs + (1 - decay) n_k)
  embed'         8 u relative of the fp64 quotient of the DOWNLOADED embed_avg' and cluster_size' (six roundings + second order)
  enorm          (dim + 2) u sum_d e^2 of the fp64 norm of the downloaded embed'
  codebook       bit-equal to the transpose of embed'
"""
import warnings

import numpy as np
import pytest
import torch

from audiodec_amd import configs, synth
import make_vq_ema_golden as MVG
import vq_ema_oracle as VO
from test_vq_ema import reference_bounds_hold

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DECAY, EPS = MVG.DECAY, MVG.EPS
NAMES = ("embed", "enorm", "codebook", "cluster_size", "embed_avg")


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return MVG.load(golden_dir)


def _padded(arr, dev, pad):
    """A device copy of `arr` with `pad` NaNs right behind it (the view handed to the library is the front)."""
    flat = torch.full((arr.size + pad,), float("nan"), dtype=torch.float32, device=dev)
    flat[:arr.size] = torch.from_numpy(np.ascontiguousarray(arr, np.float32).ravel()).to(dev)
    return flat[:arr.size].view(*arr.shape)


def run_update(dev, x, embed, cs, ea, idx, pad=0, decay=DECAY, eps=EPS):
    """adk_rvq_ema_update over given GLOBAL indices idx (n_q, N) int64: returns the five outputs as numpy arrays."""
    from audiodec_amd import codebook_ema as CE
    n_q, dim, size = embed.shape
    st = CE.State(_padded(embed, dev, pad), _padded(np.zeros((n_q, size), np.float32), dev, pad),
                  _padded(np.zeros((n_q * size, dim), np.float32), dev, pad), _padded(cs, dev, pad), _padded(ea, dev, pad))
    CE.update(st, _padded(x, dev, pad), torch.from_numpy(np.ascontiguousarray(idx, np.int64)).to(dev), decay, eps)
    return {k: getattr(st, k).cpu().numpy() for k in NAMES}


def global_idx(codes, size):
    return codes.astype(np.int64) + size * np.arange(codes.shape[0])[:, None]


def check_against_oracle(out, o, cs0, what):
    n_q, dim, size = out["embed"].shape
    d, omd = np.float64(np.float32(DECAY)), np.float64(np.float32(1.0 - DECAY))
    tol = 4 * U * (d * cs0.astype(np.float64) + omd * o["counts"])
    err = np.abs(out["cluster_size"].astype(np.float64) - o["cluster_size"])
    print(f"{what}: cluster_size' uses {np.max(err / np.maximum(tol, 1e-300)):.3f} of its bound")
    assert np.all(err <= tol), f"{what}: cluster_size'"
    dead = o["counts"] == 0
    assert np.array_equal(out["cluster_size"][dead], (np.float32(DECAY) * cs0)[dead]), f"{what}: cluster sizes of unused codes only decay"
    tol = 5 * U * o["A"]
    err = np.abs(out["embed_avg"].astype(np.float64) - o["embed_avg"])
    print(f"{what}: embed_avg' uses {np.max(err / np.maximum(tol, 1e-300)):.3f} of its bound")
    assert np.all(err <= tol), f"{what}: embed_avg'"
    q = VO.quotient(out["embed_avg"], out["cluster_size"], EPS)
    err = np.abs(out["embed"].astype(np.float64) - q)
    print(f"{what}: embed' within {np.max(err / np.maximum(np.abs(q), 1e-300)) / U:.2f} u of the quotient")
    assert np.all(err <= 8 * U * np.abs(q)), f"{what}: embed'"
    n2 = np.square(out["embed"].astype(np.float64)).sum(1)
    assert np.all(np.abs(out["enorm"].astype(np.float64) - n2) <= (dim + 2) * U * n2), f"{what}: enorm"
    assert np.array_equal(out["codebook"].reshape(n_q, size, dim), out["embed"].transpose(0, 2, 1)), f"{what}: codebook"
    for k in NAMES:
        assert not np.isnan(out[k]).any(), f"{what}: NaN in {k}"


@pytest.mark.parametrize("name", list(MVG.CASES))
def test_fixture_cases(gpu, fixture, name):
    n_q, dim, size, n = MVG.CASES[name]
    seed = int(fixture[f"{name}_seed"])
    embed, cs, ea = MVG.initial_state(seed, n_q, dim, size)
    x = MVG.latents(seed, n, dim)
    codes = fixture[f"{name}_codes"].astype(np.int64)
    out = run_update(gpu, x, embed, cs, ea, global_idx(codes, size))
    o = VO.ema_step(x, embed, cs, ea, codes, DECAY, EPS)
    check_against_oracle(out, o, cs, name)
    # the reference's STORED values on the stored columns, with the bounds the reference itself is held to (test_vq_ema.py)
    columns = np.arange(0, size, MVG.column_step(size))
    reference_bounds_hold(fixture, name, out["cluster_size"], out["embed_avg"][:, :, columns], columns, "hip")
    d, omd = np.float64(np.float32(DECAY)), np.float64(np.float32(1.0 - DECAY))
    n_k, A = o["counts"][:, None, columns], o["A"][:, :, columns]
    ref_cs, ref_ea, ref_e = (fixture[f"{name}_{k}"].astype(np.float64) for k in ("cluster_size", "embed_avg", "embed"))
    cs_scale = d * cs + omd * o["counts"]
    err, tol = np.abs(out["embed_avg"][:, :, columns] - ref_ea), (n_k + 4) * U * A
    print(f"{name}: embed_avg' against the stored values uses {np.max(err / np.maximum(tol, 1e-300)):.3f} of (n_k + 4) u A")
    assert np.all(err <= tol), f"{name}: embed_avg' against the reference's"
    err, tol = np.abs(out["cluster_size"] - ref_cs), 4 * U * cs_scale
    print(f"{name}: cluster_size' against the stored values uses {np.max(err / np.maximum(tol, 1e-300)):.3f} of 4 u (...)")
    assert np.all(err <= tol), f"{name}: cluster_size' against the reference's"
    # embed': both sides are quotients e = ea / sm of their own buffers, the reference's within (size + 8) u of its fp64 quotient q (CPU
    # test), this one within 8 u of its own.  The two fp64 quotients differ by the buffers' differences, bounded above: |d ea| <=
    # (n_k + 4) u A, and sm = (cs + eps) / (S + size eps) S moves by at most 4 u cs_scale / (cs + eps) through cs and 2 x 4 u through S
    # (every term of S within 4 u cs_scale, and cs_scale <= cs' (1 + 4 u)); one more u of second order.
    S = ref_cs.sum(1, keepdims=True)
    sm = ((ref_cs + EPS) / (S + size * EPS) * S)
    q = ref_ea / sm[:, None, columns]
    rel_sm = (4 * U * cs_scale / (ref_cs + EPS) + 9 * U)[:, None, columns]
    tol = (size + 8 + 8) * U * np.abs(q) + (n_k + 4) * U * A / sm[:, None, columns] + rel_sm * np.abs(q)
    err = np.abs(out["embed"][:, :, columns] - ref_e)
    print(f"{name}: embed' against the stored values uses {np.max(err / np.maximum(tol, 1e-300)):.3f} of its bound")
    assert np.all(err <= tol), f"{name}: embed' against the reference's"


def _drawn_case(gpu, n_q, dim, size, n, codes=None, seed=None):
    seed = n_q * 1000 + n if seed is None else seed
    rng = np.random.default_rng(seed)
    embed, cs, ea = MVG.initial_state(seed, n_q, dim, size)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    codes = rng.integers(0, size, (n_q, n)) if codes is None else codes
    out = run_update(gpu, x, embed, cs, ea, global_idx(codes, size))
    check_against_oracle(out, VO.ema_step(x, embed, cs, ea, codes, DECAY, EPS), cs, f"n_q={n_q} dim={dim} size={size} N={n}")
    return out


@pytest.mark.parametrize("n_q,dim,size,n", [(8, 64, 1024, 1), (8, 64, 1024, 97), (8, 64, 1024, 10007), (16, 64, 1024, 257),
                                             (3, 128, 1024, 333), (5, 40, 100, 61), (3, 64, 8192, 333)])
def test_shapes_against_oracle(gpu, n_q, dim, size, n):
    """One row, a prime, more rows than 256 chunks of 16 (10007: chunks grow, waves loop over rows), 16 stages, 128 components,
    nothing a multiple of 64, and 3 x 8192 bins."""
    _drawn_case(gpu, n_q, dim, size, n)


def test_engineered_segments(gpu):
    n_q, size = 8, 1024
    _drawn_case(gpu, n_q, 64, size, 3000, codes=np.full((n_q, 3000), 7))                  # one segment of every row, 1023 empty ones
    rng = np.random.default_rng(3)
    _drawn_case(gpu, n_q, 64, size, size, codes=np.stack([rng.permutation(size) for _ in range(n_q)]))     # every segment one row


def test_bitwise_reproducible_and_independent_of_chunking(gpu):
    from audiodec_amd import native
    n_q, dim, size, n = 8, 64, 1024, 5003
    rng = np.random.default_rng(11)
    embed, cs, ea = MVG.initial_state(11, n_q, dim, size)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    idx = global_idx(rng.integers(0, 40, (n_q, n)), size)              # long segments: the order of the sums matters
    a = run_update(gpu, x, embed, cs, ea, idx)
    b = run_update(gpu, x, embed, cs, ea, idx)
    try:
        others = []
        for rows in (21, 64, 1000):                                    # 239, 79 and 6 chunks; the default at 5003 rows is 251 chunks of 20
            native.set_option("rvq_ema_chunk_rows", rows)
            others.append(run_update(gpu, x, embed, cs, ea, idx))
    finally:
        native.set_option("rvq_ema_chunk_rows", 0)
    for k in NAMES:
        assert a[k].tobytes() == b[k].tobytes(), k
        for o in others:
            assert a[k].tobytes() == o[k].tobytes(), k


def test_out_of_stage_index(gpu):
    from audiodec_amd import native
    native.device_flags()                                   # start from a clean flag word
    n_q, dim, size, n = 8, 64, 1024, 50
    rng = np.random.default_rng(9)
    embed, cs, ea = MVG.initial_state(9, n_q, dim, size)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    codes = rng.integers(0, size, (n_q, n))
    idx = global_idx(codes, size)
    skip = np.zeros((n_q, n), bool)
    for s, row, v in ((1, 3, 5), (2, 0, n_q * size + 100), (4, 7, -1)):       # a code of stage 0 at stage 1, beyond the table, negative
        idx[s, row] = v
        skip[s, row] = True
    chain = np.where(skip, 0, codes)                        # the row's chain goes on with the stage's first code (adk_rvq_stats' rule)
    out = run_update(gpu, x, embed, cs, ea, idx, pad=4096)
    with pytest.raises(IndexError):
        native.raise_on_device_flags("adk_rvq_ema_update")
    check_against_oracle(out, VO.ema_step(x, embed, cs, ea, np.where(skip, 0, codes), DECAY, EPS, skip=skip, chain_codes=chain), cs, "bad index")
    assert native.device_flags() == 0


# ---- layer level ----
def test_residual_vq_train_mode(gpu):
    from audiodec_amd import layers
    n_q, dim, size, n = 4, 64, 256, 200
    embed, cs, ea = MVG.initial_state(21, n_q, dim, size)
    t = lambda a: [torch.from_numpy(v) for v in a]          # noqa: E731
    rvq = layers.ResidualVQ(t(embed), device=gpu, cluster_size=t(cs), embed_avg=t(ea), decay=DECAY, eps=EPS)
    assert rvq.training is False and rvq.train() is rvq and rvq.training and rvq.eval().training is False
    rvq.initial()
    ev = layers.ResidualVQ(t(embed), device=gpu)
    state = (embed, cs, ea)
    rvq.train()
    for step in range(2):
        x = np.random.default_rng(30 + step).standard_normal((2, n // 2, dim)).astype(np.float32)
        _, codes = rvq.forward_index(torch.from_numpy(x))                     # the HIP path's own codes on the table as it is
        codes = codes.reshape(n_q, n).cpu().numpy()
        zq, losses, ppls = rvq.forward(torch.from_numpy(x))
        if step == 0:                                                         # the returns are today's, against the old table
            zq_e, losses_e, ppls_e = ev.forward(torch.from_numpy(x))
            assert torch.equal(zq, zq_e) and torch.equal(losses, losses_e) and torch.equal(ppls, ppls_e)
        o = VO.ema_step(x.reshape(n, dim), *state, codes, DECAY, EPS)
        out = dict(embed=rvq.embed.cpu().numpy(), enorm=rvq.enorm.cpu().numpy(), codebook=rvq.codebook.cpu().numpy(),
                   cluster_size=rvq.cluster_size.cpu().numpy(), embed_avg=rvq.embed_avg.cpu().numpy())
        check_against_oracle(out, o, state[1], f"train step {step}")
        state = (out["embed"], out["cluster_size"], out["embed_avg"])
    before = [getattr(rvq, k).clone() for k in NAMES]
    rvq.eval()
    rvq.forward(torch.from_numpy(x))
    assert all(torch.equal(a, getattr(rvq, k)) for a, k in zip(before, NAMES))
    # defaults: zeros and a copy of embed, as the reference initialises them
    fresh = layers.ResidualVQ(t(embed), device=gpu)
    assert not fresh.cluster_size.any() and torch.equal(fresh.embed_avg, fresh.embed)


# ---- generator level ----
def _generator(dev, sd=None, streams=4):
    from audiodec_amd.stream_generator import AutoEncoderStreamGenerator
    _, enc_tag, _, _, _ = configs.alias("vctk_sym")
    _, _, pe = configs.experiment(enc_tag)
    g = AutoEncoderStreamGenerator(**pe)
    g.load_state_dict(sd if sd is not None else synth.synth_state_dict(enc_tag, 1337))
    return g.eval().to(dev).configure(streams, 8)


def _check_search(idx, zt, embed, what):
    """idx (n_q, N) global indices the HIP search emitted for rows zt against embed (n_q, dim, size): each equals the fp64 arg-min on
    the residual its own earlier codes leave, unless that arg-min's top-2 distance margin is below 1e-4 (README, "What parity asserts")."""
    n_q, dim, size = embed.shape
    r = zt.astype(np.float32).copy()
    for s in range(n_q):
        e = embed[s].astype(np.float64)
        dist = np.square(r.astype(np.float64)[:, :, None] - e[None]).sum(1)
        best = dist.argmin(1)
        top2 = np.partition(dist, 1, axis=1)[:, :2]
        got = idx[s] - s * size
        bad = (got != best) & (top2[:, 1] - top2[:, 0] >= 1e-4)
        assert not bad.any(), f"{what}: stage {s} rows {np.nonzero(bad)[0][:5]}"
        q = np.ascontiguousarray(embed[s].T)[got].astype(np.float32)
        r = (r - (r + (q - r)).astype(np.float32)).astype(np.float32)


def test_codebook_ema_update_install_and_state_dict(gpu):
    from audiodec_amd.codebook_ema import CodebookEMA
    g = _generator(gpu)
    x = torch.from_numpy(np.stack([synth.synth_audio(3, s, 8 * 300) for s in range(4)]))[:, None, :].to(gpu)
    with torch.no_grad():
        z = g.encode(x)
        idx_old = g.quantize(z)
        _, vq_old, ppl_old = g.quantizer_forward(z, return_stats=True)
        ema = CodebookEMA(g)
        old = {k: v.clone() for k, v in ema.state_dict().items()}
        with pytest.raises(ValueError):
            ema.update(z[:, :, :0])
        vq, ppl = ema.update(z)
        assert ema.steps() == 1 and torch.equal(vq, vq_old) and torch.equal(ppl, ppl_old)       # the batch against the OLD table
        assert torch.equal(g.quantize(z), idx_old)                                              # not installed yet
        ema.install()
        idx = g.quantize(z)
        zq = g.lookup(idx)
    new = ema.state_dict()
    embed = np.stack([new[f"quantizer.codebook.layers.{i}.embed"].numpy() for i in range(8)])
    zt = z.cpu().transpose(2, 1).reshape(-1, 64).numpy()
    # the update is the oracle's over the codes the old table gave
    o = VO.ema_step(zt, *[np.stack([old[f"quantizer.codebook.layers.{i}.{k}"].numpy() for i in range(8)])
                          for k in ("embed", "cluster_size", "embed_avg")],
                    idx_old.cpu().numpy().reshape(8, -1) - 1024 * np.arange(8)[:, None], DECAY, EPS)
    assert np.all(np.abs(np.stack([new[f"quantizer.codebook.layers.{i}.embed_avg"].numpy() for i in range(8)]) - o["embed_avg"]) <= 5 * U * o["A"])
    assert not torch.equal(idx, idx_old)
    _check_search(idx.cpu().numpy().reshape(8, -1), zt, embed, "quantize after install")
    rows = np.ascontiguousarray(embed.transpose(0, 2, 1)).reshape(-1, 64)[idx.cpu().numpy().reshape(8, -1)]     # (n_q, N, dim)
    want = np.zeros(rows.shape[1:], np.float32)
    for s in range(8):                                                        # adk_rvq_lookup's order: stages ascending, f32 adds
        want = (want + rows[s]).astype(np.float32)
    assert np.array_equal(zq.cpu().numpy().reshape(-1, 64), want)
    assert torch.equal(g._sd["quantizer.codebook.layers.3.embed"], new["quantizer.codebook.layers.3.embed"])
    # a fresh generator loaded from the saved state: the same lookup bit for bit, the same search up to the margin rule
    sd = dict(synth.synth_state_dict(configs.alias("vctk_sym")[1], 1337))
    sd.update(new)
    g2 = _generator(gpu, sd)
    with torch.no_grad():
        assert torch.equal(g2.lookup(idx), zq)
        _check_search(g2.quantize(z).cpu().numpy().reshape(8, -1), zt, embed, "quantize of a reloaded generator")
    # reconfiguring does not fall back to the old codes
    g.configure(4, 4)
    with torch.no_grad():
        assert torch.equal(g.lookup(idx), zq)
    assert ema.reset().steps() == 0


def test_quantizer_forward_with_and_without_ema(gpu):
    from audiodec_amd.codebook_ema import CodebookEMA
    g, plain = _generator(gpu), _generator(gpu)
    x = torch.from_numpy(np.stack([synth.synth_audio(5, s, 8 * 300) for s in range(4)]))[:, None, :].to(gpu)
    with torch.no_grad():
        z = plain.encode(x)
        want = plain.quantizer_forward(z, return_stats=True)
        ema = CodebookEMA(g)
        got = g.quantizer_forward(z, return_stats=True)                       # a CodebookEMA exists, nothing installed: unchanged
        assert all(torch.equal(a, b) for a, b in zip(got, want))
        trained = g.quantizer_forward(z, return_stats=True, ema=ema)         # training mode: the same returns, then the update
        assert all(torch.equal(a, b) for a, b in zip(trained, want)) and ema.steps() == 1
        assert torch.equal(g.quantizer_forward(z, ema=None), g.quantizer_forward(z))
        # an ema whose table is not this generator's is refused and nothing changes: another generator's, or an update not installed
        other = _generator(gpu)
        with pytest.raises(ValueError):
            other.quantizer_forward(z, ema=ema)
        ema.install(other)
        ema.update(z)
        with pytest.raises(ValueError):
            other.quantizer_forward(z, ema=ema)
        ema.install(g)
        after = g.quantizer_forward(z, return_stats=True)
        assert not torch.equal(after[0], want[0])                             # the new table is installed
        again = plain.quantizer_forward(z, return_stats=True)
        assert all(torch.equal(a, b) for a, b in zip(again, want))


def test_update_counts_repaired_indices_once(gpu, ckpt_root):
    """Lazy guard, one stream's frame scaled by 1e6: a split-f16 encoder conv overflows.  The update settles the log first, so it sees
    the repaired latents and indices, once."""
    from test_gpu_parity import load_audiodec
    from audiodec_amd.codebook_ema import CodebookEMA
    n, hop = 8, 300
    ad = load_audiodec(ckpt_root, "vctk_sym", 1337, n, 1, split16=True)
    for g_ in (ad.tx_encoder, ad.rx_encoder, ad.decoder):
        g_.set_guard(True, "lazy")
    tx = ad.tx_encoder
    ema = CodebookEMA(tx)
    old = [np.stack([tx._sd[f"quantizer.codebook.layers.{i}.{k}"].numpy() for i in range(8)]) for k in ("embed", "cluster_size", "embed_avg")]
    audio = np.stack([synth.synth_audio(21, s, hop) for s in range(n)])
    audio[5] *= 1e6
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with torch.no_grad():
            z = tx.encode(torch.from_numpy(audio)[:, None, :].to(gpu))
            idx = tx.quantize(z)
            ema.update(z, idx)
    assert any(issubclass(i.category, RuntimeWarning) and "f16 range" in str(i.message) for i in w), [str(i.message) for i in w]
    zt = z.cpu().transpose(2, 1).reshape(-1, 64).numpy()
    codes = idx.cpu().numpy().reshape(8, -1) - 1024 * np.arange(8)[:, None]
    o = VO.ema_step(zt, *old, codes, DECAY, EPS)
    new = ema.state_dict()
    cs = np.stack([new[f"quantizer.codebook.layers.{i}.cluster_size"].numpy() for i in range(8)])
    d, omd = np.float64(np.float32(DECAY)), np.float64(np.float32(1.0 - DECAY))
    assert np.all(np.abs(cs - o["cluster_size"]) <= 4 * U * (d * old[1] + omd * o["counts"]))
    assert np.all(o["counts"].sum(1) == n)
    ea = np.stack([new[f"quantizer.codebook.layers.{i}.embed_avg"].numpy() for i in range(8)])
    assert np.all(np.abs(ea - o["embed_avg"]) <= 5 * U * o["A"])
    assert ema.steps() == 1
