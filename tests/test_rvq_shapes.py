"""CPU: the residual-VQ search cases of tests/rvq_cases.py are sound and sharp, and adk_rvq_encode / adk_rvq_lookup refuse what they cannot run.

  * every named case meets the helper's preconditions (exact arithmetic, tie pressure, a slab-straddling tie, a winner in the ragged wave);
  * a numpy restatement of the search run as each of the searches a broken kernel would perform differs from the exact answer on at least
    10 % of the decisions of some named case -- tests/test_gpu_rvq_shapes.py holds the kernels to these cases;
  * the entry points check their arguments on the host, before any HIP call, so the refusals run without a device.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import rvq_cases as RC

ADK_OK, ADK_ERR_ARG, ADK_ERR_SHAPE = 0, -1, -2
SHARP = 0.10


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from audiodec_amd import native
    return native.lib()


@pytest.fixture(scope="module")
def exact_cases():
    return {s: RC.exact_case(s) for s in RC.EXACT_SHAPES}


@pytest.mark.parametrize("shape", RC.EXACT_SHAPES, ids=RC.case_id)
def test_exact_case_meets_its_preconditions(exact_cases, shape):
    case = exact_cases[shape]               # (exact_case() has asserted them)
    dim, size, n_q = shape
    assert case.x.shape == (RC.POOL, dim) and len(case.embeds) == n_q and all(e.shape == (dim, size) for e in case.embeds)
    assert case.idx.shape == (n_q, RC.POOL) and int(case.idx.min()) >= 0 and int(case.idx.max()) < size
    # the answer is the plain f64 arg-min too, and zq the f32 sum of the chosen codes in any order
    r = case.x.double()
    for st, e in enumerate(case.embeds):
        dist = r.pow(2).sum(1, keepdim=True) - 2 * r @ e.double() + e.double().pow(2).sum(0, keepdim=True)
        assert np.array_equal(np.argmin(dist.numpy(), 1), case.idx[st].numpy())
        r = r - e.double()[:, case.idx[st]].T
    assert torch.equal(case.x.double() - r, case.zq.double())
    print(f"{RC.case_id(shape)}: {case.decisions()} decisions, {100 * case.tied_share():.0f} % tied")


def test_the_larger_pool_of_the_fast_kernels_meets_them_too():
    case = RC.exact_case((64, 1024, 8), rows=513)
    assert case.tied_share() >= RC.MIN_TIED and case.idx.shape == (8, 513)
    small = RC.exact_case((64, 1024, 8))
    assert all(torch.equal(a, b) for a, b in zip(case.embeds, small.embeds))


@pytest.mark.parametrize("shape", RC.REAL_SHAPES, ids=RC.case_id)
def test_real_case_excuses_little(shape):
    case = RC.real_case(shape)              # (real_case() has asserted the share)
    print(f"{RC.case_id(shape)}: excusable share {case.excusable_share:.4f}, smallest margin {float(case.margin.min()):.3e}")
    assert RC.check_real(case, case.zq, case.idx, "oracle against itself") == 0.0


@pytest.mark.parametrize("wrong", RC.WRONG)
def test_a_wrong_search_is_told_apart(exact_cases, wrong):
    worst = {}
    for shape, case in exact_cases.items():
        idx, _, _ = RC.search(case.x.numpy(), [e.numpy() for e in case.embeds], wrong=wrong)
        worst[shape] = float((idx != case.idx.numpy()).mean())
    best = max(worst, key=worst.get)
    print(f"{wrong}: differs on {100 * worst[best]:.0f} % of the decisions of {RC.case_id(best)}")
    assert worst[best] >= SHARP, worst


def test_encode_refusals_need_no_device(lib):
    """Bad shapes are ADK_ERR_SHAPE, bad pointers ADK_ERR_ARG, both with a message and before any HIP call (the pointers are never dereferenced)."""
    p = C.c_void_p(0x10000)
    good = dict(z=p, embed=p, enorm=p, idx=p, zq=p, n_rows=5, n_q=8, dim=64, size=1024)

    def call(**kw):
        a = dict(good, **kw)
        return lib.adk_rvq_encode(a["z"], a["embed"], a["enorm"], a["idx"], a["zq"], a["n_rows"], a["n_q"], a["dim"], a["size"], None)

    bad = [(dict(dim=0), ADK_ERR_SHAPE), (dict(dim=129), ADK_ERR_SHAPE), (dict(size=0), ADK_ERR_SHAPE), (dict(n_q=0), ADK_ERR_SHAPE),
           (dict(n_rows=-1), ADK_ERR_SHAPE), (dict(embed=C.c_void_p(0x10004)), ADK_ERR_ARG), (dict(embed=C.c_void_p(0x10008)), ADK_ERR_ARG),
           (dict(enorm=C.c_void_p(0x10004)), ADK_ERR_ARG), (dict(enorm=C.c_void_p(0x10008)), ADK_ERR_ARG),
           (dict(z=None), ADK_ERR_ARG), (dict(embed=None), ADK_ERR_ARG), (dict(enorm=None), ADK_ERR_ARG), (dict(idx=None), ADK_ERR_ARG)]
    for kw, rc in bad:
        assert call(**kw) == rc, kw
        assert lib.adk_last_error().decode().startswith("adk_rvq_encode"), kw
    for dim, size, n_q in RC.EXACT_SHAPES + RC.REAL_SHAPES:          # nothing to do is fine at every accepted shape
        assert call(n_rows=0, dim=dim, size=size, n_q=n_q) == ADK_OK
    assert call(n_rows=0, zq=None) == ADK_OK


def test_lookup_refusals_need_no_device(lib):
    p = C.c_void_p(0x10000)
    good = dict(idx=p, codebook=p, zq=p, n_rows=5, n_q=8, dim=64, n_codes=8192)

    def call(**kw):
        a = dict(good, **kw)
        return lib.adk_rvq_lookup(a["idx"], a["codebook"], a["zq"], a["n_rows"], a["n_q"], a["dim"], a["n_codes"], None)

    bad = [(dict(dim=65), ADK_ERR_SHAPE), (dict(dim=3), ADK_ERR_SHAPE), (dict(dim=0), ADK_ERR_SHAPE), (dict(n_codes=0), ADK_ERR_SHAPE),
           (dict(n_q=0), ADK_ERR_SHAPE), (dict(n_rows=-1), ADK_ERR_SHAPE), (dict(codebook=C.c_void_p(0x10004)), ADK_ERR_ARG),
           (dict(zq=C.c_void_p(0x10008)), ADK_ERR_ARG), (dict(idx=None), ADK_ERR_ARG), (dict(codebook=None), ADK_ERR_ARG),
           (dict(zq=None), ADK_ERR_ARG)]
    for kw, rc in bad:
        assert call(**kw) == rc, kw
        assert lib.adk_last_error().decode().startswith("adk_rvq_lookup"), kw
    assert call(n_rows=0) == ADK_OK
