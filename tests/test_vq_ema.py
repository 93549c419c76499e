"""CPU: the residual-VQ EMA update entry points (adk_rvq_ema_update) and what tests/golden/vq_ema*.npz mean.

The library exports both symbols and checks every argument on the host, before any HIP call, so these run without a device.  The
fp64 restatement of the training branch (tests/golden/vq_ema_oracle.py), applied to the fixture's codes and the regenerated state
and latents, reproduces the reference's updated buffers within bounds derived from the arithmetic (u = 2^-24):
  embed_avg'     f32 recursive summation of n_k terms in any order, the cast of 1 - decay, two products and an add:
                 |err| <= (n_k + 4) u A,  A = decay |embed_avg| + (1 - decay) sum |r|
  cluster_size'  the counts are exact; the cast, two products and an add: |err| <= 4 u (decay cs + (1 - decay) n_k)
  embed'         against the fp64 quotient of the fixture's OWN embed_avg' and cluster_size': the f32 sum of `size` cluster sizes plus
                 the smoothing and the division: (size + 8) u, relative.
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import make_vq_ema_golden as MVG
import vq_ema_oracle as VO

ADK_ERR_ARG = -1
U = 2.0 ** -24


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from audiodec_amd import native
    return native.lib()


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return MVG.load(golden_dir)


def test_ema_symbols_are_exported(lib):
    from audiodec_amd import native
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("adk_rvq_ema_update", "adk_rvq_ema_workspace_bytes"):
        assert f" {name}\n" in out + "\n", f"{name} is not exported"
        assert name in native.SYMBOLS
    assert lib.adk_abi_version() == 14


def test_workspace_bytes(lib):
    ws = lib.adk_rvq_ema_workspace_bytes
    prev = 0
    for n in (1, 7, 16, 17, 256, 1000, 4096, 4097, 32768, 10 ** 6):
        b = ws(n, 8, 64, 1024)
        assert b > 0 and b % 8 == 0 and b >= prev, (n, b)
        assert b >= 8 * n * 64 * 4                  # at least the residuals of every stage
        assert ws(n, 16, 64, 1024) > b and ws(n, 8, 128, 1024) > b
        prev = b
    for bad in ((0, 8, 64, 1024), (-1, 8, 64, 1024), (5, 0, 64, 1024), (5, 17, 64, 1024), (5, 8, 0, 1024), (5, 8, 129, 1024),
                (5, 8, 64, 0), (5, 16, 64, 2 ** 28), (5, 1, 64, 2 ** 28 + 1)):
        assert ws(*bad) == ADK_ERR_ARG, bad
        assert lib.adk_last_error().decode().startswith("adk_rvq_ema"), bad


def test_argument_validation_needs_no_device(lib):
    """Every bad argument is ADK_ERR_ARG with a message, before any HIP call (the pointers below are never dereferenced)."""
    p = C.c_void_p(0x10000)
    good = dict(z=p, idx=p, n_rows=5, n_q=8, dim=64, size=1024, decay=0.8, eps=1e-5, embed=p, enorm=p, codebook=p, cluster_size=p,
                embed_avg=p, workspace=p, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.adk_rvq_ema_update(a["z"], a["idx"], a["n_rows"], a["n_q"], a["dim"], a["size"], a["decay"], a["eps"], a["embed"],
                                      a["enorm"], a["codebook"], a["cluster_size"], a["embed_avg"], a["workspace"], a["stream"])

    bad = [dict(z=None), dict(idx=None), dict(embed=None), dict(enorm=None), dict(cluster_size=None), dict(embed_avg=None),
           dict(workspace=None), dict(n_rows=0), dict(n_rows=-1), dict(dim=129), dict(dim=0), dict(n_q=0), dict(n_q=17), dict(size=0),
           dict(size=-1024), dict(n_q=16, size=2 ** 28), dict(n_q=1, size=2 ** 28 + 1), dict(decay=1.0), dict(decay=-0.1), dict(decay=float("nan")), dict(decay=1.5),
           dict(eps=0.0), dict(eps=-1e-5), dict(eps=float("nan")), dict(idx=C.c_void_p(0x10004)), dict(workspace=C.c_void_p(0x10004)),
           dict(z=C.c_void_p(0x10001)), dict(embed=C.c_void_p(0x10002)), dict(enorm=C.c_void_p(0x10002)),
           dict(codebook=C.c_void_p(0x10002)), dict(cluster_size=C.c_void_p(0x10001)), dict(embed_avg=C.c_void_p(0x10003))]
    for kw in bad:
        assert call(**kw) == ADK_ERR_ARG, kw
        assert lib.adk_last_error().decode().startswith("adk_rvq_ema"), kw


def test_chunk_option_is_host_state(lib):
    assert lib.adk_set_option(b"rvq_ema_chunk_rows", 64) == 0 and lib.adk_set_option(b"rvq_ema_chunk_rows", 0) == 0
    assert lib.adk_set_option(b"rvq_ema_chunk_rows", -1) == ADK_ERR_ARG and b"rvq_ema_chunk_rows" in lib.adk_last_error()


def reference_bounds_hold(fixture, name, got_cs, got_ea, columns, what):
    """The CPU test's bounds on (cluster_size' full, embed_avg' at `columns`) against the oracle over the fixture's codes."""
    n_q, dim, size, n = MVG.CASES[name]
    embed, cs, ea = MVG.initial_state(int(fixture[f"{name}_seed"]), n_q, dim, size)
    x = MVG.latents(int(fixture[f"{name}_seed"]), n, dim)
    codes = fixture[f"{name}_codes"].astype(np.int64)
    o = VO.ema_step(x, embed, cs, ea, codes, MVG.DECAY, MVG.EPS)
    d, omd = np.float64(np.float32(MVG.DECAY)), np.float64(np.float32(1.0 - MVG.DECAY))
    cs_tol = 4 * U * (d * cs.astype(np.float64) + omd * o["counts"])
    err = np.abs(got_cs.astype(np.float64) - o["cluster_size"])
    print(f"{what} {name}: cluster_size' uses {np.max(err / np.maximum(cs_tol, 1e-300)):.3f} of its bound")
    assert np.all(err <= cs_tol), f"{what} {name}: cluster_size'"
    ea_tol = ((o["counts"][:, None, :] + 4) * U * o["A"])[:, :, columns]
    err = np.abs(got_ea.astype(np.float64) - o["embed_avg"][:, :, columns])
    print(f"{what} {name}: embed_avg' uses {np.max(err / np.maximum(ea_tol, 1e-300)):.3f} of its bound")
    assert np.all(err <= ea_tol), f"{what} {name}: embed_avg'"
    return o


@pytest.mark.parametrize("name", list(MVG.CASES))
def test_restatement_reproduces_the_reference(fixture, name):
    n_q, dim, size, n = MVG.CASES[name]
    step = MVG.column_step(size)
    columns = np.arange(0, size, step)
    codes = fixture[f"{name}_codes"]
    assert codes.shape == (n_q, n) and codes.min() >= 0 and codes.max() < size
    ref_cs, ref_ea, ref_e = fixture[f"{name}_cluster_size"], fixture[f"{name}_embed_avg"], fixture[f"{name}_embed"]
    assert ref_cs.shape == (n_q, size) and ref_ea.shape == ref_e.shape == (n_q, dim, len(columns))
    _, cs0, _ = MVG.initial_state(int(fixture[f"{name}_seed"]), n_q, dim, size)
    assert np.all(cs0[:, ::7] == 0)                                   # dead codes are in play
    reference_bounds_hold(fixture, name, ref_cs, ref_ea, columns, "reference")
    # embed' against the fp64 quotient of the fixture's own embed_avg' and cluster_size'
    cs64 = ref_cs.astype(np.float64)
    S = cs64.sum(1, keepdims=True)
    smoothed = ((cs64 + MVG.EPS) / (S + size * MVG.EPS) * S)[:, None, columns]
    q = ref_ea.astype(np.float64) / smoothed
    rel = np.abs(ref_e.astype(np.float64) - q) / np.abs(q)
    print(f"reference {name}: embed' within {np.nanmax(rel) / U:.2f} u of the quotient")
    assert np.all(rel[np.isfinite(rel)] <= (size + 8) * U) and np.all(np.isfinite(q) == np.isfinite(ref_e))


def test_losses_are_the_eval_mode_ones(fixture):
    """The training forward's losses / perplexities are computed against the old table: test_rvq_stats.restate reproduces them."""
    from test_rvq_stats import restate
    for name, (n_q, dim, size, n) in MVG.CASES.items():
        embed, _, _ = MVG.initial_state(int(fixture[f"{name}_seed"]), n_q, dim, size)
        x = MVG.latents(int(fixture[f"{name}_seed"]), n, dim)
        losses, ppls = restate(x, list(embed), fixture[f"{name}_codes"].astype(np.int64))
        np.testing.assert_allclose(losses, fixture[f"{name}_losses"], rtol=1e-5)
        np.testing.assert_allclose(ppls, fixture[f"{name}_perplexities"], rtol=1e-6)
