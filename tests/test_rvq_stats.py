"""CPU: the residual-VQ statistics entry points (adk_rvq_stats) and what tests/golden/forward.npz means.

The library exports both symbols and checks every argument on the host, before any HIP call, so these run without a device.
An fp64 NumPy restatement of VectorQuantize.forward's loss and perplexity (layers/vq_module.py:61-88), applied to the fixture's
codes and regenerated latents, reproduces the reference's values -- the same restatement the GPU tests hold the kernel to."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from audiodec_amd import configs, synth
import make_forward_golden as MFG

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ADK_ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from audiodec_amd import native
    return native.lib()


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "forward.npz"), allow_pickle=False)


def test_stats_symbols_are_exported(lib):
    from audiodec_amd import native
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("adk_rvq_stats", "adk_rvq_stats_workspace_bytes"):
        assert f" {name}\n" in out + "\n", f"{name} is not exported"
        assert name in native.SYMBOLS


def test_workspace_bytes(lib):
    ws = lib.adk_rvq_stats_workspace_bytes
    assert ws(0, 8) == 0
    prev = 0
    for n in (1, 7, 16, 17, 256, 1000, 8192, 10 ** 6, 2 ** 31 - 1):
        b = ws(n, 8)
        assert b > 0 and b % (8 * 8) == 0 and b >= prev, (n, b)
        assert b <= 8 * 8 * 1024                    # one f64 per stage and workgroup, the grid is capped: small at any row count
        assert ws(n, 16) == 2 * b
        prev = b
    assert ws(-1, 8) == ADK_ERR_ARG and ws(5, 0) == ADK_ERR_ARG and ws(5, 17) == ADK_ERR_ARG


def test_argument_validation_needs_no_device(lib):
    """Every bad argument is ADK_ERR_ARG with a message, before any HIP call (the pointers below are never dereferenced)."""
    p = C.c_void_p(0x10000)
    good = dict(z=p, codebook=p, idx=p, n_rows=5, n_q=8, dim=64, size=1024, counts=p, sse=p, rows=p, workspace=p,
                vqloss=None, perplexity=None, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.adk_rvq_stats(a["z"], a["codebook"], a["idx"], a["n_rows"], a["n_q"], a["dim"], a["size"], a["counts"],
                                 a["sse"], a["rows"], a["workspace"], a["vqloss"], a["perplexity"], a["stream"])

    bad = [dict(z=None), dict(codebook=None), dict(idx=None), dict(counts=None), dict(sse=None), dict(rows=None),
           dict(workspace=None), dict(counts=None, n_rows=0), dict(dim=129), dict(dim=0), dict(dim=-64), dict(n_q=0), dict(n_q=17),
           dict(size=0), dict(size=-1024), dict(n_q=16, size=2 ** 28), dict(n_rows=-1), dict(idx=C.c_void_p(0x10004)),
           dict(sse=C.c_void_p(0x10004)), dict(workspace=C.c_void_p(0x10002)), dict(z=C.c_void_p(0x10001)),
           dict(vqloss=C.c_void_p(0x10002))]
    for kw in bad:
        assert call(**kw) == ADK_ERR_ARG, kw
        assert lib.adk_last_error().decode().startswith("adk_rvq_stats"), kw


# ---- the fp64 restatement of VectorQuantize.forward (eval) over given codes ----
def restate(x, embeds, codes):
    """x (N, dim) f32, embeds [n_q] x (dim, size), codes (n_q, N) per-stage code -> (losses, perplexities) in fp64.
    The residual chain is the reference's f32 arithmetic (quantize = r + (q - r); residual = residual - quantize); the loss
    mean((q - r)^2) and the perplexity exp(-sum p log(p + 1e-10)), p = count / N, are evaluated in fp64."""
    r = x.astype(np.float32).copy()
    losses, ppls = [], []
    for s, e in enumerate(embeds):
        q = np.ascontiguousarray(e.T)[codes[s]].astype(np.float32)
        losses.append(np.mean(np.square(q.astype(np.float64) - r.astype(np.float64))))
        p = np.bincount(codes[s], minlength=e.shape[1]).astype(np.float64) / len(codes[s])
        ppls.append(np.exp(-np.sum(p * np.log(p + 1e-10))))
        qp = (r + (q - r)).astype(np.float32)
        r = (r - qp).astype(np.float32)
    return np.asarray(losses), np.asarray(ppls)


def rvq_embeds(name):
    model, n_q = MFG.RVQ[name]
    _, enc_tag, _, _, _ = configs.alias(model)
    sd = synth.synth_state_dict(enc_tag, MFG.SEED)
    return [sd[f"quantizer.codebook.layers.{i}.embed"].numpy() for i in range(n_q)]


@pytest.mark.parametrize("name", list(MFG.RVQ))
def test_restatement_reproduces_the_reference(fixture, name):
    embeds = rvq_embeds(name)
    rms = fixture[f"rvq_{name}_rms"]
    assert rms == MFG.codebook_rms(embeds[0])
    for n in MFG.RVQ_ROWS:
        x = MFG.rvq_latents(MFG.rvq_seed(name, n), n, rms)[0]
        codes = fixture[f"rvq_{name}_{n}_codes"].astype(np.int64)
        assert codes.shape == (len(embeds), n) and codes.min() >= 0 and codes.max() < 1024
        losses, ppls = restate(x, embeds, codes)
        ref_l, ref_p = fixture[f"rvq_{name}_{n}_losses"], fixture[f"rvq_{name}_{n}_perplexities"]
        np.testing.assert_allclose(losses, ref_l, rtol=1e-5, err_msg=f"{name} N={n} losses")
        np.testing.assert_allclose(ppls, ref_p, rtol=1e-6, err_msg=f"{name} N={n} perplexities")
        if n == 1:
            assert np.all(ref_p == 1.0)


def test_forward_fixture_is_consistent(fixture):
    """The Generator.forward entries: shapes of the mono reshape and of the stereo model, and vqloss / perplexity per stage."""
    for name, (model, shape, streams, length) in MFG.FORWARD.items():
        assert tuple(fixture[f"{name}_shape"]) == shape and list(fixture[f"{name}_streams"]) == streams
        _, enc_tag, _, _, _ = configs.alias(model)
        _, _, pe = configs.experiment(enc_tag)
        cin, hop = pe["input_channels"], 300
        b = shape[0] * shape[1] // cin
        T = length // hop
        assert fixture[f"{name}_z"].shape == (b, 64, T) and fixture[f"{name}_zq"].shape == (b, 64, T)
        assert fixture[f"{name}_y"].shape == (b, pe["output_channels"], length)
        assert fixture[f"{name}_vqloss"].shape == (8,) and fixture[f"{name}_perplexity"].shape == (8,)
        assert np.all(fixture[f"{name}_perplexity"] >= 1.0) and np.all(fixture[f"{name}_perplexity"] <= b * T)
