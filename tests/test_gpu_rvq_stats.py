"""GPU: residual-VQ statistics (adk_rvq_stats) and the forward calls built on them.

  * ResidualVQ.forward against the reference (tests/golden/forward.npz, made by make_forward_golden.py);
  * engineered codes against the fp64 restatement of VectorQuantize.forward (test_rvq_stats.restate);
  * an index outside its stage: IndexError at the next flag check, nothing read beyond the codebook;
  * bitwise reproducibility and folding several calls into one accumulator;
  * AutoEncoderStreamGenerator.forward (Generator.forward) and quantizer_forward(return_stats=True);
  * BatchedAudioDecStreamer(track_codebook_usage=True), also across a lazy-guard repair.
"""
import os
import warnings

import numpy as np
import pytest
import torch

from audiodec_amd import configs, synth
import make_forward_golden as MFG
from test_rvq_stats import restate, rvq_embeds

pytestmark = pytest.mark.gpu

WAVE_TOL = 1e-4


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "forward.npz"), allow_pickle=False)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def run_stats(dev, x, embeds, codes, acc=None):
    """adk_rvq_stats over given per-stage codes: x (N, dim) f32, codes (n_q, N) -> (vqloss, perplexity, accumulator) on the host."""
    from audiodec_amd import codebook_usage as CU
    n_q, (dim, size) = len(embeds), embeds[0].shape
    cb = CU.row_major_codebook([torch.from_numpy(e) for e in embeds], dev)
    idx = torch.from_numpy(codes.astype(np.int64) + size * np.arange(n_q)[:, None]).to(dev).contiguous()
    acc = acc if acc is not None else CU.accumulator(n_q, size, dev)
    vq = torch.empty(n_q, device=dev)
    ppl = torch.empty(n_q, device=dev)
    CU.fold(acc, torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev), cb, idx, n_q, dim, size, vq, ppl)
    return vq.cpu().numpy(), ppl.cpu().numpy(), acc


@pytest.mark.parametrize("name", list(MFG.RVQ))
def test_residual_vq_forward_matches_reference(gpu, fixture, name):
    from audiodec_amd import layers
    embeds = rvq_embeds(name)
    rvq = layers.ResidualVQ([torch.from_numpy(e) for e in embeds], device=gpu)
    for n in MFG.RVQ_ROWS:
        x = torch.from_numpy(MFG.rvq_latents(MFG.rvq_seed(name, n), n, fixture[f"rvq_{name}_rms"]))
        zq, losses, ppls = rvq.forward(x)
        zq_i, codes = rvq.forward_index(x)
        assert np.array_equal(codes.reshape(len(embeds), n).cpu().numpy(), fixture[f"rvq_{name}_{n}_codes"]), f"{name} N={n}: codes"
        assert rel(losses.cpu(), fixture[f"rvq_{name}_{n}_losses"]) <= 1e-5, f"{name} N={n}: losses"
        assert rel(ppls.cpu(), fixture[f"rvq_{name}_{n}_perplexities"]) <= 1e-6, f"{name} N={n}: perplexities"
        assert torch.equal(zq, zq_i), f"{name} N={n}: quantized_out differs from forward_index's"
    with pytest.raises(AttributeError):
        rvq.lookup(codes)                    # forward() did not initialise the lookup codebook


def _check_against_restatement(dev, x, embeds, codes, what):
    vq, ppl, acc = run_stats(dev, x, embeds, codes)
    ref_l, ref_p = restate(x, embeds, codes)
    assert rel(vq, ref_l) <= 1e-5, f"{what}: vqloss {vq} vs {ref_l}"
    assert rel(ppl, ref_p) <= 1e-6, f"{what}: perplexity {ppl} vs {ref_p}"
    size = embeds[0].shape[1]
    counts = acc[0].view(len(embeds), size).cpu().numpy()
    for s in range(len(embeds)):
        assert np.array_equal(counts[s], np.bincount(codes[s], minlength=size)), f"{what}: counts of stage {s}"
    assert int(acc[2].item()) == x.shape[0]
    return vq, ppl


def _random_embeds(rng, n_q, dim, size):
    return [(rng.standard_normal((dim, size)) * 0.5 ** s).astype(np.float32) for s in range(n_q)]


def test_engineered_histograms(gpu):
    rng = np.random.default_rng(5)
    embeds = _random_embeds(rng, 8, 64, 1024)
    # every row on one code: perplexity 1
    n = 300
    x = rng.standard_normal((n, 64)).astype(np.float32)
    _, ppl = _check_against_restatement(gpu, x, embeds, np.full((8, n), 7), "one code")
    assert np.all(ppl == 1.0)
    # N = size rows, each on a distinct code: perplexity size
    x = rng.standard_normal((1024, 64)).astype(np.float32)
    codes = np.stack([rng.permutation(1024) for _ in range(8)])
    _, ppl = _check_against_restatement(gpu, x, embeds, codes, "distinct codes")
    assert rel(ppl, np.full(8, 1024.0)) <= 1e-6


@pytest.mark.parametrize("n_q,dim,size,n", [(8, 64, 1024, 1), (8, 64, 1024, 97), (8, 64, 1024, 1003), (8, 64, 1024, 10007),
                                             (16, 64, 1024, 257), (16, 64, 1024, 4099), (3, 128, 8192, 333), (5, 40, 100, 61)])
def test_shapes_against_restatement(gpu, n_q, dim, size, n):
    """Row counts of 1, primes and non-multiples of the 4-row workgroup, past the 1024-workgroup grid cap (10007: waves loop
    over rows), 16 stages, 128 components, a histogram too large for LDS (3 x 8192 bins) and a small odd shape."""
    rng = np.random.default_rng(n_q * 1000 + n)
    embeds = _random_embeds(rng, n_q, dim, size)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    codes = rng.integers(0, size, (n_q, n))
    _check_against_restatement(gpu, x, embeds, codes, f"n_q={n_q} dim={dim} size={size} N={n}")


def test_out_of_stage_index_raises_and_reads_nothing_beyond(gpu):
    from audiodec_amd import codebook_usage as CU, native
    native.device_flags()                                   # start from a clean flag word
    rng = np.random.default_rng(9)
    n_q, dim, size, n = 8, 64, 1024, 50
    embeds = _random_embeds(rng, n_q, dim, size)
    cb = CU.row_major_codebook([torch.from_numpy(e) for e in embeds], gpu)
    big = torch.full((n_q * size + 4096, dim), float("nan"), device=gpu)      # NaN right behind the codebook
    big[:n_q * size] = cb
    idx = torch.from_numpy(rng.integers(0, size, (n_q, n)) + size * np.arange(n_q)[:, None]).to(gpu)
    idx[1, 3] = 5                                           # a code of stage 0 at stage 1
    idx[2, 0] = n_q * size + 100                            # beyond the codebook
    idx[4, 7] = -1
    idx = idx.contiguous()
    acc = CU.accumulator(n_q, size, gpu)
    vq, ppl = torch.empty(n_q, device=gpu), torch.empty(n_q, device=gpu)
    x = torch.from_numpy(rng.standard_normal((n, dim)).astype(np.float32)).to(gpu)
    CU.fold(acc, x, big[:n_q * size], idx, n_q, dim, size, vq, ppl)
    with pytest.raises(IndexError):
        native.raise_on_device_flags("adk_rvq_stats")
    assert torch.isfinite(vq).all() and torch.isfinite(ppl).all() and torch.isfinite(acc[1]).all()
    counts = acc[0].view(n_q, size).sum(1).cpu().numpy()
    assert list(counts) == [n, n - 1, n - 1, n, n - 1, n, n, n]        # bad indices are not counted
    assert native.device_flags() == 0


def test_bitwise_reproducible_and_accumulation(gpu):
    rng = np.random.default_rng(11)
    n_q, dim, size, n = 8, 64, 1024, 5003
    embeds = _random_embeds(rng, n_q, dim, size)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    codes = rng.integers(0, size, (n_q, n))
    vq1, ppl1, acc1 = run_stats(gpu, x, embeds, codes)
    vq2, ppl2, acc2 = run_stats(gpu, x, embeds, codes)
    assert vq1.tobytes() == vq2.tobytes() and ppl1.tobytes() == ppl2.tobytes()
    assert acc1[1].cpu().numpy().tobytes() == acc2[1].cpu().numpy().tobytes()
    # three calls on row slices fold into one accumulator: the same totals as one call on all rows
    acc = None
    for a, b in ((0, 1), (1, 2048), (2048, n)):
        vq3, ppl3, acc = run_stats(gpu, x[a:b], embeds, codes[:, a:b], acc)
    assert torch.equal(acc[0], acc1[0]) and int(acc[2].item()) == n
    assert rel(acc[1].cpu(), acc1[1].cpu()) <= 1e-12
    assert rel(vq3, vq1) <= 1e-6 and np.array_equal(ppl3, ppl1)    # perplexity: from the same integer counts


# ---- generator level ----
def _generator(dev, model, split16):
    from audiodec_amd.stream_generator import AutoEncoderStreamGenerator
    _, enc_tag, _, _, _ = configs.alias(model)
    _, _, pe = configs.experiment(enc_tag)
    g = AutoEncoderStreamGenerator(**pe)
    g.load_state_dict(synth.synth_state_dict(enc_tag, MFG.SEED))
    return g.eval().to(dev).configure(1, 8).set_split16(split16)


@pytest.mark.parametrize("split16", [False, True])
@pytest.mark.parametrize("name", list(MFG.FORWARD))
def test_generator_forward_matches_reference(gpu, fixture, name, split16):
    from audiodec_amd import native
    model, shape, streams, length = MFG.FORWARD[name]
    g = _generator(gpu, model, split16)
    x = torch.from_numpy(MFG.forward_input(shape, streams, length))
    with pytest.raises(native.NativeError):
        g.forward(x)                                        # streaming mode: forward() is the offline call
    g.set_offline(True)
    with torch.no_grad():
        y, zq, z, vqloss, ppl = g.forward(x.to(gpu))
    for k, v in (("z", z), ("zq", zq), ("y", y)):
        ref = fixture[f"{name}_{k}"]
        assert tuple(v.shape) == ref.shape, (k, tuple(v.shape), ref.shape)
        err = float(np.abs(v.cpu().numpy() - ref).max())
        # zq within the waveform bar means every code agrees with the reference's (a flipped code moves zq by a code vector)
        assert err <= WAVE_TOL, f"{name}: max|d{k}| = {err:.3e}"
    assert rel(vqloss.cpu(), fixture[f"{name}_vqloss"]) <= 1e-5
    assert rel(ppl.cpu(), fixture[f"{name}_perplexity"]) <= 1e-6


@pytest.mark.parametrize("split16", [False, True])
def test_quantizer_forward_stats_leave_zq_unchanged(gpu, split16):
    from audiodec_amd import lazy_guard
    g = _generator(gpu, "vctk_sym", split16).configure(2, 8)
    x = torch.from_numpy(np.stack([synth.synth_audio(3, s, 12 * 300) for s in range(2)]))[:, None, :].to(gpu)
    with torch.no_grad():
        z = g.encode(x)
        zq0 = g.quantizer_forward(z)
        zq1, vq, ppl = g.quantizer_forward(z, return_stats=True)
        assert all(type(t) is lazy_guard.GuardedTensor for t in (zq1, vq, ppl)) == (type(zq0) is lazy_guard.GuardedTensor)
        assert tuple(zq1.shape) == tuple(zq0.shape) == (2, 64, 12)
        assert torch.equal(zq1, zq0)
        idx = g.quantize(z).cpu().numpy() - 1024 * np.arange(8)[:, None, None]
    zt = z.cpu().transpose(2, 1).reshape(-1, 64).numpy()
    sd = g._sd
    embeds = [sd[f"quantizer.codebook.layers.{i}.embed"].numpy() for i in range(8)]
    ref_l, ref_p = restate(zt, embeds, idx.reshape(8, -1))
    assert rel(vq.cpu(), ref_l) <= 1e-5 and rel(ppl.cpu(), ref_p) <= 1e-6


@pytest.mark.parametrize("overflow", [False, True])
def test_streamer_tracks_code_usage(gpu, ckpt_root, overflow):
    """256 streams, a few ticks: every stage's counts add up to ticks x streams and are the histogram of what tx.quantize
    returned.  overflow: lazy guard, one stream's frame scaled by 1e6 at tick 1 -- a split-f16 encoder conv overflows, the
    log repairs the calls in place, and the counts are those of the repaired indices (counted once)."""
    from test_gpu_parity import load_audiodec
    from audiodec_amd.batched_streamer import BatchedAudioDecStreamer
    n, hop, ticks = 256, 300, 3
    ad = load_audiodec(ckpt_root, "vctk_sym", 1337, n, 1, split16=True)
    if overflow:
        for g_ in (ad.tx_encoder, ad.rx_encoder, ad.decoder):
            g_.set_guard(True, "lazy")
    st = BatchedAudioDecStreamer(ad, frame_size=hop, max_latency=100.0, track_codebook_usage=True)
    seen = []
    quantize = st.tx.quantize

    def recording_quantize(z):
        idx = quantize(z)
        seen.append(idx)
        return idx
    st.tx.quantize = recording_quantize
    audio = np.stack([synth.synth_audio(21, s, ticks * hop) for s in range(n)])
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        for t in range(ticks):
            for s in range(n):
                frame = audio[s, t * hop:(t + 1) * hop]
                st.push(s, frame * 1e6 if (overflow and t == 1 and s == 5) else frame)
            st.tick()
    repaired = any(issubclass(i.category, RuntimeWarning) and "f16 range" in str(i.message) for i in w)
    assert repaired == overflow, [str(i.message) for i in w]
    counts = st.usage.counts().numpy()
    assert counts.shape == (8, 1024) and np.all(counts.sum(1) == ticks * n)
    idx = np.concatenate([i.cpu().numpy().reshape(8, -1) for i in seen], 1) - 1024 * np.arange(8)[:, None]
    assert idx.shape == (8, ticks * n)
    for s in range(8):
        assert np.array_equal(counts[s], np.bincount(idx[s], minlength=1024)), f"stage {s}"
    stats = st.stats()
    ppl = np.exp(-np.sum(np.where(counts > 0, counts / (ticks * n) * np.log(counts / (ticks * n) + 1e-10), 0.0), 1))
    assert rel(stats["codebook_perplexity"], ppl) <= 1e-6
    assert stats["codebook_dead_codes"] == [int(v) for v in (counts == 0).sum(1)]
    assert st.usage.rows() == ticks * n and np.all(np.isfinite(st.usage.vqloss().numpy()))
    st.usage.reset()
    assert st.usage.rows() == 0 and int(st.usage.counts().sum()) == 0
