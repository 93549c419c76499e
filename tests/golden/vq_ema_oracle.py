"""fp64 NumPy restatement of the training branch of VectorQuantize.forward (layers/vq_module.py:74-80) for every stage of one
ResidualVQ.forward (vq_module.py:119-134), over GIVEN codes.

The residual chain is the reference's f32 arithmetic (quantize = r + (q - r); residual = residual - quantize, against the OLD
codes, as test_rvq_stats.restate rebuilds it); the per-code sums, the EMA, the Laplace smoothing and the quotient are fp64.  The
EMA uses the reference's effective factors: float32(decay) and float32(1 - decay), what torch makes of the Python scalars.
"""
import numpy as np


def ema_step(x, embed, cluster_size, embed_avg, codes, decay=0.8, eps=1e-5, skip=None, chain_codes=None):
    """x (N, dim) f32; embed (n_q, dim, size), cluster_size (n_q, size), embed_avg (n_q, dim, size) f32: the state BEFORE the step;
    codes (n_q, N) per-stage code.  skip: boolean (n_q, N), rows that count and sum nothing at a stage (None: none).  chain_codes:
    the codes the residual chain is rebuilt with (None: codes).
    Returns a dict of fp64 arrays: cluster_size, embed_avg, embed (the state after the step), A (n_q, dim, size) = decay*|embed_avg|
    + (1-decay)*sum_{rows with code k} |r| -- the scale the rounding errors of embed_avg' are proportional to --, and counts."""
    n_q, dim, size = embed.shape
    d, omd = np.float64(np.float32(decay)), np.float64(np.float32(1.0 - decay))
    chain = codes if chain_codes is None else chain_codes
    r = np.ascontiguousarray(x, np.float32).copy()
    out = {k: np.zeros((n_q, dim, size)) for k in ("embed_avg", "embed", "A")}
    out["cluster_size"] = np.zeros((n_q, size))
    out["counts"] = np.zeros((n_q, size), np.int64)
    for s in range(n_q):
        keep = np.ones(len(r), bool) if skip is None else ~skip[s]
        k = codes[s][keep]
        r64 = r[keep].astype(np.float64)
        counts = np.bincount(k, minlength=size)
        sums = np.zeros((size, dim))
        sabs = np.zeros((size, dim))
        np.add.at(sums, k, r64)
        np.add.at(sabs, k, np.abs(r64))
        cs = d * cluster_size[s].astype(np.float64) + omd * counts
        ea = d * embed_avg[s].astype(np.float64) + omd * sums.T
        S = cs.sum()
        smoothed = (cs + eps) / (S + size * eps) * S
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            out["embed"][s] = ea / smoothed[None, :]
        out["cluster_size"][s], out["embed_avg"][s], out["counts"][s] = cs, ea, counts
        out["A"][s] = d * np.abs(embed_avg[s].astype(np.float64)) + omd * sabs.T
        q = np.ascontiguousarray(embed[s].T)[chain[s]].astype(np.float32)
        qp = (r + (q - r)).astype(np.float32)
        r = (r - qp).astype(np.float32)
    return out


def quotient(embed_avg, cluster_size, eps=1e-5):
    """fp64 embed = embed_avg / smoothed from given (n_q, dim, size) embed_avg and (n_q, size) cluster_size."""
    cs = np.asarray(cluster_size, np.float64)
    size = cs.shape[1]
    S = cs.sum(1, keepdims=True)
    smoothed = (cs + eps) / (S + size * eps) * S
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return np.asarray(embed_avg, np.float64) / smoothed[:, None, :]
