"""Synchronised BatchNorm in numpy float64, written from the definition (the contract of tony_amd/ops/syncbn.py),
never from the kernels' folded coefficient tables.

Rank ``r`` of ``W`` holds rows ``xs[r]`` [M_r, C]; ``N = sum_r M_r``.  Statistics are those of the concatenation of
all ranks' rows; the parameter gradients are each rank's LOCAL sums.  ``mutant`` makes the reference wrong the way a
wrong implementation would be (tests/test_syncbn_cpu.py checks that each one breaks the assertions the GPU result is
held to):

  "local"          every rank normalises with its own batch's statistics (forward) / sums (backward)
  "drop"           the last rank's packet never arrives
  "n_local"        the global sums are divided by the rank's own M_r instead of N
  "dgamma_global"  dgamma / dbeta taken from the sums over all ranks (backward only)
"""
import numpy as np

MUTANTS_FWD = ("local", "drop", "n_local")
MUTANTS_BWD = ("local", "drop", "n_local", "dgamma_global")


def eps64(eps):
    """The kernels get eps as a C float."""
    return float(np.float32(eps))


def packets(xs):
    """[W, 1 + 2C]: rank r's [M_r | sum x | sum x^2]."""
    return np.stack([np.concatenate([[float(x.shape[0])], x.sum(0), (x * x).sum(0)]) for x in xs])


def _pick(per_rank, r, mutant, total):
    """The sums rank r normalises with."""
    if mutant == "local":
        return per_rank[r]
    if mutant == "drop" and len(per_rank) > 1:
        return total - per_rank[-1]
    return total


def forward(xs, g, b, eps, relu, ress=None, mutant=None):
    W = len(xs)
    pk = packets(xs)
    C = xs[0].shape[1]
    tot = pk.sum(0)
    out = dict(packets=pk, N=tot[0], pre=[], y=[], mag=[], mean=[], var=[], invstd=[])
    for r in range(W):
        p = _pick(pk, r, mutant, tot)
        n = pk[r, 0] if mutant == "n_local" else p[0]
        mean = p[1:1 + C] / n
        var = np.maximum(p[1 + C:] / n - mean * mean, 0.0)
        invstd = 1.0 / np.sqrt(var + eps64(eps))
        k = g * invstd
        pre = (xs[r] - mean) * k + b
        mag = np.abs(xs[r]) * np.abs(k) + np.abs(mean) * np.abs(k) + np.abs(b)
        if ress is not None:
            pre = pre + ress[r]
            mag = mag + np.abs(ress[r])
        out["pre"].append(pre)
        out["y"].append(np.maximum(pre, 0.0) if relu else pre)
        out["mag"].append(mag)
        out["mean"].append(mean)
        out["var"].append(var)
        out["invstd"].append(invstd)
    # the global statistics' own magnitudes (the bound of save_* / running_*)
    allx = np.concatenate(xs)
    out["ex2"] = (allx * allx).sum(0) / allx.shape[0]
    out["absx"] = np.abs(allx).sum(0) / allx.shape[0]
    return out


def running(rm0, rv0, mean, var, N, momentum):
    unbiased = var * (N / (N - 1.0)) if N > 1 else var
    return (1 - momentum) * rm0 + momentum * mean, (1 - momentum) * rv0 + momentum * unbiased


def backward(xs, dys, g, b, mu, is_, relu, keeps=None, mutant=None):
    """BatchNorm backward with the statistics ``mu`` / ``is_`` (the forward's save_mean / save_invstd).  ``keeps``:
    per-rank ReLU masks of the residual form (the stored y > 0); else recomputed from the pre-activation."""
    W = len(xs)
    C = xs[0].shape[1]
    k = g * is_
    xh, d = [], []
    for r in range(W):
        xhat = (xs[r] - mu) * is_
        if not relu:
            keep = np.ones_like(xs[r], dtype=bool)
        elif keeps is not None:
            keep = keeps[r]
        else:
            keep = (xhat * g + b) > 0
        xh.append(xhat)
        d.append(dys[r] * keep)
    ab = np.stack([np.concatenate([d[r].sum(0), (d[r] * xh[r]).sum(0)]) for r in range(W)])
    absb = np.stack([np.abs(d[r] * xh[r]).sum(0) for r in range(W)])
    ms = np.array([float(x.shape[0]) for x in xs])
    tot, N = ab.sum(0), ms.sum()
    out = dict(ab=ab, N=N, d=d, dx=[], mag=[], dgamma=[], dbeta=[])
    for r in range(W):
        p = _pick(ab, r, mutant, tot)
        n = ms[r] if mutant in ("n_local", "local") else (N - ms[-1] if mutant == "drop" and W > 1 else N)
        A, B = p[:C], p[C:]
        out["dx"].append(k * (d[r] - A / n - xh[r] * B / n))
        out["mag"].append(np.abs(k) * (np.abs(d[r]) + np.abs(tot[:C]) / N
                                       + (np.abs(xs[r]) + np.abs(mu)) * is_ * absb.sum(0) / N))
        src = tot if mutant == "dgamma_global" else ab[r]
        out["dbeta"].append(src[:C])
        out["dgamma"].append(src[C:])
    return out
