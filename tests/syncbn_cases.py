"""Operands, shapes and the bound shared by the synchronised-BatchNorm tests (tests/test_syncbn_cpu.py,
tests/test_syncbn_gpu.py, tests/syncbn_worker.py).

Operands are those of tests/test_bn_pool_exact_gpu.py: small integers (|x| <= 4, |dy| <= 3, |res| <= 2), gamma and
beta bf16-representable, every ReLU pre-activation 2^-10 * mag away from 0, E[x^2] / var <= 4 per channel for N > 2.
Rank r's rows are offset by -2, 0, +2 so that the local statistics are far from the global ones.  The bound is that
file's: ``|got - ref64| <= 1/2 ulp_bf16(ref64) + 2^-18 * mag`` (no ulp term for fp32 outputs), with M -> N and the
global sums in ``mag``; its derivation covers this case a fortiori (the statistics are formed in double: fewer fp32
roundings).  ``save_*`` / ``running_*``: 2^-20 relative to their terms' magnitude.
"""
import functools

import numpy as np

import syncbn_ref as R

EPS = 1e-3
MOM = 0.1
SLACK = 2.0 ** -18

# C -> the ranks' row counts.  RPI = 256 // (C / 8) rows per iteration; the reductions give a workgroup at least 16
# row groups: the largest count of each C makes tony_syncbn_grid() == 3 with a ragged last workgroup, the middle
# one is no multiple of 4 * RPI (the unrolled loop's tail), 1 is one row.
SHAPES = {
    8: [(1,), (1031,), (8300,), (5, 3), (8300, 1031), (8300, 1, 1031)],        # one channel group, RPI = 256
    24: [(1,), (343,), (2800,), (5, 3), (2800, 343), (2800, 1, 343)],          # RPI = 85: 256 / 3 leaves a lane idle
    2048: [(1,), (7,), (37,), (5, 3), (37, 7), (37, 1, 6)],                    # RPI = 1, 8 table passes
}
GRID3 = {8: 8300, 24: 2800, 2048: 37}
ALL = [(C, s) for C, ss in SHAPES.items() for s in ss]


def sid(cs):
    return f"C{cs[0]}-" + "+".join(map(str, cs[1]))


def ulp_bf16(ref):
    """The bf16 ulp at ``ref``: 2^(floor(log2 |ref|) - 7); 0 at 0."""
    _, e = np.frexp(ref)
    return np.where(ref == 0, 0.0, np.ldexp(1.0, e - 8))


def to_bf16(a):
    """float64 -> the nearest bf16 (ties to even), as float64."""
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).double().numpy()


def violations(got, ref, mag, bf16):
    """(mask of elements outside the bound, excess / (2^-18 mag)); a NaN is a violation."""
    got = np.asarray(got, dtype=np.float64)
    free = 0.5 * ulp_bf16(ref) if bf16 else np.zeros_like(ref)
    err = np.abs(got - ref)
    bad = ~(err <= free + SLACK * mag)
    return bad, np.maximum(err - free, 0) / np.maximum(SLACK * mag, 1e-300)


def rel20_bad(got, ref, mag):
    return ~(np.abs(np.asarray(got, dtype=np.float64) - ref) <= 2.0 ** -20 * mag)


def split(a, slices):
    return np.split(a, np.cumsum(slices)[:-1])


@functools.lru_cache(maxsize=None)
def case(C, slices, res=False, relu=True):
    """The operands of one (C, rows per rank) case with their float64 references; computed once, read-only."""
    rng = np.random.default_rng(1000003 * sum(slices) + 131 * len(slices) + C)
    ri = lambda lo, hi, shape: rng.integers(lo, hi + 1, shape).astype(np.float64)  # noqa: E731
    W, N = len(slices), sum(slices)
    if W == 1:
        x = ri(-3, 3, (N, C)) + ri(-1, 1, (C,))
    else:  # rank offsets -2, 0, +2: clearly different means
        x = ri(-2, 2, (N, C)) + np.repeat(np.array([-2.0, 0.0, 2.0])[:W], slices)[:, None]
    dy = ri(-3, 3, (N, C))
    r = ri(-2, 2, (N, C)) if res else None
    g = ri(4, 12, (C,)) / 8
    g[::5] = -g[::5]  # a negative gamma flips the ReLU side of x
    b = ri(-8, 8, (C,)) / 16

    def fwd():
        return R.forward(split(x, slices), g, b, EPS, relu, split(r, slices) if res else None)

    if N > 2:  # precondition of the bound: E[x^2] / var <= 4; a channel that misses it gets +-4 alternating
        f = fwd()
        badc = f["ex2"] > 4 * f["var"][0]
        alt = np.tile([4.0, -4.0], N // 2 + 1)[:N]
        if N % 2:
            alt[-1] = 0
        x[:, badc] = alt[:, None]
    for _ in range(300):  # ReLU margin: nudge beta of an offending channel one bf16 step (1 / 256)
        f = fwd()
        offend = (np.abs(np.concatenate(f["pre"])) <= 2.0 ** -10 * np.concatenate(f["mag"])).any(0)
        if not relu or not offend.any():
            break
        b[offend] += 1.0 / 256
    f = fwd()
    assert not relu or (np.abs(np.concatenate(f["pre"])) > 2.0 ** -10 * np.concatenate(f["mag"])).all(), "ReLU margin"
    assert N <= 2 or (f["ex2"] <= 4 * f["var"][0]).all(), "E[x^2] / var <= 4"
    assert np.array_equal(to_bf16(g), g) and np.array_equal(to_bf16(b), b) and np.abs(b).max() < 1
    assert np.abs(x).max() <= 4 and np.abs(dy).max() <= 3
    xs, dys = split(x, slices), split(dy, slices)
    # the backward's caller-given statistics: an integer mean, a power-of-two invstd -- every sum is then exact
    mu = ri(-1, 1, (C,))
    is_ = np.tile([0.5, 0.25], C // 2 + 1)[:C].copy()
    return dict(C=C, slices=slices, W=W, N=N, xs=xs, dys=dys, ress=split(r, slices) if res else None, g=g, b=b,
                relu=relu, res=res, f=f, mu=mu, is_=is_)


def backward_ref(c, bf16, mutant=None):
    """The backward reference of ``case`` c for outputs stored as bf16 / fp32 (the residual forms mask by the STORED
    y of the forward reference)."""
    keeps = None
    if c["res"]:
        keeps = [(to_bf16(y) if bf16 else y.astype(np.float32)) > 0 for y in c["f"]["y"]]
    return R.backward(c["xs"], c["dys"], c["g"], c["b"], c["mu"], c["is_"], c["relu"], keeps, mutant)
