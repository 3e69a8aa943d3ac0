"""The kvstore's row-sparse contract (tony_amd/parallel/kvstore.py module docstring) in numpy: ``from_rows``, the
ordered merge, the assignment of a push with no optimizer, lazy SGD and lazy Adam on the touched rows, and the
counted-rounding bounds the torch (generic) path is held to.  Every fp32 operation is one numpy float32 operation, so
nothing here is contracted.

Lazy SGD, per element of a touched row (``f32`` values; the roundings are numbered):

    g1 = g * rescale_grad                       (1)
    g2 = clip(g1)                               exact (a comparison and a choice; a NaN stays NaN)
    p  = wd * w                                 (2)
    g3 = g2 + p                                 (3)
    s  = lr * g3                                (4)
    momentum == 0:   w = w - s                  (5)                       5 roundings
    momentum != 0:   m1 = momentum * m          (5)
                     m  = m1 - s                (6)
                     w  = w + m                 (7)                       7 roundings

Bound of an evaluation of the same expression with no more roundings than these (torch's CPU and GPU kernels may
fuse ``a + alpha * b`` into one): every rounding is at most e = 2^-24 times the magnitude of its result, and in units
of ``w`` every result is at most the magnitude sum

    S = |w| + |momentum * m| + lr * (|g1| + |wd * w|)

(a rounding of g1, p or g3 enters ``w`` times ``lr``).  Two such evaluations -- this reference and the one under
test -- are each within ``N e S`` of the exact value, so they differ by at most ``2 N e S``, N = 5 or 7; the
momentum's own bound is the same with N = 6 (its last rounding is (6)).

Lazy Adam (``Optimizer.update`` on the gathered rows; ``t`` counts updates of the key), with G = |g1| + |wd * w|:

    g3 as above: 3 roundings                                    eg = 3 e G
    m = b1 * m + (1 - b1) * g3: 3 roundings                     em = (1 - b1) eg + 3 e (|b1 m| + (1 - b1) G)
    v = b2 * v + (1 - b2) * g3 * g3: 4 roundings, no            ev = 2 (1 - b2) G eg + 4 e v
        cancellation (every term >= 0)
    d = sqrt(v) + eps: 2 roundings                              ed = min(ev / (2 sqrt v), sqrt ev) + 2 e d
    u = lr_t * m / d: 2 roundings                               eu = lr_t (em / d + |m| ed / d^2) + 2 e |u|
    w = w - u: 1 rounding                                       ew = eu + e (|w| + |u|)

and again twice that between two evaluations.
"""
import numpy as np

EPS = 2.0 ** -24
f32 = np.float32


def from_rows(ids, rows):
    """Sorted unique ids and the rows of each summed in order of occurrence (fp32 adds, left to right)."""
    ids = np.asarray(ids, np.int64).reshape(-1)
    rows = np.asarray(rows, np.float32).reshape(ids.size, -1)
    order = np.argsort(ids, kind="stable")
    uniq, out = [], []
    for j in order:
        if uniq and uniq[-1] == ids[j]:
            out[-1] = (out[-1] + rows[j]).astype(np.float32)
        else:
            uniq.append(ids[j])
            out.append(rows[j].copy())
    return np.asarray(uniq, np.int64), np.asarray(out, np.float32).reshape(len(uniq), rows.shape[1])


def merge(sources):
    """The ordered merge of ``[(ids, rows), ...]``: the sorted union, each row ``acc = first source having it;
    acc = acc + next source having it; ...``."""
    width = sources[0][1].shape[1] if sources[0][1].ndim == 2 else 0
    union = np.unique(np.concatenate([np.asarray(i, np.int64) for i, _ in sources]))
    out = np.zeros((union.size, width), np.float32)
    have = np.zeros(union.size, bool)
    for ids, rows in sources:
        for j, i in enumerate(np.asarray(ids, np.int64)):
            u = int(np.searchsorted(union, i))
            out[u] = (out[u] + rows[j]).astype(np.float32) if have[u] else rows[j]
            have[u] = True
    return union, out


def assign(shape, ids, rows):
    """The value a store with no optimizer holds after a merged push: the rows, zero elsewhere."""
    w = np.zeros(shape, np.float32)
    w[ids] = rows
    return w


def _g3(w_rows, g, wd, rescale, clip):
    g1 = (g * f32(rescale)).astype(np.float32)
    if clip is not None:
        c = f32(clip)
        g1 = np.where(g1 > c, c, np.where(g1 < -c, -c, g1)).astype(np.float32)
    p = (f32(wd) * w_rows).astype(np.float32)
    return (g1 + p).astype(np.float32), np.abs(g1) + np.abs(p)


def sgd(w, m, ids, g, lr=0.01, momentum=0.0, wd=0.0, rescale=1.0, clip=None):
    """Lazy SGD on rows ``ids`` of copies of ``w`` (and ``m`` when momentum != 0): ``(w, m, bound of w, bound of
    m)``, the bounds [nnz, row] as the module docstring counts them (zero rows elsewhere are not returned)."""
    w, m = w.copy(), (None if m is None else m.copy())
    wr = w[ids]
    with np.errstate(invalid="ignore", over="ignore"):
        g3, G = _g3(wr, g, wd, rescale, clip)
        s = (f32(lr) * g3).astype(np.float32)
        if momentum:
            m1 = (f32(momentum) * m[ids]).astype(np.float32)
            S = np.abs(wr) + np.abs(m1) + f32(lr) * G
            m[ids] = (m1 - s).astype(np.float32)
            w[ids] = (wr + m[ids]).astype(np.float32)
            return w, m, 2 * 7 * EPS * S.astype(np.float64), 2 * 6 * EPS * S.astype(np.float64)
        S = np.abs(wr) + f32(lr) * G
        w[ids] = (wr - s).astype(np.float32)
        return w, m, 2 * 5 * EPS * S.astype(np.float64), None


def adam(w, m, v, t, ids, g, lr=0.01, beta1=0.9, beta2=0.999, epsilon=1e-8, wd=0.0, rescale=1.0, clip=None):
    """Lazy Adam on rows ``ids`` of copies of ``w``, ``m``, ``v`` at update count ``t`` (already incremented):
    ``(w, m, v, bound of w, bound of m, bound of v)``."""
    w, m, v = w.copy(), m.copy(), v.copy()
    wr = w[ids]
    g3, G = _g3(wr, g, wd, rescale, clip)
    b1m = (f32(beta1) * m[ids]).astype(np.float32)
    mn = (b1m + (f32(1 - beta1) * g3).astype(np.float32)).astype(np.float32)
    vn = ((f32(beta2) * v[ids]).astype(np.float32)
          + (f32(1 - beta2) * (g3 * g3).astype(np.float32)).astype(np.float32)).astype(np.float32)
    lr_t = f32(lr * (1 - beta2 ** t) ** 0.5 / (1 - beta1 ** t))
    d = (np.sqrt(vn).astype(np.float32) + f32(epsilon)).astype(np.float32)
    u = (lr_t * (mn / d).astype(np.float32)).astype(np.float32)
    w[ids] = (wr - u).astype(np.float32)
    m[ids], v[ids] = mn, vn
    G, d64, v64 = G.astype(np.float64), d.astype(np.float64), vn.astype(np.float64)
    eg = 3 * EPS * G
    em = (1 - beta1) * eg + 3 * EPS * (np.abs(b1m) + (1 - beta1) * G)
    ev = 2 * (1 - beta2) * G * eg + 4 * EPS * v64
    with np.errstate(divide="ignore", invalid="ignore"):
        ed = np.where(v64 > 0, np.minimum(ev / (2 * np.sqrt(v64)), np.sqrt(ev)), np.sqrt(ev)) + 2 * EPS * d64
    eu = float(lr_t) * (em / d64 + np.abs(mn) * ed / d64 ** 2) + 2 * EPS * np.abs(u)
    ew = eu + EPS * (np.abs(wr) + np.abs(u))
    return w, m, v, 2 * ew, 2 * em, 2 * ev


def within(got, want, bound, what):
    """``|got - want| <= bound`` elementwise, with the worst element named."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    excess = np.abs(got - want) - bound
    assert np.all(excess <= 0), (f"{what}: off by {np.abs(got - want).max():.3e}, bound "
                                 f"{bound.reshape(-1)[np.argmax(excess)]:.3e} at {np.argmax(excess)}")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
