"""The contract of the kvstore's fused optimizer kinds (tony_amd/parallel/kvstore.py module docstring: nag, adagrad,
rmsprop plain and centered, ftrl) in numpy, one ``float32`` operation per line, and the counted-rounding bound of
every result, in the style of kv_sparse_ref.py.

Every function takes the dense weight and state arrays, the row ids of a lazy update (``None``: a dense update of
every element) and the gradient (compact rows for a lazy update), and returns copies: the new weight, the new states
and, per result, the bound of its touched elements.  Hyperparameters are rounded once to fp32; ``1 - gamma1`` is formed
in double first.

The bounds.  With e = 2^-24 every fp32 operation returns its exact result times (1 + d), |d| <= e, so a value x
computed by a chain of operations carries an error E(x) that grows by the rule of its last operation (first order in
e; the inputs w, the states and g are exact):

    x = a * b        E(x) = |a| E(b) + |b| E(a) + e |x|           (a constant has E = 0)
    x = a +- b       E(x) = E(a) + E(b) + e |x|
    x = a / b        E(x) = E(a) / |b| + |a| E(b) / b^2 + e |x|
    x = sqrt(a)      E(x) = min(E(a) / (2 x), sqrt(E(a))) + e |x|   (|sqrt a - sqrt b| <= sqrt |a - b| covers a near 0)
    x = clip(a)      E(x) = E(a)                                  (the clip is 1-Lipschitz and rounds nothing)

ftrl's branch needs no case of its own: at ``|z| = lamda1`` the numerator ``copysign(lamda1, z) - z`` is zero, so the
weight is continuous in ``z`` across it and an evaluation that takes the other branch differs by at most
``E(z) / den``; the rule of the division gives exactly that with ``num = 0``.

The functions apply these rules line by line in float64 beside the fp32 lines.  Two evaluations of the same lines
with no more roundings than these -- this reference and the one under test, or this reference and a float64
evaluation, which has (almost) none -- are each within E of the exact value, so they differ by at most 2 E: that is
the bound returned (the factor also covers the terms of second order in e, which are 2^-24 of the first).
"""
import numpy as np

EPS = 2.0 ** -24
f32 = np.float32

KINDS = ("nag", "adagrad", "rmsprop", "ftrl")
STATES = {"nag": ("mom",), "adagrad": ("history",), "rmsprop": ("n", "g", "delta"), "ftrl": ("z", "n")}
DEFAULTS = dict(learning_rate=0.01, momentum=0.0, wd=0.0, rescale_grad=1.0, clip_gradient=None, epsilon=None,
                gamma1=0.9, gamma2=0.9, centered=False, lamda1=0.01, beta=1.0)


def state_names(kind, cfg):
    """The state tensors a setting keeps."""
    if kind == "nag":
        return ("mom",) if cfg.get("momentum") else ()
    if kind == "rmsprop" and not cfg.get("centered"):
        return ("n",)
    return STATES[kind]


def _a(x):
    return np.abs(np.asarray(x, np.float64))


def _sqrt_err(ea, x):
    """E(sqrt(a)) from E(a) and x = sqrt(a)."""
    x = np.asarray(x, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(x > 0, np.minimum(ea / (2 * x), np.sqrt(ea)), np.sqrt(ea)) + EPS * x


def _g2(g, rescale, clip):
    """The rescaled, clipped gradient and its error."""
    g1 = (g * f32(rescale)).astype(np.float32)
    eg = EPS * _a(g1)
    if clip is not None:
        c = f32(clip)
        g1 = np.where(g1 > c, c, np.where(g1 < -c, -c, g1)).astype(np.float32)
    return g1, eg


def _sel(ids):
    return slice(None) if ids is None else ids


def nag(w, m, ids, g, lr=0.01, momentum=0.0, wd=0.0, rescale=1.0, clip=None):
    """``(w, m, bound of w, bound of m)``; ``m`` is None (and stays None) at momentum 0."""
    w, m, at = w.copy(), (None if m is None else m.copy()), _sel(ids)
    wr = np.array(w[at])  # (a copy: basic slicing would alias the result)
    with np.errstate(invalid="ignore", over="ignore"):
        g2, eg2 = _g2(g, rescale, clip)
        p = (f32(wd) * wr).astype(np.float32)
        g3 = (g2 + p).astype(np.float32)
        eg3 = eg2 + EPS * _a(p) + EPS * _a(g3)
        if not momentum:
            s = (f32(lr) * g3).astype(np.float32)
            w[at] = (wr - s).astype(np.float32)
            es = float(f32(lr)) * eg3 + EPS * _a(s)
            return w, m, 2 * (es + EPS * _a(w[at])), None
        mo = f32(momentum)
        m1 = (mo * m[at]).astype(np.float32)
        mn = (m1 + g3).astype(np.float32)
        q = (mo * mn).astype(np.float32)
        g4 = (g3 + q).astype(np.float32)
        s = (f32(lr) * g4).astype(np.float32)
        w[at] = (wr - s).astype(np.float32)
        m[at] = mn
        em = EPS * _a(m1) + eg3 + EPS * _a(mn)
        eq = float(mo) * em + EPS * _a(q)
        eg4 = eg3 + eq + EPS * _a(g4)
        es = float(f32(lr)) * eg4 + EPS * _a(s)
        return w, m, 2 * (es + EPS * _a(w[at])), 2 * em


def adagrad(w, h, ids, g, lr=0.01, eps=1e-7, wd=0.0, rescale=1.0, clip=None):
    """``(w, history, bound of w, bound of history)``."""
    w, h, at = w.copy(), h.copy(), _sel(ids)
    wr = np.array(w[at])  # (a copy: basic slicing would alias the result)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        g2, eg2 = _g2(g, rescale, clip)
        q = (g2 * g2).astype(np.float32)
        hn = (h[at] + q).astype(np.float32)
        e = (hn + f32(eps)).astype(np.float32)
        r = np.sqrt(e).astype(np.float32)
        d = (g2 / r).astype(np.float32)
        p = (f32(wd) * wr).astype(np.float32)
        u = (d + p).astype(np.float32)
        s = (f32(lr) * u).astype(np.float32)
        w[at] = (wr - s).astype(np.float32)
        h[at] = hn
        eq = 2 * _a(g2) * eg2 + EPS * _a(q)
        eh = eq + EPS * _a(hn)
        ee = eh + EPS * _a(e)
        er = _sqrt_err(ee, r)
        r64 = r.astype(np.float64)
        ed = eg2 / r64 + _a(g2) * er / r64 ** 2 + EPS * _a(d)
        eu = ed + EPS * _a(p) + EPS * _a(u)
        es = float(f32(lr)) * eu + EPS * _a(s)
        return w, h, 2 * (es + EPS * _a(w[at])), 2 * eh


def rmsprop(w, n, gb, delta, ids, g, lr=0.01, gamma1=0.9, gamma2=0.9, eps=1e-8, centered=False, wd=0.0, rescale=1.0,
            clip=None):
    """``(w, n, g, delta, bound of w, of n, of g, of delta)``; ``g`` and ``delta`` (and their bounds) are None unless
    centered (``rmsprop_radicand`` gives a centered caller the sign of ``n - g^2 + eps``)."""
    w, n, at = w.copy(), n.copy(), _sel(ids)
    gb, delta = (None if gb is None else gb.copy()), (None if delta is None else delta.copy())
    wr = np.array(w[at])  # (a copy: basic slicing would alias the result)
    g1c, omg = f32(gamma1), f32(1 - gamma1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        g2, eg2 = _g2(g, rescale, clip)
        p = (f32(wd) * wr).astype(np.float32)
        g3 = (g2 + p).astype(np.float32)
        q = (g3 * g3).astype(np.float32)
        a = (omg * q).astype(np.float32)
        b = (g1c * n[at]).astype(np.float32)
        nn = (a + b).astype(np.float32)
        eg3 = eg2 + EPS * _a(p) + EPS * _a(g3)
        eq = 2 * _a(g3) * eg3 + EPS * _a(q)
        ea = float(omg) * eq + EPS * _a(a)
        en = ea + EPS * _a(b) + EPS * _a(nn)
        n[at] = nn
        if not centered:
            e = (nn + f32(eps)).astype(np.float32)
            r = np.sqrt(e).astype(np.float32)
            d = (g3 / r).astype(np.float32)
            s = (f32(lr) * d).astype(np.float32)
            w[at] = (wr - s).astype(np.float32)
            ee = en + EPS * _a(e)
            er, r64 = _sqrt_err(ee, r), r.astype(np.float64)
            ed = eg3 / r64 + _a(g3) * er / r64 ** 2 + EPS * _a(d)
            es = float(f32(lr)) * ed + EPS * _a(s)
            return w, n, gb, delta, 2 * (es + EPS * _a(w[at])), 2 * en, None, None
        c = (omg * g3).astype(np.float32)
        b2 = (g1c * gb[at]).astype(np.float32)
        gn = (c + b2).astype(np.float32)
        gg = (gn * gn).astype(np.float32)
        e1 = (nn - gg).astype(np.float32)
        e = (e1 + f32(eps)).astype(np.float32)
        r = np.sqrt(e).astype(np.float32)
        d = (g3 / r).astype(np.float32)
        s = (f32(lr) * d).astype(np.float32)
        dl = (f32(gamma2) * delta[at]).astype(np.float32)
        dn = (dl - s).astype(np.float32)
        w[at] = (wr + dn).astype(np.float32)
        gb[at], delta[at] = gn, dn
        ec = float(omg) * eg3 + EPS * _a(c)
        egb = ec + EPS * _a(b2) + EPS * _a(gn)
        egg = 2 * _a(gn) * egb + EPS * _a(gg)
        ee1 = en + egg + EPS * _a(e1)
        ee = ee1 + EPS * _a(e)
        er, r64 = _sqrt_err(ee, r), r.astype(np.float64)
        ed = eg3 / r64 + _a(g3) * er / r64 ** 2 + EPS * _a(d)
        es = float(f32(lr)) * ed + EPS * _a(s)
        edl = EPS * _a(dl) + es + EPS * _a(dn)
        return w, n, gb, delta, 2 * (edl + EPS * _a(w[at])), 2 * en, 2 * egb, 2 * edl


def rmsprop_radicand(n, gb, eps):
    """``(n - gb * gb) + eps`` of centered rmsprop's new states, as the contract rounds it: what the square root is
    taken of (a test asserts it positive wherever the gradient was finite)."""
    with np.errstate(invalid="ignore", over="ignore"):
        gg = (gb * gb).astype(np.float32)
        return ((n - gg).astype(np.float32) + f32(eps)).astype(np.float32)


def ftrl(w, z, n, ids, g, lr=0.01, lamda1=0.01, beta=1.0, wd=0.0, rescale=1.0, clip=None):
    """``(w, z, n, bound of w, of z, of n)``."""
    w, z, n, at = w.copy(), z.copy(), n.copy(), _sel(ids)
    wr = np.array(w[at])  # (a copy: basic slicing would alias the result)
    l1, lr32 = f32(lamda1), f32(lr)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        g2, eg2 = _g2(g, rescale, clip)
        q = (g2 * g2).astype(np.float32)
        n1 = (n[at] + q).astype(np.float32)
        r1 = np.sqrt(n1).astype(np.float32)
        r0 = np.sqrt(n[at]).astype(np.float32)
        dr = (r1 - r0).astype(np.float32)
        sg = (dr / lr32).astype(np.float32)
        t = (sg * wr).astype(np.float32)
        z1 = (z[at] + g2).astype(np.float32)
        zn = (z1 - t).astype(np.float32)
        num = (np.copysign(l1, zn) - zn).astype(np.float32)
        b1 = (f32(beta) + r1).astype(np.float32)
        d0 = (b1 / lr32).astype(np.float32)
        den = (d0 + f32(wd)).astype(np.float32)
        zero = np.abs(zn) <= l1  # False for a NaN z: the division carries it on
        wn = np.where(zero, f32(0.0), (num / den).astype(np.float32)).astype(np.float32)
        w[at], z[at], n[at] = wn, zn, n1
        lr64 = float(lr32)
        eq = 2 * _a(g2) * eg2 + EPS * _a(q)
        en1 = eq + EPS * _a(n1)
        er1 = _sqrt_err(en1, r1)
        er0 = EPS * _a(r0)
        edr = er1 + er0 + EPS * _a(dr)
        esg = edr / lr64 + EPS * _a(sg)
        et = esg * _a(wr) + EPS * _a(t)
        ez = eg2 + EPS * _a(z1) + et + EPS * _a(zn)
        anum = np.where(zero, 0.0, _a(num))
        eden = (er1 + EPS * _a(b1)) / lr64 + EPS * _a(d0) + EPS * _a(den)
        den64 = _a(den)
        ew = (ez + EPS * anum) / den64 + anum * eden / den64 ** 2 + EPS * _a(wn)
        return w, z, n, 2 * ew, 2 * ez, 2 * en1


def step(kind, w, states, ids, g, **cfg):
    """One update of ``kind`` under the ``Optimizer`` keyword arguments ``cfg``: ``(w, states, bounds)`` with
    ``states`` and ``bounds`` dicts by state name (``bounds["w"]`` the weight's); a missing state is zero."""
    c = dict(DEFAULTS, **cfg)
    names = state_names(kind, c)
    st = {k: (states[k] if k in states else np.zeros_like(w)) for k in names}
    common = dict(lr=c["learning_rate"], wd=c["wd"], rescale=c["rescale_grad"], clip=c["clip_gradient"])
    if kind == "nag":
        w, m, bw, bm = nag(w, st.get("mom"), ids, g, momentum=c["momentum"], **common)
        return w, ({"mom": m} if names else {}), ({"w": bw, "mom": bm} if names else {"w": bw})
    if kind == "adagrad":
        eps = 1e-7 if c["epsilon"] is None else c["epsilon"]
        w, h, bw, bh = adagrad(w, st["history"], ids, g, eps=eps, **common)
        return w, {"history": h}, {"w": bw, "history": bh}
    if kind == "rmsprop":
        eps = 1e-8 if c["epsilon"] is None else c["epsilon"]
        w, n, gb, dl, bw, bn, bg, bd = rmsprop(w, st["n"], st.get("g"), st.get("delta"), ids, g, gamma1=c["gamma1"],
                                               gamma2=c["gamma2"], eps=eps, centered=c["centered"], **common)
        if c["centered"]:
            return w, {"n": n, "g": gb, "delta": dl}, {"w": bw, "n": bn, "g": bg, "delta": bd}
        return w, {"n": n}, {"w": bw, "n": bn}
    if kind == "ftrl":
        w, z, n, bw, bz, bn = ftrl(w, st["z"], st["n"], ids, g, lamda1=c["lamda1"], beta=c["beta"], **common)
        return w, {"z": z, "n": n}, {"w": bw, "z": bz, "n": bn}
    raise ValueError(kind)


def step64(kind, w, states, g, **cfg):
    """The same update of every element evaluated in float64 from the fp32 inputs and the fp32-rounded
    hyperparameters (``1 - gamma1`` as the contract forms it): ``(w, states)``, nothing rounded to fp32."""
    c = dict(DEFAULTS, **cfg)
    d = lambda x: float(f32(x))  # noqa: E731
    w = np.asarray(w, np.float64)
    st = {k: np.asarray(states[k], np.float64) if k in states else np.zeros_like(w) for k in state_names(kind, c)}
    lr, wd = d(c["learning_rate"]), d(c["wd"])
    g2 = np.asarray(g, np.float64) * d(c["rescale_grad"])
    if c["clip_gradient"] is not None:
        cl = d(c["clip_gradient"])
        g2 = np.where(g2 > cl, cl, np.where(g2 < -cl, -cl, g2))
    if kind == "nag":
        g3 = g2 + wd * w
        if not c["momentum"]:
            return w - lr * g3, {}
        m = d(c["momentum"]) * st["mom"] + g3
        return w - lr * (g3 + d(c["momentum"]) * m), {"mom": m}
    if kind == "adagrad":
        h = st["history"] + g2 * g2
        eps = d(1e-7 if c["epsilon"] is None else c["epsilon"])
        return w - lr * (g2 / np.sqrt(h + eps) + wd * w), {"history": h}
    if kind == "rmsprop":
        g1, omg, eps = d(c["gamma1"]), d(1 - c["gamma1"]), d(1e-8 if c["epsilon"] is None else c["epsilon"])
        g3 = g2 + wd * w
        n = omg * g3 * g3 + g1 * st["n"]
        if not c["centered"]:
            return w - lr * g3 / np.sqrt(n + eps), {"n": n}
        gb = omg * g3 + g1 * st["g"]
        delta = d(c["gamma2"]) * st["delta"] - lr * g3 / np.sqrt(n - gb * gb + eps)
        return w + delta, {"n": n, "g": gb, "delta": delta}
    l1, beta = d(c["lamda1"]), d(c["beta"])
    n1 = st["n"] + g2 * g2
    r1 = np.sqrt(n1)
    z = st["z"] + g2 - (r1 - np.sqrt(st["n"])) / lr * w
    wn = np.where(np.abs(z) <= l1, 0.0, (np.copysign(l1, z) - z) / ((beta + r1) / lr + wd))
    return wn, {"z": z, "n": n1}


def within(got, want, bound, what):
    """``|got - want| <= bound`` elementwise, with the worst element named."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), got.shape)
    excess = np.abs(got - want) - bound
    assert np.all(excess <= 0), (f"{what}: off by {np.abs(got - want).max():.3e}, bound "
                                 f"{bound.reshape(-1)[np.argmax(excess)]:.3e} at {np.argmax(excess)}")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
