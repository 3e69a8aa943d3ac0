"""An independent float64 per-tensor LARS / LAMB loop shared by the layer-wise optimizer tests (CPU, GPU and the
2-rank workers).  ``segs`` is a list of ``(lo, hi, tensor)`` over the flat vector the reference holds and ``adapt``
one boolean per tensor id: a tensor may be made of several segments, its norms are taken over all of them."""
import math

import torch


class _Ref:
    def __init__(self, w0, segs, adapt, lr, weight_decay=0.0, grad_scale=1.0, clip_norm=None, ema_decay=None):
        self.w = w0.detach().double().cpu().clone()
        self.segs, self.adapt = list(segs), list(adapt)
        self.lr, self.wd, self.gs, self.clip, self.d = lr, weight_decay, grad_scale, clip_norm, ema_decay
        self.ema = self.w.clone() if ema_decay is not None else None
        self.t = 0
        self.ratios = [1.0] * len(self.adapt)
        self.norm = float("nan")

    def _grad(self, grad):
        g = grad.detach().double().cpu() * self.gs
        self.norm = g.norm().item()
        if self.clip is not None:
            g = g * (self.clip / max(self.norm, self.clip))
        return g

    def _sq(self, x, t):
        return sum(x[lo:hi].square().sum().item() for lo, hi, tt in self.segs if tt == t)

    def _ema(self):
        if self.ema is not None:
            self.ema += (1.0 - self.d) * (self.w - self.ema)


class RefLARS(_Ref):
    def __init__(self, w0, segs, adapt, lr, momentum=0.9, weight_decay=0.0, nesterov=False, trust_coef=0.001, eps=0.0,
                 **kw):
        super().__init__(w0, segs, adapt, lr, weight_decay, **kw)
        self.mu, self.nesterov, self.tc, self.eps = momentum, nesterov, trust_coef, eps
        self.v = torch.zeros_like(self.w)

    def step(self, grad):
        self.t += 1
        g = self._grad(grad)
        for t, ad in enumerate(self.adapt):
            ratio, wd = 1.0, 0.0
            if ad:
                wn, gn, wd = math.sqrt(self._sq(self.w, t)), math.sqrt(self._sq(g, t)), self.wd
                if wn > 0.0 and gn > 0.0:
                    ratio = self.tc * wn / (gn + wd * wn + self.eps)
            self.ratios[t] = ratio
            for lo, hi, tt in self.segs:
                if tt != t:
                    continue
                gk = ratio * (g[lo:hi] + wd * self.w[lo:hi])
                self.v[lo:hi] = self.mu * self.v[lo:hi] + gk
                self.w[lo:hi] -= self.lr * (gk + self.mu * self.v[lo:hi] if self.nesterov else self.v[lo:hi])
        self._ema()


class RefLAMB(_Ref):
    def __init__(self, w0, segs, adapt, lr, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, **kw):
        super().__init__(w0, segs, adapt, lr, weight_decay, **kw)
        self.b1, self.b2, self.eps = betas[0], betas[1], eps
        self.m, self.v = torch.zeros_like(self.w), torch.zeros_like(self.w)

    def step(self, grad):
        self.t += 1
        g = self._grad(grad)
        self.m = self.b1 * self.m + (1 - self.b1) * g
        self.v = self.b2 * self.v + (1 - self.b2) * g * g
        bc1, bc2 = 1 - self.b1 ** self.t, 1 - self.b2 ** self.t
        base = (self.m / bc1) / ((self.v / bc2).sqrt() + self.eps)
        for t, ad in enumerate(self.adapt):
            wd = self.wd if ad else 0.0
            u = base + wd * self.w
            ratio = 1.0
            if ad:
                wn, un = math.sqrt(self._sq(self.w, t)), math.sqrt(self._sq(u, t))
                if wn > 0.0 and un > 0.0:
                    ratio = wn / un
            self.ratios[t] = ratio
            for lo, hi, tt in self.segs:
                if tt == t:
                    self.w[lo:hi] -= self.lr * ratio * u[lo:hi]
        self._ema()


def segs_of(sizes):
    """Consecutive segments of ``sizes`` floats, one tensor each: (segs, starts)."""
    starts = [0]
    for s in sizes:
        starts.append(starts[-1] + s)
    return [(starts[i], starts[i + 1], i) for i in range(len(sizes))], starts
