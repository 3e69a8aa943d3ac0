// The element-wise optimizer updates shared by the flat-shard apply kernels (optim.hip) and the
// parameter-server data plane (ps_plane.hip): 4 elements per call, fp32 math, TF / torch.optim
// semantics (SGD with (Nesterov) momentum and L2 weight decay; Adam / AdamW with bias correction;
// Adagrad; RMSProp in torch's and in TF's form).
#pragma once
#include "common.h"

namespace tony {

// v = mu v + (g gs + wd w);  w -= lr (nesterov ? g' + mu v : v)
__device__ __forceinline__ void sgd_update4(float* wf, float* vf, const float* gf, float lr, float mu, float wd,
                                            float gs, bool nesterov) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float gk = fmaf(gf[k], gs, wd * wf[k]);
    vf[k] = fmaf(mu, vf[k], gk);
    const float upd = nesterov ? fmaf(mu, vf[k], gk) : vf[k];
    wf[k] = fmaf(-lr, upd, wf[k]);
  }
}

// m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  w -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps)
// (decoupled: w *= 1 - lr wd first, AdamW; else g += wd w)
__device__ __forceinline__ void adam_update4(float* wf, float* mf, float* vf, const float* gf, float lr, float b1,
                                             float b2, float eps, float wd, float gs, float step_size,
                                             float inv_sqrt_bc2, bool decoupled) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float gk = gf[k] * gs;
    if (decoupled)
      wf[k] *= (1.f - lr * wd);
    else
      gk = fmaf(wd, wf[k], gk);
    mf[k] = fmaf(b1, mf[k], (1.f - b1) * gk);
    vf[k] = fmaf(b2, vf[k], (1.f - b2) * gk * gk);
    const float denom = sqrtf(vf[k]) * inv_sqrt_bc2 + eps;
    wf[k] = fmaf(-step_size, mf[k] / denom, wf[k]);
  }
}

// g' = g gs + wd w;  h += g'^2;  w -= lr g' / (sqrt(h) + eps)   (torch.optim.Adagrad, lr_decay 0; Keras Adagrad)
__device__ __forceinline__ void adagrad_update4(float* wf, float* hf, const float* gf, float lr, float eps, float wd,
                                                float gs) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float gk = fmaf(gf[k], gs, wd * wf[k]);
    hf[k] = fmaf(gk, gk, hf[k]);
    wf[k] = fmaf(-lr, gk / (sqrtf(hf[k]) + eps), wf[k]);
  }
}

// g' = g gs + wd w;  ms = alpha ms + (1-alpha) g'^2   (not centered; mom is kept even when mu = 0)
//   torch (tf_style false): mom = mu mom + g' / (sqrt(ms) + eps);      w -= lr mom   (torch.optim.RMSprop)
//   TF    (tf_style true):  mom = mu mom + lr g' / sqrt(ms + eps);     w -= mom      (tf.train.RMSPropOptimizer)
__device__ __forceinline__ void rmsprop_update4(float* wf, float* sf, float* mf, const float* gf, float lr,
                                                float alpha, float mu, float eps, float wd, float gs, bool tf_style) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float gk = fmaf(gf[k], gs, wd * wf[k]);
    sf[k] = fmaf(alpha, sf[k], (1.f - alpha) * gk * gk);
    if (tf_style) {
      mf[k] = fmaf(mu, mf[k], lr * gk / sqrtf(sf[k] + eps));
      wf[k] -= mf[k];
    } else {
      mf[k] = fmaf(mu, mf[k], gk / (sqrtf(sf[k]) + eps));
      wf[k] = fmaf(-lr, mf[k], wf[k]);
    }
  }
}

// LAMB (csrc/layerwise.hip).  The moments are Adam's with gk = g gs (gs carries the clip coefficient):
//   m = b1 m + (1-b1) gk;  v = b2 v + (1-b2) gk^2
__device__ __forceinline__ void lamb_moments4(float* mf, float* vf, const float* gf, float b1, float b2, float gs) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float gk = gf[k] * gs;
    mf[k] = fmaf(b1, mf[k], (1.f - b1) * gk);
    vf[k] = fmaf(b2, vf[k], (1.f - b2) * gk * gk);
  }
}

// u = (m / bc1) / (sqrt(v / bc2) + eps) + wd_t w: the norm pass and the apply both form it with these very
// operations from the stored m, v and the old w, so the norm is the norm of what is applied.
__device__ __forceinline__ void lamb_u4(float* uf, const float* wf, const float* mf, const float* vf, float bc1,
                                        float bc2, float eps, float wd) {
#pragma unroll
  for (int k = 0; k < 4; ++k) uf[k] = fmaf(wd, wf[k], (mf[k] / bc1) / (sqrtf(vf[k] / bc2) + eps));
}

// ema += (1 - d) (w - ema)  (tf.train.ExponentialMovingAverage.apply; omd = 1 - d, formed on the host in double)
__device__ __forceinline__ void ema_update4(float* ef, const float* wf, float omd) {
#pragma unroll
  for (int k = 0; k < 4; ++k) ef[k] = fmaf(omd, wf[k] - ef[k], ef[k]);
}

}  // namespace tony
