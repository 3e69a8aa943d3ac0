// The element-wise pieces shared by the flat-shard apply kernel (optim.hip), the layer-wise kernels
// (layerwise.hip) and the parameter-server data plane (ps_plane.hip): the 4-element loads and stores, the
// bf16 resync, the updates themselves (fp32 math, TF / torch.optim semantics: SGD with (Nesterov) momentum
// and L2 weight decay; Adam / AdamW with bias correction; Adagrad; RMSProp in torch's and in TF's form) and
// kind_update4, the one place that maps a kind's hp layout onto its update.
#pragma once
#include "common.h"

namespace tony {

// The kind codes of ops/optim.py plane_state(), tony_optim_apply_x and tony_ps_apply.
enum OptKind : int { kSGD = 0, kAdam = 1, kAdagrad = 2, kRMSProp = 3 };

// -- 4 elements in and out --------------------------------------------------------------------------------
template <bool kGradBf16>
__device__ __forceinline__ void load_grad4(const void* g, int64_t i, float* out) {
  if constexpr (kGradBf16) {
    const uint2 v = *reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(g) + i);
    out[0] = __uint_as_float(v.x << 16);
    out[1] = __uint_as_float(v.x & 0xffff0000u);
    out[2] = __uint_as_float(v.y << 16);
    out[3] = __uint_as_float(v.y & 0xffff0000u);
  } else {
    const float4 v = *reinterpret_cast<const float4*>(static_cast<const float*>(g) + i);
    out[0] = v.x;
    out[1] = v.y;
    out[2] = v.z;
    out[3] = v.w;
  }
}

__device__ __forceinline__ void load4(const float* p, float* f) {
  const float4 v = *reinterpret_cast<const float4*>(p);
  f[0] = v.x;
  f[1] = v.y;
  f[2] = v.z;
  f[3] = v.w;
}

__device__ __forceinline__ void store4(float* p, const float* f) {
  *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
}

__device__ __forceinline__ void store_bf16x4(uint16_t* p, const float* f) {
  uint2 v;
  v.x = static_cast<uint32_t>(f2bf(f[0])) | (static_cast<uint32_t>(f2bf(f[1])) << 16);
  v.y = static_cast<uint32_t>(f2bf(f[2])) | (static_cast<uint32_t>(f2bf(f[3])) << 16);
  *reinterpret_cast<uint2*>(p) = v;
}

// An element whose bf16 compute copy no longer equals bf16(master) was overwritten behind the optimizer
// (load_state_dict, a Horovod broadcast_parameters, a checkpoint restore into the module): it counts, and is
// updated, with the copy's value.
__device__ __forceinline__ void resync4(float* wf, const uint16_t* w_bf16) {
  const uint2 cv = *reinterpret_cast<const uint2*>(w_bf16);
  const uint16_t cur[4] = {static_cast<uint16_t>(cv.x & 0xffffu), static_cast<uint16_t>(cv.x >> 16),
                           static_cast<uint16_t>(cv.y & 0xffffu), static_cast<uint16_t>(cv.y >> 16)};
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (cur[k] != f2bf(wf[k])) wf[k] = bf2f(cur[k]);
}

// -- the updates ------------------------------------------------------------------------------------------

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

// The update of kKind from that kind's hp layout (csrc/optim.hip): s0f = SGD v / Adam m / Adagrad h / RMSProp ms,
// s1f = Adam v / RMSProp mom (untouched by the one-state kinds).  kScaled: the gradient scale is hp's times
// gs_mul (the clip coefficient); otherwise hp's own, with no multiply at all.
template <int kKind, bool kScaled>
__device__ __forceinline__ void kind_update4(float* wf, float* s0f, float* s1f, const float* gf, const float* hp,
                                             float gs_mul) {
  constexpr int kGs = kKind == kSGD || kKind == kAdagrad ? 3 : 5;
  const float gs = kScaled ? hp[kGs] * gs_mul : hp[kGs];
  if constexpr (kKind == kSGD) {
    sgd_update4(wf, s0f, gf, hp[0], hp[1], hp[2], gs, hp[4] != 0.f);
  } else if constexpr (kKind == kAdam) {
    const float lr = hp[0];
    adam_update4(wf, s0f, s1f, gf, lr, hp[1], hp[2], hp[3], hp[4], gs, lr / hp[6], rsqrtf(hp[7]), hp[8] != 0.f);
  } else if constexpr (kKind == kAdagrad) {
    adagrad_update4(wf, s0f, gf, hp[0], hp[1], hp[2], gs);
  } else {
    static_assert(kKind == kRMSProp, "unknown optimizer kind");
    rmsprop_update4(wf, s0f, s1f, gf, hp[0], hp[1], hp[2], hp[3], hp[4], gs, hp[6] != 0.f);
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
