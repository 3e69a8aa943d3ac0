// Layer-wise adaptive optimizers over flat parameter shards: LARS (SGD-momentum) and LAMB (Adam), which scale each
// parameter TENSOR's update by a trust ratio ||w|| / ||update|| taken over that tensor alone.
//
// The flat optimizers of optim.hip see one anonymous run of floats.  Here the host describes the shard as a work
// list of items (lo4, hi4, tensor, 0) -- float4 indices into the master shard, at most kItemFloats floats each, every
// item inside ONE tensor's segment -- and every streaming kernel runs one workgroup per item, so the tensor of an
// element is a uniform load, never a search.  A step is
//   norm pass   one (sum w^2, sum x^2) pair per item, stored (no float atomics: the same inputs give the same bits)
//               LARS: x = g, read only (with resync: w as the apply will see it, from the bf16 compute copy)
//               LAMB: the Adam moment update (writes m, v), x = u = (m/bc1) / (sqrt(v/bc2) + eps) + wd_t w
//   fold        tsum[T][2] = each tensor's pairs summed in item order, in double, stored as fp32
//               (a sharded parameter server all-reduces tsum here: a tensor cut by a piece boundary has items on
//               two ranks)
//   ratio       table[T] = (ratio_t, wd_t), formed in double and rounded once; non-adapted tensors get (1, 0)
//   apply       LARS: sgd_update4 with gs' = gs coef ratio_t, wd' = wd_t ratio_t  (v = mu v + ratio (g + wd w))
//               LAMB: w -= lr ratio_t u, u recomputed from the stored m, v and the old w
// with the EMA beside the master, the bf16 compute copy and the non-finite skip of optim.hip's tony_optim_apply_x.
//   LARS hp = [lr, momentum, weight_decay, grad_scale, nesterov, resync, trust_coef, eps]   (SGD's six first)
//   LAMB hp = [lr, beta1, beta2, eps, weight_decay, grad_scale, bias_corr1, bias_corr2]
//   xhp, ctl: as in optim.hip (ctl = [coef, skip, norm, skipped steps]; nullptr: coef 1, no skip)
// `off4` is the float4 index (in master coordinates) of the first element of the gradient and of the bf16 copy
// handed to a launch: a sharded caller passes one bucket's piece of both.
#include "common.h"
#include "optim_math.h"

using namespace tony;

namespace {

constexpr int kThreads = 256;
constexpr int kItemFloats = 4096;  // 4 float4 per thread: ~6,600 workgroups for the 27M-parameter shard
constexpr int kFoldThreads = 64;

// The workgroup's (a, b) in a fixed order: lanes by butterfly, the four waves in wave order.
__device__ __forceinline__ void store_pair(float a, float b, float2* out) {
  __shared__ float part[kThreads / kWave][2];
  a = wave_sum(a);
  b = wave_sum(b);
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  if (lane == 0) {
    part[wid][0] = a;
    part[wid][1] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float ta = 0.f, tb = 0.f;
    for (int k = 0; k < kThreads / kWave; ++k) {
      ta += part[k][0];
      tb += part[k][1];
    }
    *out = make_float2(ta, tb);
  }
}

template <bool kGradBf16>
__global__ __launch_bounds__(kThreads) void lars_norm_kernel(const float* __restrict__ w, const void* __restrict__ g,
                                                             const uint16_t* __restrict__ w_bf16, int64_t off4,
                                                             const int4* __restrict__ items,
                                                             float2* __restrict__ partials,
                                                             const float* __restrict__ hp) {
  const int4 it = items[blockIdx.x];
  const bool resync = hp[5] != 0.f && w_bf16 != nullptr;
  float sw = 0.f, sg = 0.f;
#pragma unroll 4
  for (int64_t q = it.x + threadIdx.x; q < it.y; q += kThreads) {
    const int64_t i = q * 4, j = (q - off4) * 4;
    float gf[4], wf[4];
    load_grad4<kGradBf16>(g, j, gf);
    load4(w + i, wf);
    if (resync) resync4(wf, w_bf16 + j);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      sw = fmaf(wf[k], wf[k], sw);
      sg = fmaf(gf[k], gf[k], sg);
    }
  }
  store_pair(sw, sg, partials + blockIdx.x);
}

template <bool kGradBf16>
__global__ __launch_bounds__(kThreads) void lamb_norm_kernel(const float* __restrict__ w, float* __restrict__ m,
                                                             float* __restrict__ v, const void* __restrict__ g,
                                                             int64_t off4, const int4* __restrict__ items,
                                                             const int* __restrict__ adapt,
                                                             float2* __restrict__ partials,
                                                             const float* __restrict__ hp,
                                                             const float* __restrict__ ctl) {
  float coef = 1.f;
  if (ctl != nullptr) {
    if (ctl[1] != 0.f) return;  // a skipped step touches nothing, the moments included
    coef = ctl[0];
  }
  const int4 it = items[blockIdx.x];
  const float b1 = hp[1], b2 = hp[2], eps = hp[3], gs = hp[5] * coef, bc1 = hp[6], bc2 = hp[7];
  const float wd = adapt[it.z] != 0 ? hp[4] : 0.f;
  float sw = 0.f, su = 0.f;
#pragma unroll 2
  for (int64_t q = it.x + threadIdx.x; q < it.y; q += kThreads) {
    const int64_t i = q * 4;
    float gf[4], wf[4], mf[4], vf[4], uf[4];
    load_grad4<kGradBf16>(g, (q - off4) * 4, gf);
    load4(w + i, wf);
    load4(m + i, mf);
    load4(v + i, vf);
    lamb_moments4(mf, vf, gf, b1, b2, gs);
    store4(m + i, mf);
    store4(v + i, vf);
    lamb_u4(uf, wf, mf, vf, bc1, bc2, eps, wd);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      sw = fmaf(wf[k], wf[k], sw);
      su = fmaf(uf[k], uf[k], su);
    }
  }
  store_pair(sw, su, partials + blockIdx.x);
}

// tsum[t] = the pairs of tensor t's items (order[tstart[t] .. tstart[t+1])) summed in that order, in double: each
// thread a contiguous run, the runs in thread order.  A tensor without an item on this shard gets (0, 0).
__global__ __launch_bounds__(kFoldThreads) void fold_kernel(const float2* __restrict__ partials,
                                                            const int* __restrict__ order,
                                                            const int* __restrict__ tstart,
                                                            float2* __restrict__ tsum) {
  __shared__ double run[kFoldThreads][2];
  const int t = blockIdx.x;
  const int lo = tstart[t], hi = tstart[t + 1];
  const int per = (hi - lo + kFoldThreads - 1) / kFoldThreads;
  const int a = lo + threadIdx.x * per;
  const int b = a + per < hi ? a + per : hi;
  double s0 = 0.0, s1 = 0.0;
  for (int j = a; j < b; ++j) {
    const float2 p = partials[order[j]];
    s0 += static_cast<double>(p.x);
    s1 += static_cast<double>(p.y);
  }
  run[threadIdx.x][0] = s0;
  run[threadIdx.x][1] = s1;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double S0 = 0.0, S1 = 0.0;
  for (int k = 0; k < kFoldThreads; ++k) {
    S0 += run[k][0];
    S1 += run[k][1];
  }
  tsum[t] = make_float2(static_cast<float>(S0), static_cast<float>(S1));
}

// kind 0 LARS: ratio = trust_coef wn / (gn + wd wn + eps), gn = gs coef sqrt(sum g^2)   (1 unless wn, gn > 0)
// kind 1 LAMB: ratio = wn / un                                                         (1 unless wn, un > 0)
__global__ __launch_bounds__(kThreads) void ratio_kernel(int kind, const float2* __restrict__ tsum,
                                                         const int* __restrict__ adapt, int T,
                                                         const float* __restrict__ hp,
                                                         const float* __restrict__ ctl,
                                                         float2* __restrict__ table) {
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= T) return;
  double coef = 1.0;
  if (ctl != nullptr) {
    if (ctl[1] != 0.f) return;  // skipped: the table of the last applied step stays
    coef = static_cast<double>(ctl[0]);
  }
  if (adapt[t] == 0) {
    table[t] = make_float2(1.f, 0.f);
    return;
  }
  const float2 s = tsum[t];
  const double wn = sqrt(static_cast<double>(s.x));
  double ratio = 1.0;
  float wd;
  if (kind == 0) {
    wd = hp[2];
    const double gn = static_cast<double>(hp[3]) * coef * sqrt(static_cast<double>(s.y));
    if (wn > 0.0 && gn > 0.0)
      ratio = static_cast<double>(hp[6]) * wn / (gn + static_cast<double>(wd) * wn + static_cast<double>(hp[7]));
  } else {
    wd = hp[4];
    const double un = sqrt(static_cast<double>(s.y));
    if (wn > 0.0 && un > 0.0) ratio = wn / un;
  }
  table[t] = make_float2(static_cast<float>(ratio), wd);
}

template <bool kGradBf16>
__global__ __launch_bounds__(kThreads) void lars_apply_kernel(float* __restrict__ w, float* __restrict__ v,
                                                              float* __restrict__ ema, const void* __restrict__ g,
                                                              uint16_t* __restrict__ w_bf16, int64_t off4,
                                                              const int4* __restrict__ items,
                                                              const float2* __restrict__ table,
                                                              const float* __restrict__ hp,
                                                              const float* __restrict__ xhp,
                                                              const float* __restrict__ ctl) {
  float coef = 1.f;
  if (ctl != nullptr) {
    if (ctl[1] != 0.f) return;  // a skipped step touches nothing
    coef = ctl[0];
  }
  const int4 it = items[blockIdx.x];
  const float2 rt = table[it.z];
  const float lr = hp[0], mu = hp[1], gs = hp[3] * coef * rt.x, wd = rt.y * rt.x;
  const bool nesterov = hp[4] != 0.f;
  const bool resync = hp[5] != 0.f && w_bf16 != nullptr;
  const float omd = ema != nullptr ? xhp[4] : 0.f;
#pragma unroll 2
  for (int64_t q = it.x + threadIdx.x; q < it.y; q += kThreads) {
    const int64_t i = q * 4, j = (q - off4) * 4;
    float gf[4], wf[4], vf[4];
    load_grad4<kGradBf16>(g, j, gf);
    load4(w + i, wf);
    load4(v + i, vf);
    if (resync) resync4(wf, w_bf16 + j);
    sgd_update4(wf, vf, gf, lr, mu, wd, gs, nesterov);
    store4(w + i, wf);
    store4(v + i, vf);
    if (ema != nullptr) {
      float ef[4];
      load4(ema + i, ef);
      ema_update4(ef, wf, omd);
      store4(ema + i, ef);
    }
    if (w_bf16 != nullptr) store_bf16x4(w_bf16 + j, wf);
  }
}

__global__ __launch_bounds__(kThreads) void lamb_apply_kernel(float* __restrict__ w, const float* __restrict__ m,
                                                              const float* __restrict__ v, float* __restrict__ ema,
                                                              uint16_t* __restrict__ w_bf16, int64_t off4,
                                                              const int4* __restrict__ items,
                                                              const float2* __restrict__ table,
                                                              const float* __restrict__ hp,
                                                              const float* __restrict__ xhp,
                                                              const float* __restrict__ ctl) {
  if (ctl != nullptr && ctl[1] != 0.f) return;  // a skipped step touches nothing
  const int4 it = items[blockIdx.x];
  const float2 rt = table[it.z];
  const float step = hp[0] * rt.x, eps = hp[3], bc1 = hp[6], bc2 = hp[7];
  const float omd = ema != nullptr ? xhp[4] : 0.f;
#pragma unroll 2
  for (int64_t q = it.x + threadIdx.x; q < it.y; q += kThreads) {
    const int64_t i = q * 4;
    float wf[4], mf[4], vf[4], uf[4];
    load4(w + i, wf);
    load4(m + i, mf);
    load4(v + i, vf);
    lamb_u4(uf, wf, mf, vf, bc1, bc2, eps, rt.y);
#pragma unroll
    for (int k = 0; k < 4; ++k) wf[k] = fmaf(-step, uf[k], wf[k]);
    store4(w + i, wf);
    if (ema != nullptr) {
      float ef[4];
      load4(ema + i, ef);
      ema_update4(ef, wf, omd);
      store4(ema + i, ef);
    }
    if (w_bf16 != nullptr) store_bf16x4(w_bf16 + (q - off4) * 4, wf);
  }
}

}  // namespace

// Floats of the longest work item the kernels are tuned for (the host cuts segments into items of this length).
TONY_API int tony_layerwise_item_floats() { return kItemFloats; }

// partials[i] = (sum w^2, sum g^2) of item i, i in [0, n_items).  `off` (a multiple of 4): master index of g[0] and
// of w_bf16[0].  w_bf16 is read only, and only when hp[5] (resync) is set.
TONY_API int tony_lars_norm(const float* w, const void* g, int grad_bf16, const void* w_bf16, int64_t off,
                            const void* items, int n_items, float* partials, const float* hp, hipStream_t stream) {
  if (n_items < 0 || off % 4) return -1;
  if (n_items == 0) return 0;
  const int4* it = static_cast<const int4*>(items);
  float2* part = reinterpret_cast<float2*>(partials);
  const uint16_t* cp = static_cast<const uint16_t*>(w_bf16);
  if (grad_bf16)
    lars_norm_kernel<true><<<n_items, kThreads, 0, stream>>>(w, g, cp, off / 4, it, part, hp);
  else
    lars_norm_kernel<false><<<n_items, kThreads, 0, stream>>>(w, g, cp, off / 4, it, part, hp);
  TONY_LAUNCH_CHECK();
  return 0;
}

// The Adam moment update of every item (m, v written) and partials[i] = (sum w^2, sum u^2); nothing at all when
// ctl[1] is set.  adapt[t] != 0: tensor t takes weight decay (and, later, a trust ratio).
TONY_API int tony_lamb_norm(const float* w, float* m, float* v, const void* g, int grad_bf16, int64_t off,
                            const void* items, int n_items, const int* adapt, float* partials, const float* hp,
                            const float* ctl, hipStream_t stream) {
  if (n_items < 0 || off % 4) return -1;
  if (n_items == 0) return 0;
  const int4* it = static_cast<const int4*>(items);
  float2* part = reinterpret_cast<float2*>(partials);
  if (grad_bf16)
    lamb_norm_kernel<true><<<n_items, kThreads, 0, stream>>>(w, m, v, g, off / 4, it, adapt, part, hp, ctl);
  else
    lamb_norm_kernel<false><<<n_items, kThreads, 0, stream>>>(w, m, v, g, off / 4, it, adapt, part, hp, ctl);
  TONY_LAUNCH_CHECK();
  return 0;
}

// tsum[T][2] from the item pairs: order[tstart[t] .. tstart[t+1]) are tensor t's items.
TONY_API int tony_layerwise_fold(const float* partials, const int* order, const int* tstart, int n_tensors,
                                 float* tsum, hipStream_t stream) {
  if (n_tensors <= 0) return -1;
  fold_kernel<<<n_tensors, kFoldThreads, 0, stream>>>(reinterpret_cast<const float2*>(partials), order, tstart,
                                                      reinterpret_cast<float2*>(tsum));
  TONY_LAUNCH_CHECK();
  return 0;
}

// table[T][2] = (ratio_t, wd_t) of `kind` (0 LARS, 1 LAMB) from tsum; left as it is when ctl[1] is set.
TONY_API int tony_layerwise_ratio(int kind, const float* tsum, const int* adapt, int n_tensors, const float* hp,
                                  const float* ctl, float* table, hipStream_t stream) {
  if (n_tensors <= 0) return -1;
  if (kind != 0 && kind != 1) return -4;
  ratio_kernel<<<(n_tensors + kThreads - 1) / kThreads, kThreads, 0, stream>>>(
      kind, reinterpret_cast<const float2*>(tsum), adapt, n_tensors, hp, ctl, reinterpret_cast<float2*>(table));
  TONY_LAUNCH_CHECK();
  return 0;
}

TONY_API int tony_lars_apply(float* w, float* v, float* ema, const void* g, int grad_bf16, void* w_bf16, int64_t off,
                             const void* items, int n_items, const float* table, const float* hp, const float* xhp,
                             const float* ctl, hipStream_t stream) {
  if (n_items < 0 || off % 4) return -1;
  if (ema != nullptr && xhp == nullptr) return -2;
  if (n_items == 0) return 0;
  const int4* it = static_cast<const int4*>(items);
  const float2* tb = reinterpret_cast<const float2*>(table);
  uint16_t* out = static_cast<uint16_t*>(w_bf16);
  if (grad_bf16)
    lars_apply_kernel<true><<<n_items, kThreads, 0, stream>>>(w, v, ema, g, out, off / 4, it, tb, hp, xhp, ctl);
  else
    lars_apply_kernel<false><<<n_items, kThreads, 0, stream>>>(w, v, ema, g, out, off / 4, it, tb, hp, xhp, ctl);
  TONY_LAUNCH_CHECK();
  return 0;
}

TONY_API int tony_lamb_apply(float* w, const float* m, const float* v, float* ema, void* w_bf16, int64_t off,
                             const void* items, int n_items, const float* table, const float* hp, const float* xhp,
                             const float* ctl, hipStream_t stream) {
  if (n_items < 0 || off % 4) return -1;
  if (ema != nullptr && xhp == nullptr) return -2;
  if (n_items == 0) return 0;
  lamb_apply_kernel<<<n_items, kThreads, 0, stream>>>(w, m, v, ema, static_cast<uint16_t*>(w_bf16), off / 4,
                                                      static_cast<const int4*>(items),
                                                      reinterpret_cast<const float2*>(table), hp, xhp, ctl);
  TONY_LAUNCH_CHECK();
  return 0;
}
