// Fused optimizer apply over flat parameter shards.
//
// The parameter server (tony_amd/parallel/ps.py) and the data-parallel engine
// keep every trainable tensor as a view into ONE flat buffer, so a
// "multi-tensor apply" is a single vectorised streaming kernel over the shard
// the rank owns: read fp32 master w, fp32 state, bf16/fp32 grad; write fp32 w,
// state, and the bf16 compute copy that workers pull.  ~20 B/param -> the
// kernel is HBM-bound by construction (27M params ~ 0.1 ms at 6 TB/s).
//
// Hyper-parameters live in a small device array `hp` (not kernel arguments) so
// a captured HIP graph replays with the current learning rate / step.  kind_update4 (optim_math.h) is the
// one reader of these layouts:
//   SGD  hp = [lr, momentum, weight_decay, grad_scale, nesterov, resync]
//        resync != 0 (with a bf16 compute copy): an element whose compute copy no longer equals
//        bf16(master) was overwritten outside the optimizer (load_state_dict, a Horovod
//        broadcast_parameters from rank 0, a checkpoint restore into the module) and its master is
//        re-seeded from it before the update -- one extra 2-byte read per parameter
//   Adam hp = [lr, beta1, beta2, eps, weight_decay, grad_scale, bias_corr1, bias_corr2, decoupled]
//   Adagrad hp = [lr, eps, weight_decay, grad_scale]
//   RMSProp hp = [lr, alpha, momentum, eps, weight_decay, grad_scale, tf_style]
//        tf_style != 0: TF's form (eps inside the root, lr folded into the momentum; optim_math.h)
#include "common.h"
#include "optim_math.h"

using namespace tony;

namespace {

constexpr int kThreads = 256;

// Sum of squares + non-finite flag over a flat bf16/fp32 gradient (H12):
// out[0] += sum(g^2), out[1] = 1 if any element is inf/nan.
template <bool kGradBf16>
__global__ __launch_bounds__(kThreads) void grad_stats_kernel(const void* __restrict__ g, int64_t n4,
                                                              float* __restrict__ out) {
  __shared__ float part[kThreads / kWave];
  float acc = 0.f;
  bool bad = false;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
  for (int64_t q = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; q < n4; q += stride) {
    float gf[4];
    load_grad4<kGradBf16>(g, q * 4, gf);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      acc = fmaf(gf[k], gf[k], acc);
      bad |= !isfinite(gf[k]);
    }
  }
  acc = wave_sum(acc);
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  if (lane == 0) part[wid] = acc;
  if (__any(bad) && lane == 0) out[1] = 1.f;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int k = 0; k < kThreads / kWave; ++k) t += part[k];
    atomicAdd(out, t);
  }
}

int grid_for(int64_t n4) {
  int64_t g = (n4 + kThreads - 1) / kThreads;
  if (g > 8192) g = 8192;  // 32 WGs per CU, grid-stride beyond that
  return static_cast<int>(g < 1 ? 1 : g);
}

// -- global-norm clipping, non-finite step skip, EMA of the variables ------------------------------------
// Three launches on one stream: grad_sumsq (one fp32 partial per workgroup of a FIXED grid, stored, so the
// result does not depend on arrival order), clip_ctl (one workgroup folds the partials of every bucket into
// ctl = [coef, skip, norm, skipped steps]) and tony_optim_apply_x (optim_apply_kernel with kExt: the update of
// `kind`, its gradient scale times coef, nothing at all when skip is set, the EMA beside the master).
//   xhp = [clip_norm, base_grad_scale, skip_nonfinite, ema_decay, 1 - ema_decay]   (host-pushed, like hp)
constexpr int kSumsqGrid = 1024;  // workgroups of every grad_sumsq launch = floats of one partial block

template <bool kGradBf16>
__global__ __launch_bounds__(kThreads) void grad_sumsq_kernel(const void* __restrict__ g, int64_t n4,
                                                              float* __restrict__ partials) {
  __shared__ float part[kThreads / kWave];
  float acc = 0.f;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
#pragma unroll 4
  for (int64_t q = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; q < n4; q += stride) {
    float gf[4];
    load_grad4<kGradBf16>(g, q * 4, gf);
#pragma unroll
    for (int k = 0; k < 4; ++k) acc = fmaf(gf[k], gf[k], acc);
  }
  acc = wave_sum(acc);
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  if (lane == 0) part[wid] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int k = 0; k < kThreads / kWave; ++k) t += part[k];
    partials[blockIdx.x] = t;  // a workgroup past the end of the gradient stores its 0
  }
}

// S = sum of the partials in index order (each thread a contiguous run, the runs in thread order), in double.
__global__ __launch_bounds__(kThreads) void clip_ctl_kernel(const float* __restrict__ partials, int n,
                                                            const float* __restrict__ xhp,
                                                            float* __restrict__ ctl) {
  __shared__ double run[kThreads];
  const int per = (n + kThreads - 1) / kThreads;
  const int lo = threadIdx.x * per;
  const int hi = lo + per < n ? lo + per : n;
  double s = 0.0;
  for (int i = lo; i < hi; ++i) s += static_cast<double>(partials[i]);
  run[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double S = 0.0;
  for (int k = 0; k < kThreads; ++k) S += run[k];
  const float clip = xhp[0], gs = xhp[1];
  const bool skip = xhp[2] != 0.f && !isfinite(S);
  const float norm = static_cast<float>(static_cast<double>(gs) * sqrt(S));
  // tf.clip_by_global_norm: exactly 1 when nothing clips, no epsilon
  const float coef = clip > 0.f ? clip / fmaxf(norm, clip) : 1.f;
  ctl[0] = coef;
  ctl[1] = skip ? 1.f : 0.f;
  ctl[2] = norm;
  if (skip) ctl[3] += 1.f;
}

// The one apply kernel of the four kinds (OptKind, optim_math.h): s0 / s1 as kind_update4 takes them, s1 unused by
// the one-state kinds.  kExt false is the plain step (ema, xhp, ctl unused); kExt true adds the clip coefficient
// and the skip of ctl (nullptr: coef 1, no skip) and the EMA beside the master (nullptr: none).
template <int kKind, bool kGradBf16, bool kExt>
__global__ __launch_bounds__(kThreads) void optim_apply_kernel(float* __restrict__ w, float* __restrict__ s0,
                                                               float* __restrict__ s1, float* __restrict__ ema,
                                                               const void* __restrict__ g,
                                                               uint16_t* __restrict__ w_bf16, int64_t n4,
                                                               const float* __restrict__ hp,
                                                               const float* __restrict__ xhp,
                                                               const float* __restrict__ ctl) {
  float coef = 1.f, omd = 0.f;
  if constexpr (kExt) {
    if (ctl != nullptr) {
      if (ctl[1] != 0.f) return;  // a skipped step touches nothing
      coef = ctl[0];
    }
    if (ema != nullptr) omd = xhp[4];
  }
  constexpr bool kTwo = kKind == kAdam || kKind == kRMSProp;
  const bool resync = kKind == kSGD && hp[5] != 0.f && w_bf16 != nullptr;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
  for (int64_t q = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; q < n4; q += stride) {
    const int64_t i = q * 4;
    float gf[4], wf[4], af[4], bf[4];
    load_grad4<kGradBf16>(g, i, gf);
    load4(w + i, wf);
    load4(s0 + i, af);
    if constexpr (kTwo) load4(s1 + i, bf);
    if (resync) resync4(wf, w_bf16 + i);
    kind_update4<kKind, kExt>(wf, af, bf, gf, hp, coef);
    store4(w + i, wf);
    store4(s0 + i, af);
    if constexpr (kTwo) store4(s1 + i, bf);
    if constexpr (kExt) {
      if (ema != nullptr) {
        float ef[4];
        load4(ema + i, ef);
        ema_update4(ef, wf, omd);
        store4(ema + i, ef);
      }
    }
    if (w_bf16 != nullptr) store_bf16x4(w_bf16 + i, wf);
  }
}

// n must be a multiple of 4 (flat buffers are padded by the caller).
template <int kKind, bool kExt>
int launch_apply(float* w, float* s0, float* s1, float* ema, const void* g, int grad_bf16, void* w_bf16, int64_t n,
                 const float* hp, const float* xhp, const float* ctl, hipStream_t stream) {
  if (n % 4) return -1;
  const int64_t n4 = n / 4;
  uint16_t* out = static_cast<uint16_t*>(w_bf16);
  if (grad_bf16)
    optim_apply_kernel<kKind, true, kExt><<<grid_for(n4), kThreads, 0, stream>>>(w, s0, s1, ema, g, out, n4, hp, xhp,
                                                                                 ctl);
  else
    optim_apply_kernel<kKind, false, kExt><<<grid_for(n4), kThreads, 0, stream>>>(w, s0, s1, ema, g, out, n4, hp, xhp,
                                                                                  ctl);
  TONY_LAUNCH_CHECK();
  return 0;
}

}  // namespace

TONY_API int tony_sgd_step(float* w, float* v, const void* g, int grad_bf16, void* w_bf16, int64_t n,
                           const float* hp, hipStream_t stream) {
  return launch_apply<kSGD, false>(w, v, nullptr, nullptr, g, grad_bf16, w_bf16, n, hp, nullptr, nullptr, stream);
}

TONY_API int tony_adam_step(float* w, float* m, float* v, const void* g, int grad_bf16, void* w_bf16,
                            int64_t n, const float* hp, hipStream_t stream) {
  return launch_apply<kAdam, false>(w, m, v, nullptr, g, grad_bf16, w_bf16, n, hp, nullptr, nullptr, stream);
}

TONY_API int tony_adagrad_step(float* w, float* h, const void* g, int grad_bf16, void* w_bf16, int64_t n,
                               const float* hp, hipStream_t stream) {
  return launch_apply<kAdagrad, false>(w, h, nullptr, nullptr, g, grad_bf16, w_bf16, n, hp, nullptr, nullptr, stream);
}

TONY_API int tony_rmsprop_step(float* w, float* ms, float* mom, const void* g, int grad_bf16, void* w_bf16,
                               int64_t n, const float* hp, hipStream_t stream) {
  return launch_apply<kRMSProp, false>(w, ms, mom, nullptr, g, grad_bf16, w_bf16, n, hp, nullptr, nullptr, stream);
}

TONY_API int tony_grad_stats(const void* g, int grad_bf16, int64_t n, float* out, hipStream_t stream) {
  if (n % 4) return -1;
  const int64_t n4 = n / 4;
  (void)hipMemsetAsync(out, 0, 2 * sizeof(float), stream);
  const int grid = grid_for(n4) > 1024 ? 1024 : grid_for(n4);
  if (grad_bf16)
    grad_stats_kernel<true><<<grid, kThreads, 0, stream>>>(g, n4, out);
  else
    grad_stats_kernel<false><<<grid, kThreads, 0, stream>>>(g, n4, out);
  TONY_LAUNCH_CHECK();
  return 0;
}

// Floats of one partial block: every tony_grad_sumsq launch stores exactly this many.
TONY_API int tony_grad_sumsq_blocks() { return kSumsqGrid; }

// partials[0 .. kSumsqGrid) = per-workgroup sums of g^2, in a fixed order (no atomics: bit-reproducible).
TONY_API int tony_grad_sumsq(const void* g, int grad_bf16, int64_t n, float* partials, hipStream_t stream) {
  if (n % 4 || n < 0) return -1;
  const int64_t n4 = n / 4;
  if (grad_bf16)
    grad_sumsq_kernel<true><<<kSumsqGrid, kThreads, 0, stream>>>(g, n4, partials);
  else
    grad_sumsq_kernel<false><<<kSumsqGrid, kThreads, 0, stream>>>(g, n4, partials);
  TONY_LAUNCH_CHECK();
  return 0;
}

// ctl = [coef, skip, norm, skipped steps (+= skip)] from the partial blocks of every bucket, laid end to end.
TONY_API int tony_clip_ctl(const float* partials, int n_partials, const float* xhp, float* ctl,
                           hipStream_t stream) {
  if (n_partials < 0) return -1;
  clip_ctl_kernel<<<1, kThreads, 0, stream>>>(partials, n_partials, xhp, ctl);
  TONY_LAUNCH_CHECK();
  return 0;
}

// The update of `kind` (0 SGD, 1 Adam, 2 Adagrad, 3 RMSProp; hp in that kind's layout above) with the gradient
// scale times ctl[0], nothing at all when ctl[1] is set, and ema += xhp[4] (w_new - ema) when ema is given.
// ctl == nullptr: coef 1, no skip.  s1 is ignored by the one-state kinds.
TONY_API int tony_optim_apply_x(int kind, float* w, float* s0, float* s1, float* ema, const void* g, int grad_bf16,
                                void* w_bf16, int64_t n, const float* hp, const float* xhp, const float* ctl,
                                hipStream_t stream) {
  if (n % 4 || n < 0) return -1;
  if (ema != nullptr && xhp == nullptr) return -2;
  if ((kind == kAdam || kind == kRMSProp) && s1 == nullptr) return -3;
  switch (kind) {
    case kSGD: return launch_apply<kSGD, true>(w, s0, s1, ema, g, grad_bf16, w_bf16, n, hp, xhp, ctl, stream);
    case kAdam: return launch_apply<kAdam, true>(w, s0, s1, ema, g, grad_bf16, w_bf16, n, hp, xhp, ctl, stream);
    case kAdagrad: return launch_apply<kAdagrad, true>(w, s0, s1, ema, g, grad_bf16, w_bf16, n, hp, xhp, ctl, stream);
    case kRMSProp: return launch_apply<kRMSProp, true>(w, s0, s1, ema, g, grad_bf16, w_bf16, n, hp, xhp, ctl, stream);
    default: return -4;
  }
}

// dst (bf16 or fp32) += src (fp32), n elements: folds an fp32 weight-gradient
// workspace into the flat gradient buffer in one pass (no cast + add pair).
namespace {
template <bool kDstBf16>
__global__ __launch_bounds__(kThreads) void add_f32_kernel(void* __restrict__ dst, const float* __restrict__ src,
                                                           int64_t n) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) {
    if constexpr (kDstBf16) {
      uint16_t* d = static_cast<uint16_t*>(dst) + i;
      *d = f2bf(bf2f(*d) + src[i]);
    } else {
      static_cast<float*>(dst)[i] += src[i];
    }
  }
}
}  // namespace

TONY_API int tony_add_f32(void* dst, int dst_bf16, const float* src, int64_t n, hipStream_t stream) {
  int64_t g = (n + kThreads - 1) / kThreads;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  if (dst_bf16)
    add_f32_kernel<true><<<static_cast<int>(g), kThreads, 0, stream>>>(dst, src, n);
  else
    add_f32_kernel<false><<<static_cast<int>(g), kThreads, 0, stream>>>(dst, src, n);
  TONY_LAUNCH_CHECK();
  return 0;
}
