// Adasum (Horovod's adaptive summation) of two flat gradient buffers, per parameter TENSOR:
//   dot = sum a_i b_i   na = sum a_i^2   nb = sum b_i^2                      (over that tensor alone)
//   ca = 1 - dot / (2 na) if na >= sqrt(DBL_MIN) else 1        cb = 1 - dot / (2 nb) if nb >= sqrt(DBL_MIN) else 1
//   out_i = fl32(fl32(ca a_i) + fl32(cb b_i))                                 (bf16 buffers: rounded once more, RNE)
// The contract and why it is fixed to the bit are in ops/adasum.py; the layout is layerwise.hip's: the host describes
// the buffer as a work list of items (lo, hi, tensor, 0) -- indices of 16-byte vectors (4 fp32 or 8 bf16), at most
// kItemFloats elements each, every item inside ONE tensor's segment and cut from that segment's own start -- and the
// streaming kernels run one workgroup per item, so the tensor of an element is a uniform load, never a search.
//   dots     one (a.b, a.a, b.b) triple of doubles per item, stored: every product is exact in double (24 + 24 and
//            8 + 8 significand bits fit in 53), so only the additions round, and they run in a fixed order (a lane's
//            elements in index order, lanes by butterfly, waves in wave order): no atomics, the same inputs give the
//            same bits
//   coef     coef[t] = (ca, cb): tensor t's triples summed in double (each thread a contiguous run of the tensor's
//            items, the runs in thread order: a function of the tensor's own item count and nothing else), the two
//            ratios formed in double and rounded once to fp32
//   combine  dst = ca a + cb b in place, dst being the a side or the b side; two rounded products and one rounded
//            sum, never a fused multiply-add, so both partners of an exchange compute the same bits
#include "common.h"

using namespace tony;

namespace {

constexpr int kThreads = 256;
constexpr int kItemFloats = 4096;  // elements of the longest item: 4 float4 (2 bf16x8) per thread
constexpr int kFoldThreads = 64;
constexpr double kTiny = 1.4916681462400413e-154;  // sqrt(DBL_MIN): below it a squared norm counts as zero

// One separately rounded operation each (the plain operators under the default contraction mode may meet in one fma).
__device__ __forceinline__ float rn_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float rn_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ double coef_of(double dot, double nn) {
#pragma clang fp contract(off)
  return nn >= kTiny ? 1.0 - dot / (2.0 * nn) : 1.0;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// kN elements of one 16-byte vector as floats (exact for bf16)
template <bool kBf16>
struct Vec;
template <>
struct Vec<false> {
  static constexpr int kN = 4;
  __device__ __forceinline__ static void load(const void* p, int64_t q, float* f) {
    const float4 v = static_cast<const float4*>(p)[q];
    f[0] = v.x, f[1] = v.y, f[2] = v.z, f[3] = v.w;
  }
  __device__ __forceinline__ static void store(void* p, int64_t q, const float* f) {
    static_cast<float4*>(p)[q] = make_float4(f[0], f[1], f[2], f[3]);
  }
};
template <>
struct Vec<true> {
  static constexpr int kN = 8;
  __device__ __forceinline__ static void load(const void* p, int64_t q, float* f) {
    bf16x8 v;
    v.raw = static_cast<const uint4*>(p)[q];
    v.to_float(f);
  }
  __device__ __forceinline__ static void store(void* p, int64_t q, const float* f) {
    static_cast<uint4*>(p)[q] = bf16x8::from_float(f).raw;
  }
};

template <bool kBf16>
__global__ __launch_bounds__(kThreads) void dots_kernel(const void* __restrict__ a, const void* __restrict__ b,
                                                        const int4* __restrict__ items,
                                                        double* __restrict__ partials) {
  constexpr int kN = Vec<kBf16>::kN;
  __shared__ double part[kThreads / kWave][3];
  const int4 it = items[blockIdx.x];
  double sd = 0.0, sa = 0.0, sb = 0.0;
#pragma unroll 4
  for (int64_t q = it.x + threadIdx.x; q < it.y; q += kThreads) {
    float af[kN], bf[kN];
    Vec<kBf16>::load(a, q, af);
    Vec<kBf16>::load(b, q, bf);
#pragma unroll
    for (int k = 0; k < kN; ++k) {
      const double x = static_cast<double>(af[k]), y = static_cast<double>(bf[k]);
      sd = fma(x, y, sd);  // the product is exact: an fma and a product followed by a sum round alike
      sa = fma(x, x, sa);
      sb = fma(y, y, sb);
    }
  }
  sd = wave_sum_d(sd);
  sa = wave_sum_d(sa);
  sb = wave_sum_d(sb);
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  if (lane == 0) {
    part[wid][0] = sd;
    part[wid][1] = sa;
    part[wid][2] = sb;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
    for (int k = 0; k < kThreads / kWave; ++k) {
      t0 += part[k][0];
      t1 += part[k][1];
      t2 += part[k][2];
    }
    double* out = partials + 3 * static_cast<int64_t>(blockIdx.x);
    out[0] = t0;
    out[1] = t1;
    out[2] = t2;
  }
}

// coef[t] from the triples of tensor t's items (order[tstart[t] .. tstart[t+1])); a tensor without an item gets (1, 1).
__global__ __launch_bounds__(kFoldThreads) void coef_kernel(const double* __restrict__ partials,
                                                            const int* __restrict__ order,
                                                            const int* __restrict__ tstart,
                                                            float2* __restrict__ coef) {
  __shared__ double run[kFoldThreads][3];
  const int t = blockIdx.x;
  const int lo = tstart[t], hi = tstart[t + 1];
  const int per = (hi - lo + kFoldThreads - 1) / kFoldThreads;
  const int a = lo + threadIdx.x * per;
  const int b = a + per < hi ? a + per : hi;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int j = a; j < b; ++j) {
    const double* p = partials + 3 * static_cast<int64_t>(order[j]);
    s0 += p[0];
    s1 += p[1];
    s2 += p[2];
  }
  run[threadIdx.x][0] = s0;
  run[threadIdx.x][1] = s1;
  run[threadIdx.x][2] = s2;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double dot = 0.0, na = 0.0, nb = 0.0;
  for (int k = 0; k < kFoldThreads; ++k) {
    dot += run[k][0];
    na += run[k][1];
    nb += run[k][2];
  }
  coef[t] = make_float2(static_cast<float>(coef_of(dot, na)), static_cast<float>(coef_of(dot, nb)));
}

template <bool kBf16, bool kDstIsA>
__global__ __launch_bounds__(kThreads) void combine_kernel(void* __restrict__ dst, const void* __restrict__ other,
                                                           const int4* __restrict__ items,
                                                           const float2* __restrict__ coef) {
  constexpr int kN = Vec<kBf16>::kN;
  const int4 it = items[blockIdx.x];
  const float2 c = coef[it.z];
  const float cd = kDstIsA ? c.x : c.y, co = kDstIsA ? c.y : c.x;  // the coefficients of dst and of the other side
#pragma unroll 4
  for (int64_t q = it.x + threadIdx.x; q < it.y; q += kThreads) {
    float df[kN], of[kN];
    Vec<kBf16>::load(dst, q, df);
    Vec<kBf16>::load(other, q, of);
#pragma unroll
    for (int k = 0; k < kN; ++k) df[k] = rn_add(rn_mul(cd, df[k]), rn_mul(co, of[k]));  // the sum commutes
    Vec<kBf16>::store(dst, q, df);
  }
}

inline bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace

// Elements of the longest work item the kernels are tuned for (the host cuts segments into items of this length).
TONY_API int tony_adasum_item_floats() { return kItemFloats; }

// partials[i] = (a.b, a.a, b.b) of item i as doubles, i in [0, n_items).  a, b: 16-byte aligned fp32 or bf16 buffers.
TONY_API int tony_adasum_dots(const void* a, const void* b, int is_bf16, const void* items, int n_items,
                              double* partials, hipStream_t stream) {
  if (n_items < 0 || a == nullptr || b == nullptr || items == nullptr || partials == nullptr) return -1;
  if (misaligned16(a) || misaligned16(b) || misaligned16(items)) return -2;
  if (n_items == 0) return 0;
  const int4* it = static_cast<const int4*>(items);
  if (is_bf16)
    dots_kernel<true><<<n_items, kThreads, 0, stream>>>(a, b, it, partials);
  else
    dots_kernel<false><<<n_items, kThreads, 0, stream>>>(a, b, it, partials);
  TONY_LAUNCH_CHECK();
  return 0;
}

// coef[T][2] = (ca, cb) as fp32 from the item triples: order[tstart[t] .. tstart[t+1]) are tensor t's items.
TONY_API int tony_adasum_coef(const double* partials, const int* order, const int* tstart, int n_tensors, float* coef,
                              hipStream_t stream) {
  if (n_tensors <= 0 || partials == nullptr || order == nullptr || tstart == nullptr || coef == nullptr) return -1;
  coef_kernel<<<n_tensors, kFoldThreads, 0, stream>>>(partials, order, tstart, reinterpret_cast<float2*>(coef));
  TONY_LAUNCH_CHECK();
  return 0;
}

// dst = ca a + cb b over every item, in place; dst is the a side when dst_is_a, else the b side.
TONY_API int tony_adasum_combine(void* dst, const void* other, int dst_is_a, int is_bf16, const void* items,
                                 int n_items, const float* coef, hipStream_t stream) {
  if (n_items < 0 || dst == nullptr || other == nullptr || items == nullptr || coef == nullptr) return -1;
  if (misaligned16(dst) || misaligned16(other) || misaligned16(items) || (reinterpret_cast<uintptr_t>(coef) & 7))
    return -2;
  if (n_items == 0) return 0;
  const int4* it = static_cast<const int4*>(items);
  const float2* cf = reinterpret_cast<const float2*>(coef);
  if (is_bf16) {
    if (dst_is_a)
      combine_kernel<true, true><<<n_items, kThreads, 0, stream>>>(dst, other, it, cf);
    else
      combine_kernel<true, false><<<n_items, kThreads, 0, stream>>>(dst, other, it, cf);
  } else {
    if (dst_is_a)
      combine_kernel<false, true><<<n_items, kThreads, 0, stream>>>(dst, other, it, cf);
    else
      combine_kernel<false, false><<<n_items, kThreads, 0, stream>>>(dst, other, it, cf);
  }
  TONY_LAUNCH_CHECK();
  return 0;
}
