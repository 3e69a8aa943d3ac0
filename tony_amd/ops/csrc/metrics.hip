// Top-k evaluation counters with tf.math.in_top_k's semantics: a row is a top-k hit iff its target logit is
// finite and fewer than k classes have a STRICTLY greater logit, so ties that straddle the boundary all count.
// One wave per row; per row counters += [hit@1, hit@k, 1] with integer atomics (exact, hence deterministic).
// Nothing is read back: the job reads the three counters once at the end.
#include "common.h"

using namespace tony;

namespace {

constexpr int kThreads = 256;
constexpr int kRowsPerBlock = kThreads / kWave;

template <bool kBf16>
__device__ __forceinline__ float ldl(const void* p, int64_t i) {
  if constexpr (kBf16) return bf2f(static_cast<const uint16_t*>(p)[i]);
  return static_cast<const float*>(p)[i];
}

template <bool kBf16>
__global__ __launch_bounds__(kThreads) void topk_count_kernel(const void* __restrict__ logits, int64_t rows,
                                                              int classes, int64_t ld_,
                                                              const int64_t* __restrict__ targets, int k,
                                                              unsigned long long* __restrict__ counters) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t row = static_cast<int64_t>(blockIdx.x) * kRowsPerBlock + threadIdx.x / kWave;
  if (row >= rows) return;  // (whole waves leave: no lane of a live wave is missing from the shuffles)
  const int64_t t = targets[row];
  const bool in_range = t >= 0 && t < classes;
  const float xt = in_range ? ldl<kBf16>(logits, row * ld_ + t) : NAN;
  int greater = 0;
  for (int c = lane; c < classes; c += kWave) greater += ldl<kBf16>(logits, row * ld_ + c) > xt ? 1 : 0;
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) greater += __shfl_xor(greater, o, kWave);
  if (lane == 0) {
    const bool finite = in_range && fabsf(xt) < INFINITY;  // false for NaN and for +-inf
    if (finite && greater < 1) atomicAdd(counters + 0, 1ull);
    if (finite && greater < k) atomicAdd(counters + 1, 1ull);
    atomicAdd(counters + 2, 1ull);
  }
}

}  // namespace

TONY_API int tony_topk_count(const void* logits, int is_bf16, int64_t rows, int classes, int64_t ld_,
                             const int64_t* targets, int k, int64_t* counters, hipStream_t stream) {
  if (!logits || !targets || !counters || rows < 0 || classes <= 0 || ld_ < classes || k < 1) return -1;
  if (rows == 0) return 0;
  if (rows > (int64_t{1} << 30)) return -2;
  const int blocks = ceil_div(rows, kRowsPerBlock);
  auto* cnt = reinterpret_cast<unsigned long long*>(counters);
  if (is_bf16)
    topk_count_kernel<true><<<blocks, kThreads, 0, stream>>>(logits, rows, classes, ld_, targets, k, cnt);
  else
    topk_count_kernel<false><<<blocks, kThreads, 0, stream>>>(logits, rows, classes, ld_, targets, k, cnt);
  TONY_LAUNCH_CHECK();
  return 0;
}
