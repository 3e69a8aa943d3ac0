// The kvstore's fused optimizer updates (parallel/kvstore.py module docstring: nag, adagrad, rmsprop plain and
// centered, ftrl) on fp32 keys, dense and lazy (the touched rows of a row-sparse key), one launch each.  The contract
// is fixed to the bit: every line of the docstring is one rn_* call below, so nothing is contracted into an fma and
// every division and square root is the correctly rounded one (rn_math.h).
//
// One kernel template over the kind and over dense / rows.  Dense: a grid-stride loop over 16-byte chunks, a lane's
// chunk of the gradient, the weight and each state tensor loaded together (3 to 5 independent 16-B loads per lane; at
// the grid cap of 1024 workgroups, four to a CU, that is 48-80 KiB in flight per CU, above the ~32 KiB per CU a
// streaming kernel needs to cover HBM latency, so a lane keeps one chunk in flight and the registers stay low), and a
// scalar tail for n % 4 elements.  Rows: the thread map of kv_rsp_sgd_kernel (ps_plane.hip) -- a wave handles one
// pass (64 chunks) of one row, four waves per workgroup, at most 1024 workgroups; ids strictly increasing, so no row
// is written by two waves; an id outside [0, R) is skipped.  No atomics, no LDS, plain vector loads and stores.
#include <algorithm>
#include <cstdint>

#include "common.h"
#include "rn_math.h"

using namespace tony;

namespace {

// the kinds of the C entry points, and nag at momentum 0 (no state: lazy SGD's momentum == 0 lines)
enum : int { kNag = 0, kAdagrad = 1, kRmsprop = 2, kRmspropCentered = 3, kFtrl = 4, kKinds = 5, kNagPlain = 5 };

struct KvOptHp {
  float lr, wd, rescale, clip, momentum, eps, gamma1, omg1, gamma2, lamda1, beta;  // omg1 = fl32(1 - gamma1)
  int has_clip;
};

constexpr int states_of(int kind) {
  return kind == kNagPlain ? 0 : kind == kRmspropCentered ? 3 : kind == kFtrl ? 2 : 1;
}

// state: mom (none when MOM is false)
template <bool MOM>
__device__ __forceinline__ void nag1(float& w, float& m, float g2, const KvOptHp& hp) {
  const float p = rn_mul(hp.wd, w);
  const float g3 = rn_add(g2, p);
  if constexpr (MOM) {
    m = rn_mul(hp.momentum, m);
    m = rn_add(m, g3);
    const float q = rn_mul(hp.momentum, m);
    const float g4 = rn_add(g3, q);
    const float s = rn_mul(hp.lr, g4);
    w = rn_sub(w, s);
  } else {
    const float s = rn_mul(hp.lr, g3);
    w = rn_sub(w, s);
  }
}

// state: history
__device__ __forceinline__ void adagrad1(float& w, float& h, float g2, const KvOptHp& hp) {
  const float q = rn_mul(g2, g2);
  h = rn_add(h, q);
  const float e = rn_add(h, hp.eps);
  const float r = rn_sqrt(e);
  const float d = rn_div(g2, r);
  const float p = rn_mul(hp.wd, w);
  const float u = rn_add(d, p);
  const float s = rn_mul(hp.lr, u);
  w = rn_sub(w, s);
}

// states: n, and when CENTERED g (gb) and delta
template <bool CENTERED>
__device__ __forceinline__ void rmsprop1(float& w, float& n, float& gb, float& delta, float g2, const KvOptHp& hp) {
  const float p = rn_mul(hp.wd, w);
  const float g3 = rn_add(g2, p);
  const float q = rn_mul(g3, g3);
  const float a = rn_mul(hp.omg1, q);
  const float b = rn_mul(hp.gamma1, n);
  n = rn_add(a, b);
  if constexpr (CENTERED) {
    const float c = rn_mul(hp.omg1, g3);
    const float b2 = rn_mul(hp.gamma1, gb);
    gb = rn_add(c, b2);
    const float gg = rn_mul(gb, gb);
    const float e1 = rn_sub(n, gg);
    const float e = rn_add(e1, hp.eps);
    const float r = rn_sqrt(e);
    const float d = rn_div(g3, r);
    const float s = rn_mul(hp.lr, d);
    const float dl = rn_mul(hp.gamma2, delta);
    delta = rn_sub(dl, s);
    w = rn_add(w, delta);
  } else {
    const float e = rn_add(n, hp.eps);
    const float r = rn_sqrt(e);
    const float d = rn_div(g3, r);
    const float s = rn_mul(hp.lr, d);
    w = rn_sub(w, s);
  }
}

// states: z, n; wd enters only the denominator
__device__ __forceinline__ void ftrl1(float& w, float& z, float& n, float g2, const KvOptHp& hp) {
  const float q = rn_mul(g2, g2);
  const float n1 = rn_add(n, q);
  const float r1 = rn_sqrt(n1);
  const float r0 = rn_sqrt(n);
  const float dr = rn_sub(r1, r0);
  const float sg = rn_div(dr, hp.lr);
  const float t = rn_mul(sg, w);
  const float z1 = rn_add(z, g2);
  z = rn_sub(z1, t);
  n = n1;
  if (fabsf(z) <= hp.lamda1) {  // (a NaN z compares false: the division carries it on)
    w = 0.f;
  } else {
    const float num = rn_sub(copysignf(hp.lamda1, z), z);
    const float b1 = rn_add(hp.beta, r1);
    const float d0 = rn_div(b1, hp.lr);
    const float den = rn_add(d0, hp.wd);
    w = rn_div(num, den);
  }
}

// one element: the rescale and the clip common to every kind, then the kind's lines
template <int KIND>
__device__ __forceinline__ void opt1(float& w, float& s0, float& s1, float& s2, float g, const KvOptHp& hp) {
  const float g1 = rn_mul(g, hp.rescale);
  const float g2 = hp.has_clip ? (g1 > hp.clip ? hp.clip : (g1 < -hp.clip ? -hp.clip : g1)) : g1;  // a NaN stays
  if constexpr (KIND == kNag) nag1<true>(w, s0, g2, hp);
  if constexpr (KIND == kNagPlain) nag1<false>(w, s0, g2, hp);
  if constexpr (KIND == kAdagrad) adagrad1(w, s0, g2, hp);
  if constexpr (KIND == kRmsprop) rmsprop1<false>(w, s0, s1, s2, g2, hp);
  if constexpr (KIND == kRmspropCentered) rmsprop1<true>(w, s0, s1, s2, g2, hp);
  if constexpr (KIND == kFtrl) ftrl1(w, s0, s1, g2, hp);
}

// chunk `at` of the weight and of the kind's state tensors from the gradient chunk g
template <int KIND>
__device__ __forceinline__ void opt_chunk(float4* __restrict__ W, float4* __restrict__ S0, float4* __restrict__ S1,
                                          float4* __restrict__ S2, int64_t at, const float4 g, const KvOptHp& hp) {
  constexpr int NS = states_of(KIND);
  float4 w = W[at];
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a, c = a;
  if constexpr (NS >= 1) a = S0[at];
  if constexpr (NS >= 2) b = S1[at];
  if constexpr (NS >= 3) c = S2[at];
  opt1<KIND>(w.x, a.x, b.x, c.x, g.x, hp);
  opt1<KIND>(w.y, a.y, b.y, c.y, g.y, hp);
  opt1<KIND>(w.z, a.z, b.z, c.z, g.z, hp);
  opt1<KIND>(w.w, a.w, b.w, c.w, g.w, hp);
  W[at] = w;
  if constexpr (NS >= 1) S0[at] = a;
  if constexpr (NS >= 2) S1[at] = b;
  if constexpr (NS >= 3) S2[at] = c;
}

// ROWS false: n elements of w (and states) from the dense gradient g.  ROWS true: rows ids[0, n) of w [R, 4 rc]
// (and states) from the compact gradient rows g [n, 4 rc].
template <int KIND, bool ROWS>
__global__ __launch_bounds__(256) void kv_opt_kernel(float* __restrict__ w, float* __restrict__ s0,
                                                     float* __restrict__ s1, float* __restrict__ s2,
                                                     const float* __restrict__ g, const int64_t* __restrict__ ids,
                                                     int64_t n, int64_t rc, int64_t R, KvOptHp hp) {
  float4* W = reinterpret_cast<float4*>(w);
  float4* S0 = reinterpret_cast<float4*>(s0);
  float4* S1 = reinterpret_cast<float4*>(s1);
  float4* S2 = reinterpret_cast<float4*>(s2);
  const float4* G = reinterpret_cast<const float4*>(g);
  if constexpr (ROWS) {
    const int lane = threadIdx.x & 63;
    const int64_t passes = (rc + 63) >> 6, items = n * passes;
    const int64_t first =
        static_cast<int64_t>(blockIdx.x) * 4 + __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    for (int64_t it = first; it < items; it += static_cast<int64_t>(gridDim.x) * 4) {
      const int64_t i = passes == 1 ? it : it / passes;
      const int64_t c = (it - i * passes) * 64 + lane;
      const int64_t id = ids[i];
      if (static_cast<uint64_t>(id) >= static_cast<uint64_t>(R) || c >= rc) continue;
      opt_chunk<KIND>(W, S0, S1, S2, id * rc + c, G[i * rc + c], hp);
    }
  } else {
    constexpr int NS = states_of(KIND);
    const int64_t n4 = n >> 2;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n4;
         i += static_cast<int64_t>(gridDim.x) * 256)
      opt_chunk<KIND>(W, S0, S1, S2, i, G[i], hp);
    if (blockIdx.x == 0 && static_cast<int64_t>(threadIdx.x) < (n & 3)) {  // the n % 4 elements past the chunks
      const int64_t i = (n4 << 2) + threadIdx.x;
      float x = w[i], a = 0.f, b = 0.f, c = 0.f;
      if constexpr (NS >= 1) a = s0[i];
      if constexpr (NS >= 2) b = s1[i];
      if constexpr (NS >= 3) c = s2[i];
      opt1<KIND>(x, a, b, c, g[i], hp);
      w[i] = x;
      if constexpr (NS >= 1) s0[i] = a;
      if constexpr (NS >= 2) s1[i] = b;
      if constexpr (NS >= 3) s2[i] = c;
    }
  }
}

inline bool misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

// the internal kind of a request, or -1: a kind out of range, a state pointer the kind does not take, a missing or
// misaligned one (nag takes mom exactly when momentum != 0, as tony_kv_rsp_sgd does)
int checked_kind(int kind, const float* s0, const float* s1, const float* s2, float momentum) {
  if (kind < 0 || kind >= kKinds) return -1;
  if (kind == kNag && momentum == 0.f) kind = kNagPlain;
  const int ns = states_of(kind);
  const float* s[3] = {s0, s1, s2};
  for (int k = 0; k < 3; ++k)
    if ((s[k] != nullptr) != (k < ns) || misaligned(s[k], 15)) return -1;
  return kind;
}

template <bool ROWS>
void launch(int kind, int blocks, hipStream_t stream, float* w, float* s0, float* s1, float* s2, const float* g,
            const int64_t* ids, int64_t n, int64_t rc, int64_t R, const KvOptHp& hp) {
#define TONY_KV_OPT_CASE(K) \
  case K:                   \
    kv_opt_kernel<K, ROWS><<<blocks, 256, 0, stream>>>(w, s0, s1, s2, g, ids, n, rc, R, hp); \
    break;
  switch (kind) {
    TONY_KV_OPT_CASE(kNag)
    TONY_KV_OPT_CASE(kAdagrad)
    TONY_KV_OPT_CASE(kRmsprop)
    TONY_KV_OPT_CASE(kRmspropCentered)
    TONY_KV_OPT_CASE(kFtrl)
    TONY_KV_OPT_CASE(kNagPlain)
  }
#undef TONY_KV_OPT_CASE
}

}  // namespace

// One update of the n fp32 elements of w, and of the kind's state tensors, from the gradient g, in one launch.
// kind: 0 nag (s0 = mom, null when momentum is 0), 1 adagrad (s0 = history), 2 rmsprop (s0 = n), 3 centered rmsprop
// (s0 = n, s1 = g, s2 = delta), 4 ftrl (s0 = z, s1 = n); the state pointers a kind does not take are null.  clip is
// read only when has_clip; one_minus_gamma1 is the host's fl32(1 - gamma1).  Every pointer 16-B aligned.
TONY_API int tony_kv_opt_dense(int kind, float* w, float* s0, float* s1, float* s2, const float* g, int64_t n,
                               float lr, float wd, float rescale, int has_clip, float clip, float momentum, float eps,
                               float gamma1, float one_minus_gamma1, float gamma2, float lamda1, float beta,
                               hipStream_t stream) {
  const int k = checked_kind(kind, s0, s1, s2, momentum);
  if (k < 0 || w == nullptr || g == nullptr || n < 0 || misaligned(w, 15) || misaligned(g, 15)) return -1;
  if (n == 0) return 0;
  const KvOptHp hp{lr, wd, rescale, clip, momentum, eps, gamma1, one_minus_gamma1, gamma2, lamda1, beta, has_clip};
  const int64_t n4 = (n >> 2) + 1;
  const int blocks = static_cast<int>(std::min<int64_t>(1024, (n4 + 255) / 256));
  launch<false>(k, blocks, stream, w, s0, s1, s2, g, nullptr, n, 0, 0, hp);
  TONY_LAUNCH_CHECK();
  return 0;
}

// The same update on rows ids[0, nnz) (strictly increasing; an id outside [0, R) is skipped) of w [R, row_elems]
// and of the kind's state tensors, from the compact gradient rows [nnz, row_elems]; row_elems a multiple of 4.
TONY_API int tony_kv_opt_rows(int kind, float* w, float* s0, float* s1, float* s2, const int64_t* ids,
                              const float* rows, int64_t nnz, int64_t row_elems, int64_t R, float lr, float wd,
                              float rescale, int has_clip, float clip, float momentum, float eps, float gamma1,
                              float one_minus_gamma1, float gamma2, float lamda1, float beta, hipStream_t stream) {
  const int k = checked_kind(kind, s0, s1, s2, momentum);
  if (k < 0 || w == nullptr || ids == nullptr || rows == nullptr || nnz < 0 || row_elems <= 0 || (row_elems & 3) ||
      R <= 0 || misaligned(w, 15) || misaligned(rows, 15) || misaligned(ids, 7))
    return -1;
  if (nnz == 0) return 0;
  const KvOptHp hp{lr, wd, rescale, clip, momentum, eps, gamma1, one_minus_gamma1, gamma2, lamda1, beta, has_clip};
  const int64_t rc = row_elems >> 2;
  const int64_t items = nnz * ((rc + 63) >> 6);
  const int blocks = static_cast<int>(std::min<int64_t>(1024, (items + 3) / 4));
  launch<true>(k, blocks, stream, w, s0, s1, s2, rows, ids, nnz, rc, R, hp);
  TONY_LAUNCH_CHECK();
  return 0;
}
