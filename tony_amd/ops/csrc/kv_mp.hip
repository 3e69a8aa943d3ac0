// Multi-precision kvstore keys (parallel/kvstore.py module docstring): a bf16 or fp16 stored value over an fp32 master
// w32 and fp32 optimizer states.  One launch does a key's whole round: the ordered fp32 sum of up to 8 pushed sources
// (each fp32, fp16 or bf16, read in place and widened exactly), the kind's update lines on the master (kv_update.h;
// lazy SGD with momentum is one more kind here), and the stored value as the master rounded to nearest even.
//
// One kernel template over the kind, the key's 16-bit type and dense / rows.  A lane owns 8 consecutive elements per
// turn: one 16-byte load per 16-bit source and two per fp32 source, all issued before the first is used (the source
// table is a by-value kernel argument indexed by unrolled constants, so it stays in scalar registers), two 16-byte
// loads each for the master and every state, the same stores and one 16-byte store of the 16-bit value.  With one
// bf16 source and one state that is 80 B in flight per lane, 80 KiB per CU at the grid cap of 1024 workgroups (four
// to a CU), above the ~32 KiB a streaming kernel needs to cover HBM latency; eight fp32 sources hold 64 registers of
// raw loads, which still fits four workgroups to a CU.  Dense: a grid-stride loop over the chunks of 8, and the
// n % 8 elements past them one by one in a single lane.  Rows: the thread map of kv_opt_kernel (kv_optim.hip) -- a
// wave handles one pass (64 chunks) of one row of the sorted ids, an id outside [0, R) is skipped -- on the master,
// the states and the 16-bit table from one compact gradient.  No atomics, no LDS, plain vector loads and stores.
#include <algorithm>
#include <cstdint>

#include "common.h"
#include "kv_update.h"

using namespace tony;

namespace {

constexpr int kSgdMom = 6;  // lazy SGD with momentum (state mom); at momentum 0 its lines are kNagPlain's
constexpr int kMaxSrc = 8;
enum : int { kF32 = 0, kF16 = 1, kBF16 = 2 };  // a source's element type (the codes of parallel/kvstore.py _DTYPES)

constexpr int mp_states_of(int kind) { return kind == kSgdMom ? 1 : states_of(kind); }

struct MpSrcs {
  const void* p[kMaxSrc];
  int code[kMaxSrc];
  int n;
};

template <int KIND>
__device__ __forceinline__ void mp1(float& w, float& s0, float& s1, float& s2, float g, const KvOptHp& hp) {
  if constexpr (KIND == kSgdMom) {
    const float g2 = grad2(g, hp);
    const float p = rn_mul(hp.wd, w);
    const float g3 = rn_add(g2, p);
    s0 = rn_mul(hp.momentum, s0);
    const float s = rn_mul(hp.lr, g3);
    s0 = rn_sub(s0, s);
    w = rn_add(w, s0);
  } else {
    opt1<KIND>(w, s0, s1, s2, g, hp);
  }
}

// exact widening of a 16-bit element (fp16 subnormals included)
__device__ __forceinline__ float widen16(uint32_t bits, int code) {
  return code == kBF16 ? __uint_as_float(bits << 16)
                       : static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(bits)));
}

// round to nearest even to the key's type: v_cvt_f16_f32 (subnormals, overflow to inf) or v_cvt_pk_bf16_f32; both
// keep a NaN a NaN
template <bool FP16>
__device__ __forceinline__ uint32_t rne16(float f) {
  if constexpr (FP16) return __builtin_bit_cast(uint16_t, static_cast<_Float16>(f));
  return f2bf(f);
}

// 8 consecutive elements of a source as loaded: 16 B of a 16-bit source (hi unused), 32 B of an fp32 one
struct Raw8 {
  uint4 lo, hi;
};

__device__ __forceinline__ Raw8 load_raw(const void* p, int code, int64_t chunk) {
  Raw8 r;
  if (code == kF32) {
    const uint4* q = static_cast<const uint4*>(p) + 2 * chunk;
    r.lo = q[0];
    r.hi = q[1];
  } else {
    r.lo = static_cast<const uint4*>(p)[chunk];
    r.hi = r.lo;
  }
  return r;
}

__device__ __forceinline__ void widen_raw(const Raw8& r, int code, float* f) {
  const uint32_t lo[4] = {r.lo.x, r.lo.y, r.lo.z, r.lo.w};
  if (code == kF32) {
    const uint32_t hi[4] = {r.hi.x, r.hi.y, r.hi.z, r.hi.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) f[i] = __uint_as_float(lo[i]), f[4 + i] = __uint_as_float(hi[i]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) f[2 * i] = widen16(lo[i] & 0xffffu, code), f[2 * i + 1] = widen16(lo[i] >> 16, code);
  }
}

__device__ __forceinline__ float load_elem(const void* p, int code, int64_t i) {
  return code == kF32 ? static_cast<const float*>(p)[i] : widen16(static_cast<const uint16_t*>(p)[i], code);
}

// chunk `at` (8 elements) of the master, the states and the 16-bit value from chunk `gat` of the first NSRC-capped
// sources: every load issued, then g = widen(s_0); g = g + widen(s_i) in order, the kind's lines, the stores
template <int KIND, bool FP16, int NSRC>
__device__ __forceinline__ void mp_chunk(uint16_t* __restrict__ w16, float* __restrict__ w32, float* __restrict__ s0,
                                         float* __restrict__ s1, float* __restrict__ s2, int64_t at, const MpSrcs& src,
                                         int64_t gat, const KvOptHp& hp) {
  constexpr int NS = mp_states_of(KIND);
  Raw8 raw[NSRC];
#pragma unroll
  for (int s = 0; s < NSRC; ++s)
    if (s < src.n) raw[s] = load_raw(src.p[s], src.code[s], gat);
  float w[8], a[8] = {}, b[8] = {}, c[8] = {};
  V8<float>::load(w32 + 8 * at).to_float(w);
  if constexpr (NS >= 1) V8<float>::load(s0 + 8 * at).to_float(a);
  if constexpr (NS >= 2) V8<float>::load(s1 + 8 * at).to_float(b);
  if constexpr (NS >= 3) V8<float>::load(s2 + 8 * at).to_float(c);
  float g[8];
  widen_raw(raw[0], src.code[0], g);
#pragma unroll
  for (int s = 1; s < NSRC; ++s)
    if (s < src.n) {
      float t[8];
      widen_raw(raw[s], src.code[s], t);
#pragma unroll
      for (int j = 0; j < 8; ++j) g[j] = rn_add(g[j], t[j]);
    }
  uint32_t h[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    mp1<KIND>(w[j], a[j], b[j], c[j], g[j], hp);
    h[j] = rne16<FP16>(w[j]);
  }
  V8<float>::from_float(w).store(w32 + 8 * at);
  if constexpr (NS >= 1) V8<float>::from_float(a).store(s0 + 8 * at);
  if constexpr (NS >= 2) V8<float>::from_float(b).store(s1 + 8 * at);
  if constexpr (NS >= 3) V8<float>::from_float(c).store(s2 + 8 * at);
  reinterpret_cast<uint4*>(w16)[at] =
      make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
}

// ROWS false: the n elements of the key from src.n sources of n elements.  ROWS true: rows ids[0, n) of the key
// [R, 8 rc] from the compact gradient rows src.p[0] [n, 8 rc].
template <int KIND, bool FP16, bool ROWS>
__global__ __launch_bounds__(256) void kv_mp_kernel(uint16_t* __restrict__ w16, float* __restrict__ w32,
                                                    float* __restrict__ s0, float* __restrict__ s1,
                                                    float* __restrict__ s2, const MpSrcs src,
                                                    const int64_t* __restrict__ ids, int64_t n, int64_t rc, int64_t R,
                                                    KvOptHp hp) {
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
      mp_chunk<KIND, FP16, 1>(w16, w32, s0, s1, s2, id * rc + c, src, i * rc + c, hp);
    }
  } else {
    constexpr int NS = mp_states_of(KIND);
    const int64_t n8 = n >> 3;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n8;
         i += static_cast<int64_t>(gridDim.x) * 256)
      mp_chunk<KIND, FP16, kMaxSrc>(w16, w32, s0, s1, s2, i, src, i, hp);
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // the n % 8 elements past the chunks, one by one
      for (int64_t i = n8 << 3; i < n; ++i) {
        float g = load_elem(src.p[0], src.code[0], i);
#pragma unroll
        for (int s = 1; s < kMaxSrc; ++s)
          if (s < src.n) g = rn_add(g, load_elem(src.p[s], src.code[s], i));
        float x = w32[i], a = 0.f, b = 0.f, c = 0.f;
        if constexpr (NS >= 1) a = s0[i];
        if constexpr (NS >= 2) b = s1[i];
        if constexpr (NS >= 3) c = s2[i];
        mp1<KIND>(x, a, b, c, g, hp);
        w32[i] = x;
        if constexpr (NS >= 1) s0[i] = a;
        if constexpr (NS >= 2) s1[i] = b;
        if constexpr (NS >= 3) s2[i] = c;
        w16[i] = static_cast<uint16_t>(rne16<FP16>(x));
      }
    }
  }
}

inline bool misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

// the internal kind of a request, or -1: a kind out of range, a state pointer the kind does not take, a missing or
// misaligned one (nag and sgd take mom exactly when momentum != 0)
int checked_kind(int kind, const float* s0, const float* s1, const float* s2, float momentum) {
  if ((kind < 0 || kind >= kKinds) && kind != kSgdMom) return -1;
  if ((kind == kNag || kind == kSgdMom) && momentum == 0.f) kind = kNagPlain;
  const int ns = mp_states_of(kind);
  const float* s[3] = {s0, s1, s2};
  for (int k = 0; k < 3; ++k)
    if ((s[k] != nullptr) != (k < ns) || misaligned(s[k], 15)) return -1;
  return kind;
}

template <bool ROWS>
void launch(int kind, int fp16, int blocks, hipStream_t stream, uint16_t* w16, float* w32, float* s0, float* s1,
            float* s2, const MpSrcs& src, const int64_t* ids, int64_t n, int64_t rc, int64_t R, const KvOptHp& hp) {
#define TONY_KV_MP_CASE(K)                                                                                      \
  case K:                                                                                                       \
    if (fp16)                                                                                                   \
      kv_mp_kernel<K, true, ROWS><<<blocks, 256, 0, stream>>>(w16, w32, s0, s1, s2, src, ids, n, rc, R, hp);    \
    else                                                                                                        \
      kv_mp_kernel<K, false, ROWS><<<blocks, 256, 0, stream>>>(w16, w32, s0, s1, s2, src, ids, n, rc, R, hp);   \
    break;
  switch (kind) {
    TONY_KV_MP_CASE(kNag)
    TONY_KV_MP_CASE(kAdagrad)
    TONY_KV_MP_CASE(kRmsprop)
    TONY_KV_MP_CASE(kRmspropCentered)
    TONY_KV_MP_CASE(kFtrl)
    TONY_KV_MP_CASE(kNagPlain)
    TONY_KV_MP_CASE(kSgdMom)
  }
#undef TONY_KV_MP_CASE
}

}  // namespace

// One update of the n elements of a multi-precision key in one launch: g = the ordered fp32 sum of the nsrc (1 to 8)
// sources (srcs[i] the address of n elements of type codes[i]: 0 fp32, 1 fp16, 2 bf16), the kind's lines on the fp32
// master w32 and the kind's fp32 states, and w16 = the master rounded to nearest even to fp16 (is_fp16) or bf16.
// kind and the state pointers as tony_kv_opt_dense's, and kind 6: lazy SGD (s0 = mom, null when momentum is 0).
// Every pointer 16-B aligned.
TONY_API int tony_kv_mp_dense(int kind, int is_fp16, void* w16, float* w32, float* s0, float* s1, float* s2,
                              const int64_t* srcs, const int64_t* codes, int nsrc, int64_t n, float lr, float wd,
                              float rescale, int has_clip, float clip, float momentum, float eps, float gamma1,
                              float one_minus_gamma1, float gamma2, float lamda1, float beta, hipStream_t stream) {
  const int k = checked_kind(kind, s0, s1, s2, momentum);
  if (k < 0 || w16 == nullptr || w32 == nullptr || srcs == nullptr || codes == nullptr || nsrc < 1 ||
      nsrc > kMaxSrc || n < 0 || misaligned(w16, 15) || misaligned(w32, 15))
    return -1;
  MpSrcs src{};
  src.n = nsrc;
  for (int i = 0; i < nsrc; ++i) {
    src.p[i] = reinterpret_cast<const void*>(static_cast<uintptr_t>(srcs[i]));
    src.code[i] = static_cast<int>(codes[i]);
    if (src.p[i] == nullptr || misaligned(src.p[i], 15) || codes[i] < kF32 || codes[i] > kBF16) return -1;
  }
  if (n == 0) return 0;
  const KvOptHp hp{lr, wd, rescale, clip, momentum, eps, gamma1, one_minus_gamma1, gamma2, lamda1, beta, has_clip};
  const int64_t chunks = (n >> 3) + 1;
  const int blocks = static_cast<int>(std::min<int64_t>(1024, (chunks + 255) / 256));
  launch<false>(k, is_fp16, blocks, stream, static_cast<uint16_t*>(w16), w32, s0, s1, s2, src, nullptr, n, 0, 0, hp);
  TONY_LAUNCH_CHECK();
  return 0;
}

// The same update on rows ids[0, nnz) (strictly increasing; an id outside [0, R) is skipped) of a multi-precision key
// [R, row_elems] -- master, states and 16-bit table -- from the compact gradient rows [nnz, row_elems] of type
// rows_code; row_elems a multiple of 8.
TONY_API int tony_kv_mp_rows(int kind, int is_fp16, void* w16, float* w32, float* s0, float* s1, float* s2,
                             const int64_t* ids, const void* rows, int rows_code, int64_t nnz, int64_t row_elems,
                             int64_t R, float lr, float wd, float rescale, int has_clip, float clip, float momentum,
                             float eps, float gamma1, float one_minus_gamma1, float gamma2, float lamda1, float beta,
                             hipStream_t stream) {
  const int k = checked_kind(kind, s0, s1, s2, momentum);
  if (k < 0 || w16 == nullptr || w32 == nullptr || ids == nullptr || rows == nullptr || rows_code < kF32 ||
      rows_code > kBF16 || nnz < 0 || row_elems <= 0 || (row_elems & 7) || R <= 0 || misaligned(w16, 15) ||
      misaligned(w32, 15) || misaligned(rows, 15) || misaligned(ids, 7))
    return -1;
  if (nnz == 0) return 0;
  const KvOptHp hp{lr, wd, rescale, clip, momentum, eps, gamma1, one_minus_gamma1, gamma2, lamda1, beta, has_clip};
  MpSrcs src{};
  src.n = 1;
  src.p[0] = rows;
  src.code[0] = rows_code;
  const int64_t rc = row_elems >> 3;
  const int64_t items = nnz * ((rc + 63) >> 6);
  const int blocks = static_cast<int>(std::min<int64_t>(1024, (items + 3) / 4));
  launch<true>(k, is_fp16, blocks, stream, static_cast<uint16_t*>(w16), w32, s0, s1, s2, src, ids, nnz, rc, R, hp);
  TONY_LAUNCH_CHECK();
  return 0;
}
