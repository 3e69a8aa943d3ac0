// The worker side of the kvstore's row-sparse path (parallel/kvstore.py module docstring, "CSR x row-sparse dot"):
// tony_kv_csr_dot, out[b] = the ordered sum over sample b's CSR entries of value * w_row[column], and
// tony_kv_rows_segsum, out[u] = the ordered sum over a segment of entry numbers of value * rows[source row] -- the
// transposed dot (a row-sparse gradient) and RowSparse.from_rows.  The contract is fixed to the bit: every product and
// every add is one rn_* call (rn_math.h), the adds of one output row run left to right in entry order, no atomics.
//
// Work split.  A lane owns one 16-byte chunk of an output row, and a lane group of G lanes owns one output row: G is
// the power of two at or above the row's chunks, at most 64 (a 64-B row: 4 lanes, 16 rows per wave, so a short row
// does not leave most of a wave idle); a row of more than 64 chunks is walked in passes of a whole wave.  The unit of
// work is (output row, pass), group after group in a grid-stride loop.
//
// Data movement, per turn of up to G entries of the row.  Every lane of the group takes ONE entry: it loads the
// entry's number, column / source row and value and, for a row-sparse w, binary-searches the column in w's sorted ids
// (up to 64 searches in flight per wave, as kv_rsp_merge_kernel searches), and keeps the descriptor (position or -1,
// value) in registers.  The group then walks the turn's descriptors in order: kDepth at a time are broadcast with a
// cross-lane shuffle and their row chunks loaded together (kDepth 16-byte loads in flight per lane before the first
// add), then added strictly in entry order.  Nothing per entry goes to memory or to LDS.  The adds of one output row
// are a dependent chain by contract: a long segment is bound by the add latency with its loads hidden behind it.
//
// Every loop a shuffle sits in has a wave-uniform trip count (__any over the groups' own counts): all 64 lanes
// execute every shuffle, a group that is done merely predicates its loads and adds off.  Every index read from memory
// is range checked before it is used as an address; an entry that fails contributes nothing.
#include <algorithm>
#include <climits>
#include <cstdint>

#include "common.h"
#include "rn_math.h"

using namespace tony;

namespace {

constexpr int kDepth = 8;  // row chunks in flight per lane before the first ordered add

__device__ __forceinline__ float4 mul4(float v, const float4 r) {
  return make_float4(rn_mul(v, r.x), rn_mul(v, r.y), rn_mul(v, r.z), rn_mul(v, r.w));
}
__device__ __forceinline__ float4 add4(const float4 a, const float4 b) {
  return make_float4(rn_add(a.x, b.x), rn_add(a.y, b.y), rn_add(a.z, b.z), rn_add(a.w, b.w));
}

// where this lane stands: its group (G lanes from lane `base`), its place in it, and the wave's first unit
struct Lanes {
  int G, logG, lig, base, grp;
  int64_t wave, waves;
  __device__ __forceinline__ Lanes(int logG_) : logG(logG_) {
    const int lane = threadIdx.x & 63;
    G = 1 << logG;
    lig = lane & (G - 1);
    base = lane - lig;
    grp = lane >> logG;
    wave = static_cast<int64_t>(blockIdx.x) * 4 + __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    waves = static_cast<int64_t>(gridDim.x) * 4;
  }
};

// One turn: the group's cnt descriptors (pos, val), one per lane from lane `base` on, applied in order to this lane's
// chunk c of rows [*, rc].  acc / have carry the row's running sum across turns (have: a first term was taken).
template <bool DATA>
__device__ __forceinline__ void ordered_turn(const float4* __restrict__ rows, int64_t rc, int64_t c, bool has_chunk,
                                             int pos, float val, int cnt, const Lanes& L, float4& acc, bool& have) {
  for (int j0 = 0; __any(j0 < cnt); j0 += kDepth) {
    float4 r[kDepth];
    float v[kDepth];
    bool ok[kDepth];
#pragma unroll
    for (int k = 0; k < kDepth; ++k) {
      const int j = j0 + k;
      ok[k] = false;
      v[k] = 1.f;
      r[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (j >= L.G) continue;  // (wave-uniform: a group narrower than kDepth)
      const int p = __shfl(pos, L.base + j);
      if constexpr (DATA) v[k] = __shfl(val, L.base + j);
      ok[k] = has_chunk && j < cnt && p >= 0;
      if (ok[k]) r[k] = rows[static_cast<int64_t>(p) * rc + c];
    }
#pragma unroll
    for (int k = 0; k < kDepth; ++k) {
      if (!ok[k]) continue;
      const float4 t = DATA ? mul4(v[k], r[k]) : r[k];
      acc = have ? add4(acc, t) : t;
      have = true;
    }
  }
}

// out[b] (B rows of rc chunks) from the CSR (indptr [B + 1], indices / data [E]) and w: wrows [wn, rc], its rows
// named by the sorted wids [wn] or, DENSE, row r being column r.  DATA false: every stored value is 1, no multiply.
template <bool DATA, bool DENSE>
__global__ __launch_bounds__(256) void kv_csr_dot_kernel(const int64_t* __restrict__ indptr,
                                                         const int64_t* __restrict__ indices,
                                                         const float* __restrict__ data,
                                                         const int64_t* __restrict__ wids, int64_t wn,
                                                         const float4* __restrict__ wrows, float4* __restrict__ out,
                                                         int64_t B, int64_t E, int64_t rc, int logG) {
  const Lanes L(logG);
  const int64_t passes = (rc + 63) >> 6, units = B * passes;
  const int gpw = 64 >> logG;
  for (int64_t u0 = L.wave * gpw; u0 < units; u0 += L.waves * gpw) {
    const int64_t unit = u0 + L.grp;
    const bool valid = unit < units;
    const int64_t b = !valid ? 0 : (passes == 1 ? unit : unit / passes);
    const int64_t c = (unit - b * passes) * 64 + L.lig;
    const bool has_chunk = valid && c < rc;
    int64_t e0 = 0, len = 0;
    if (valid) {
      e0 = indptr[b];
      len = indptr[b + 1] - e0;
      if (e0 < 0 || len < 0 || e0 + len > E) len = 0;
    }
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);  // a sample with no entry that w holds: +0.0
    bool have = false;
    for (int64_t t0 = 0; __any(t0 < len); t0 += L.G) {
      int pos = -1;
      float val = 1.f;
      const int64_t k = t0 + L.lig;
      if (k < len) {
        const int64_t col = indices[e0 + k];
        if constexpr (DATA) val = data[e0 + k];
        if constexpr (DENSE) {
          if (static_cast<uint64_t>(col) < static_cast<uint64_t>(wn)) pos = static_cast<int>(col);
        } else {
          int64_t lo = 0, hi = wn;
          while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (wids[mid] < col) lo = mid + 1; else hi = mid;
          }
          if (lo < wn && wids[lo] == col) pos = static_cast<int>(lo);
        }
      }
      const int64_t left = len - t0;
      const int cnt = left <= 0 ? 0 : static_cast<int>(min(static_cast<int64_t>(L.G), left));
      ordered_turn<DATA>(wrows, rc, c, has_chunk, pos, val, cnt, L, acc, have);
    }
    if (has_chunk) out[b * rc + c] = acc;
  }
}

// out[u] (nu rows of rc chunks) = the ordered sum over k in [starts[u], starts[u + 1]) of val[e] * rows[SRC ? src[e]
// : e], e = order[k]; order holds E entry numbers, rows has nrows rows.
template <bool DATA, bool SRC>
__global__ __launch_bounds__(256) void kv_rows_segsum_kernel(const float4* __restrict__ rows,
                                                             const int64_t* __restrict__ starts,
                                                             const int64_t* __restrict__ order,
                                                             const int64_t* __restrict__ src,
                                                             const float* __restrict__ val_of,
                                                             float4* __restrict__ out, int64_t nu, int64_t E,
                                                             int64_t nrows, int64_t rc, int logG) {
  const Lanes L(logG);
  const int64_t passes = (rc + 63) >> 6, units = nu * passes;
  const int gpw = 64 >> logG;
  for (int64_t u0 = L.wave * gpw; u0 < units; u0 += L.waves * gpw) {
    const int64_t unit = u0 + L.grp;
    const bool valid = unit < units;
    const int64_t u = !valid ? 0 : (passes == 1 ? unit : unit / passes);
    const int64_t c = (unit - u * passes) * 64 + L.lig;
    const bool has_chunk = valid && c < rc;
    int64_t s0 = 0, len = 0;
    if (valid) {
      s0 = starts[u];
      len = starts[u + 1] - s0;
      if (s0 < 0 || len < 0 || s0 + len > E) len = 0;
    }
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    bool have = false;
    for (int64_t t0 = 0; __any(t0 < len); t0 += L.G) {
      int pos = -1;
      float val = 1.f;
      const int64_t k = t0 + L.lig;
      if (k < len) {
        const int64_t e = order[s0 + k];
        if (static_cast<uint64_t>(e) < static_cast<uint64_t>(E)) {
          int64_t r = e;
          if constexpr (SRC) r = src[e];
          if constexpr (DATA) val = val_of[e];
          if (static_cast<uint64_t>(r) < static_cast<uint64_t>(nrows)) pos = static_cast<int>(r);
        }
      }
      const int64_t left = len - t0;
      const int cnt = left <= 0 ? 0 : static_cast<int>(min(static_cast<int64_t>(L.G), left));
      ordered_turn<DATA>(rows, rc, c, has_chunk, pos, val, cnt, L, acc, have);
    }
    if (has_chunk) out[u * rc + c] = acc;
  }
}

inline bool misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

// log2 of the lane group of a row of rc chunks, and the workgroups (4 waves each) of n output rows
int group_log(int64_t rc) {
  int lg = 0;
  while (lg < 6 && (int64_t{1} << lg) < rc) ++lg;
  return lg;
}

int blocks_of(int64_t n, int64_t rc, int logG) {
  const int64_t units = n * ((rc + 63) >> 6), per_block = 4 * (64 >> logG);
  return static_cast<int>(std::min<int64_t>(2048, (units + per_block - 1) / per_block));
}

}  // namespace

// out [B, row_elems] <- the CSR (indptr [B + 1], indices [E] column ids, data [E] or null: every value 1) times w:
// w_rows [w_n, row_elems], its rows named by the strictly increasing w_ids [w_n], or, w_ids null, row r being column
// r (dense).  A column w does not hold contributes nothing; a sample with none gives +0.0.  fp32, row_elems a
// multiple of 4, out / w_rows 16-byte aligned, w_n and E at most INT32_MAX.
TONY_API int tony_kv_csr_dot(float* out, const int64_t* indptr, const int64_t* indices, const float* data,
                             const int64_t* w_ids, const float* w_rows, int64_t w_n, int64_t B, int64_t E,
                             int64_t row_elems, hipStream_t stream) {
  if (out == nullptr || indptr == nullptr || B < 0 || E < 0 || w_n < 0 || E > INT32_MAX || w_n > INT32_MAX ||
      row_elems <= 0 || (row_elems & 3) || (E > 0 && indices == nullptr) || (w_n > 0 && w_rows == nullptr) ||
      misaligned(out, 15) || misaligned(w_rows, 15) || misaligned(indptr, 7) || misaligned(indices, 7) ||
      misaligned(w_ids, 7) || misaligned(data, 3))
    return -1;
  if (B == 0) return 0;
  const int64_t rc = row_elems >> 2;
  const int lg = group_log(rc);
  const int blocks = blocks_of(B, rc, lg);
  const float4* W = reinterpret_cast<const float4*>(w_rows);
  float4* O = reinterpret_cast<float4*>(out);
#define TONY_CSR_DOT(DATA, DENSE) \
  kv_csr_dot_kernel<DATA, DENSE><<<blocks, 256, 0, stream>>>(indptr, indices, data, w_ids, w_n, W, O, B, E, rc, lg)
  if (data != nullptr) {
    if (w_ids == nullptr) TONY_CSR_DOT(true, true); else TONY_CSR_DOT(true, false);
  } else {
    if (w_ids == nullptr) TONY_CSR_DOT(false, true); else TONY_CSR_DOT(false, false);
  }
#undef TONY_CSR_DOT
  TONY_LAUNCH_CHECK();
  return 0;
}

// out [nu, row_elems] <- for every u the ordered sum over k in [starts[u], starts[u + 1]) of val[e] * rows[src ?
// src[e] : e], e = order[k].  starts [nu + 1] non-decreasing within [0, E], order [E] entry numbers in [0, E), src
// [E] (nullable) rows of `rows` [nrows, row_elems], val [E] (nullable: every value 1, no multiply).  An empty segment
// gives +0.0.  fp32, row_elems a multiple of 4, out / rows 16-byte aligned, E and nrows at most INT32_MAX.
TONY_API int tony_kv_rows_segsum(float* out, const float* rows, const int64_t* starts, const int64_t* order,
                                 const int64_t* src, const float* val, int64_t nu, int64_t E, int64_t nrows,
                                 int64_t row_elems, hipStream_t stream) {
  if (out == nullptr || starts == nullptr || nu < 0 || E < 0 || nrows < 0 || E > INT32_MAX || nrows > INT32_MAX ||
      row_elems <= 0 || (row_elems & 3) || (E > 0 && (order == nullptr || rows == nullptr)) || misaligned(out, 15) ||
      misaligned(rows, 15) || misaligned(starts, 7) || misaligned(order, 7) || misaligned(src, 7) ||
      misaligned(val, 3))
    return -1;
  if (nu == 0) return 0;
  const int64_t rc = row_elems >> 2;
  const int lg = group_log(rc);
  const int blocks = blocks_of(nu, rc, lg);
  const float4* Rw = reinterpret_cast<const float4*>(rows);
  float4* O = reinterpret_cast<float4*>(out);
#define TONY_SEGSUM(DATA, SRC) \
  kv_rows_segsum_kernel<DATA, SRC><<<blocks, 256, 0, stream>>>(Rw, starts, order, src, val, O, nu, E, nrows, rc, lg)
  if (val != nullptr) {
    if (src != nullptr) TONY_SEGSUM(true, true); else TONY_SEGSUM(true, false);
  } else {
    if (src != nullptr) TONY_SEGSUM(false, true); else TONY_SEGSUM(false, false);
  }
#undef TONY_SEGSUM
  TONY_LAUNCH_CHECK();
  return 0;
}
