// The classifier head of the MNIST networks as one op: per-row softmax cross-entropy of x w^T + b for x [M, K],
// w [N, K], b [N], labels [M] (int64), fp32, N <= 32 classes; one launch forward, one backward.  K % 4 == 0, M is
// arbitrary.  A label outside [0, N) marks an ignored row: loss 0, a zero gradient row (ops.cross_entropy's rule).
// No atomics: both grids and every summation order are functions of (M, N, K) alone, so the same inputs give the
// same bits.
//
// The products run on v_mfma_f32_32x32x2_f32 with the operand map of dense.hip: a lane of half h = l / 32 takes the
// four consecutive reduction indices 8 t + 4 h .. + 3 of group t and feeds them to four MFMAs; accumulator r of lane l
// is D[8 * (r / 4) + 4 * h + r % 4][l % 32].  The few helpers of that map are repeated here so that dense.hip's
// translation unit stays as it is.
//
//   forward   One workgroup of four waves per 32 batch rows; the N classes are the (zero-padded) 32 columns of the
//             tile, so the whole of K belongs to one workgroup and nothing is split or folded.  K streams through two
//             LDS buffers in chunks of 64 exactly as in dense_fwd_kernel (16-byte loads, clamped and zeroed by register
//             selects, the next chunk's loads issued before this chunk's MFMAs, one barrier a chunk, each wave a
//             quarter of every chunk).  The waves' partial tiles meet in LDS in wave order 0, 1, 2, 3, the bias is
//             added, and the logits tile is written back to LDS as [row][33].  All threads then store its M x N part
//             as one contiguous run, while lanes 0 .. 31 of wave 0 own a row each: maximum over the first N columns,
//             se = sum __expf(v - mx), lse = mx + __logf(se), loss = lse - v[label], the arithmetic and order of
//             xent_fwd_kernel (loss.hip) without smoothing.
//   backward  One workgroup per 32 of the K input features; a wave holds w[:, slice] as its B operand in 16 registers
//             for the whole launch (class rows past N zero).  The waves take the row tiles of 32 batch rows
//             round-robin.  For a tile a wave forms d[m][n] = gout[m] (__expf(logits[m][n] - lse[m]) - (n == label[m]))
//             (xent_bwd_kernel's line; zero for ignored rows, rows past M and columns past N) straight into its own
//             [32][36] LDS tile, one row a lane pair, while x[tile, slice] comes in as 16 coalesced register loads (128
//             bytes a half-wave a row).  Both products read that one d tile: dx[tile, slice] = d w[:, slice] takes d
//             along n (one 16-byte LDS read per four MFMAs) and is stored at once, only when asked for;
//             dw[:, slice] += d^T x[tile, slice] takes d along m (32 banks a half-wave) and stays in the accumulator
//             across the wave's tiles.  At the end the waves' dw partials are added through LDS in wave order and
//             stored.  db: workgroup 0's waves sum their tiles' columns of d in row order, and the four sums are added
//             in wave order.  Every workgroup recomputes d (M x N exponentials): no buffer, no second launch.
#include "common.h"

using namespace tony;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kTile = 32;                           // batch rows of a tile; the padded class count
constexpr int kFwdKC = 64;                          // K of a forward chunk, 16 per wave
constexpr int kFwdStride = kFwdKC + 4;              // floats of a staged row
constexpr int kFwdPanel = kTile * kFwdStride;       // floats of one operand's panel
constexpr int kRed = (kWaves - 1) * 16 * kWave;     // floats of the partial tiles of waves 1 .. 3
constexpr int kLogitStride = kTile + 1;             // the logits tile [row][33]: a lane a row, no bank shared
constexpr int kSlice = 32;                          // input features of a backward workgroup
constexpr int kDStride = kTile + 4;                 // the d tile [m][36]: 16-byte rows, eight rows cover the banks
constexpr int kDTile = kTile * kDStride;

__device__ __forceinline__ f32x16 zero16() {
  return f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
}

// row of accumulator register r in a lane of half h
__device__ __forceinline__ int acc_row(int r, int half) { return 8 * (r / 4) + 4 * half + r % 4; }

__device__ __forceinline__ f32x16 mfma4(const float4 a, const float4 b, f32x16 acc) {
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// v, or zeros: a select in registers, never a guarded load
__device__ __forceinline__ float4 keep4(const float4 v, const bool ok) {
  return make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f);
}

// rows r .. r + 3 of the column at p (row stride ld), a row past `rows` loading the last one: four unconditional
// loads in bounds; keep_rows4 zeroes those rows in registers once the values are needed
__device__ __forceinline__ float4 ld_rows4(const float* __restrict__ p, const int r, const int rows, const int ld) {
  return make_float4(p[static_cast<int64_t>(min(r, rows - 1)) * ld], p[static_cast<int64_t>(min(r + 1, rows - 1)) * ld],
                     p[static_cast<int64_t>(min(r + 2, rows - 1)) * ld], p[static_cast<int64_t>(min(r + 3, rows - 1)) * ld]);
}
__device__ __forceinline__ float4 keep_rows4(const float4 v, const int r, const int rows) {
  return make_float4(r < rows ? v.x : 0.f, r + 1 < rows ? v.y : 0.f, r + 2 < rows ? v.z : 0.f, r + 3 < rows ? v.w : 0.f);
}

__global__ __launch_bounds__(kThreads) void dense_xent_fwd_kernel(const float* __restrict__ x,
                                                                  const float* __restrict__ w,
                                                                  const float* __restrict__ bias,
                                                                  const int64_t* __restrict__ labels,
                                                                  float* __restrict__ logits,
                                                                  float* __restrict__ lse_out, float* __restrict__ loss,
                                                                  const int M, const int N, const int K) {
  __shared__ __attribute__((aligned(16))) float sm[2 * 2 * kFwdPanel];  // [buffer][x | w][row][kFwdStride]
  static_assert(2 * 2 * kFwdPanel >= kRed + kTile * kLogitStride, "the waves meet, and the logits stay, in this LDS");
  const int m0 = blockIdx.x * kTile;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int half = lane >> 5, l32 = lane & 31;
  // staging: a thread moves the float4 at column 4 * sc4 of rows srow and srow + 16 of both panels; rows past M or N
  // are clamped to the last one and a column past K to the row's last float4, so every load is unconditional and in
  // bounds; what lies outside is zeroed in registers
  const int srow = threadIdx.x >> 4, sc4 = 4 * (threadIdx.x & 15);
  const float* x0 = x + static_cast<int64_t>(min(m0 + srow, M - 1)) * K;
  const float* x1 = x + static_cast<int64_t>(min(m0 + srow + 16, M - 1)) * K;
  const float* w0 = w + static_cast<int64_t>(min(srow, N - 1)) * K;
  const float* w1 = w + static_cast<int64_t>(min(srow + 16, N - 1)) * K;
  const bool x0in = m0 + srow < M, x1in = m0 + srow + 16 < M;
  const bool w0in = srow < N, w1in = srow + 16 < N;
  float* st = sm + srow * kFwdStride + sc4;  // this thread's float4 of row srow of buffer 0's x panel
  const int chunks = (K + kFwdKC - 1) / kFwdKC;
  const int opoff = l32 * kFwdStride + 16 * wave + 4 * half;
  f32x16 acc = zero16();
  {
    const int kc = min(sc4, K - 4);
    const bool kin = sc4 < K;  // K and sc4 are multiples of 4: a float4 is inside the row or outside it
    *reinterpret_cast<float4*>(st) = keep4(ld4(x0 + kc), kin && x0in);
    *reinterpret_cast<float4*>(st + 16 * kFwdStride) = keep4(ld4(x1 + kc), kin && x1in);
    *reinterpret_cast<float4*>(st + kFwdPanel) = keep4(ld4(w0 + kc), kin && w0in);
    *reinterpret_cast<float4*>(st + kFwdPanel + 16 * kFwdStride) = keep4(ld4(w1 + kc), kin && w1in);
  }
  __syncthreads();
  for (int c = 0; c < chunks; ++c) {
    // the next chunk's loads go out before this chunk's MFMAs and land in the other buffer after them; past the last
    // chunk they fetch the row's last float4 again and store zeros nobody reads
    const int kn = (c + 1) * kFwdKC + sc4, kc = min(kn, K - 4);
    const bool kin = kn < K;
    const float4 rx0 = ld4(x0 + kc), rx1 = ld4(x1 + kc), rw0 = ld4(w0 + kc), rw1 = ld4(w1 + kc);
    __builtin_amdgcn_sched_barrier(0);  // or the scheduler sinks the loads below the MFMAs to save registers
    const float* a = sm + (c & 1) * 2 * kFwdPanel + opoff;
#pragma unroll
    for (int t = 0; t < 2; ++t) acc = mfma4(ld4(a + 8 * t), ld4(a + kFwdPanel + 8 * t), acc);
    __builtin_amdgcn_sched_barrier(0);  // the wait for the loads stands behind the last MFMA
    float* sn = st + ((c + 1) & 1) * 2 * kFwdPanel;  // last read as chunk c - 1, before the previous barrier
    *reinterpret_cast<float4*>(sn) = keep4(rx0, kin && x0in);
    *reinterpret_cast<float4*>(sn + 16 * kFwdStride) = keep4(rx1, kin && x1in);
    *reinterpret_cast<float4*>(sn + kFwdPanel) = keep4(rw0, kin && w0in);
    *reinterpret_cast<float4*>(sn + kFwdPanel + 16 * kFwdStride) = keep4(rw1, kin && w1in);
    __syncthreads();
  }
  float* red = sm;          // [wave - 1][r][lane]
  float* tl = sm + kRed;    // the logits tile [row][kLogitStride]
  if (wave > 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[((wave - 1) * 16 + r) * kWave + lane] = acc[r];
  }
  __syncthreads();
  if (wave == 0) {
    const float bv = l32 < N ? bias[l32] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float v = acc[r];
#pragma unroll
      for (int q = 0; q < kWaves - 1; ++q) v += red[(q * 16 + r) * kWave + lane];
      tl[acc_row(r, half) * kLogitStride + l32] = v + bv;
    }
  }
  __syncthreads();
  const int rows = min(kTile, M - m0);
  // rows m0 .. m0 + rows - 1 of logits [M, N] are one contiguous run
  float* lg = logits + static_cast<int64_t>(m0) * N;
  for (int i = threadIdx.x; i < rows * N; i += kThreads) {
    const int r = i / N;
    lg[i] = tl[r * kLogitStride + (i - r * N)];
  }
  if (static_cast<int>(threadIdx.x) < rows) {
    const float* v = tl + threadIdx.x * kLogitStride;
    float mx = -INFINITY;
    for (int n = 0; n < N; ++n) mx = fmaxf(mx, v[n]);
    float se = 0.f;
    for (int n = 0; n < N; ++n) se += __expf(v[n] - mx);
    const float lse = mx + __logf(se);
    const int64_t t = labels[m0 + threadIdx.x];
    const bool live = t >= 0 && t < N;  // else an ignored row: loss 0 (and a zero gradient row), lse still stored
    const float xt = live ? v[live ? static_cast<int>(t) : 0] : lse;
    loss[m0 + threadIdx.x] = live ? lse - xt : 0.f;
    lse_out[m0 + threadIdx.x] = lse;
  }
}

__global__ __launch_bounds__(kThreads) void dense_xent_bwd_kernel(const float* __restrict__ gout, const int64_t gs,
                                                                  const float* __restrict__ logits,
                                                                  const float* __restrict__ lse,
                                                                  const int64_t* __restrict__ labels,
                                                                  const float* __restrict__ x,
                                                                  const float* __restrict__ w, float* __restrict__ dx,
                                                                  float* __restrict__ dw, float* __restrict__ db,
                                                                  const int M, const int N, const int K) {
  __shared__ __attribute__((aligned(16))) float sm[kWaves * kDTile];  // a d tile [m][kDStride] per wave
  __shared__ float dbs[kWaves][kTile];
  static_assert(kWaves * kDTile >= kRed, "the waves' dw partials meet in this LDS");
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int half = lane >> 5, l32 = lane & 31;
  const int col = blockIdx.x * kSlice + l32;
  const bool colin = col < K;  // a lane past K loads its last column and stores nothing
  const float* wp = w + min(col, K - 1);
  const float* xp = x + min(col, K - 1);
  float4 wr[4];  // w[n = 8 t + 4 half .. + 3][col]
#pragma unroll
  for (int t = 0; t < 4; ++t) wr[t] = keep_rows4(ld_rows4(wp, 8 * t + 4 * half, N, K), 8 * t + 4 * half, N);
  float* dt = sm + wave * kDTile;
  f32x16 accw = zero16();
  float dbsum = 0.f;
  const int tiles = (M + kTile - 1) / kTile, rounds = (tiles + kWaves - 1) / kWaves;
  for (int it = 0; it < rounds; ++it) {
    const int tile = it * kWaves + wave, m0 = tile * kTile;
    const bool active = tile < tiles;  // per wave
    float4 xr[4];                      // x[m0 + 8 t + 4 half .. + 3][col]
    __syncthreads();                   // the previous tile's operand reads are done
    if (active) {
#pragma unroll
      for (int t = 0; t < 4; ++t) xr[t] = ld_rows4(xp, m0 + 8 * t + 4 * half, M, K);
      // row m0 + l32 of d, columns 16 half .. + 15
      const int m = min(m0 + l32, M - 1);
      const int64_t lab = labels[m];
      const bool live = m0 + l32 < M && lab >= 0 && lab < N;
      const float go = gout[m * gs], l = lse[m];
      const float* lg = logits + static_cast<int64_t>(m) * N;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float d[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int n = 16 * half + 4 * j + q;
          const float p = __expf(lg[min(n, N - 1)] - l);
          d[q] = live && n < N ? (p - (n == lab ? 1.f : 0.f)) * go : 0.f;
        }
        *reinterpret_cast<float4*>(dt + l32 * kDStride + 16 * half + 4 * j) = make_float4(d[0], d[1], d[2], d[3]);
      }
    }
    __syncthreads();
    if (active) {
      if (blockIdx.x == 0 && lane < kTile)
        for (int r = 0; r < kTile; ++r) dbsum += dt[r * kDStride + lane];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float* a = dt + (8 * t + 4 * half) * kDStride + l32;
        accw = mfma4(make_float4(a[0], a[kDStride], a[2 * kDStride], a[3 * kDStride]),
                     keep_rows4(xr[t], m0 + 8 * t + 4 * half, M), accw);
      }
      if (dx != nullptr) {
        f32x16 accx = zero16();
#pragma unroll
        for (int t = 0; t < 4; ++t) accx = mfma4(ld4(dt + l32 * kDStride + 8 * t + 4 * half), wr[t], accx);
        if (colin) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int m = m0 + acc_row(r, half);
            if (m < M) dx[static_cast<int64_t>(m) * K + col] = accx[r];
          }
        }
      }
    }
  }
  __syncthreads();  // every wave is done with its d tile
  float* red = sm;  // [wave - 1][r][lane]
  if (wave > 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[((wave - 1) * 16 + r) * kWave + lane] = accw[r];
  }
  if (lane < kTile) dbs[wave][lane] = dbsum;
  __syncthreads();
  if (wave == 0) {
    if (colin) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = acc_row(r, half);
        float v = accw[r];
#pragma unroll
        for (int q = 0; q < kWaves - 1; ++q) v += red[(q * 16 + r) * kWave + lane];
        if (n < N) dw[static_cast<int64_t>(n) * K + col] = v;
      }
    }
    if (blockIdx.x == 0 && lane < N) db[lane] = ((dbs[0][lane] + dbs[1][lane]) + dbs[2][lane]) + dbs[3][lane];
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// The supported form: 0, or the negative code of the first violated rule.
inline int check_form(const float* x, const float* w, int64_t M, int64_t N, int64_t K) {
  if (M < 1 || N < 1 || N > kTile || K < 4 || K % 4 != 0) return -2;
  if (M * K >= (int64_t{1} << 31)) return -3;
  if (!aligned16(x) || !aligned16(w)) return -4;
  return 0;
}

}  // namespace

// logits[M,N] = x[M,K] w[N,K]^T + bias, lse[M] = their row log-sum-exp, loss[M] = lse - logits[m][labels[m]], 0 for a
// label outside [0, N).  Contiguous fp32, int64 labels, 16-byte-aligned x and w, N <= 32.
TONY_API int tony_dense_xent_fwd(const float* x, const float* w, const float* bias, const int64_t* labels,
                                 float* logits, float* lse, float* loss, int64_t M, int64_t N, int64_t K,
                                 hipStream_t stream) {
  if (x == nullptr || w == nullptr || bias == nullptr || labels == nullptr || logits == nullptr || lse == nullptr ||
      loss == nullptr)
    return -1;
  if (const int rc = check_form(x, w, M, N, K)) return rc;
  dense_xent_fwd_kernel<<<ceil_div(M, kTile), kThreads, 0, stream>>>(x, w, bias, labels, logits, lse, loss,
                                                                     static_cast<int>(M), static_cast<int>(N),
                                                                     static_cast<int>(K));
  TONY_LAUNCH_CHECK();
  return 0;
}

// With d[m][n] = gout[m * gout_stride] (exp(logits[m][n] - lse[m]) - (n == labels[m])), a zero row for a label outside
// [0, N): dx[M,K] = d w (dx may be null: not computed), dw[N,K] = d^T x, db[N] = the column sums of d.  gout_stride is
// 1, or 0 for one value shared by every row (the gradient of a sum or a mean).
TONY_API int tony_dense_xent_bwd(const float* gout, int64_t gout_stride, const float* logits, const float* lse,
                                 const int64_t* labels, const float* x, const float* w, float* dx, float* dw, float* db,
                                 int64_t M, int64_t N, int64_t K, hipStream_t stream) {
  if (gout == nullptr || logits == nullptr || lse == nullptr || labels == nullptr || x == nullptr || w == nullptr ||
      dw == nullptr || db == nullptr)
    return -1;
  if (gout_stride != 0 && gout_stride != 1) return -2;
  if (const int rc = check_form(x, w, M, N, K)) return rc;
  dense_xent_bwd_kernel<<<ceil_div(K, kSlice), kThreads, 0, stream>>>(gout, gout_stride, logits, lse, labels, x, w, dx,
                                                                      dw, db, static_cast<int>(M), static_cast<int>(N),
                                                                      static_cast<int>(K));
  TONY_LAUNCH_CHECK();
  return 0;
}
