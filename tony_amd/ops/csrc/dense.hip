// Dense layers of the MNIST networks, fp32 in and out: y = x w^T + b (optionally ReLU) for x [M, K], w [N, K], b [N],
// and its data, weight and bias gradients with ReLU's backward mask (not y <= 0) applied as dy is staged, so no masked
// copy of dy ever exists in memory.  K % 4 == 0 (every row takes 16-byte loads); M and N are arbitrary, ragged tiles
// are zero-filled on the way in and masked on the way out.  No atomics: every grid and every summation order is a
// function of (M, N, K) alone, so the same inputs give the same bits.
//
// All three products run on v_mfma_f32_32x32x2_f32 (lane l, half h = l / 32: A[i = l % 32][k = h], B[k = h][j = l % 32],
// accumulator r of lane l is D[8 * (r / 4) + 4 * h + r % 4][l % 32]).  The instruction's two k indices need not be
// neighbours of the reduction: a lane of half h takes FOUR consecutive reduction indices 8 t + 4 h .. + 3 (one 16-byte
// LDS read where the operand is reduction-contiguous) and feeds them to four MFMAs, so MFMA j of group t adds the
// products of indices 8 t + j and 8 t + 4 + j.  A and B use the same map, which is all the sum asks for.
//
//   forward  NT: both operands are K-contiguous.  A workgroup owns one 32 x 32 tile of y and one of S slices of K; it
//            walks its slice in chunks of 64, both 32-row panels staged [row][64] in LDS with 16-byte global loads
//            and a row stride of 68 floats (16-byte rows; eight rows x four banks cover the 32 banks of a b128 read).
//            Two LDS buffers: the next chunk's global loads are issued into registers before this chunk's MFMAs and
//            written to the other buffer after them, one barrier a chunk.  The four waves take the quarters of every
//            chunk (16 k each: two b128 reads an operand, eight MFMAs) and meet in LDS in wave order.  With S == 1
//            bias and ReLU are this kernel's epilogue; otherwise it stores a partial tile and dense_fold_kernel adds
//            the S partials in index order, the bias, and applies ReLU.
//   dgrad    dx[M, K] = dy'[M, N] w[N, K]: the reduction is N and w is contiguous along the OUTPUT column, so a wave's
//            B operand is a coalesced global load straight into registers (128 bytes a half-wave), no LDS: the next
//            group's four loads are issued before this group's MFMAs and waited for behind them, rows past N
//            clamped and zeroed in registers so that no load is conditional.  The 32 rows of dy' are staged masked, 256 of N at a time.  A workgroup is four
//            waves on four neighbouring 32-column tiles of one row tile.
//   wgrad    dw[N, K] = dy'^T[N, M] x[M, K], db = column sums of dy': the reduction is M, x is again a coalesced
//            register operand and dy' (staged masked as [m][64 n]) is read along n: the 32 lanes of a half-wave hit 32
//            distinct banks; the two halves read rows 4 apart, the same banks, which costs nothing only if a b32
//            read is served a half-wave at a time (derived from nothing firmer, and not measured).  A wave holds TWO
//            row tiles of dw (64 n) per x load, so x is read ceil(N / 64) times; a workgroup walks all of M for 64 n
//            x 128 k.  Every half-wave stores 128 contiguous bytes of a dw row.  The workgroups of column block 0 also
//            sum their dy' columns into db.
#include "common.h"

using namespace tony;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kTile = 32;                      // rows and columns of a wave's accumulator tile
constexpr int kFwdKC = 64;                     // K of a forward chunk, 16 per wave
constexpr int kFwdStride = kFwdKC + 4;         // floats of a staged row
constexpr int kFwdPanel = kTile * kFwdStride;  // floats of one operand's panel
constexpr int kMinSlice = 256;                 // a forward K slice is never shorter (unless K is)
constexpr int kTargetGrid = 256;               // workgroups the forward split aims at: one per CU
constexpr int kColBlock = kWaves * kTile;      // output columns of a dgrad / wgrad workgroup
constexpr int kDgNC = 256;                     // N of a dgrad chunk
constexpr int kDgStride = kDgNC + 4;
constexpr int kWgMC = 128;                     // M of a wgrad chunk
constexpr int kWgN = 2 * kTile;                // dw rows of a wgrad workgroup

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

// v, or zeros: a select in registers (a guarded load became a select between addresses, with the zeros in scratch)
__device__ __forceinline__ float4 keep4(const float4 v, const bool ok) {
  return make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f);
}

// rows r .. r + 3 of the column at p (row stride ld), a row past `rows` loading the last one: four unconditional
// loads in bounds that can stay in flight; keep_rows4 zeroes those rows in registers once the values are needed
__device__ __forceinline__ float4 ld_rows4(const float* __restrict__ p, const int r, const int rows, const int ld) {
  return make_float4(p[static_cast<int64_t>(min(r, rows - 1)) * ld], p[static_cast<int64_t>(min(r + 1, rows - 1)) * ld],
                     p[static_cast<int64_t>(min(r + 2, rows - 1)) * ld], p[static_cast<int64_t>(min(r + 3, rows - 1)) * ld]);
}
__device__ __forceinline__ float4 keep_rows4(const float4 v, const int r, const int rows) {
  return make_float4(r < rows ? v.x : 0.f, r + 1 < rows ? v.y : 0.f, r + 2 < rows ? v.z : 0.f, r + 3 < rows ? v.w : 0.f);
}

struct Shape {
  int M, N, K;
  int S, slice;  // forward: K slices and the K of one (a multiple of 4)
  int tn;        // forward: column tiles
  int kt;        // dgrad / wgrad: column blocks of kColBlock
};

__global__ __launch_bounds__(kThreads) void dense_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                             const float* __restrict__ bias, float* __restrict__ out,
                                                             const Shape g, const int relu) {
  __shared__ __attribute__((aligned(16))) float sm[2 * 2 * kFwdPanel];  // [buffer][x | w][row][kFwdStride]
  static_assert(2 * 2 * kFwdPanel >= (kWaves - 1) * 16 * kWave, "the waves meet in this LDS");
  const int tile = blockIdx.x / g.S, s = blockIdx.x - tile * g.S;
  const int m0 = (tile / g.tn) * kTile, n0 = (tile % g.tn) * kTile;
  const int k0 = s * g.slice, k1 = min(g.K, k0 + g.slice);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int half = lane >> 5, l32 = lane & 31;
  // staging: a thread moves the float4 at column 4 * sc4 of rows srow and srow + 16 of both panels
  const int srow = threadIdx.x >> 4, sc4 = 4 * (threadIdx.x & 15);
  // rows past M or N are clamped to the last one and a column past the slice to the last float4 of the row, so every
  // load is unconditional and in bounds; what lies outside is zeroed in registers
  const float* x0 = x + static_cast<int64_t>(min(m0 + srow, g.M - 1)) * g.K;
  const float* x1 = x + static_cast<int64_t>(min(m0 + srow + 16, g.M - 1)) * g.K;
  const float* w0 = w + static_cast<int64_t>(min(n0 + srow, g.N - 1)) * g.K;
  const float* w1 = w + static_cast<int64_t>(min(n0 + srow + 16, g.N - 1)) * g.K;
  const bool x0in = m0 + srow < g.M, x1in = m0 + srow + 16 < g.M;
  const bool w0in = n0 + srow < g.N, w1in = n0 + srow + 16 < g.N;
  float* st = sm + srow * kFwdStride + sc4;  // this thread's float4 of row srow of buffer 0's x panel
  const int chunks = (k1 - k0 + kFwdKC - 1) / kFwdKC;
  const int opoff = l32 * kFwdStride + 16 * wave + 4 * half;
  f32x16 acc = zero16();
  {
    const int kc = min(k0 + sc4, g.K - 4);
    const bool kin = k0 + sc4 < k1;  // k0, k1 and sc4 are multiples of 4: a float4 is inside the slice or outside it
    *reinterpret_cast<float4*>(st) = keep4(ld4(x0 + kc), kin && x0in);
    *reinterpret_cast<float4*>(st + 16 * kFwdStride) = keep4(ld4(x1 + kc), kin && x1in);
    *reinterpret_cast<float4*>(st + kFwdPanel) = keep4(ld4(w0 + kc), kin && w0in);
    *reinterpret_cast<float4*>(st + kFwdPanel + 16 * kFwdStride) = keep4(ld4(w1 + kc), kin && w1in);
  }
  __syncthreads();
  for (int c = 0; c < chunks; ++c) {
    // the next chunk's loads go out before this chunk's MFMAs and land in the other buffer after them; past the last
    // chunk they fetch the row's last float4 again and store zeros nobody reads
    const int kn = k0 + (c + 1) * kFwdKC + sc4, kc = min(kn, g.K - 4);
    const bool kin = kn < k1;
    const float4 rx0 = ld4(x0 + kc), rx1 = ld4(x1 + kc), rw0 = ld4(w0 + kc), rw1 = ld4(w1 + kc);
    __builtin_amdgcn_sched_barrier(0);  // or the scheduler sinks the loads below the MFMAs to save registers
    const float* a = sm + (c & 1) * 2 * kFwdPanel + opoff;
#pragma unroll
    for (int t = 0; t < 2; ++t)
      acc = mfma4(*reinterpret_cast<const float4*>(a + 8 * t), *reinterpret_cast<const float4*>(a + kFwdPanel + 8 * t),
                  acc);
    __builtin_amdgcn_sched_barrier(0);  // the wait for the loads stands behind the last MFMA
    float* sn = st + ((c + 1) & 1) * 2 * kFwdPanel;  // last read as chunk c - 1, before the previous barrier
    *reinterpret_cast<float4*>(sn) = keep4(rx0, kin && x0in);
    *reinterpret_cast<float4*>(sn + 16 * kFwdStride) = keep4(rx1, kin && x1in);
    *reinterpret_cast<float4*>(sn + kFwdPanel) = keep4(rw0, kin && w0in);
    *reinterpret_cast<float4*>(sn + kFwdPanel + 16 * kFwdStride) = keep4(rw1, kin && w1in);
    __syncthreads();
  }
  float* red = sm;  // [wave - 1][r][lane]
  if (wave > 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[((wave - 1) * 16 + r) * kWave + lane] = acc[r];
  }
  __syncthreads();
  const int n = n0 + l32;
  if (wave == 0 && n < g.N) {
    const float bv = g.S == 1 ? bias[n] : 0.f;
    float* o = out + (g.S == 1 ? 0 : static_cast<int64_t>(s) * g.M * g.N) + n;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + acc_row(r, half);
      float v = acc[r];
#pragma unroll
      for (int q = 0; q < kWaves - 1; ++q) v += red[(q * 16 + r) * kWave + lane];
      if (g.S == 1) {
        v += bv;
        if (relu) v = relu_f(v);
      }
      if (m < g.M) o[static_cast<int64_t>(m) * g.N] = v;
    }
  }
}

// y[i] = act(bias[i % N] + the S partials [M, N] added in index order)
__global__ __launch_bounds__(kThreads) void dense_fold_kernel(const float* __restrict__ partials,
                                                              const float* __restrict__ bias, float* __restrict__ y,
                                                              const int S, const int N, const int64_t mn,
                                                              const int relu) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= mn) return;
  float v = partials[i];
#pragma unroll 4
  for (int s = 1; s < S; ++s) v += partials[s * mn + i];
  v += bias[i % N];
  y[i] = relu ? relu_f(v) : v;
}

// dy' at [m][n], zero outside the matrix; y == nullptr without ReLU.  The mask is torch's threshold_backward,
// y <= 0 ? 0 : dy: NaN <= 0 is false, so the gradient passes through a NaN activation (y > 0 would drop it).
__device__ __forceinline__ float masked_dy(const float* __restrict__ dy, const float* __restrict__ y, int m, int n,
                                           const Shape& g) {
  if (m >= g.M || n >= g.N) return 0.f;
  const int64_t off = static_cast<int64_t>(m) * g.N + n;
  const float v = dy[off];
  return y == nullptr || !(y[off] <= 0.f) ? v : 0.f;
}

__global__ __launch_bounds__(kThreads) void dense_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                               const float* __restrict__ w, float* __restrict__ dx,
                                                               const Shape g) {
  __shared__ __attribute__((aligned(16))) float dt[kTile * kDgStride];  // [m][n of the chunk]
  const int mb = blockIdx.x / g.kt, kb = blockIdx.x - mb * g.kt;
  const int m0 = mb * kTile;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int half = lane >> 5, l32 = lane & 31;
  const int col = kb * kColBlock + wave * kTile + l32;
  const bool active = kb * kColBlock + wave * kTile < g.K;  // per wave
  const float* wp = w + min(col, g.K - 1);                  // a lane past K loads its last column and stores nothing
  f32x16 acc = zero16();
  for (int nc = 0; nc < g.N; nc += kDgNC) {
    const int ncols = min(kDgNC, (g.N - nc + 7) & ~7);  // N padded with zeros to a group of 8
    __syncthreads();                                    // the previous chunk's operand reads are done
    if (static_cast<int>(threadIdx.x) < ncols)
      for (int r = 0; r < kTile; ++r) dt[r * kDgStride + threadIdx.x] = masked_dy(dy, y, m0 + r, nc + threadIdx.x, g);
    __syncthreads();
    if (active) {
      const float* ap = dt + l32 * kDgStride + 4 * half;
      const int groups = ncols / 8;
      float4 b = keep_rows4(ld_rows4(wp, nc + 4 * half, g.N, g.K), nc + 4 * half, g.N);
      for (int t = 0; t < groups; ++t) {
        // the next group's rows go out before this group's MFMAs (past the last group: the last one's again)
        const int rn = nc + 8 * min(t + 1, groups - 1) + 4 * half;
        const float4 bn = ld_rows4(wp, rn, g.N, g.K);
        const float4 a = *reinterpret_cast<const float4*>(ap + 8 * t);
        __builtin_amdgcn_sched_barrier(0);  // keeps the loads above the MFMAs and their wait below
        acc = mfma4(a, b, acc);
        __builtin_amdgcn_sched_barrier(0);
        b = keep_rows4(bn, rn, g.N);
      }
    }
  }
  if (active && col < g.K) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + acc_row(r, half);
      if (m < g.M) dx[static_cast<int64_t>(m) * g.K + col] = acc[r];
    }
  }
}

__global__ __launch_bounds__(kThreads) void dense_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                               const float* __restrict__ x, float* __restrict__ dw,
                                                               float* __restrict__ db, const Shape g) {
  __shared__ float dt[kWgMC * kWgN];  // [m of the chunk][n]
  const int nb = blockIdx.x / g.kt, kb = blockIdx.x - nb * g.kt;
  const int n0 = nb * kWgN;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int half = lane >> 5, l32 = lane & 31;
  const int col = kb * kColBlock + wave * kTile + l32;
  const bool active = kb * kColBlock + wave * kTile < g.K;  // per wave
  const bool two = n0 + kTile < g.N;                        // per workgroup: the second row tile exists
  const float* xp = x + min(col, g.K - 1);
  f32x16 acc0 = zero16(), acc1 = zero16();
  float dbs = 0.f;
  const int sn = threadIdx.x & (kWgN - 1), sm0 = threadIdx.x / kWgN;  // staging: column, first row
  for (int mc = 0; mc < g.M; mc += kWgMC) {
    const int rows = min(kWgMC, (g.M - mc + 7) & ~7);  // M padded with zeros to a group of 8
    __syncthreads();
    for (int r = sm0; r < rows; r += kThreads / kWgN) dt[r * kWgN + sn] = masked_dy(dy, y, mc + r, n0 + sn, g);
    __syncthreads();
    if (kb == 0 && threadIdx.x < kWgN)
      for (int r = 0; r < rows; ++r) dbs += dt[r * kWgN + threadIdx.x];
    if (active) {
      const float* ap = dt + 4 * half * kWgN + l32;
      const int groups = rows / 8;
      float4 b = keep_rows4(ld_rows4(xp, mc + 4 * half, g.M, g.K), mc + 4 * half, g.M);
      for (int t = 0; t < groups; ++t) {
        const int rn = mc + 8 * min(t + 1, groups - 1) + 4 * half;
        const float4 bn = ld_rows4(xp, rn, g.M, g.K);
        const float* a = ap + 8 * t * kWgN;
        const float4 a0 = make_float4(a[0], a[kWgN], a[2 * kWgN], a[3 * kWgN]);
        const float4 a1 = make_float4(a[kTile], a[kWgN + kTile], a[2 * kWgN + kTile], a[3 * kWgN + kTile]);
        __builtin_amdgcn_sched_barrier(0);  // keeps the loads above the MFMAs and their wait below
        acc0 = mfma4(a0, b, acc0);
        if (two) acc1 = mfma4(a1, b, acc1);
        __builtin_amdgcn_sched_barrier(0);
        b = keep_rows4(bn, rn, g.M);
      }
    }
  }
  if (active && col < g.K) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = n0 + acc_row(r, half);
      if (n < g.N) dw[static_cast<int64_t>(n) * g.K + col] = acc0[r];
      if (n + kTile < g.N) dw[static_cast<int64_t>(n + kTile) * g.K + col] = acc1[r];
    }
  }
  if (kb == 0 && threadIdx.x < kWgN && n0 + static_cast<int>(threadIdx.x) < g.N) db[n0 + threadIdx.x] = dbs;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// The supported form; fills g.  0, or the negative code of the first violated rule.
inline int make_shape(int64_t M, int64_t N, int64_t K, Shape* g) {
  constexpr int64_t lim = int64_t{1} << 31;
  if (M < 1 || N < 1 || K < 4 || K % 4 != 0) return -2;
  if (M >= lim || N >= lim || K >= lim || M * K >= lim || N * K >= lim || M * N >= lim) return -3;
  g->M = static_cast<int>(M), g->N = static_cast<int>(N), g->K = static_cast<int>(K);
  const int64_t tm = (M + kTile - 1) / kTile, tn = (N + kTile - 1) / kTile;
  g->tn = static_cast<int>(tn);
  g->kt = static_cast<int>((K + kColBlock - 1) / kColBlock);
  // K slices: enough for kTargetGrid workgroups, none shorter than kMinSlice, each a multiple of 4
  int64_t want = (kTargetGrid + tm * tn - 1) / (tm * tn);
  if (want > K / kMinSlice) want = K / kMinSlice;
  if (want < 1) want = 1;
  const int64_t slice = ((K + want - 1) / want + 3) / 4 * 4;
  g->slice = static_cast<int>(slice);
  g->S = static_cast<int>((K + slice - 1) / slice);
  if (tm * tn * g->S >= lim || tm * g->kt >= lim || ((N + kWgN - 1) / kWgN) * g->kt >= lim) return -3;
  return 0;
}

}  // namespace

// K slices of tony_dense_fwd for this shape (a function of the shape alone), 0 for a shape outside the form.  With
// S > 1 the forward needs S * M * N floats of partials and tony_dense_fold after it.
TONY_API int tony_dense_splits(int64_t M, int64_t N, int64_t K) {
  Shape g;
  return make_shape(M, N, K, &g) ? 0 : g.S;
}

// S == 1: y[M,N] = act(x[M,K] w[N,K]^T + bias) (partials unused).  S > 1: partials [S][M][N], each one K slice's
// product; y is not written.  Contiguous fp32, 16-byte-aligned x and w.
TONY_API int tony_dense_fwd(const float* x, const float* w, const float* bias, float* y, float* partials, int64_t M,
                            int64_t N, int64_t K, int relu, hipStream_t stream) {
  if (x == nullptr || w == nullptr || bias == nullptr || y == nullptr) return -1;
  Shape g;
  if (const int rc = make_shape(M, N, K, &g)) return rc;
  if (!aligned16(x) || !aligned16(w)) return -4;
  if (g.S > 1 && partials == nullptr) return -1;
  const unsigned grid = static_cast<unsigned>(((M + kTile - 1) / kTile) * g.tn * g.S);
  dense_fwd_kernel<<<grid, kThreads, 0, stream>>>(x, w, bias, g.S > 1 ? partials : y, g, relu);
  TONY_LAUNCH_CHECK();
  return 0;
}

// y[M,N] = act(bias + the S partials of tony_dense_fwd, added in index order).
TONY_API int tony_dense_fold(const float* partials, const float* bias, float* y, int S, int64_t M, int64_t N, int relu,
                             hipStream_t stream) {
  if (partials == nullptr || bias == nullptr || y == nullptr) return -1;
  if (S < 1 || M < 1 || N < 1 || M * N >= (int64_t{1} << 31)) return -2;
  dense_fold_kernel<<<ceil_div(M * N, kThreads), kThreads, 0, stream>>>(partials, bias, y, S, static_cast<int>(N), M * N,
                                                                        relu);
  TONY_LAUNCH_CHECK();
  return 0;
}

// dx[M,K] = dy' w with dy' = relu ? (y <= 0 ? 0 : dy) : dy; y may be null without relu.
TONY_API int tony_dense_dgrad(const float* dy, const float* y, const float* w, float* dx, int64_t M, int64_t N,
                              int64_t K, int relu, hipStream_t stream) {
  if (dy == nullptr || w == nullptr || dx == nullptr || (relu && y == nullptr)) return -1;
  Shape g;
  if (const int rc = make_shape(M, N, K, &g)) return rc;
  const unsigned grid = static_cast<unsigned>(((M + kTile - 1) / kTile) * g.kt);
  dense_dgrad_kernel<<<grid, kThreads, 0, stream>>>(dy, relu ? y : nullptr, w, dx, g);
  TONY_LAUNCH_CHECK();
  return 0;
}

// dw[N,K] = dy'^T x and db[N] = the column sums of dy'.
TONY_API int tony_dense_wgrad(const float* dy, const float* y, const float* x, float* dw, float* db, int64_t M,
                              int64_t N, int64_t K, int relu, hipStream_t stream) {
  if (dy == nullptr || x == nullptr || dw == nullptr || db == nullptr || (relu && y == nullptr)) return -1;
  Shape g;
  if (const int rc = make_shape(M, N, K, &g)) return rc;
  const unsigned grid = static_cast<unsigned>(((N + kWgN - 1) / kWgN) * g.kt);
  dense_wgrad_kernel<<<grid, kThreads, 0, stream>>>(dy, relu ? y : nullptr, x, dw, db, g);
  TONY_LAUNCH_CHECK();
  return 0;
}
