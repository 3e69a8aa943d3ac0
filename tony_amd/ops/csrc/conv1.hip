// First-layer convolution of the MNIST CNNs, fp32: y = relu(b + conv(x, w)) with ONE input channel and 32 output
// channels, k in {3, 5}, stride 1, padding 0 or (k - 1) / 2, and its weight / bias gradient.  The layer reads the
// image, so there is no data gradient.
//
// Both directions are the matrix product of a [32 channels] x [k*k + 1] panel with the im2col of the image on
// v_mfma_f32_32x32x2_f32, the im2col formed only in LDS addresses.  The extra K row is all ones on the pixel side and
// the bias on the weight side, so the bias (forward) and its gradient (backward) ride in the product.
//
// Tiles.  The output plane of one image is cut into bands of R rows by column chunks of at most kTilePix columns, R
// the most rows with R * chunk width <= kTilePix: a tile has at most kTilePix pixels and its input patch, halo
// included, at most kXtFloats floats.  A workgroup stages the patch in LDS with the zero padding WRITTEN there, so no
// tap branches on the border.
//
// Operand layout of the 32x32x2 MFMA (lane l, half h = l / 32): A[i = l % 32][k = h], B[k = h][j = l % 32], and
// accumulator r of lane l is D[8 * (r / 4) + 4 * h + r % 4][l % 32].
//   forward   D[channel][pixel] = Wt[32 x K] . Xcol[K x 32 pixels], K = k*k + 1 in K / 2 steps.  A lane keeps its K / 2
//             weights (the last one of the upper half is the bias) in registers; pixels run along the lanes, so the 32
//             lanes of a half store 128 contiguous bytes of one channel plane.  ReLU on the accumulators.
//   backward  D[channel][tap] = dY'[32 x L] . Xcol[L x K] reduced over the L = N * OH * OW pixels two per step, column
//             k*k the sum of dY' (the bias gradient), columns past it unused.  dy and y are read coalesced (lanes along
//             a channel plane), masked (dy' = y <= 0 ? 0 : dy, torch's: 0 at 0, dy at a NaN) and laid into LDS as
//             [channel][pixel] rows of odd stride, from which the lane-per-channel operand reads are conflict free.
//             A workgroup reduces a fixed run of images -- the grid is a function of N alone -- its four waves
//             taking the pixel pairs of every row in turn; their accumulators meet in LDS in wave order and ONE 32x32
//             partial is stored.  tony_conv1_fold adds the partials in index order: no atomics, the same bits
//             every run.
#include "common.h"

using namespace tony;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kCout = 32;
constexpr int kTilePix = 256;                       // output pixels of a tile, at most
constexpr int kXtFloats = (kTilePix + 4) * 5;       // (R + k - 1) * (chunk + k - 1) at R * chunk <= 256, k <= 5
constexpr int kDyStride = kTilePix + 1;             // odd: lanes along channels hit 32 distinct banks
constexpr int kBwdImages = 2;                       // images of a backward workgroup's slice ...
constexpr int kBwdMaxGrid = 1024;                   // ... doubled and so on once N needs more workgroups than this

struct Geo {
  int N, H, W, OH, OW, pad;
  int R, CW, nb, nc;  // band rows, chunk columns, bands and chunks per image
  int64_t ohw;
};

struct Tile {
  int r0, rb, c0, cw, npix;  // first row / rows, first column / columns, pixels
};

__device__ __forceinline__ Tile tile_of(const Geo& g, int b, int c) {
  Tile t;
  t.r0 = b * g.R;
  t.rb = min(g.R, g.OH - t.r0);
  t.c0 = c * g.CW;
  t.cw = min(g.CW, g.OW - t.c0);
  t.npix = t.rb * t.cw;
  return t;
}

// the tile's input patch, (rb + KS - 1) rows of tw = cw + KS - 1 floats, zeros where the padding is
template <int KS>
__device__ __forceinline__ void stage_x(float* __restrict__ xt, const float* __restrict__ x, const Geo& g,
                                        const Tile& t, int n) {
  const int tw = t.cw + KS - 1, cnt = (t.rb + KS - 1) * tw;
  const float* img = x + static_cast<int64_t>(n) * g.H * g.W;
  for (int i = threadIdx.x; i < cnt; i += kThreads) {
    const int row = i / tw, col = i - row * tw;
    const int ih = t.r0 + row - g.pad, iw = t.c0 + col - g.pad;
    xt[i] = (ih >= 0 && ih < g.H && iw >= 0 && iw < g.W) ? img[static_cast<int64_t>(ih) * g.W + iw] : 0.f;
  }
}

template <int KS>
__global__ __launch_bounds__(kThreads) void conv1_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                             const float* __restrict__ bias, float* __restrict__ y,
                                                             const Geo g) {
  constexpr int KK = KS * KS, STEPS = (KK + 1) / 2;
  __shared__ float xt[kXtFloats];
  const int per = g.nb * g.nc;
  const int n = blockIdx.x / per, rem = blockIdx.x - n * per;
  const Tile t = tile_of(g, rem / g.nc, rem % g.nc);
  const int tw = t.cw + KS - 1;
  stage_x<KS>(xt, x, g, t, n);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int half = lane >> 5, l32 = lane & 31;
  float a[STEPS];
  int toff[STEPS];
#pragma unroll
  for (int s = 0; s < STEPS; ++s) {
    const int kk = 2 * s + half, kc = min(kk, KK - 1);  // kk == KK: the ones row against the bias
    a[s] = kk < KK ? w[l32 * KK + kk] : bias[l32];
    toff[s] = (kc / KS) * tw + kc % KS;
  }
  __syncthreads();
  for (int m = wave; m * 32 < t.npix; m += kWaves) {
    const int q = m * 32 + l32;
    const int qc = min(q, t.npix - 1);  // a lane past the tile computes its last pixel again and stores nothing
    const int row = qc / t.cw, col = qc - row * t.cw;
    const float* xp = xt + row * tw + col;
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
      float b = xp[toff[s]];
      if (s == STEPS - 1 && half) b = 1.f;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b, acc, 0, 0, 0);
    }
    if (q < t.npix) {
      float* yp = y + static_cast<int64_t>(n) * kCout * g.ohw + static_cast<int64_t>(t.r0 + row) * g.OW + t.c0 + col;
#pragma unroll
      for (int r = 0; r < 16; ++r) yp[(8 * (r / 4) + 4 * half + r % 4) * g.ohw] = relu_f(acc[r]);
    }
  }
}

template <int KS>
__global__ __launch_bounds__(kThreads) void conv1_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                             const float* __restrict__ x, float* __restrict__ partials,
                                                             const Geo g, const int images) {
  constexpr int KK = KS * KS;
  __shared__ float xt[kXtFloats];
  __shared__ float dyt[kCout * kDyStride];
  static_assert(kCout * kDyStride >= kWaves * kCout * 32, "the waves' accumulators meet in the dy tile's LDS");
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int half = lane >> 5, l32 = lane & 31;
  const int kc = min(l32, KK - 1);  // this lane's column of D: tap l32, the ones column at KK, unused past it
  const int kh = kc / KS, kw = kc % KS;
  f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int n0 = blockIdx.x * images, n1 = min(g.N, n0 + images);
  for (int n = n0; n < n1; ++n)
    for (int b = 0; b < g.nb; ++b)
      for (int c = 0; c < g.nc; ++c) {
        const Tile t = tile_of(g, b, c);
        const int tw = t.cw + KS - 1;
        __syncthreads();  // the previous tile's operand reads are done
        stage_x<KS>(xt, x, g, t, n);
        // a wave stages 8 channel planes, its lanes along the pixels
        for (int px = lane; px < t.npix; px += kWave) {
          const int row = px / t.cw, col = px - row * t.cw;
          const int64_t off = (static_cast<int64_t>(n) * kCout + wave * 8) * g.ohw +
                              static_cast<int64_t>(t.r0 + row) * g.OW + t.c0 + col;
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const float d = dy[off + k * g.ohw], v = y[off + k * g.ohw];
            dyt[(wave * 8 + k) * kDyStride + px] = !(v <= 0.f) ? d : 0.f;  // threshold_backward: a NaN y passes dy
          }
        }
        __syncthreads();
        const int toff = kh * tw + kw, pairs = (t.cw + 1) >> 1;
        for (int row = 0; row < t.rb; ++row)
          for (int pr = wave; pr < pairs; pr += kWaves) {
            const int col = 2 * pr + half;
            const bool ok = col < t.cw;  // the odd column past a row of odd width adds zeros
            const int cc = ok ? col : t.cw - 1;
            const float av = dyt[l32 * kDyStride + row * t.cw + cc];
            const float bv = l32 == KK ? 1.f : xt[row * tw + cc + toff];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ok ? av : 0.f, ok ? bv : 0.f, acc, 0, 0, 0);
          }
      }
  __syncthreads();
  float* red = dyt;  // [wave][channel][column]
#pragma unroll
  for (int r = 0; r < 16; ++r) red[(wave * kCout + 8 * (r / 4) + 4 * half + r % 4) * 32 + l32] = acc[r];
  __syncthreads();
  float* out = partials + static_cast<int64_t>(blockIdx.x) * (kCout * 32);
  for (int i = threadIdx.x; i < kCout * 32; i += kThreads) {
    float s = red[i];
#pragma unroll
    for (int wv = 1; wv < kWaves; ++wv) s += red[wv * kCout * 32 + i];
    out[i] = s;
  }
}

// dW[c][tap] and db[c] = the sum over the G partials of D[c][tap] and D[c][k*k], in index order
__global__ __launch_bounds__(kThreads) void conv1_fold_kernel(const float* __restrict__ partials, int G, int kk,
                                                              float* __restrict__ dw, float* __restrict__ db) {
  const int i = blockIdx.x * kThreads + threadIdx.x;  // < 32 * 32
  const int c = i >> 5, col = i & 31;
  if (col > kk) return;
  float s = 0.f;
#pragma unroll 8
  for (int gi = 0; gi < G; ++gi) s += partials[static_cast<int64_t>(gi) * (kCout * 32) + i];
  if (col == kk)
    db[c] = s;
  else
    dw[c * kk + col] = s;
}

// Images per backward workgroup: kBwdImages until that needs more than kBwdMaxGrid workgroups.
inline int bwd_images(int64_t N) {
  const int64_t unit = static_cast<int64_t>(kBwdImages) * kBwdMaxGrid;
  return static_cast<int>(kBwdImages * ((N + unit - 1) / unit));
}

// The supported form; fills g.  0, or the negative code of the first violated rule.
inline int make_geo(int64_t N, int H, int W, int ks, int pad, Geo* g) {
  if (ks != 3 && ks != 5) return -2;
  if (pad != 0 && pad != (ks - 1) / 2) return -3;
  if (N < 1 || H < ks || W < ks) return -4;
  const int64_t OH = static_cast<int64_t>(H) + 2 * pad - ks + 1, OW = static_cast<int64_t>(W) + 2 * pad - ks + 1;
  if (N * OH * OW >= (int64_t{1} << 31)) return -5;
  g->N = static_cast<int>(N), g->H = H, g->W = W, g->OH = static_cast<int>(OH), g->OW = static_cast<int>(OW);
  g->pad = pad;
  g->ohw = OH * OW;
  g->CW = static_cast<int>(OW < kTilePix ? OW : kTilePix);
  g->R = static_cast<int>(OH < kTilePix / g->CW ? OH : kTilePix / g->CW);
  g->nb = (g->OH + g->R - 1) / g->R;
  g->nc = (g->OW + g->CW - 1) / g->CW;
  if ((g->R + ks - 1) * (g->CW + ks - 1) > kXtFloats || g->R * g->CW > kTilePix) return -6;
  return 0;
}

}  // namespace

// y[N,32,OH,OW] = relu(bias + conv(x[N,1,H,W], w[32,1,ks,ks])), contiguous fp32.
TONY_API int tony_conv1_fwd(const float* x, const float* w, const float* bias, float* y, int64_t N, int H, int W,
                            int ks, int pad, hipStream_t stream) {
  if (x == nullptr || w == nullptr || bias == nullptr || y == nullptr) return -1;
  Geo g;
  if (const int rc = make_geo(N, H, W, ks, pad, &g)) return rc;
  const int64_t grid = N * g.nb * g.nc;  // <= N * OH * OW < 2^31
  if (ks == 3)
    conv1_fwd_kernel<3><<<static_cast<unsigned>(grid), kThreads, 0, stream>>>(x, w, bias, y, g);
  else
    conv1_fwd_kernel<5><<<static_cast<unsigned>(grid), kThreads, 0, stream>>>(x, w, bias, y, g);
  TONY_LAUNCH_CHECK();
  return 0;
}

// Workgroups of tony_conv1_bwd for a batch of N images = 32x32 partials it stores (a function of N alone).
TONY_API int tony_conv1_bwd_grid(int64_t N) {
  if (N < 1 || N >= (int64_t{1} << 31)) return 0;
  const int per = bwd_images(N);
  return static_cast<int>((N + per - 1) / per);
}

// partials[tony_conv1_bwd_grid(N)][32][32]: D[c][tap] = sum of dy' x over the workgroup's images, D[c][ks*ks] = sum dy'.
TONY_API int tony_conv1_bwd(const float* dy, const float* y, const float* x, float* partials, int64_t N, int H, int W,
                            int ks, int pad, hipStream_t stream) {
  if (dy == nullptr || y == nullptr || x == nullptr || partials == nullptr) return -1;
  Geo g;
  if (const int rc = make_geo(N, H, W, ks, pad, &g)) return rc;
  const int per = bwd_images(N), grid = tony_conv1_bwd_grid(N);
  if (ks == 3)
    conv1_bwd_kernel<3><<<grid, kThreads, 0, stream>>>(dy, y, x, partials, g, per);
  else
    conv1_bwd_kernel<5><<<grid, kThreads, 0, stream>>>(dy, y, x, partials, g, per);
  TONY_LAUNCH_CHECK();
  return 0;
}

// dw[32][ks*ks], db[32] from the G partials of tony_conv1_bwd, added in index order.
TONY_API int tony_conv1_fold(const float* partials, int G, int ks, float* dw, float* db, hipStream_t stream) {
  if (partials == nullptr || dw == nullptr || db == nullptr || G < 1) return -1;
  if (ks != 3 && ks != 5) return -2;
  conv1_fold_kernel<<<kCout * 32 / kThreads, kThreads, 0, stream>>>(partials, G, ks * ks, dw, db);
  TONY_LAUNCH_CHECK();
  return 0;
}
