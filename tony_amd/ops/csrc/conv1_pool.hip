// First layer of deepnn with its pooling, fp32: y = maxpool2x2(relu(b + conv(x, w))) with ONE input channel and 32
// output channels, k in {3, 5}, stride 1, padding 0 or (k - 1) / 2, floor pooling (an odd last conv row or column is
// never computed), and its weight / bias gradient.  The layer reads the image, so there is no data gradient.  Neither
// the full-resolution activation nor its gradient ever exists in memory: the forward writes the pooled y and a uint8
// idx (the window position 0..3 of the maximum, the first one in row-major order), the backward reads (dy, y, idx).
//
// Both directions are conv1.hip's products on v_mfma_f32_32x32x2_f32 (lane l, half h = l / 32: A[i = l % 32][k = h],
// B[k = h][j = l % 32], accumulator r of lane l is D[8 * (r / 4) + 4 * h + r % 4][l % 32]) with the bias as an extra K
// row against ones, here over POOLED pixels with one accumulator tile per window position (i, j).
//
// Tiles.  The pooled plane of one image is cut into bands of PR pooled rows by chunks of PCW pooled columns, PR * PCW
// <= kPoolPix = 128 (a 32-pixel MFMA tile for each of the four waves; rows and columns are spread evenly over the
// bands and chunks, so deepnn's 14x14 plane is two tiles of 7 rows = 98 pixels and all four waves of both work).  A
// workgroup stages the tile's input patch, (2 PR + k - 1) x (2 PCW + k - 1) floats, with the zero padding WRITTEN
// there, so no tap branches on the border.
//
//   forward   D(i,j)[channel][pooled pixel] = Wt[32 x K] . Xcol(i,j)[K x 32], K = k*k + 1 in K / 2 steps.  A lane keeps
//             its K / 2 weights (the last one of the upper half is the bias) in registers; column l of tile (i, j) is
//             conv pixel (2 ph + i, 2 pw + j) of pooled pixel l, so the four B operands are one patch address plus
//             0, 1, tw, tw + 1 and one A register feeds four MFMAs.  ReLU, the 2x2 maximum and its position are
//             elementwise over four registers of a lane; the 32 lanes of a half store contiguous floats (and bytes of
//             idx) of one pooled channel plane.
//   backward  D[channel][tap] = dY'[32 x L] . Xcol[L x K] over the L conv pixels, column k*k the sum of dY' (the bias
//             gradient).  dY' -- dy of the pooled pixel at the window position idx names unless y <= 0, 0 at the other
//             three positions and under a dropped odd row or column -- is formed in REGISTERS: dy, y and idx are read
//             coalesced (lanes along a pooled channel plane), dy masked by !(y <= 0) is laid in LDS as [channel][pooled
//             pixel] rows of odd stride with idx as bytes beside it (row stride 4 * 33: the lane-per-channel byte
//             reads hit 32 distinct banks too), and a step reads one (value, position) of two pooled pixels and issues
//             FOUR MFMAs, A = the value where the position matches and 0 elsewhere, B = the patch at the tap plus
//             0, 1, tw, tw + 1, into four accumulator tiles.  Against expanding dY' to the conv plane in LDS this
//             stages a quarter of the elements, reads A once for four MFMAs, and makes the four MFMAs of a step
//             independent of each other where conv1_bwd_kernel's are one dependent chain.  Skipping the three zero
//             positions altogether is not a matrix product: the position differs per channel, so B would depend on
//             the A row.  The order of additions depends on the shapes alone: a workgroup reduces a fixed run of
//             images (the grid is a function of N), wave w takes the pooled-pixel pairs w, w + 4, ... of every tile,
//             its four tiles are added in position order, the waves meet in LDS in wave order and ONE 32x32 partial
//             is stored.  tony_conv1_fold adds the partials in index order: no atomics, the same bits every run.
#include "common.h"

using namespace tony;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kCout = 32;
constexpr int kPoolPix = kWaves * 32;                    // pooled pixels of a tile, at most: 512 conv pixels
constexpr int kPatchFloats = 6 * (2 * kPoolPix + 4);     // (2 PR + k - 1) * (2 PCW + k - 1) at PR * PCW <= 128, k <= 5
constexpr int kDyStride = kPoolPix + 1;                  // odd: lanes along channels hit 32 distinct banks
constexpr int kIdxStride = 4 * 33;                       // bytes, >= kPoolPix: an odd number of banks a row
constexpr int kBwdImages = 2;                            // images of a backward workgroup's slice ...
constexpr int kBwdMaxGrid = 1024;                        // ... doubled and so on once N needs more workgroups than this

struct Geo {
  int N, H, W, PH, PW, pad;
  int PR, PCW, nb, nc;  // pooled rows of a band, pooled columns of a chunk, bands and chunks per image
  int64_t phw;
};

struct Tile {
  int r0, rb, c0, cw, npool;  // first pooled row / rows, first pooled column / columns, pooled pixels
};

__device__ __forceinline__ Tile tile_of(const Geo& g, int b, int c) {
  Tile t;
  t.r0 = b * g.PR;
  t.rb = min(g.PR, g.PH - t.r0);
  t.c0 = c * g.PCW;
  t.cw = min(g.PCW, g.PW - t.c0);
  t.npool = t.rb * t.cw;
  return t;
}

__device__ __forceinline__ f32x16 zero16() {
  return f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
}

// the tile's input patch, (2 rb + KS - 1) rows of tw = 2 cw + KS - 1 floats, zeros where the padding is
template <int KS>
__device__ __forceinline__ void stage_x(float* __restrict__ xt, const float* __restrict__ x, const Geo& g,
                                        const Tile& t, int n) {
  const int tw = 2 * t.cw + KS - 1, cnt = (2 * t.rb + KS - 1) * tw;
  const float* img = x + static_cast<int64_t>(n) * g.H * g.W;
  for (int i = threadIdx.x; i < cnt; i += kThreads) {
    const int row = i / tw, col = i - row * tw;
    const int ih = 2 * t.r0 + row - g.pad, iw = 2 * t.c0 + col - g.pad;
    xt[i] = (ih >= 0 && ih < g.H && iw >= 0 && iw < g.W) ? img[static_cast<int64_t>(ih) * g.W + iw] : 0.f;
  }
}

template <int KS>
__global__ __launch_bounds__(kThreads) void conv1_pool_fwd_kernel(const float* __restrict__ x,
                                                                  const float* __restrict__ w,
                                                                  const float* __restrict__ bias, float* __restrict__ y,
                                                                  uint8_t* __restrict__ idx, const Geo g) {
  constexpr int KK = KS * KS, STEPS = (KK + 1) / 2;
  __shared__ float xt[kPatchFloats];
  const int per = g.nb * g.nc;
  const int n = blockIdx.x / per, rem = blockIdx.x - n * per;
  const Tile t = tile_of(g, rem / g.nc, rem % g.nc);
  const int tw = 2 * t.cw + KS - 1;
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
  if (wave * 32 >= t.npool) return;  // per wave, past the only barrier
  const int q = wave * 32 + l32;
  const int qc = min(q, t.npool - 1);  // a lane past the tile computes its last pixel again and stores nothing
  const int row = qc / t.cw, col = qc - row * t.cw;
  const float* xp = xt + 2 * row * tw + 2 * col;
  f32x16 acc[4] = {zero16(), zero16(), zero16(), zero16()};
#pragma unroll
  for (int s = 0; s < STEPS; ++s) {
    const float* bp = xp + toff[s];
    float b0 = bp[0], b1 = bp[1], b2 = bp[tw], b3 = bp[tw + 1];
    if (s == STEPS - 1 && half) b0 = b1 = b2 = b3 = 1.f;
    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b0, acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b1, acc[1], 0, 0, 0);
    acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b2, acc[2], 0, 0, 0);
    acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b3, acc[3], 0, 0, 0);
  }
  if (q < t.npool) {
    const int64_t base = static_cast<int64_t>(n) * kCout * g.phw + static_cast<int64_t>(t.r0 + row) * g.PW + t.c0 + col;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t o = base + (8 * (r / 4) + 4 * half + r % 4) * g.phw;
      float best = relu_f(acc[0][r]);
      int bi = 0;
#pragma unroll
      for (int p = 1; p < 4; ++p) {  // a strict > keeps the first maximum; a NaN wins, as in torch
        const float v = relu_f(acc[p][r]);
        if (v > best || v != v) best = v, bi = p;
      }
      y[o] = best;
      idx[o] = static_cast<uint8_t>(bi);
    }
  }
}

template <int KS>
__global__ __launch_bounds__(kThreads) void conv1_pool_bwd_kernel(const float* __restrict__ dy,
                                                                  const float* __restrict__ y,
                                                                  const uint8_t* __restrict__ idx,
                                                                  const float* __restrict__ x,
                                                                  float* __restrict__ partials, const Geo g,
                                                                  const int images) {
  constexpr int KK = KS * KS;
  __shared__ float xt[kPatchFloats];
  __shared__ float dyt[kCout * kDyStride];       // [channel][pooled pixel]: y <= 0 ? 0 : dy
  __shared__ uint8_t post[kCout * kIdxStride];   // [channel][pooled pixel]: idx
  __shared__ int xoff[kPoolPix];                 // [pooled pixel]: patch offset of its window's first conv pixel
  static_assert(kCout * kDyStride >= kWaves * kCout * 32, "the waves' accumulators meet in the dy tile's LDS");
  static_assert(kIdxStride >= kPoolPix && kIdxStride % 4 == 0 && (kIdxStride / 4) % 2 == 1, "idx rows");
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int half = lane >> 5, l32 = lane & 31;
  const int kc = min(l32, KK - 1);  // this lane's column of D: tap l32, the ones column at KK, unused past it
  const int kh = kc / KS, kw = kc % KS;
  f32x16 acc[4] = {zero16(), zero16(), zero16(), zero16()};
  const int n0 = blockIdx.x * images, n1 = min(g.N, n0 + images);
  for (int n = n0; n < n1; ++n)
    for (int b = 0; b < g.nb; ++b)
      for (int c = 0; c < g.nc; ++c) {
        const Tile t = tile_of(g, b, c);
        const int tw = 2 * t.cw + KS - 1;
        __syncthreads();  // the previous tile's operand reads are done
        stage_x<KS>(xt, x, g, t, n);
        if (threadIdx.x < t.npool) {
          const int row = threadIdx.x / t.cw, col = threadIdx.x - row * t.cw;
          xoff[threadIdx.x] = 2 * row * tw + 2 * col;
        }
        // a wave stages 8 channel planes, its lanes along the pooled pixels
        for (int px = lane; px < t.npool; px += kWave) {
          const int row = px / t.cw, col = px - row * t.cw;
          const int64_t off = (static_cast<int64_t>(n) * kCout + wave * 8) * g.phw +
                              static_cast<int64_t>(t.r0 + row) * g.PW + t.c0 + col;
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const float d = dy[off + k * g.phw], v = y[off + k * g.phw];
            dyt[(wave * 8 + k) * kDyStride + px] = !(v <= 0.f) ? d : 0.f;  // threshold_backward: a NaN y passes dy
            post[(wave * 8 + k) * kIdxStride + px] = idx[off + k * g.phw];
          }
        }
        __syncthreads();
        const int toff = kh * tw + kw, pairs = (t.npool + 1) >> 1;
        for (int pr = wave; pr < pairs; pr += kWaves) {
          const int q = 2 * pr + half;
          const bool ok = q < t.npool;  // the odd pixel past a tile of odd size adds zeros
          const int qc = ok ? q : t.npool - 1;
          const float v = ok ? dyt[l32 * kDyStride + qc] : 0.f;
          const int p = post[l32 * kIdxStride + qc];
          const float* bp = xt + xoff[qc] + toff;
          float b0 = bp[0], b1 = bp[1], b2 = bp[tw], b3 = bp[tw + 1];
          if (l32 == KK) b0 = b1 = b2 = b3 = 1.f;
          if (!ok) b0 = b1 = b2 = b3 = 0.f;
          acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(p == 0 ? v : 0.f, b0, acc[0], 0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(p == 1 ? v : 0.f, b1, acc[1], 0, 0, 0);
          acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(p == 2 ? v : 0.f, b2, acc[2], 0, 0, 0);
          acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(p == 3 ? v : 0.f, b3, acc[3], 0, 0, 0);
        }
      }
  __syncthreads();
  float* red = dyt;  // [wave][channel][column]
#pragma unroll
  for (int r = 0; r < 16; ++r)
    red[(wave * kCout + 8 * (r / 4) + 4 * half + r % 4) * 32 + l32] = ((acc[0][r] + acc[1][r]) + acc[2][r]) + acc[3][r];
  __syncthreads();
  float* out = partials + static_cast<int64_t>(blockIdx.x) * (kCout * 32);
  for (int i = threadIdx.x; i < kCout * 32; i += kThreads) {
    float s = red[i];
#pragma unroll
    for (int wv = 1; wv < kWaves; ++wv) s += red[wv * kCout * 32 + i];
    out[i] = s;
  }
}

// Images per backward workgroup: kBwdImages until that needs more than kBwdMaxGrid workgroups.
inline int bwd_images(int64_t N) {
  const int64_t unit = static_cast<int64_t>(kBwdImages) * kBwdMaxGrid;
  return static_cast<int>(kBwdImages * ((N + unit - 1) / unit));
}

inline int imin(int a, int b) { return a < b ? a : b; }

// The supported form; fills g.  0, or the negative code of the first violated rule.
inline int make_geo(int64_t N, int H, int W, int ks, int pad, Geo* g) {
  if (ks != 3 && ks != 5) return -2;
  if (pad != 0 && pad != (ks - 1) / 2) return -3;
  if (N < 1 || H < ks || W < ks) return -4;
  const int64_t OH = static_cast<int64_t>(H) + 2 * pad - ks + 1, OW = static_cast<int64_t>(W) + 2 * pad - ks + 1;
  if (OH < 2 || OW < 2) return -4;
  if (N * OH * OW >= (int64_t{1} << 31)) return -5;
  g->N = static_cast<int>(N), g->H = H, g->W = W, g->pad = pad;
  g->PH = static_cast<int>(OH / 2), g->PW = static_cast<int>(OW / 2);
  g->phw = static_cast<int64_t>(g->PH) * g->PW;
  // as few chunks and bands as the tile allows, the columns and rows spread evenly over them
  g->nc = (g->PW + kPoolPix - 1) / kPoolPix;
  g->PCW = (g->PW + g->nc - 1) / g->nc;
  g->nb = (g->PH + imin(g->PH, kPoolPix / g->PCW) - 1) / imin(g->PH, kPoolPix / g->PCW);
  g->PR = (g->PH + g->nb - 1) / g->nb;
  if (g->PR * g->PCW > kPoolPix || (2 * g->PR + ks - 1) * (2 * g->PCW + ks - 1) > kPatchFloats) return -6;
  return 0;
}

}  // namespace

// y[N,32,OH/2,OW/2] = maxpool2x2(relu(bias + conv(x[N,1,H,W], w[32,1,ks,ks]))), idx the window position of each maximum
// (uint8, 0..3, the first in row-major order); contiguous fp32.
TONY_API int tony_conv1_pool_fwd(const float* x, const float* w, const float* bias, float* y, uint8_t* idx, int64_t N,
                                 int H, int W, int ks, int pad, hipStream_t stream) {
  if (x == nullptr || w == nullptr || bias == nullptr || y == nullptr || idx == nullptr) return -1;
  Geo g;
  if (const int rc = make_geo(N, H, W, ks, pad, &g)) return rc;
  const int64_t grid = N * g.nb * g.nc;  // <= N * PH * PW < 2^31
  if (ks == 3)
    conv1_pool_fwd_kernel<3><<<static_cast<unsigned>(grid), kThreads, 0, stream>>>(x, w, bias, y, idx, g);
  else
    conv1_pool_fwd_kernel<5><<<static_cast<unsigned>(grid), kThreads, 0, stream>>>(x, w, bias, y, idx, g);
  TONY_LAUNCH_CHECK();
  return 0;
}

// Workgroups of tony_conv1_pool_bwd for a batch of N images = 32x32 partials it stores (a function of N alone).
TONY_API int tony_conv1_pool_bwd_grid(int64_t N) {
  if (N < 1 || N >= (int64_t{1} << 31)) return 0;
  const int per = bwd_images(N);
  return static_cast<int>((N + per - 1) / per);
}

// partials[tony_conv1_pool_bwd_grid(N)][32][32] from the pooled dy, y and idx of tony_conv1_pool_fwd, in
// tony_conv1_bwd's layout (D[c][tap], D[c][ks*ks] = sum dy'): tony_conv1_fold folds them.
TONY_API int tony_conv1_pool_bwd(const float* dy, const float* y, const uint8_t* idx, const float* x, float* partials,
                                 int64_t N, int H, int W, int ks, int pad, hipStream_t stream) {
  if (dy == nullptr || y == nullptr || idx == nullptr || x == nullptr || partials == nullptr) return -1;
  Geo g;
  if (const int rc = make_geo(N, H, W, ks, pad, &g)) return rc;
  const int per = bwd_images(N), grid = tony_conv1_pool_bwd_grid(N);
  if (ks == 3)
    conv1_pool_bwd_kernel<3><<<grid, kThreads, 0, stream>>>(dy, y, idx, x, partials, g, per);
  else
    conv1_pool_bwd_kernel<5><<<grid, kThreads, 0, stream>>>(dy, y, idx, x, partials, g, per);
  TONY_LAUNCH_CHECK();
  return 0;
}
