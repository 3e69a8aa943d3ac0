// Second convolution of the MNIST CNNs, fp32: y = maxpool2x2(relu(b + conv(x, w))) with 32 input and 64 output
// channels, k in {3, 5}, stride 1, padding 0 or (k - 1) / 2, a padded plane at most 64 wide, and its data, weight and
// bias gradients.  Neither the full-resolution activation nor its gradient ever exists in memory: the forward writes
// the pooled y and a uint8 idx (the window position 0..3 of the maximum, the first one in row-major order), the
// backward expands (dy, y, idx) into dY' -- dy at position idx unless y <= 0, zeros elsewhere -- while staging it.
//
// All three products run on v_mfma_f32_32x32x2_f32 (lane l, half h = l / 32: A[i = l % 32][k = h], B[k = h][j = l % 32],
// accumulator r of lane l is D[8 * (r / 4) + 4 * h + r % 4][l % 32]), the im2col formed only in LDS addresses and the
// zero padding WRITTEN into LDS, so no tap branches.  K is walked in channel groups: a group's band of the plane and its
// weight panel are staged together, so LDS stays under 64 KB whatever the plane (several workgroups per CU) and needs
// no dynamic allocation.  Panels have an odd row stride: the lane-per-channel A reads hit 32 distinct banks.
//
//   forward  D[64 co][pixel] = Wt[64 x K] . Xcol[K x pixels], K = 32*k*k in groups of 8 (k = 3) or 4 (k = 5) input channels.  A
//            workgroup owns a band of whole POOLED rows of one image, at most 64 pooled pixels; wave w owns channels
//            32 * (w & 1) .. + 32 of pooled pixels 32 * (w >> 1) .. + 32 and keeps FOUR accumulator tiles, one per
//            window position (i, j): column l of tile (i, j) is conv pixel (2 ph + i, 2 pw + j) of pooled pixel l.  The
//            four B operands are one patch address plus 0, 1, tw, tw + 1; the A operand is read once for four MFMAs.
//            Bias, ReLU, the 2x2 maximum and its position are elementwise over four registers of a lane; the 32 lanes
//            of a half store contiguous floats (and bytes of idx) of one pooled channel plane.
//   dgrad    D[32 ci][input pixel] = Wf[32 x K] . dY'col[K x pixels], K = 64*k*k in groups of 8 output channels, Wf the
//            weights with their taps reversed.  A band of whole input rows, at most 256 pixels, two pixel tiles a wave.
//   wgrad    per tap, D[64 co][32 ci] = dY'[64 x L] . X(tap)[L x 32] reduced over the L conv pixels two per step: a
//            32 x 32 tile is (half of the output channels) x (all input channels) of ONE tap, so no column of a tile
//            is idle.  The grid is (image slice) x (kernel row kh); a workgroup stages a band of dY' as [co][pixel] and
//            the band of x shifted by kh as [ci][pixel] (odd strides), wave w takes the channels 32 * (w & 1) and the
//            pixel pairs of parity w >> 1, and holds the k tiles of its kernel row: one A read feeds k MFMAs.  The two
//            pixel parities meet in LDS in wave order and ONE partial [k taps][64][32] is stored; the workgroups of
//            kh == 0 also sum their dY' rows into a partial of db.  tony_conv2_fold adds the partials in index order:
//            no atomics, the same bits every run.
#include "common.h"

using namespace tony;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kThreads = 256;
constexpr int kCin = 32;
constexpr int kCout = 64;
constexpr int kMaxPlaneW = 64;     // W + 2 pad, at most: a band is whole rows, no column chunks
constexpr int kFwdPool = 64;       // pooled pixels of a forward band, at most (2 tiles x 2 channel halves = 4 waves)
constexpr int kFwdRows = 16;       // pooled rows of a forward band, at most
constexpr int kFwdPatch = 512;     // floats of a channel's forward patch: (2 rows + k - 1) * (2 PW + k - 1), at most
constexpr int kDgPix = 256;        // input pixels of a dgrad band, at most (2 tiles x 4 waves)
constexpr int kDgRows = 32;
constexpr int kDgPatch = 544;      // (rows + k - 1) * (W + k - 1), at most
constexpr int kDgCg = 8;           // output channels of a dgrad K group
constexpr int kWgPix = 128;        // conv pixels of a wgrad band, at most
constexpr int kWgRows = 16;
constexpr int kWgDyStride = kWgPix + 1;  // odd: lanes along channels hit 32 distinct banks
constexpr int kWgXStride = 193;          // odd, >= rows * (2 PW + k - 1)
constexpr int kWgImages = 2;       // images of a wgrad workgroup's slice ...
constexpr int kWgMaxSlices = 256;  // ... doubled and so on once N needs more slices than this
constexpr int kTile = kCout * kCin;  // floats of one tap's [co][ci] block of a partial

template <int KS>
struct FwdCfg {
  static constexpr int KK = KS * KS;
  static constexpr int CG = KS == 3 ? 8 : 4;  // input channels of a K group
  static constexpr int KG = CG * KK;          // K of a group (even)
  static constexpr int S = KG | 1;            // the panel's row stride
};

struct Geo {
  int N, H, W, pad, PH, PW;
  int fpr, fnb;  // forward: pooled rows of a band, bands per image
  int drb, dnb;  // dgrad: input rows of a band, bands per image
  int wrb, wnb;  // wgrad: conv rows of a band, bands per image
  int64_t phw, hw;
};

// NCH channel planes of x from ci0, rows row0 .. + nrows and columns col0 .. + ncols of the image (zeros outside it),
// as dst[c * chs + r * ncols + col]
template <int NCH>
__device__ __forceinline__ void stage_x(float* __restrict__ dst, int chs, const float* __restrict__ x, const Geo& g,
                                        int n, int ci0, int row0, int nrows, int col0, int ncols) {
  const int cnt = nrows * ncols;
  const float* img = x + (static_cast<int64_t>(n) * kCin + ci0) * g.hw;
  for (int i = threadIdx.x; i < NCH * cnt; i += kThreads) {
    const int c = i / cnt, e = i - c * cnt;
    const int r = e / ncols, col = e - r * ncols;
    const int ih = row0 + r, iw = col0 + col;
    dst[c * chs + e] =
        (ih >= 0 && ih < g.H && iw >= 0 && iw < g.W) ? img[c * g.hw + static_cast<int64_t>(ih) * g.W + iw] : 0.f;
  }
}

// NCO channel planes of dY' from co0, rows row0 .. + nrows and columns col0 .. + ncols of the CONV plane, as
// dst[c * chs + r * ncols + col]: dy of the pooled pixel at the window position idx names unless y <= 0 (0 at relu ==
// 0, dy at a NaN y), zeros at the other three positions, under an odd last row / column and outside the plane
template <int NCO>
__device__ __forceinline__ void stage_dyx(float* __restrict__ dst, int chs, const float* __restrict__ dy,
                                          const float* __restrict__ y, const uint8_t* __restrict__ idx, const Geo& g,
                                          int n, int co0, int row0, int nrows, int col0, int ncols) {
  const int cnt = nrows * ncols;
  const int64_t base = (static_cast<int64_t>(n) * kCout + co0) * g.phw;
  for (int i = threadIdx.x; i < NCO * cnt; i += kThreads) {
    const int c = i / cnt, e = i - c * cnt;
    const int r = e / ncols, col = e - r * ncols;
    const int oh = row0 + r, ow = col0 + col;
    float v = 0.f;
    if (oh >= 0 && oh < 2 * g.PH && ow >= 0 && ow < 2 * g.PW) {
      const int64_t off = base + c * g.phw + static_cast<int64_t>(oh >> 1) * g.PW + (ow >> 1);
      if (idx[off] == 2 * (oh & 1) + (ow & 1) && !(y[off] <= 0.f)) v = dy[off];  // threshold_backward: NaN passes
    }
    dst[c * chs + e] = v;
  }
}

// LDS offset of K index kk = channel * k*k + tap of a group's patch (kk is a constant once the K loop is unrolled)
template <int KS>
__device__ __forceinline__ int tap_off(int kk, int chs, int tw) {
  const int c = kk / (KS * KS), t = kk - c * (KS * KS);
  return c * chs + (t / KS) * tw + t % KS;
}

__device__ __forceinline__ f32x16 zero16() {
  return f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
}

template <int KS>
__global__ __launch_bounds__(kThreads) void conv2_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                             const float* __restrict__ bias, float* __restrict__ y,
                                                             uint8_t* __restrict__ idx, const Geo g) {
  using C = FwdCfg<KS>;
  constexpr int KK = C::KK, CG = C::CG, KG = C::KG, S = C::S, STEPS = KG / 2;
  __shared__ float xt[CG * kFwdPatch];
  __shared__ float wt[kCout * S];
  const int n = blockIdx.x / g.fnb, b = blockIdx.x - n * g.fnb;
  const int pr0 = b * g.fpr, prb = min(g.fpr, g.PH - pr0), npool = prb * g.PW;
  const int tw = 2 * g.PW + KS - 1, nrows = 2 * prb + KS - 1, chs = nrows * tw;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int half = lane >> 5, l32 = lane & 31;
  const int chalf = wave & 1, ptile = wave >> 1;
  const int q = ptile * 32 + l32;
  const int qc = min(q, npool - 1);  // a lane past the band computes its last pixel again and stores nothing
  const int prow = qc / g.PW, pcol = qc - prow * g.PW;
  const bool active = ptile * 32 < npool;  // per wave
  const float* xp = xt + 2 * prow * tw + 2 * pcol;
  const float* ap = wt + (chalf * 32 + l32) * S + half;
  f32x16 acc[4] = {zero16(), zero16(), zero16(), zero16()};
  for (int cg = 0; cg < kCin / CG; ++cg) {
    __syncthreads();  // the previous group's operand reads are done
    stage_x<CG>(xt, chs, x, g, n, cg * CG, 2 * pr0 - g.pad, nrows, -g.pad, tw);
    for (int i = threadIdx.x; i < kCout * KG; i += kThreads) {  // a channel's KG weights of the group are contiguous
      const int co = i / KG, j = i - co * KG;
      wt[co * S + j] = w[(co * kCin + cg * CG) * KK + j];
    }
    __syncthreads();
    if (active) {
#pragma unroll
      for (int s = 0; s < STEPS; ++s) {
        const float* bp = xp + (half ? tap_off<KS>(2 * s + 1, chs, tw) : tap_off<KS>(2 * s, chs, tw));
        const float a = ap[2 * s];
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[0], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[1], acc[1], 0, 0, 0);
        acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[tw], acc[2], 0, 0, 0);
        acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[tw + 1], acc[3], 0, 0, 0);
      }
    }
  }
  if (active && q < npool) {
    const int64_t base = (static_cast<int64_t>(n) * kCout + chalf * 32) * g.phw + static_cast<int64_t>(pr0) * g.PW + qc;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = 8 * (r / 4) + 4 * half + r % 4;
      const float bv = bias[chalf * 32 + c];
      float best = relu_f(acc[0][r] + bv);
      int bi = 0;
#pragma unroll
      for (int p = 1; p < 4; ++p) {  // a strict > keeps the first maximum; a NaN wins, as in torch
        const float v = relu_f(acc[p][r] + bv);
        if (v > best || v != v) best = v, bi = p;
      }
      y[base + c * g.phw] = best;
      idx[base + c * g.phw] = static_cast<uint8_t>(bi);
    }
  }
}

template <int KS>
__global__ __launch_bounds__(kThreads) void conv2_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                               const uint8_t* __restrict__ idx,
                                                               const float* __restrict__ w, float* __restrict__ dx,
                                                               const Geo g) {
  constexpr int KK = KS * KS, CG = kDgCg, KG = CG * KK, S = KG | 1, STEPS = KG / 2;
  __shared__ float dt[CG * kDgPatch];
  __shared__ float wt[kCin * S];
  const int n = blockIdx.x / g.dnb, b = blockIdx.x - n * g.dnb;
  const int r0 = b * g.drb, rb = min(g.drb, g.H - r0), npix = rb * g.W;
  const int tw = g.W + KS - 1, nrows = rb + KS - 1, chs = nrows * tw;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int half = lane >> 5, l32 = lane & 31;
  int q[2], qc[2], xoff[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    q[j] = (2 * wave + j) * 32 + l32;
    qc[j] = min(q[j], npix - 1);
    const int row = qc[j] / g.W;
    xoff[j] = row * tw + (qc[j] - row * g.W);
  }
  const bool active = 2 * wave * 32 < npix;  // per wave
  const float* ap = wt + l32 * S + half;
  f32x16 acc[2] = {zero16(), zero16()};
  for (int cg = 0; cg < kCout / CG; ++cg) {
    __syncthreads();
    // dX[ih][iw] = sum over taps of w[kh][kw] dY'[ih + pad - kh][iw + pad - kw]: a correlation of dY', its halo of
    // k - 1 - pad zeros staged, with the reversed taps
    stage_dyx<CG>(dt, chs, dy, y, idx, g, n, cg * CG, r0 + g.pad - (KS - 1), nrows, g.pad - (KS - 1), tw);
    for (int i = threadIdx.x; i < CG * kCin * KK; i += kThreads) {  // [co of the group, reversed tap] x [ci]
      const int c = i / (kCin * KK), rem = i - c * (kCin * KK);
      const int ci = rem / KK, t = rem - ci * KK;
      wt[ci * S + c * KK + (KK - 1 - t)] = w[static_cast<int64_t>(cg * CG + c) * (kCin * KK) + rem];
    }
    __syncthreads();
    if (active) {
#pragma unroll
      for (int s = 0; s < STEPS; ++s) {
        const int off = half ? tap_off<KS>(2 * s + 1, chs, tw) : tap_off<KS>(2 * s, chs, tw);
        const float a = ap[2 * s];
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, dt[xoff[0] + off], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, dt[xoff[1] + off], acc[1], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j)
    if (active && q[j] < npix) {
      float* out = dx + static_cast<int64_t>(n) * kCin * g.hw + static_cast<int64_t>(r0) * g.W + qc[j];
#pragma unroll
      for (int r = 0; r < 16; ++r) out[(8 * (r / 4) + 4 * half + r % 4) * g.hw] = acc[j][r];
    }
}

template <int KS>
__global__ __launch_bounds__(kThreads) void conv2_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                               const uint8_t* __restrict__ idx,
                                                               const float* __restrict__ x, float* __restrict__ partials,
                                                               const Geo g, const int images) {
  constexpr int KK = KS * KS;
  __shared__ float sm[kCout * kWgDyStride + kCin * kWgXStride];
  static_assert(kCout * kWgDyStride + kCin * kWgXStride >= 2 * KS * 16 * kWave, "the wave pairs meet in this LDS");
  float* dyt = sm;                        // [co][pixel of the band]
  float* xt = sm + kCout * kWgDyStride;   // [ci][pixel of the band shifted by kh, k - 1 columns wider]
  const int slice = blockIdx.x, kh = blockIdx.y;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int half = lane >> 5, l32 = lane & 31;
  const int chalf = wave & 1, parity = wave >> 1;
  const int owe = 2 * g.PW, ohe = 2 * g.PH, tw = owe + KS - 1;  // the last row / column of an odd plane has dY' = 0
  f32x16 acc[KS];
#pragma unroll
  for (int k = 0; k < KS; ++k) acc[k] = zero16();
  float dbs = 0.f;
  const int n0 = slice * images, n1 = min(g.N, n0 + images);
  for (int n = n0; n < n1; ++n)
    for (int b = 0; b < g.wnb; ++b) {
      const int r0 = b * g.wrb, rb = min(g.wrb, ohe - r0), npix = rb * owe;
      __syncthreads();  // the previous band's operand reads are done
      stage_dyx<kCout>(dyt, kWgDyStride, dy, y, idx, g, n, 0, r0, rb, 0, owe);
      stage_x<kCin>(xt, kWgXStride, x, g, n, 0, r0 + kh - g.pad, rb, -g.pad, tw);
      __syncthreads();
      if (kh == 0 && threadIdx.x < kCout)
        for (int i = 0; i < npix; ++i) dbs += dyt[threadIdx.x * kWgDyStride + i];
      const float* ap = dyt + (chalf * 32 + l32) * kWgDyStride + half;
      const float* bp = xt + l32 * kWgXStride + half;
      for (int s = parity; s < rb * g.PW; s += 2) {  // a row of the even width owe is PW pixel pairs
        const int row = s / g.PW, pc = s - row * g.PW;
        const float a = ap[row * owe + 2 * pc];
        const float* xp = bp + row * tw + 2 * pc;
#pragma unroll
        for (int k = 0; k < KS; ++k) acc[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, xp[k], acc[k], 0, 0, 0);
      }
    }
  __syncthreads();
  float* red = sm;  // [channel half][kw][r][lane]
  if (parity == 1) {
#pragma unroll
    for (int k = 0; k < KS; ++k)
#pragma unroll
      for (int r = 0; r < 16; ++r) red[((chalf * KS + k) * 16 + r) * kWave + lane] = acc[k][r];
  }
  __syncthreads();
  if (parity == 0) {
    float* out = partials + (static_cast<int64_t>(slice) * KK + kh * KS) * kTile + chalf * 32 * kCin + l32;
#pragma unroll
    for (int k = 0; k < KS; ++k)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        out[k * kTile + (8 * (r / 4) + 4 * half + r % 4) * kCin] =
            acc[k][r] + red[((chalf * KS + k) * 16 + r) * kWave + lane];
  }
  if (kh == 0 && threadIdx.x < kCout)
    partials[static_cast<int64_t>(gridDim.x) * KK * kTile + slice * kCout + threadIdx.x] = dbs;
}

// dW[co][ci][tap] and db[co] = the sums over the G partials [tap][co][ci] and, behind them, [co], in index order
__global__ __launch_bounds__(kThreads) void conv2_fold_kernel(const float* __restrict__ partials, int G, int kk,
                                                              float* __restrict__ dw, float* __restrict__ db) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const int nw = kk * kTile;
  if (i >= nw + kCout) return;
  const float* src = i < nw ? partials + i : partials + static_cast<int64_t>(G) * nw + (i - nw);
  const int64_t stride = i < nw ? nw : kCout;
  float s = 0.f;
#pragma unroll 4
  for (int gi = 0; gi < G; ++gi) s += src[gi * stride];
  if (i < nw)
    dw[(i % kTile) * kk + i / kTile] = s;
  else
    db[i - nw] = s;
}

// Images per wgrad workgroup: kWgImages until that needs more than kWgMaxSlices slices.
inline int wg_images(int64_t N) {
  const int64_t unit = static_cast<int64_t>(kWgImages) * kWgMaxSlices;
  return static_cast<int>(kWgImages * ((N + unit - 1) / unit));
}

inline int imin(int a, int b) { return a < b ? a : b; }
inline int imax(int a, int b) { return a > b ? a : b; }

// The supported form; fills g.  0, or the negative code of the first violated rule.
inline int make_geo(int64_t N, int H, int W, int ks, int pad, Geo* g) {
  if (ks != 3 && ks != 5) return -2;
  if (pad != 0 && pad != (ks - 1) / 2) return -3;
  if (N < 1 || H < 1 || W < 1 || W + 2 * pad > kMaxPlaneW) return -4;
  const int64_t OH = static_cast<int64_t>(H) + 2 * pad - ks + 1, OW = static_cast<int64_t>(W) + 2 * pad - ks + 1;
  if (OH < 2 || OW < 2) return -4;
  if (N * kCout * OH * OW >= (int64_t{1} << 31)) return -5;
  g->N = static_cast<int>(N), g->H = H, g->W = W, g->pad = pad;
  g->PH = static_cast<int>(OH / 2), g->PW = static_cast<int>(OW / 2);
  g->phw = static_cast<int64_t>(g->PH) * g->PW, g->hw = static_cast<int64_t>(H) * W;
  g->fpr = imin(g->PH, imin(kFwdRows, imax(1, kFwdPool / g->PW)));
  g->fnb = (g->PH + g->fpr - 1) / g->fpr;
  g->drb = imin(H, imin(kDgRows, imax(1, kDgPix / W)));
  g->dnb = (H + g->drb - 1) / g->drb;
  g->wrb = imin(2 * g->PH, imin(kWgRows, imax(1, kWgPix / (2 * g->PW))));
  g->wnb = (2 * g->PH + g->wrb - 1) / g->wrb;
  const int tw = 2 * g->PW + ks - 1;
  if (g->fpr * g->PW > kFwdPool || (2 * g->fpr + ks - 1) * tw > kFwdPatch) return -6;
  if (g->drb * W > kDgPix || (g->drb + ks - 1) * (W + ks - 1) > kDgPatch) return -6;
  if (g->wrb * 2 * g->PW > kWgPix || g->wrb * tw > kWgXStride) return -6;
  return 0;
}

}  // namespace

// y[N,64,OH/2,OW/2] = maxpool2x2(relu(bias + conv(x[N,32,H,W], w[64,32,ks,ks]))), idx the window position of each
// maximum (uint8, 0..3, the first in row-major order); contiguous fp32.
TONY_API int tony_conv2_fwd(const float* x, const float* w, const float* bias, float* y, uint8_t* idx, int64_t N, int H,
                            int W, int ks, int pad, hipStream_t stream) {
  if (x == nullptr || w == nullptr || bias == nullptr || y == nullptr || idx == nullptr) return -1;
  Geo g;
  if (const int rc = make_geo(N, H, W, ks, pad, &g)) return rc;
  const unsigned grid = static_cast<unsigned>(N * g.fnb);  // <= N * OH < 2^31
  if (ks == 3)
    conv2_fwd_kernel<3><<<grid, kThreads, 0, stream>>>(x, w, bias, y, idx, g);
  else
    conv2_fwd_kernel<5><<<grid, kThreads, 0, stream>>>(x, w, bias, y, idx, g);
  TONY_LAUNCH_CHECK();
  return 0;
}

// dx[N,32,H,W] from the pooled dy, y and idx of tony_conv2_fwd.
TONY_API int tony_conv2_dgrad(const float* dy, const float* y, const uint8_t* idx, const float* w, float* dx, int64_t N,
                              int H, int W, int ks, int pad, hipStream_t stream) {
  if (dy == nullptr || y == nullptr || idx == nullptr || w == nullptr || dx == nullptr) return -1;
  Geo g;
  if (const int rc = make_geo(N, H, W, ks, pad, &g)) return rc;
  if (N * g.dnb >= (int64_t{1} << 31)) return -5;
  const unsigned grid = static_cast<unsigned>(N * g.dnb);
  if (ks == 3)
    conv2_dgrad_kernel<3><<<grid, kThreads, 0, stream>>>(dy, y, idx, w, dx, g);
  else
    conv2_dgrad_kernel<5><<<grid, kThreads, 0, stream>>>(dy, y, idx, w, dx, g);
  TONY_LAUNCH_CHECK();
  return 0;
}

// Image slices of tony_conv2_wgrad for a batch of N images (a function of N alone); its partials hold
// slices * (ks*ks * 64 * 32 + 64) floats.
TONY_API int tony_conv2_wgrad_grid(int64_t N) {
  if (N < 1 || N >= (int64_t{1} << 31)) return 0;
  const int per = wg_images(N);
  return static_cast<int>((N + per - 1) / per);
}

// partials: [slice][tap][64][32] sums of dy' x over the slice's images, then [slice][64] sums of dy'.
TONY_API int tony_conv2_wgrad(const float* dy, const float* y, const uint8_t* idx, const float* x, float* partials,
                              int64_t N, int H, int W, int ks, int pad, hipStream_t stream) {
  if (dy == nullptr || y == nullptr || idx == nullptr || x == nullptr || partials == nullptr) return -1;
  Geo g;
  if (const int rc = make_geo(N, H, W, ks, pad, &g)) return rc;
  const int per = wg_images(N);
  const dim3 grid(tony_conv2_wgrad_grid(N), ks);
  if (ks == 3)
    conv2_wgrad_kernel<3><<<grid, kThreads, 0, stream>>>(dy, y, idx, x, partials, g, per);
  else
    conv2_wgrad_kernel<5><<<grid, kThreads, 0, stream>>>(dy, y, idx, x, partials, g, per);
  TONY_LAUNCH_CHECK();
  return 0;
}

// dw[64][32][ks*ks], db[64] from the G slices of tony_conv2_wgrad, added in index order.
TONY_API int tony_conv2_fold(const float* partials, int G, int ks, float* dw, float* db, hipStream_t stream) {
  if (partials == nullptr || dw == nullptr || db == nullptr || G < 1) return -1;
  if (ks != 3 && ks != 5) return -2;
  const int total = ks * ks * kTile + kCout;
  conv2_fold_kernel<<<(total + kThreads - 1) / kThreads, kThreads, 0, stream>>>(partials, G, ks * ks, dw, db);
  TONY_LAUNCH_CHECK();
  return 0;
}
