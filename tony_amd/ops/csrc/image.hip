// Image input pipeline: one launch turns a uint8 NHWC batch into the model's input.
//
//   out[n, oy, ox, c] = bilinear(crop_n(src))[oy, ox(, flipped), c] * scale[c] + bias[c]
//
// `boxes` is a device int32 table [N, 5] of (y0, x0, h, w, flip): every sample has its own crop box, which is
// why the stock composition needs a Python loop over samples.  The output [N, OH, OW, 3] (the memory of a
// channels_last [N, 3, OH, OW] tensor) is treated as ONE flat array of N*OH*OW*3 elements; each lane produces
// 8 consecutive elements and stores them as one 16-byte vector (bf16) or two (fp32).  299*3 and 299*299*3 are
// odd, so a group of 8 may straddle a row and a sample: (n, oy, ox, c) is decoded once per group and then
// stepped pixel by pixel over the four pixels the group can touch.
//
// Sample positions are exact rationals (torch's bilinear, align_corners=False, antialias=False on the crop):
//   num = max((2*o+1)*len - O, 0);  i0 = num / (2*O);  l = float(num % (2*O)) / float(2*O);  i1 = min(i0+1, len-1)
// A float coordinate near 2^11 already carries a 2^-12 error, which shows at bf16.  H, W, OH, OW <= 4096 keeps
// (2*o+1)*len inside int32.  Neighbours clamp to the crop box; every source row / column formed is clamped into
// the image as well, and the box is clamped on load, so no table can make the kernel read outside `src`.
#include "common.h"

using namespace tony;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxDim = 4096;
constexpr int kDivShift = 38;

struct Norm3 {
  float s[3], b[3];
};

// n / d for 0 <= n < 2^25 and 2 <= d <= 2^13 as one 64-bit multiply: m = ceil(2^38 / d) = (2^38 + e) / d with
// 0 <= e < d, so n * m / 2^38 = n / d + n * e / (d * 2^38), and n * e < 2^38 keeps the excess under 1 / d: the
// floor is exact.  ((2 * 4095 + 1) * 4096 < 2^25 and 2 * 4096 = 2^13: the host's size limits.)
struct Div {
  uint64_t m;
  int d;
  __device__ __forceinline__ int quot(int n) const {
    return static_cast<int>((static_cast<uint64_t>(static_cast<uint32_t>(n)) * m) >> kDivShift);
  }
};

struct Box {  // one row of the table, clamped into the image
  int y0, x0, h, w, flip;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ Box load_box(const int* __restrict__ boxes, int n, int H, int W) {
  const int* bx = boxes + static_cast<int64_t>(n) * 5;
  return Box{clampi(bx[0], 0, H - 1), clampi(bx[1], 0, W - 1), clampi(bx[2], 1, H), clampi(bx[3], 1, W), bx[4]};
}

__device__ __forceinline__ void put(uint16_t* p, float v) { *p = f2bf(v); }
__device__ __forceinline__ void put(float* p, float v) { *p = v; }

// Eight consecutive elements starting at channel c0 of pixel pix0 lie in pixels pix0 .. pix0+3: the lane samples
// those four pixels in uniform control flow (no branch on c0, so the lanes of a wave, whose c0 differ, stay
// together and the 40 byte loads are issued back to back), computes the ten values v[3k + c] that any c0 can ask
// for, and picks its eight.
template <class T>
__global__ __launch_bounds__(kThreads) void image_preprocess_kernel(const uint8_t* __restrict__ src,
                                                                    const int* __restrict__ boxes,
                                                                    T* __restrict__ out, int H, int W, int OH, int OW,
                                                                    int total, Div dy, Div dx, Norm3 nm) {
  const int64_t base = (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x) * 8;
  if (base >= total) return;
  const int npix = total / 3;
  const int pix0 = static_cast<int>(base / 3);
  const int c0 = static_cast<int>(base) - pix0 * 3;
  int n = pix0 / (OH * OW);
  const int r = pix0 - n * OH * OW;
  int oy = r / OW, ox = r - oy * OW;
  Box bx = load_box(boxes, n, H, W);
  float v[12];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    // (a pixel past the end of the batch -- n == N -- is not formed: the lane samples its last pixel again)
    if (k > 0 && pix0 + k < npix) {
      if (++ox == OW) {
        ox = 0;
        if (++oy == OH) {
          oy = 0;
          bx = load_box(boxes, ++n, H, W);
        }
      }
    }
    const int sx = bx.flip ? OW - 1 - ox : ox;
    const int ny = max((2 * oy + 1) * bx.h - OH, 0), nx = max((2 * sx + 1) * bx.w - OW, 0);
    const int iy0 = dy.quot(ny), ix0 = dx.quot(nx);
    const float ly = static_cast<float>(ny - iy0 * dy.d) / static_cast<float>(dy.d);
    const float lx = static_cast<float>(nx - ix0 * dx.d) / static_cast<float>(dx.d);
    const int iy1 = min(iy0 + 1, bx.h - 1), ix1 = min(ix0 + 1, bx.w - 1);
    const int r0 = min(bx.y0 + iy0, H - 1), r1 = min(bx.y0 + iy1, H - 1);
    const int q0 = min(bx.x0 + ix0, W - 1), q1 = min(bx.x0 + ix1, W - 1);
    const uint8_t* img = src + static_cast<int64_t>(n) * H * W * 3;
    const uint8_t *p00 = img + (r0 * W + q0) * 3, *p01 = img + (r0 * W + q1) * 3;
    const uint8_t *p10 = img + (r1 * W + q0) * 3, *p11 = img + (r1 * W + q1) * 3;
#pragma unroll
    for (int c = 0; c < (k < 3 ? 3 : 1); ++c) {
      const float a = p00[c], b = p01[c], cc = p10[c], d = p11[c];
      const float top = fmaf(lx, b - a, a);
      const float bot = fmaf(lx, d - cc, cc);
      v[3 * k + c] = fmaf(fmaf(ly, bot - top, top), nm.s[c], nm.b[c]);
    }
  }
  float f[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = c0 == 0 ? v[j] : (c0 == 1 ? v[j + 1] : v[j + 2]);
  if (base + 8 <= total) {
    V8<T>::from_float(f).store(out + base);
  } else {  // the scalar tail of the flat array
    const int count = static_cast<int>(total - base);
    for (int j = 0; j < count; ++j) put(out + base + j, f[j]);
  }
}

Div make_div(int d) { return Div{((uint64_t{1} << kDivShift) + d - 1) / d, d}; }

// -- colour distortion (Inception's training recipe) -------------------------------------------------------
// `colour` is a device float32 table [N, 5] of (order, brightness delta, saturation factor, hue delta, contrast
// factor) beside the box table.  A sample whose order is 0..5 computes u = v / 255 from the bilinear value v,
// applies its ops in its order, clips to [0, 1] and writes u * (255 * scale[c]) + bias[c]; any other order
// (-1, a fraction, a NaN) writes fmaf(v, scale[c], bias[c]) exactly as image_preprocess_kernel does.  With
// M = max, m = min, R = M - m of a pixel, its hue sextant coordinate h6 in [0, 6) and the channel weights
// d_r = clamp(|h6-3| - 1, 0, 1), d_g = clamp(2 - |h6-2|, 0, 1), d_b = clamp(2 - |h6-4|, 0, 1):
//   brightness(d)  x_c + d
//   saturation(f)  R' = max(0, min(R*f, M));  (M - R') + R' * d_c(h6)
//   hue(d)         h6' = (h6 + 6*d) mod 6;  m + R * d_c(h6')
//   contrast(f)    (x_c - mean_c) * f + mean_c, mean_c over the sample's OH x OW pixels of the value entering it
// (the RGB -> HSV -> RGB formulas on [0, 1], continuous everywhere: no rounding error can flip a branch into a
// different value).  Three launches on one stream when the table may hold contrast: image_colour_stats_kernel
// (per-workgroup partial sums of the pre-contrast values, summed in double and STORED, a fixed grid, so the
// means do not depend on arrival order), image_colour_fold_kernel (the partials of a sample in index order ->
// its three means) and image_colour_kernel; the last alone otherwise.  The table only selects arithmetic: memory
// is indexed by the (clamped) box table and the grid alone.
constexpr int kStatBlocks = 64;  // at most this many partial sums per sample and channel

enum : uint32_t { kEnd = 0, kBright = 1, kSat = 2, kHue = 3, kContrast = 4 };

struct Colour {
  int order;
  float db, fs, dh, fc;
};

struct Scale3 {
  float k[3];
};

__device__ __forceinline__ Colour load_colour(const float* __restrict__ colour, int n) {
  const float* t = colour + static_cast<int64_t>(n) * 5;
  const float o = t[0];  // (a NaN fails both comparisons)
  return Colour{(o >= 0.f && o <= 5.f && o == floorf(o)) ? static_cast<int>(o) : -1, t[1], t[2], t[3], t[4]};
}

// The ops of an order, first op in the low 4 bits: 0 bshc, 1 sbch, 2 chbs, 3 hscb, 4 bs, 5 sb.
__device__ __forceinline__ uint32_t colour_seq(int order) {
  constexpr uint64_t kFull = 0x1423213434124321ull;
  constexpr uint32_t kFast = 0x00120021u;
  if (order < 0) return 0u;
  return order < 4 ? static_cast<uint32_t>(kFull >> (16 * order)) & 0xffffu : (kFast >> (16 * (order - 4))) & 0xffffu;
}

__device__ __forceinline__ bool has_contrast(int order) { return order >= 0 && order <= 3; }

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

__device__ __forceinline__ float hue6(const float* x, float M, float R) {
  const float num = M == x[0] ? x[1] - x[2] : (M == x[1] ? x[2] - x[0] : x[0] - x[1]);
  const float off = M == x[0] ? 0.f : (M == x[1] ? 2.f : 4.f);
  float h = num / R + off;
  h = h < 0.f ? h + 6.f : h;
  return R == 0.f ? 0.f : h;
}

__device__ __forceinline__ void hue_weights(float h, float* d) {
  d[0] = clamp01(fabsf(h - 3.f) - 1.f);
  d[1] = clamp01(2.f - fabsf(h - 2.f));
  d[2] = clamp01(2.f - fabsf(h - 4.f));
}

// The ops of `seq` on one pixel x (in [0, 1] units).  Both passes call this one function: with
// stop_at_contrast the statistics pass gets the value that enters the contrast stage, and the apply pass, given
// the means of those values, goes on from the same arithmetic.
__device__ __forceinline__ void colour_ops(float* x, uint32_t seq, const Colour& cl, const float* mean,
                                           bool stop_at_contrast) {
#pragma unroll 1
  for (; seq != kEnd; seq >>= 4) {
    const uint32_t op = seq & 15u;
    if (op == kBright) {
#pragma unroll
      for (int c = 0; c < 3; ++c) x[c] += cl.db;
    } else if (op == kContrast) {
      if (stop_at_contrast) return;
#pragma unroll
      for (int c = 0; c < 3; ++c) x[c] = fmaf(x[c] - mean[c], cl.fc, mean[c]);
    } else {
      const float M = fmaxf(x[0], fmaxf(x[1], x[2])), m = fminf(x[0], fminf(x[1], x[2]));
      const float R = M - m;
      float h = hue6(x, M, R), d[3];
      if (op == kSat) {
        const float rp = fmaxf(0.f, fminf(R * cl.fs, M)), base = M - rp;
        hue_weights(h, d);
#pragma unroll
        for (int c = 0; c < 3; ++c) x[c] = fmaf(rp, d[c], base);
      } else {
        h = fmaf(6.f, cl.dh, h);
        h -= 6.f * floorf(h * (1.f / 6.f));
        h = h >= 6.f ? h - 6.f : (h < 0.f ? h + 6.f : h);
        hue_weights(h, d);
#pragma unroll
        for (int c = 0; c < 3; ++c) x[c] = fmaf(R, d[c], m);
      }
    }
  }
}

// The bilinear value v[0..3) in [0, 255] of output pixel (oy, ox) of sample n: image_preprocess_kernel's
// arithmetic, expression for expression.
__device__ __forceinline__ void sample_pixel(const uint8_t* __restrict__ src, int n, const Box& bx, int oy, int ox,
                                             int H, int W, int OH, int OW, const Div& dy, const Div& dx, float* v) {
  const int sx = bx.flip ? OW - 1 - ox : ox;
  const int ny = max((2 * oy + 1) * bx.h - OH, 0), nx = max((2 * sx + 1) * bx.w - OW, 0);
  const int iy0 = dy.quot(ny), ix0 = dx.quot(nx);
  const float ly = static_cast<float>(ny - iy0 * dy.d) / static_cast<float>(dy.d);
  const float lx = static_cast<float>(nx - ix0 * dx.d) / static_cast<float>(dx.d);
  const int iy1 = min(iy0 + 1, bx.h - 1), ix1 = min(ix0 + 1, bx.w - 1);
  const int r0 = min(bx.y0 + iy0, H - 1), r1 = min(bx.y0 + iy1, H - 1);
  const int q0 = min(bx.x0 + ix0, W - 1), q1 = min(bx.x0 + ix1, W - 1);
  const uint8_t* img = src + static_cast<int64_t>(n) * H * W * 3;
  const uint8_t *p00 = img + (r0 * W + q0) * 3, *p01 = img + (r0 * W + q1) * 3;
  const uint8_t *p10 = img + (r1 * W + q0) * 3, *p11 = img + (r1 * W + q1) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float a = p00[c], b = p01[c], cc = p10[c], d = p11[c];
    const float top = fmaf(lx, b - a, a);
    const float bot = fmaf(lx, d - cc, cc);
    v[c] = fmaf(ly, bot - top, top);
  }
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// Workgroup j of sample n (blockIdx.x = n * B + j) sums the pre-contrast values of pixels j*256 + t, + B*256, ...
// of that sample and stores partials[(n * B + j) * 3 + c].  A sample without contrast leaves at once.  Two pixels
// per trip, so that the byte loads of both are in flight together (a pixel past the sample's end is formed as its
// last pixel and not added); OH * OW < 2^25 and OW <= 2^13: Div's range (OW == 1: m = 2^38, the quotient is n).
__global__ __launch_bounds__(kThreads) void image_colour_stats_kernel(const uint8_t* __restrict__ src,
                                                                      const int* __restrict__ boxes,
                                                                      const float* __restrict__ colour,
                                                                      float* __restrict__ partials, int H, int W,
                                                                      int OH, int OW, int B, Div dy, Div dx, Div dw) {
  __shared__ double part[kThreads / kWave][3];
  const int n = blockIdx.x / B, j = blockIdx.x - n * B;
  const Colour cl = load_colour(colour, n);
  if (!has_contrast(cl.order)) return;  // the same in every lane
  const uint32_t seq = colour_seq(cl.order);
  const Box bx = load_box(boxes, n, H, W);
  const int P = OH * OW;
  double acc[3] = {0.0, 0.0, 0.0};
  const int stride = B * kThreads;
  for (int p0 = j * kThreads + threadIdx.x; p0 < P; p0 += 2 * stride) {
    float x[2][3];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int p = min(p0 + u * stride, P - 1);
      const int oy = dw.quot(p), ox = p - oy * OW;
      sample_pixel(src, n, bx, oy, ox, H, W, OH, OW, dy, dx, x[u]);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int c = 0; c < 3; ++c) x[u][c] = x[u][c] / 255.f;
      colour_ops(x[u], seq, cl, nullptr, true);
      if (p0 + u * stride < P) {
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += static_cast<double>(x[u][c]);
      }
    }
  }
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double t = wave_sum_f64(acc[c]);
    if (lane == 0) part[wid][c] = t;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    double t = 0.0;
    for (int k = 0; k < kThreads / kWave; ++k) t += part[k][threadIdx.x];
    partials[static_cast<int64_t>(blockIdx.x) * 3 + threadIdx.x] = static_cast<float>(t);
  }
}

// means[n * 3 + c] = (the B partials of sample n, channel c, in index order, in double) / (OH * OW).
__global__ __launch_bounds__(kThreads) void image_colour_fold_kernel(const float* __restrict__ colour,
                                                                     const float* __restrict__ partials,
                                                                     float* __restrict__ means, int N, int B,
                                                                     double pixels) {
  const int i = blockIdx.x * kThreads + threadIdx.x;  // one lane per sample and channel
  const int n = i / 3, c = i - n * 3;
  if (n >= N || !has_contrast(load_colour(colour, n).order)) return;
  double t = 0.0;
  for (int j = 0; j < B; ++j) t += static_cast<double>(partials[(static_cast<int64_t>(n) * B + j) * 3 + c]);
  means[i] = static_cast<float>(t / pixels);
}

// Colour ops need whole pixels: a lane owns 8 consecutive pixels of the flat [N*OH*OW] pixel array, 24 elements,
// stored as three 16-byte vectors (bf16) or six (fp32) at a 48- / 96-byte aligned offset.  The 8 pixels may lie
// in two samples (or more, for outputs under 8 pixels), so the box, the order, the parameters and the means are
// reloaded when the pixel walk enters a new sample; the branches on the order are uniform over a wave except in
// a wave that straddles samples.  means == nullptr (no statistics were made): contrast about a zero mean.
template <class T>
__global__ __launch_bounds__(kThreads) void image_colour_kernel(const uint8_t* __restrict__ src,
                                                                const int* __restrict__ boxes,
                                                                const float* __restrict__ colour,
                                                                const float* __restrict__ means, T* __restrict__ out,
                                                                int H, int W, int OH, int OW, int npix, Div dy,
                                                                Div dx, Norm3 nm, Scale3 sk) {
  const int64_t first = (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x) * 8;
  if (first >= npix) return;
  const int pix0 = static_cast<int>(first);
  int n = pix0 / (OH * OW);
  const int r = pix0 - n * OH * OW;
  int oy = r / OW, ox = r - oy * OW;
  Box bx;
  Colour cl;
  uint32_t seq;
  float mean[3];
  auto enter = [&]() {
    bx = load_box(boxes, n, H, W);
    cl = load_colour(colour, n);
    seq = colour_seq(cl.order);
    const bool stats = means != nullptr && has_contrast(cl.order);
#pragma unroll
    for (int c = 0; c < 3; ++c) mean[c] = stats ? means[n * 3 + c] : 0.f;
  };
  enter();
  float f[24];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    // (a pixel past the end of the batch -- n == N -- is not formed: the lane samples its last pixel again)
    if (k > 0 && pix0 + k < npix) {
      if (++ox == OW) {
        ox = 0;
        if (++oy == OH) {
          oy = 0;
          ++n;
          enter();
        }
      }
    }
    float x[3];
    sample_pixel(src, n, bx, oy, ox, H, W, OH, OW, dy, dx, x);
    if (cl.order < 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) f[3 * k + c] = fmaf(x[c], nm.s[c], nm.b[c]);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) x[c] = x[c] / 255.f;
      colour_ops(x, seq, cl, mean, false);
#pragma unroll
      for (int c = 0; c < 3; ++c) f[3 * k + c] = fmaf(clamp01(x[c]), sk.k[c], nm.b[c]);
    }
  }
  T* dst = out + first * 3;
  if (pix0 + 8 <= npix) {
#pragma unroll
    for (int q = 0; q < 3; ++q) V8<T>::from_float(f + 8 * q).store(dst + 8 * q);
  } else {  // the scalar tail of the flat array
    const int count = (npix - pix0) * 3;
#pragma unroll
    for (int q = 0; q < 21; ++q)
      if (q < count) put(dst + q, f[q]);
  }
}

int stat_blocks(int OH, int OW) { return std::min(kStatBlocks, ceil_div(static_cast<int64_t>(OH) * OW, kThreads)); }

}  // namespace

// Refusals (before any launch): -1 a null pointer or an empty dimension, -2 H / W / OH / OW above 4096,
// -3 `out` not 16-byte aligned, -4 N*OH*OW*3 >= 2^31, -5 a source that is not uint8, -6 N*H*W*3 >= 2^40.
TONY_API int tony_image_preprocess(const void* src, int src_is_u8, const int* boxes, void* out, int out_is_bf16, int N,
                                   int H, int W, int OH, int OW, float s0, float s1, float s2, float b0, float b1,
                                   float b2, hipStream_t stream) {
  if (!src_is_u8) return -5;
  if (!src || !boxes || !out || N <= 0 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0) return -1;
  if (H > kMaxDim || W > kMaxDim || OH > kMaxDim || OW > kMaxDim) return -2;
  if (reinterpret_cast<uintptr_t>(out) % 16 != 0) return -3;
  const int64_t total = static_cast<int64_t>(N) * OH * OW * 3;
  if (total >= (int64_t{1} << 31)) return -4;
  if (static_cast<int64_t>(N) * H * W * 3 >= (int64_t{1} << 40)) return -6;
  const Norm3 nm{{s0, s1, s2}, {b0, b1, b2}};
  const Div dy = make_div(2 * OH), dx = make_div(2 * OW);
  const int blocks = ceil_div(ceil_div(total, 8), kThreads);
  const auto* s8 = static_cast<const uint8_t*>(src);
  const int tot = static_cast<int>(total);
  if (out_is_bf16)
    image_preprocess_kernel<uint16_t><<<blocks, kThreads, 0, stream>>>(s8, boxes, static_cast<uint16_t*>(out), H, W,
                                                                       OH, OW, tot, dy, dx, nm);
  else
    image_preprocess_kernel<float><<<blocks, kThreads, 0, stream>>>(s8, boxes, static_cast<float*>(out), H, W, OH, OW,
                                                                    tot, dy, dx, nm);
  TONY_LAUNCH_CHECK();
  return 0;
}

// fp32 elements of the statistics scratch of an [N, OH, OW] launch: N * (B + 1) * 3 with B = min(64,
// ceil(OH * OW / 256)) partial sums per sample and channel, then the N * 3 means.  -1 an empty dimension, -2 OH / OW
// above 4096, -4 a size that does not fit an int.
TONY_API int tony_image_colour_scratch_floats(int N, int OH, int OW) {
  if (N <= 0 || OH <= 0 || OW <= 0) return -1;
  if (OH > kMaxDim || OW > kMaxDim) return -2;
  const int64_t floats = static_cast<int64_t>(N) * (stat_blocks(OH, OW) + 1) * 3;
  return floats >= (int64_t{1} << 31) ? -4 : static_cast<int>(floats);
}

// tony_image_preprocess with the colour table `colour` (float32 [N, 5], above).  has_contrast != 0: the table may
// hold an order 0..3, and `scratch` (fp32, at least tony_image_colour_scratch_floats elements, every one the
// launches use rewritten by them) receives the statistics; has_contrast == 0 launches the apply pass alone and
// never touches `scratch`.  Refusals (before any launch): tony_image_preprocess's -1 .. -6, -7 no colour table,
// -8 a scratch that is missing, too small or not 4-byte aligned when has_contrast is set.
TONY_API int tony_image_preprocess_colour(const void* src, int src_is_u8, const int* boxes, const float* colour,
                                          int has_contrast, float* scratch, int64_t scratch_floats, void* out,
                                          int out_is_bf16, int N, int H, int W, int OH, int OW, float s0, float s1,
                                          float s2, float b0, float b1, float b2, hipStream_t stream) {
  if (!src_is_u8) return -5;
  if (!src || !boxes || !out || N <= 0 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0) return -1;
  if (H > kMaxDim || W > kMaxDim || OH > kMaxDim || OW > kMaxDim) return -2;
  if (reinterpret_cast<uintptr_t>(out) % 16 != 0) return -3;
  const int64_t total = static_cast<int64_t>(N) * OH * OW * 3;
  if (total >= (int64_t{1} << 31)) return -4;
  if (static_cast<int64_t>(N) * H * W * 3 >= (int64_t{1} << 40)) return -6;
  if (!colour) return -7;
  const int B = stat_blocks(OH, OW);
  const int64_t need = static_cast<int64_t>(N) * (B + 1) * 3;
  if (has_contrast) {
    if (need >= (int64_t{1} << 31)) return -4;
    if (!scratch || scratch_floats < need || reinterpret_cast<uintptr_t>(scratch) % 4 != 0) return -8;
  }
  const Norm3 nm{{s0, s1, s2}, {b0, b1, b2}};
  const Scale3 sk{{255.f * s0, 255.f * s1, 255.f * s2}};
  const Div dy = make_div(2 * OH), dx = make_div(2 * OW);
  const auto* s8 = static_cast<const uint8_t*>(src);
  float* means = nullptr;
  if (has_contrast) {
    means = scratch + static_cast<int64_t>(N) * B * 3;
    image_colour_stats_kernel<<<N * B, kThreads, 0, stream>>>(s8, boxes, colour, scratch, H, W, OH, OW, B, dy, dx,
                                                              make_div(OW));
    TONY_LAUNCH_CHECK();
    image_colour_fold_kernel<<<ceil_div(3 * static_cast<int64_t>(N), kThreads), kThreads, 0, stream>>>(
        colour, scratch, means, N, B, static_cast<double>(OH) * OW);
    TONY_LAUNCH_CHECK();
  }
  const int npix = static_cast<int>(total / 3);
  const int blocks = ceil_div(ceil_div(npix, 8), kThreads);
  if (out_is_bf16)
    image_colour_kernel<uint16_t><<<blocks, kThreads, 0, stream>>>(
        s8, boxes, colour, means, static_cast<uint16_t*>(out), H, W, OH, OW, npix, dy, dx, nm, sk);
  else
    image_colour_kernel<float><<<blocks, kThreads, 0, stream>>>(s8, boxes, colour, means, static_cast<float*>(out), H,
                                                                W, OH, OW, npix, dy, dx, nm, sk);
  TONY_LAUNCH_CHECK();
  return 0;
}
