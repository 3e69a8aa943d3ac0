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
