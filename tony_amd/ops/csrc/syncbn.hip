// Synchronised BatchNorm (+ optional ReLU, + optional residual add) on NHWC rows: the statistics of
// a layer are those of ALL ranks' batches (ops/syncbn.py states the contract).
//
// Forward  = stats (per-workgroup double partials [G][2C] of sum x / sum x^2) -> fold (ascending
//            workgroup order, into the rank's packet [M | S | Q]) -> the ranks all-gather the packets
//            (parallel/collectives.py) -> merge (one small launch: mean / invstd in double from the
//            gathered [W][1 + 2C], save_*, the running statistics, the fp32 coefficient table) ->
//            apply (the row pass from the table).
// Backward = bwd_reduce (double partials of sum dy' / sum dy' * xhat, folded into [A | B]; dgamma /
//            dbeta are these LOCAL sums) -> all-gather -> bwd_merge (the 5-row table) -> bwd_apply.
//
// No float atomics anywhere: a workgroup's partial is stored, the fold adds the partials in ascending
// workgroup order and the grid depends on (M, C) only, so two runs give the same bits.  Every element
// is converted exactly to double and accumulated in double (a bf16 / fp32 square is exact there).
//
// Thread map of bn_act.hip: one 16-byte (8-channel) vector per lane, a 256-thread workgroup covers
// RPI = 256 / (C / 8) rows per iteration, loads 4 deep; the block reduction's LDS is sized to C.
#include "common.h"

using namespace tony;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxC = 2048;
constexpr int kFoldThreads = 64;
constexpr int kFoldDepth = 32;

extern __shared__ __attribute__((aligned(16))) double sbn_dyn[];
inline size_t sbn_lds_reduce(int C) {  // [2][RPI][C] doubles: at most 32 KB (RPI * C <= 2048)
  return static_cast<size_t>(2) * (kThreads / (C / 8)) * C * sizeof(double);
}

struct RowMap {
  int CG, RPI, cg, rsub;
  bool active;
  __device__ RowMap(int C) {
    CG = C >> 3;
    RPI = kThreads / CG;
    cg = threadIdx.x % CG;
    rsub = threadIdx.x / CG;
    active = rsub < RPI;
  }
};

__device__ __forceinline__ float load_param(const void* p, int idx, int is_bf16, float dflt) {
  if (p == nullptr) return dflt;
  return is_bf16 ? bf2f(static_cast<const uint16_t*>(p)[idx]) : static_cast<const float*>(p)[idx];
}

// The forward's fp32 coefficients, y = fma(x, k, sh): one definition, used by the merge kernels and by
// the backward reduction that recomputes the ReLU mask, so the three agree to the bit.
__device__ __forceinline__ void fwd_coef(float g, float b, float mu, float is, float& k, float& sh) {
  k = g * is;
  sh = fmaf(-mu, k, b);
}

// double -> float rounded to odd: a following round-to-nearest to bf16 is then the single rounding
// of the double
__device__ __forceinline__ float to_float_odd(double d) {
  float f = static_cast<float>(d);
  if (static_cast<double>(f) == d || !(f == f) || fabsf(f) == INFINITY) return f;
  uint32_t u = __float_as_uint(f);
  if (fabs(static_cast<double>(f)) > fabs(d)) u -= 1;  // back to the truncated magnitude
  return __uint_as_float(u | 1u);
}

// a parameter gradient from its double sum: written, or added to what is there, rounded once
__device__ __forceinline__ void store_grad(void* p, int idx, int is_bf16, double v, int accumulate) {
  if (p == nullptr) return;
  if (is_bf16) {
    uint16_t* q = static_cast<uint16_t*>(p) + idx;
    if (accumulate) v += static_cast<double>(bf2f(*q));
    *q = f2bf(to_float_odd(v));
  } else {
    float* q = static_cast<float*>(p) + idx;
    if (accumulate) v += static_cast<double>(*q);
    *q = static_cast<float>(v);
  }
}

// The RPI row-lanes' partials meet in LDS; channel c's two sums (row-lanes in ascending order) are
// stored as this workgroup's partial: part[2C] = [a | b].
__device__ __forceinline__ void block_reduce_store(double* red, const RowMap& rm, int C, const double* a,
                                                   const double* b, double* __restrict__ part) {
  if (rm.active) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      red[rm.rsub * C + rm.cg * 8 + j] = a[j];
      red[rm.RPI * C + rm.rsub * C + rm.cg * 8 + j] = b[j];
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += kThreads) {
    double sa = 0.0, sb = 0.0;
    for (int k = 0; k < rm.RPI; ++k) {
      sa += red[k * C + c];
      sb += red[rm.RPI * C + k * C + c];
    }
    part[c] = sa;
    part[C + c] = sb;
  }
}

template <class T>
__global__ __launch_bounds__(kThreads) void syncbn_stats_kernel(const T* __restrict__ x, int64_t M, int C, int64_t ldx,
                                                                int64_t rows_per_block, double* __restrict__ partials) {
  double* red = sbn_dyn;
  RowMap rm(C);
  double s[8], q[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = q[j] = 0.0;
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * rows_per_block;
  const int64_t r1 = min(M, r0 + rows_per_block);
  if (rm.active) {
    const T* base = x + rm.cg * 8;
    int64_t r = r0 + rm.rsub;
    const int64_t step = rm.RPI;
    auto body = [&](const V8<T>& v) {
      float f[8];
      v.to_float(f);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const double d = static_cast<double>(f[j]);
        s[j] += d;
        q[j] = fma(d, d, q[j]);
      }
    };
    for (; r + 3 * step < r1; r += 4 * step) {
      V8<T> v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = V8<T>::load(base + (r + u * step) * ldx);
#pragma unroll
      for (int u = 0; u < 4; ++u) body(v[u]);
    }
    for (; r < r1; r += step) body(V8<T>::load(base + r * ldx));
  }
  block_reduce_store(red, rm, C, s, q, partials + static_cast<int64_t>(blockIdx.x) * 2 * C);
}

// out[c] = sum over workgroups g = 0 .. G-1, in that order, of partials[g][c], c < n = 2C.  count >= 0:
// the packet form, out[0] = count and the sums follow; count < 0: the sums start at out[0].
// dbeta (columns < C) / dgamma (columns >= C): also the parameter gradients of the backward's fold.
__global__ __launch_bounds__(kFoldThreads) void syncbn_fold_kernel(const double* __restrict__ partials, int G, int C,
                                                                   double* __restrict__ out, int64_t count, void* dgamma,
                                                                   void* dbeta, int param_bf16, int accumulate) {
  const int n = 2 * C;
  const int c = blockIdx.x * kFoldThreads + threadIdx.x;
  if (c >= n) return;
  // kFoldDepth loads are issued before the first is added (one dependent load per workgroup made the fold cost
  // ten times the statistics pass: 0.27 us per workgroup, tools/syncbn_bench.py); the additions keep their order
  const double* p = partials + c;
  double s = 0.0;
  int g = 0;
  for (; g + kFoldDepth <= G; g += kFoldDepth) {
    double v[kFoldDepth];
#pragma unroll
    for (int u = 0; u < kFoldDepth; ++u) v[u] = p[static_cast<int64_t>(g + u) * n];
#pragma unroll
    for (int u = 0; u < kFoldDepth; ++u) s += v[u];
  }
  for (; g < G; ++g) s += p[static_cast<int64_t>(g) * n];
  double* o = out;
  if (count >= 0) {
    if (c == 0) out[0] = static_cast<double>(count);
    o = out + 1;
  }
  o[c] = s;
  if (c < C) store_grad(dbeta, c, param_bf16, s, accumulate);
  else store_grad(dgamma, c - C, param_bf16, s, accumulate);
}

// gathered [W][1 + 2C] -> save_mean / save_invstd (double statistics rounded once), the running
// statistics (fp32, as bn_fwd_apply_kernel), the forward table coef[2][C] = [k | sh] and the global
// row count N (a double, for the backward).  Ranks are summed in ascending order.
__global__ __launch_bounds__(kThreads) void syncbn_merge_kernel(
    const double* __restrict__ gathered, int W, int C, const void* gamma, const void* beta, int param_bf16, float eps,
    float momentum, float* __restrict__ save_mean, float* __restrict__ save_invstd, float* __restrict__ running_mean,
    float* __restrict__ running_var, float* __restrict__ coef, double* __restrict__ count_out) {
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c >= C) return;
  const int64_t P = 1 + 2 * static_cast<int64_t>(C);
  double N = 0.0, S = 0.0, Q = 0.0;
  for (int r = 0; r < W; ++r) {
    N += gathered[r * P];
    S += gathered[r * P + 1 + c];
    Q += gathered[r * P + 1 + C + c];
  }
  const double mean = S / N;
  const double var = fmax(Q / N - mean * mean, 0.0);
  const double invstd = 1.0 / sqrt(var + static_cast<double>(eps));
  const float mu = static_cast<float>(mean), is = static_cast<float>(invstd);
  save_mean[c] = mu;
  save_invstd[c] = is;
  if (running_mean != nullptr) {
    const float varf = static_cast<float>(var), n = static_cast<float>(N);
    const float unbiased = N > 1.0 ? varf * (n / (n - 1.f)) : varf;
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mu;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * unbiased;
  }
  float k, sh;
  fwd_coef(load_param(gamma, c, param_bf16, 1.f), load_param(beta, c, param_bf16, 0.f), mu, is, k, sh);
  coef[c] = k;
  coef[C + c] = sh;
  if (c == 0 && count_out != nullptr) *count_out = N;
}

// gathered [W][2C] = the ranks' [A | B], N -> tab[5][C]: dx = dy' * q0 + x * q1 + q2 with the ReLU test
// x * q3 + q4 > 0 (bn_bwd_apply_kernel's folding; A / N and B / N in double, each coefficient rounded once)
__global__ __launch_bounds__(kThreads) void syncbn_bwd_merge_kernel(
    const double* __restrict__ gathered, int W, int C, const double* __restrict__ count, const float* __restrict__ mean,
    const float* __restrict__ invstd, const void* gamma, const void* beta, int param_bf16, float* __restrict__ tab) {
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c >= C) return;
  double A = 0.0, B = 0.0;
  for (int r = 0; r < W; ++r) {
    A += gathered[static_cast<int64_t>(r) * 2 * C + c];
    B += gathered[static_cast<int64_t>(r) * 2 * C + C + c];
  }
  const double N = *count;
  const float mu = mean[c], is = invstd[c];
  float k, sh;
  fwd_coef(load_param(gamma, c, param_bf16, 1.f), load_param(beta, c, param_bf16, 0.f), mu, is, k, sh);
  const double am = A / N, bm = B / N, kd = k, isd = is, mud = mu;
  tab[c] = k;
  tab[C + c] = static_cast<float>(-kd * bm * isd);
  tab[2 * C + c] = static_cast<float>(kd * (bm * isd * mud - am));
  tab[3 * C + c] = k;
  tab[4 * C + c] = sh;
}

__device__ __forceinline__ void load8f(const float* p, float* f) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  f[0] = a.x, f[1] = a.y, f[2] = a.z, f[3] = a.w, f[4] = b.x, f[5] = b.y, f[6] = b.z, f[7] = b.w;
}

// y = act(fma(x, k, sh) [+ res]) from the merge's table
template <bool RES, class T>
__global__ __launch_bounds__(kThreads) void syncbn_apply_kernel(const T* __restrict__ x, int64_t M, int C, int64_t ldx,
                                                                int64_t rows_per_block, const T* __restrict__ res,
                                                                int64_t ldr, T* __restrict__ y, int64_t ldy,
                                                                const float* __restrict__ coef, int relu) {
  RowMap rm(C);
  if (!rm.active) return;
  float sc[8], sh[8];
  load8f(coef + rm.cg * 8, sc);
  load8f(coef + C + rm.cg * 8, sh);
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * rows_per_block;
  const int64_t r1 = min(M, r0 + rows_per_block);
  const int64_t step = rm.RPI;
  int64_t r = r0 + rm.rsub;
  auto body = [&](const V8<T>& v, const V8<T>& rv, int64_t row) {
    float f[8], q[8];
    v.to_float(f);
    if (RES) rv.to_float(q);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float t = fmaf(f[j], sc[j], sh[j]);
      if (RES) t += q[j];
      f[j] = relu ? relu_f(t) : t;
    }
    V8<T>::from_float(f).store(y + row * ldy + rm.cg * 8);
  };
  V8<T> none{};
  for (; r + 3 * step < r1; r += 4 * step) {
    V8<T> v[4], rv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      v[u] = V8<T>::load(x + (r + u * step) * ldx + rm.cg * 8);
      if (RES) rv[u] = V8<T>::load(res + (r + u * step) * ldr + rm.cg * 8);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) body(v[u], RES ? rv[u] : none, r + u * step);
  }
  for (; r < r1; r += step)
    body(V8<T>::load(x + r * ldx + rm.cg * 8), RES ? V8<T>::load(res + r * ldr + rm.cg * 8) : none, r);
}

// Partials of A = sum dy', B = sum dy' * xhat over this workgroup's rows.  dy' is dy masked by the ReLU:
// recomputed from x with the forward's coefficients, or -- YMASK, the residual form -- from the saved y <= 0
// (relu == 0: no mask in either form).
template <bool YMASK, class T>
__global__ __launch_bounds__(kThreads) void syncbn_bwd_reduce_kernel(
    const T* __restrict__ x, int64_t ldx, const T* __restrict__ dy, int64_t lddy, const T* __restrict__ ym, int64_t ldym,
    int64_t M, int C, int64_t rows_per_block, const float* __restrict__ mean, const float* __restrict__ invstd,
    const void* gamma, const void* beta, int param_bf16, int relu, double* __restrict__ partials) {
  double* red = sbn_dyn;
  RowMap rm(C);
  double a[8], b[8];
  float p0[8], p1[8], p2[8], p3[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    a[j] = b[j] = 0.0;
    const int c = (rm.active ? rm.cg * 8 : 0) + j;
    const float mu = mean[c], is = invstd[c];
    p0[j] = is;
    p1[j] = -mu * is;
    fwd_coef(load_param(gamma, c, param_bf16, 1.f), load_param(beta, c, param_bf16, 0.f), mu, is, p2[j], p3[j]);
  }
  if (rm.active) {
    const int64_t r0 = static_cast<int64_t>(blockIdx.x) * rows_per_block;
    const int64_t r1 = min(M, r0 + rows_per_block);
    const int64_t step = rm.RPI;
    auto body = [&](const V8<T>& xv, const V8<T>& gv, const V8<T>& yv) {
      float xf[8], gf[8], yf[8];
      xv.to_float(xf);
      gv.to_float(gf);
      if (YMASK) yv.to_float(yf);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float xh = fmaf(xf[j], p0[j], p1[j]);
        float d = gf[j];
        if (YMASK) {
          if (relu && yf[j] <= 0.f) d = 0.f;
        } else if (relu && fmaf(xf[j], p2[j], p3[j]) <= 0.f) {
          d = 0.f;
        }
        const double dd = static_cast<double>(d);
        a[j] += dd;
        b[j] = fma(dd, static_cast<double>(xh), b[j]);
      }
    };
    V8<T> none{};
    int64_t r = r0 + rm.rsub;
    for (; r + 3 * step < r1; r += 4 * step) {
      V8<T> xv[4], gv[4], yv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        xv[u] = V8<T>::load(x + (r + u * step) * ldx + rm.cg * 8);
        gv[u] = V8<T>::load(dy + (r + u * step) * lddy + rm.cg * 8);
        if (YMASK) yv[u] = V8<T>::load(ym + (r + u * step) * ldym + rm.cg * 8);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) body(xv[u], gv[u], YMASK ? yv[u] : none);
    }
    for (; r < r1; r += step)
      body(V8<T>::load(x + r * ldx + rm.cg * 8), V8<T>::load(dy + r * lddy + rm.cg * 8),
           YMASK ? V8<T>::load(ym + r * ldym + rm.cg * 8) : none);
  }
  block_reduce_store(red, rm, C, a, b, partials + static_cast<int64_t>(blockIdx.x) * 2 * C);
}

// dx = dy' * q0 + x * q1 + q2 from the backward merge's table; YMASK also writes dres = dy'
template <bool YMASK, class T>
__global__ __launch_bounds__(kThreads) void syncbn_bwd_apply_kernel(
    const T* __restrict__ x, int64_t ldx, const T* __restrict__ dy, int64_t lddy, const T* __restrict__ ym, int64_t ldym,
    T* __restrict__ dres, int64_t lddr, T* __restrict__ dx, int64_t lddx, int64_t M, int C, int64_t rows_per_block,
    const float* __restrict__ tab, int relu) {
  RowMap rm(C);
  if (!rm.active) return;
  float q0[8], q1[8], q2[8], q3[8], q4[8];
  load8f(tab + rm.cg * 8, q0);
  load8f(tab + C + rm.cg * 8, q1);
  load8f(tab + 2 * C + rm.cg * 8, q2);
  load8f(tab + 3 * C + rm.cg * 8, q3);
  load8f(tab + 4 * C + rm.cg * 8, q4);
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * rows_per_block;
  const int64_t r1 = min(M, r0 + rows_per_block);
  const int64_t step = rm.RPI;
  auto body = [&](const V8<T>& xv, const V8<T>& gv, const V8<T>& yv, int64_t row) {
    float xf[8], gf[8], yf[8], o[8];
    xv.to_float(xf);
    gv.to_float(gf);
    if (YMASK) yv.to_float(yf);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float d = gf[j];
      if (YMASK) {
        if (relu && yf[j] <= 0.f) d = 0.f;
        gf[j] = d;
      } else if (relu && fmaf(xf[j], q3[j], q4[j]) <= 0.f) {
        d = 0.f;
      }
      o[j] = fmaf(d, q0[j], fmaf(xf[j], q1[j], q2[j]));
    }
    V8<T>::from_float(o).store(dx + row * lddx + rm.cg * 8);
    if (YMASK && dres != nullptr) V8<T>::from_float(gf).store(dres + row * lddr + rm.cg * 8);
  };
  V8<T> none{};
  int64_t r = r0 + rm.rsub;
  for (; r + 3 * step < r1; r += 4 * step) {
    V8<T> xv[4], gv[4], yv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      xv[u] = V8<T>::load(x + (r + u * step) * ldx + rm.cg * 8);
      gv[u] = V8<T>::load(dy + (r + u * step) * lddy + rm.cg * 8);
      if (YMASK) yv[u] = V8<T>::load(ym + (r + u * step) * ldym + rm.cg * 8);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) body(xv[u], gv[u], YMASK ? yv[u] : none, r + u * step);
  }
  for (; r < r1; r += step)
    body(V8<T>::load(x + r * ldx + rm.cg * 8), V8<T>::load(dy + r * lddy + rm.cg * 8),
         YMASK ? V8<T>::load(ym + r * ldym + rm.cg * 8) : none, r);
}

// Rows per workgroup and the grid: at least `min_iters` row groups per workgroup, at most `max_blocks`
// workgroups; a function of (M, C) alone.
void plan_rows(int64_t M, int C, int min_iters, int max_blocks, int64_t* rpb, int* grid) {
  const int RPI = kThreads / (C / 8);
  int64_t g = (M + static_cast<int64_t>(RPI) * min_iters - 1) / (static_cast<int64_t>(RPI) * min_iters);
  if (g > max_blocks) g = max_blocks;
  if (g < 1) g = 1;
  int64_t r = (M + g - 1) / g;
  r = ((r + RPI - 1) / RPI) * RPI;
  *rpb = r;
  *grid = static_cast<int>((M + r - 1) / r);
}

// the reductions: few workgroups (each stores 2C doubles), 16 row groups deep at least
void plan_reduce(int64_t M, int C, int64_t* rpb, int* grid) { plan_rows(M, C, 16, 512, rpb, grid); }

bool bad_c(int C) { return C <= 0 || C % 8 != 0 || C > kMaxC; }
bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

int launch_fold(const double* partials, int G, int C, double* out, int64_t count, void* dgamma, void* dbeta,
                int param_bf16, int accumulate, hipStream_t stream) {
  syncbn_fold_kernel<<<ceil_div(2 * C, kFoldThreads), kFoldThreads, 0, stream>>>(partials, G, C, out, count, dgamma,
                                                                                 dbeta, param_bf16, accumulate);
  TONY_LAUNCH_CHECK();
  return 0;
}

}  // namespace

// Workgroups of the stats / bwd_reduce launches for M rows of C channels (= rows of the partials buffer)
TONY_API int tony_syncbn_grid(int64_t M, int C) {
  if (bad_c(C) || M < 1) return -1;
  int64_t rpb;
  int grid;
  plan_reduce(M, C, &rpb, &grid);
  return grid;
}

// partials[tony_syncbn_grid(M, C)][2C] doubles <- per-workgroup [sum x | sum x^2]; is_f32: fp32 rows, else bf16
TONY_API int tony_syncbn_stats(const void* x, int64_t M, int C, int64_t ldx, int is_f32, double* partials,
                               hipStream_t stream) {
  if (bad_c(C) || M < 1 || (ldx % 8) || ldx < C || misaligned(x) || partials == nullptr) return -1;
  int64_t rpb;
  int grid;
  plan_reduce(M, C, &rpb, &grid);
  if (is_f32)
    syncbn_stats_kernel<float><<<grid, kThreads, sbn_lds_reduce(C), stream>>>(static_cast<const float*>(x), M, C, ldx,
                                                                             rpb, partials);
  else
    syncbn_stats_kernel<uint16_t><<<grid, kThreads, sbn_lds_reduce(C), stream>>>(static_cast<const uint16_t*>(x), M, C,
                                                                                ldx, rpb, partials);
  TONY_LAUNCH_CHECK();
  return 0;
}

// count >= 0: out[1 + 2C] = [count | fold]; count < 0: out[2C] = fold
TONY_API int tony_syncbn_fold(const double* partials, int G, int C, double* out, int64_t count, hipStream_t stream) {
  if (bad_c(C) || G < 1 || partials == nullptr || out == nullptr) return -1;
  return launch_fold(partials, G, C, out, count, nullptr, nullptr, 0, 0, stream);
}

// partials (as tony_syncbn_stats) and out[2C] = this rank's [A | B]; dgamma / dbeta (null: skipped) are stored
// from, or -- accumulate -- added to by, the local B / A.  y non-null: the residual form, dy masked by y <= 0.
TONY_API int tony_syncbn_bwd_reduce(const void* x, int64_t ldx, const void* dy, int64_t lddy, const void* y, int64_t ldy,
                                    int64_t M, int C, int is_f32, const float* mean, const float* invstd,
                                    const void* gamma, const void* beta, int param_bf16, int relu, double* partials,
                                    double* out, void* dgamma, void* dbeta, int accumulate, hipStream_t stream) {
  if (bad_c(C) || M < 1 || (ldx % 8) || (lddy % 8) || ldx < C || lddy < C || misaligned(x) || misaligned(dy) ||
      (y != nullptr && ((ldy % 8) || ldy < C || misaligned(y))) || partials == nullptr || out == nullptr)
    return -1;
  int64_t rpb;
  int grid;
  plan_reduce(M, C, &rpb, &grid);
  const size_t lds = sbn_lds_reduce(C);
#define SBN_RED(YM, T)                                                                                              \
  syncbn_bwd_reduce_kernel<YM, T><<<grid, kThreads, lds, stream>>>(                                                 \
      static_cast<const T*>(x), ldx, static_cast<const T*>(dy), lddy, static_cast<const T*>(y), ldy, M, C, rpb, mean, \
      invstd, gamma, beta, param_bf16, relu, partials)
  if (y != nullptr) {
    if (is_f32) SBN_RED(true, float);
    else SBN_RED(true, uint16_t);
  } else {
    if (is_f32) SBN_RED(false, float);
    else SBN_RED(false, uint16_t);
  }
#undef SBN_RED
  TONY_LAUNCH_CHECK();
  return launch_fold(partials, grid, C, out, -1, dgamma, dbeta, param_bf16, accumulate, stream);
}

// gathered [W][1 + 2C] -> save_mean, save_invstd, running_* (null: none kept), coef[2C], count_out (null: skipped)
TONY_API int tony_syncbn_merge(const double* gathered, int W, int C, const void* gamma, const void* beta, int param_bf16,
                               float eps, float momentum, float* save_mean, float* save_invstd, float* running_mean,
                               float* running_var, float* coef, double* count_out, hipStream_t stream) {
  if (bad_c(C) || W < 1 || gathered == nullptr || save_mean == nullptr || save_invstd == nullptr || coef == nullptr ||
      misaligned(coef) || (running_mean == nullptr) != (running_var == nullptr))
    return -1;
  syncbn_merge_kernel<<<ceil_div(C, kThreads), kThreads, 0, stream>>>(gathered, W, C, gamma, beta, param_bf16, eps,
                                                                      momentum, save_mean, save_invstd, running_mean,
                                                                      running_var, coef, count_out);
  TONY_LAUNCH_CHECK();
  return 0;
}

// gathered [W][2C], *count = N -> tab[5C]
TONY_API int tony_syncbn_bwd_merge(const double* gathered, int W, int C, const double* count, const float* mean,
                                   const float* invstd, const void* gamma, const void* beta, int param_bf16, float* tab,
                                   hipStream_t stream) {
  if (bad_c(C) || W < 1 || gathered == nullptr || count == nullptr || mean == nullptr || invstd == nullptr ||
      tab == nullptr || misaligned(tab))
    return -1;
  syncbn_bwd_merge_kernel<<<ceil_div(C, kThreads), kThreads, 0, stream>>>(gathered, W, C, count, mean, invstd, gamma,
                                                                          beta, param_bf16, tab);
  TONY_LAUNCH_CHECK();
  return 0;
}

// y = act(fma(x, coef[c], coef[C + c]) [+ res]); res non-null: the residual form
TONY_API int tony_syncbn_apply(const void* x, int64_t M, int C, int64_t ldx, const void* res, int64_t ldr, void* y,
                               int64_t ldy, int is_f32, const float* coef, int relu, hipStream_t stream) {
  if (bad_c(C) || M < 1 || (ldx % 8) || (ldy % 8) || ldx < C || ldy < C || misaligned(x) || misaligned(y) ||
      (res != nullptr && ((ldr % 8) || ldr < C || misaligned(res))) || coef == nullptr || misaligned(coef))
    return -1;
  int64_t rpb;
  int grid;
  plan_rows(M, C, 4, 8192, &rpb, &grid);
#define SBN_APPLY(RS, T)                                                                                              \
  syncbn_apply_kernel<RS, T><<<grid, kThreads, 0, stream>>>(static_cast<const T*>(x), M, C, ldx, rpb,                 \
                                                            static_cast<const T*>(res), ldr, static_cast<T*>(y), ldy, \
                                                            coef, relu)
  if (res != nullptr) {
    if (is_f32) SBN_APPLY(true, float);
    else SBN_APPLY(true, uint16_t);
  } else {
    if (is_f32) SBN_APPLY(false, float);
    else SBN_APPLY(false, uint16_t);
  }
#undef SBN_APPLY
  TONY_LAUNCH_CHECK();
  return 0;
}

// dx from tab[5C]; y non-null: the residual form (dy masked by y <= 0), which also writes dres = dy' when non-null
TONY_API int tony_syncbn_bwd_apply(const void* x, int64_t ldx, const void* dy, int64_t lddy, const void* y, int64_t ldy,
                                   void* dres, int64_t lddr, void* dx, int64_t lddx, int64_t M, int C, int is_f32,
                                   const float* tab, int relu, hipStream_t stream) {
  if (bad_c(C) || M < 1 || (ldx % 8) || (lddy % 8) || (lddx % 8) || ldx < C || lddy < C || lddx < C || misaligned(x) ||
      misaligned(dy) || misaligned(dx) || (y != nullptr && ((ldy % 8) || ldy < C || misaligned(y))) ||
      (dres != nullptr && (y == nullptr || (lddr % 8) || lddr < C || misaligned(dres))) || tab == nullptr ||
      misaligned(tab))
    return -1;
  int64_t rpb;
  int grid;
  plan_rows(M, C, 4, 8192, &rpb, &grid);
#define SBN_BAPPLY(YM, T)                                                                                           \
  syncbn_bwd_apply_kernel<YM, T><<<grid, kThreads, 0, stream>>>(                                                    \
      static_cast<const T*>(x), ldx, static_cast<const T*>(dy), lddy, static_cast<const T*>(y), ldy,                 \
      static_cast<T*>(dres), lddr, static_cast<T*>(dx), lddx, M, C, rpb, tab, relu)
  if (y != nullptr) {
    if (is_f32) SBN_BAPPLY(true, float);
    else SBN_BAPPLY(true, uint16_t);
  } else {
    if (is_f32) SBN_BAPPLY(false, float);
    else SBN_BAPPLY(false, uint16_t);
  }
#undef SBN_BAPPLY
  TONY_LAUNCH_CHECK();
  return 0;
}
