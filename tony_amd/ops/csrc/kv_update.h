// The per-element update lines of the kvstore's optimizer kinds (parallel/kvstore.py module docstring), shared by the
// fp32 kernels (kv_optim.hip) and the multi-precision ones (kv_mp.hip).  Every line of the docstring is one rn_* call,
// so nothing is contracted into an fma and every division and square root is the correctly rounded one (rn_math.h).
#pragma once
#include "common.h"
#include "rn_math.h"

using namespace tony;

namespace {

// the kinds of the C entry points, and nag at momentum 0 (no state: lazy SGD's momentum == 0 lines)
enum : int { kNag = 0, kAdagrad = 1, kRmsprop = 2, kRmspropCentered = 3, kFtrl = 4, kKinds = 5, kNagPlain = 5 };

struct KvOptHp {
  float lr, wd, rescale, clip, momentum, eps, gamma1, omg1, gamma2, lamda1, beta;  // omg1 = fl32(1 - gamma1)
  int has_clip;
};

constexpr int states_of(int kind) {
  return kind == kNagPlain ? 0 : kind == kRmspropCentered ? 3 : kind == kFtrl ? 2 : 1;
}

// state: mom (none when MOM is false)
template <bool MOM>
__device__ __forceinline__ void nag1(float& w, float& m, float g2, const KvOptHp& hp) {
  const float p = rn_mul(hp.wd, w);
  const float g3 = rn_add(g2, p);
  if constexpr (MOM) {
    m = rn_mul(hp.momentum, m);
    m = rn_add(m, g3);
    const float q = rn_mul(hp.momentum, m);
    const float g4 = rn_add(g3, q);
    const float s = rn_mul(hp.lr, g4);
    w = rn_sub(w, s);
  } else {
    const float s = rn_mul(hp.lr, g3);
    w = rn_sub(w, s);
  }
}

// state: history
__device__ __forceinline__ void adagrad1(float& w, float& h, float g2, const KvOptHp& hp) {
  const float q = rn_mul(g2, g2);
  h = rn_add(h, q);
  const float e = rn_add(h, hp.eps);
  const float r = rn_sqrt(e);
  const float d = rn_div(g2, r);
  const float p = rn_mul(hp.wd, w);
  const float u = rn_add(d, p);
  const float s = rn_mul(hp.lr, u);
  w = rn_sub(w, s);
}

// states: n, and when CENTERED g (gb) and delta
template <bool CENTERED>
__device__ __forceinline__ void rmsprop1(float& w, float& n, float& gb, float& delta, float g2, const KvOptHp& hp) {
  const float p = rn_mul(hp.wd, w);
  const float g3 = rn_add(g2, p);
  const float q = rn_mul(g3, g3);
  const float a = rn_mul(hp.omg1, q);
  const float b = rn_mul(hp.gamma1, n);
  n = rn_add(a, b);
  if constexpr (CENTERED) {
    const float c = rn_mul(hp.omg1, g3);
    const float b2 = rn_mul(hp.gamma1, gb);
    gb = rn_add(c, b2);
    const float gg = rn_mul(gb, gb);
    const float e1 = rn_sub(n, gg);
    const float e = rn_add(e1, hp.eps);
    const float r = rn_sqrt(e);
    const float d = rn_div(g3, r);
    const float s = rn_mul(hp.lr, d);
    const float dl = rn_mul(hp.gamma2, delta);
    delta = rn_sub(dl, s);
    w = rn_add(w, delta);
  } else {
    const float e = rn_add(n, hp.eps);
    const float r = rn_sqrt(e);
    const float d = rn_div(g3, r);
    const float s = rn_mul(hp.lr, d);
    w = rn_sub(w, s);
  }
}

// states: z, n; wd enters only the denominator
__device__ __forceinline__ void ftrl1(float& w, float& z, float& n, float g2, const KvOptHp& hp) {
  const float q = rn_mul(g2, g2);
  const float n1 = rn_add(n, q);
  const float r1 = rn_sqrt(n1);
  const float r0 = rn_sqrt(n);
  const float dr = rn_sub(r1, r0);
  const float sg = rn_div(dr, hp.lr);
  const float t = rn_mul(sg, w);
  const float z1 = rn_add(z, g2);
  z = rn_sub(z1, t);
  n = n1;
  if (fabsf(z) <= hp.lamda1) {  // (a NaN z compares false: the division carries it on)
    w = 0.f;
  } else {
    const float num = rn_sub(copysignf(hp.lamda1, z), z);
    const float b1 = rn_add(hp.beta, r1);
    const float d0 = rn_div(b1, hp.lr);
    const float den = rn_add(d0, hp.wd);
    w = rn_div(num, den);
  }
}

// the rescale and the clip common to every kind
__device__ __forceinline__ float grad2(float g, const KvOptHp& hp) {
  const float g1 = rn_mul(g, hp.rescale);
  return hp.has_clip ? (g1 > hp.clip ? hp.clip : (g1 < -hp.clip ? -hp.clip : g1)) : g1;  // a NaN stays
}

// one element: the rescale and the clip, then the kind's lines
template <int KIND>
__device__ __forceinline__ void opt1(float& w, float& s0, float& s1, float& s2, float g, const KvOptHp& hp) {
  const float g2 = grad2(g, hp);
  if constexpr (KIND == kNag) nag1<true>(w, s0, g2, hp);
  if constexpr (KIND == kNagPlain) nag1<false>(w, s0, g2, hp);
  if constexpr (KIND == kAdagrad) adagrad1(w, s0, g2, hp);
  if constexpr (KIND == kRmsprop) rmsprop1<false>(w, s0, s1, s2, g2, hp);
  if constexpr (KIND == kRmspropCentered) rmsprop1<true>(w, s0, s1, s2, g2, hp);
  if constexpr (KIND == kFtrl) ftrl1(w, s0, s1, g2, hp);
}

}  // namespace
