// CrazyFlie device dynamics shared by the fused env step (env_step.hip) and
// the fused GCBF+ loss prologue (loss_prep.hip): ONE definition of the
// nominal controller, xdot = f(x) + g u(x) with the low-level LQR, and the
// RK4 step, generic over the scalar type. `float` is the value path of both
// kernels; `CfDual` (value + one tangent) is forward-mode differentiation of
// the very same code, so no Jacobian is written by hand.
// State order (x,y,z, psi,theta,phi, u,v,w, r,q,p). All gains, physical
// constants and limits come from the `cst` block (crazyflie_consts.h).
// The 12-element state/stage vectors are only ever indexed by unrolled
// compile-time constants so they stay in registers.
#pragma once
#include <hip/hip_runtime.h>

#include "crazyflie_consts.h"

// ---- forward-mode dual number: v + d * eps --------------------------------
struct CfDual {
  float v, d;
  __device__ __forceinline__ CfDual() {}
  __device__ __forceinline__ CfDual(float v_) : v(v_), d(0.f) {}
  __device__ __forceinline__ CfDual(float v_, float d_) : v(v_), d(d_) {}
};

__device__ __forceinline__ CfDual operator-(const CfDual& a) { return CfDual(-a.v, -a.d); }
__device__ __forceinline__ CfDual operator+(const CfDual& a, const CfDual& b) {
  return CfDual(a.v + b.v, a.d + b.d);
}
__device__ __forceinline__ CfDual operator+(float a, const CfDual& b) {
  return CfDual(a + b.v, b.d);
}
__device__ __forceinline__ CfDual operator-(const CfDual& a, const CfDual& b) {
  return CfDual(a.v - b.v, a.d - b.d);
}
__device__ __forceinline__ CfDual operator-(float a, const CfDual& b) {
  return CfDual(a - b.v, -b.d);
}
__device__ __forceinline__ CfDual operator*(const CfDual& a, const CfDual& b) {
  return CfDual(a.v * b.v, a.d * b.v + a.v * b.d);
}
__device__ __forceinline__ CfDual operator*(float a, const CfDual& b) {
  return CfDual(a * b.v, a * b.d);
}
__device__ __forceinline__ CfDual operator*(const CfDual& a, float b) {
  return CfDual(a.v * b, a.d * b);
}
__device__ __forceinline__ CfDual operator/(const CfDual& a, const CfDual& b) {
  const float q = a.v / b.v;
  return CfDual(q, (a.d - q * b.d) / b.v);
}
__device__ __forceinline__ CfDual operator/(const CfDual& a, float b) {
  return CfDual(a.v / b, a.d / b);
}
__device__ __forceinline__ CfDual& operator+=(CfDual& a, const CfDual& b) {
  a.v += b.v;
  a.d += b.d;
  return a;
}

__device__ __forceinline__ void cf_sincos(float x, float* s, float* c) { sincosf(x, s, c); }
__device__ __forceinline__ float cf_tan(float x) { return tanf(x); }
__device__ __forceinline__ void cf_sincos(const CfDual& x, CfDual* s, CfDual* c) {
  float sv, cv;
  sincosf(x.v, &sv, &cv);
  *s = CfDual(sv, cv * x.d);
  *c = CfDual(cv, -sv * x.d);
}
__device__ __forceinline__ CfDual cf_tan(const CfDual& x) {
  const float t = tanf(x.v);
  return CfDual(t, (1.f + t * t) * x.d);
}

template <typename T>
struct CfStateT {
  T v[12];
};
typedef CfStateT<float> CfState;

// ---- nominal controller ----------------------------------------------------
// err = agent - goal with the position part rescaled to comm when farther
// than comm
__device__ __forceinline__ void crazyflie_goal_err(const CfState& x,
                                                   const float* __restrict__ gl,
                                                   const float* __restrict__ cst,
                                                   float (&err)[12]) {
#pragma unroll
  for (int s = 0; s < 12; ++s) err[s] = x.v[s] - gl[s];
  const float comm = cst[CF_COMM];
  const float dist = sqrtf(err[0] * err[0] + err[1] * err[1] + err[2] * err[2]);
  const float coef = dist > comm ? comm / fmaxf(dist, 1e-4f) : 1.f;
  err[0] *= coef;
  err[1] *= coef;
  err[2] *= coef;
}

// u_ref[u] = clip(-K_nom[u] . err)
__device__ __forceinline__ float crazyflie_uref(const float (&err)[12], int u,
                                                const float* __restrict__ cst) {
  float acc = 0.f;
#pragma unroll
  for (int s = 0; s < 12; ++s) acc += cst[CF_KNOM + u * 12 + s] * err[s];
  return fminf(fmaxf(-acc, cst[CF_ALO + u]), cst[CF_AHI + u]);
}

// ---- xdot = f(x) + g u(x), vt = scaled (clipped) velocity targets ----------
template <typename T>
__device__ __forceinline__ CfStateT<T> crazyflie_xdot(const CfStateT<T>& x, const T (&vt)[4],
                                                      const float* __restrict__ cst) {
  T sph, cph, sth, cth, sps, cps;
  cf_sincos(x.v[5], &sph, &cph);
  cf_sincos(x.v[4], &sth, &cth);
  cf_sincos(x.v[3], &sps, &cps);
  const T tth = cf_tan(x.v[4]);
  // body -> world rotation (rotmat)
  const T R00 = cps * cth, R01 = cps * sth * sph - sps * cph,
          R02 = cps * sth * cph + sps * sph;
  const T R10 = sps * cth, R11 = sps * sth * sph + cps * cph,
          R12 = sps * sth * cph - cps * sph;
  const T R20 = -sth, R21 = cth * sph, R22 = cth * cph;
  const T u = x.v[6], v = x.v[7], w = x.v[8];
  const T p = x.v[11], q = x.v[10], r = x.v[9];
  const float grav = cst[CF_GRAV];
  const float Ix = cst[CF_INERTIA], Iy = cst[CF_INERTIA + 1], Iz = cst[CF_INERTIA + 2];

  CfStateT<T> k;
  // world-frame velocity
  k.v[0] = R00 * u + R01 * v + R02 * w;
  k.v[1] = R10 * u + R11 * v + R12 * w;
  k.v[2] = R20 * u + R21 * v + R22 * w;
  // euler rates (psi., theta., phi.) = mat . pqr
  k.v[3] = (sph / cth) * q + (cph / cth) * r;
  k.v[4] = cph * q - sph * r;
  k.v[5] = p + (sph * tth) * q + (cph * tth) * r;
  // body accel: -pqr x uvw + body-frame gravity
  k.v[6] = -(q * w - r * v) - R20 * grav;
  k.v[7] = -(r * u - p * w) - R21 * grav;
  k.v[8] = -(p * v - q * u) - R22 * grav;
  // pqr. = -pqr x (I pqr) / I, stored flipped (r, q, p)
  const T Ip = Ix * p, Iq = Iy * q, Ir = Iz * r;
  k.v[11] = -(q * Ir - r * Iq) / Ix;
  k.v[10] = -(r * Ip - p * Ir) / Iy;
  k.v[9] = -(p * Iq - q * Ip) / Iz;

  // low-level LQR on (phi, theta, psi, p, q, r, v_W) - des
  T d[9];
  d[0] = x.v[5];
  d[1] = x.v[4];
  d[2] = x.v[3];
  d[3] = p;
  d[4] = q;
  d[5] = r - vt[3];
  d[6] = k.v[0] - vt[0];
  d[7] = k.v[1] - vt[1];
  d[8] = k.v[2] - vt[2];
  T motor[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    T acc = 0.f;
#pragma unroll
    for (int j = 0; j < 9; ++j) acc += cst[CF_KLL + m * 9 + j] * d[j];
    motor[m] = cst[CF_UEQ + m] - acc;
  }
  T wpqr[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    T acc = 0.f;
#pragma unroll
    for (int m = 0; m < 4; ++m) acc += cst[CF_MM + i * 4 + m] * motor[m];
    wpqr[i] = acc;
  }
  k.v[8] += wpqr[0];
  k.v[11] += wpqr[1];
  k.v[10] += wpqr[2];
  k.v[9] += wpqr[3];
  return k;
}

// ---- classic RK4, LL controller re-evaluated per stage; no state clip ------
template <typename T>
__device__ __forceinline__ CfStateT<T> crazyflie_rk4(const CfStateT<T>& x, const T (&vt)[4],
                                                     const float* __restrict__ cst) {
  const float dt = cst[CF_DT];
  const float hdt = 0.5f * dt;
  CfStateT<T> k = crazyflie_xdot(x, vt, cst);
  CfStateT<T> sum = k, xs;
#pragma unroll
  for (int s = 0; s < 12; ++s) xs.v[s] = x.v[s] + hdt * k.v[s];
  k = crazyflie_xdot(xs, vt, cst);
#pragma unroll
  for (int s = 0; s < 12; ++s) {
    sum.v[s] += 2.f * k.v[s];
    xs.v[s] = x.v[s] + hdt * k.v[s];
  }
  k = crazyflie_xdot(xs, vt, cst);
#pragma unroll
  for (int s = 0; s < 12; ++s) {
    sum.v[s] += 2.f * k.v[s];
    xs.v[s] = x.v[s] + dt * k.v[s];
  }
  k = crazyflie_xdot(xs, vt, cst);
  const float dt6 = dt / 6.f;
  CfStateT<T> xn;
#pragma unroll
  for (int s = 0; s < 12; ++s) xn.v[s] = x.v[s] + dt6 * (sum.v[s] + k.v[s]);
  return xn;
}
