// CrazyFlie edge-state transform and its vjp, shared by the mode-2 kernels of
// edge_msg.hip (layer-0 GNN input, forward and backward) and the fused
// edge_grad_to_state_jac kernel: ONE definition of
//   es = [pos, R (u,v,w), R[:,2], R (p,q,r)],  R = rotmat(phi, theta, psi)
// (env/crazyflie.py `_edge_states`) and of d(es)/d(state)^T applied to a
// cotangent. State order (x,y,z, psi,theta,phi, u,v,w, r,q,p). sincosf, not
// the fast intrinsics: psi is unbounded. Arrays are indexed by compile-time
// constants only, so they stay in registers.
#pragma once
#include <hip/hip_runtime.h>

struct CfRot {
  float r00, r01, r02, r10, r11, r12, r20, r21, r22;
  float sph, cph, sth, cth, sps, cps;
};

__device__ __forceinline__ CfRot cf_rotmat(float phi, float theta, float psi) {
  CfRot m;
  sincosf(phi, &m.sph, &m.cph);
  sincosf(theta, &m.sth, &m.cth);
  sincosf(psi, &m.sps, &m.cps);
  m.r00 = m.cps * m.cth;
  m.r01 = m.cps * m.sth * m.sph - m.sps * m.cph;
  m.r02 = m.cps * m.sth * m.cph + m.sps * m.sph;
  m.r10 = m.sps * m.cth;
  m.r11 = m.sps * m.sth * m.sph + m.cps * m.cph;
  m.r12 = m.sps * m.sth * m.cph - m.cps * m.sph;
  m.r20 = -m.sth;
  m.r21 = m.cth * m.sph;
  m.r22 = m.cth * m.cph;
  return m;
}

// 12 contiguous floats on a 16 B aligned, 48 B strided row: three b128 accesses
__device__ __forceinline__ void cf_load12(const float* __restrict__ p, float (&v)[12]) {
  const float4 a = *(const float4*)p, b = *(const float4*)(p + 4), c = *(const float4*)(p + 8);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w;
}

__device__ __forceinline__ void cf_store12(float* __restrict__ p, const float (&v)[12]) {
  *(float4*)p = float4{v[0], v[1], v[2], v[3]};
  *(float4*)(p + 4) = float4{v[4], v[5], v[6], v[7]};
  *(float4*)(p + 8) = float4{v[8], v[9], v[10], v[11]};
}

// forward: st (12) -> es (12)
__device__ __forceinline__ void cf_edge_state(const float (&st)[12], float (&es)[12]) {
  const CfRot m = cf_rotmat(st[5], st[4], st[3]);
  const float u = st[6], v = st[7], w = st[8];
  const float p = st[11], q = st[10], r = st[9];
  es[0] = st[0];
  es[1] = st[1];
  es[2] = st[2];
  es[3] = m.r00 * u + m.r01 * v + m.r02 * w;
  es[4] = m.r10 * u + m.r11 * v + m.r12 * w;
  es[5] = m.r20 * u + m.r21 * v + m.r22 * w;
  es[6] = m.r02;
  es[7] = m.r12;
  es[8] = m.r22;
  es[9] = m.r00 * p + m.r01 * q + m.r02 * r;
  es[10] = m.r10 * p + m.r11 * q + m.r12 * r;
  es[11] = m.r20 * p + m.r21 * q + m.r22 * r;
}

// vjp: ds = (d es / d st)^T g at state st. The transform is linear in uvw and
// pqr (their cotangents are R^T g); the three angles see
//   sum_ij G_ij dR_ij/d(angle),  G = g_vel uvw^T + g_om pqr^T + g_z e_3^T,
// with the closed-form dR: d/dpsi swaps rows 0/1, d/dphi swaps columns 1/2.
__device__ __forceinline__ void cf_edge_state_vjp(const float (&st)[12], const float (&g)[12],
                                                  float (&ds)[12]) {
  const CfRot m = cf_rotmat(st[5], st[4], st[3]);
  const float u = st[6], v = st[7], w = st[8];
  const float p = st[11], q = st[10], r = st[9];
  ds[0] = g[0];
  ds[1] = g[1];
  ds[2] = g[2];
  // uvw and pqr: R^T g
  ds[6] = m.r00 * g[3] + m.r10 * g[4] + m.r20 * g[5];
  ds[7] = m.r01 * g[3] + m.r11 * g[4] + m.r21 * g[5];
  ds[8] = m.r02 * g[3] + m.r12 * g[4] + m.r22 * g[5];
  ds[11] = m.r00 * g[9] + m.r10 * g[10] + m.r20 * g[11];
  ds[10] = m.r01 * g[9] + m.r11 * g[10] + m.r21 * g[11];
  ds[9] = m.r02 * g[9] + m.r12 * g[10] + m.r22 * g[11];
  // G rows (i = world axis), columns (j = body axis)
  const float G00 = g[3] * u + g[9] * p, G01 = g[3] * v + g[9] * q,
              G02 = g[3] * w + g[9] * r + g[6];
  const float G10 = g[4] * u + g[10] * p, G11 = g[4] * v + g[10] * q,
              G12 = g[4] * w + g[10] * r + g[7];
  const float G20 = g[5] * u + g[11] * p, G21 = g[5] * v + g[11] * q,
              G22 = g[5] * w + g[11] * r + g[8];
  // psi: dR/dpsi = [-row1; row0; 0]
  ds[3] = -(G00 * m.r10 + G01 * m.r11 + G02 * m.r12) + (G10 * m.r00 + G11 * m.r01 + G12 * m.r02);
  // theta
  ds[4] = G00 * (-m.cps * m.sth) + G01 * (m.cps * m.cth * m.sph) + G02 * (m.cps * m.cth * m.cph) +
          G10 * (-m.sps * m.sth) + G11 * (m.sps * m.cth * m.sph) + G12 * (m.sps * m.cth * m.cph) +
          G20 * (-m.cth) + G21 * (-m.sth * m.sph) + G22 * (-m.sth * m.cph);
  // phi: dR/dphi = [0, col2, -col1]
  ds[5] = G01 * m.r02 - G02 * m.r01 + G11 * m.r12 - G12 * m.r11 + G21 * m.r22 - G22 * m.r21;
}
