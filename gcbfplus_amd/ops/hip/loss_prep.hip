// Fused GCBF+ minibatch prologue for the DoubleIntegrator family:
//   u_ref (clipped-error LQR)  ->  action = clamp(2*actor_raw + u_ref)
//   next_agent = clip_state(euler(agent, action))
//   big_states = [ states ; next_states ]   (the 2B-batched CBF input)
// Replaces ~20 eager kernels per minibatch. Backward chains to actor_raw
// only (mb states are leaves): dactor = 2 * m_act o (daction +
// (dt/m) * m_vel o dnext_vel).
// The CrazyFlie prologue (RK4, dual-number backward) follows further down.
#include "common.h"

__launch_bounds__(256) __global__
void di_loss_prep_fwd_kernel(const float* __restrict__ states,  // (B,V,4)
                             const float* __restrict__ raw,     // (B,N,2)
                             const float* __restrict__ Kmat,    // (2,4)
                             float* __restrict__ action,        // (B,N,2)
                             float* __restrict__ big,           // (2B,V,4)
                             int B, int V, int N, float dt, float inv_m,
                             float comm, float vmax) {
  const long rows = (long)2 * B * V;
  for (long row = (long)blockIdx.x * blockDim.x + threadIdx.x; row < rows;
       row += (long)gridDim.x * blockDim.x) {
    const int v = row % V;
    const long bb = row / V;
    const int half = bb / B;     // 0: current, 1: next
    const int b = bb % B;
    const float* src = states + ((long)b * V + v) * 4;
    float* dst = big + row * 4;
    if (half == 0 || v >= N) {
      *(float4*)dst = *(const float4*)src;
      continue;
    }
    // next agent state for agent i = v
    const int i = v;
    const float* gl = states + ((long)b * V + N + i) * 4;
    float err[4], nrm = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      err[s] = gl[s] - src[s];
      nrm += err[s] * err[s];
    }
    nrm = fmaxf(sqrtf(nrm), 1e-9f);
    float uref[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int s0 = u * 4;
      float e2[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float emax = fabsf(err[s] / nrm * comm);
        e2[s] = fminf(fmaxf(err[s], -emax), emax);
      }
      float acc = 0.f;
#pragma unroll
      for (int s = 0; s < 4; ++s) acc += Kmat[s0 + s] * e2[s];
      uref[u] = fminf(fmaxf(acc, -1.f), 1.f);
    }
    float act[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      act[u] = fminf(fmaxf(2.f * raw[((long)b * N + i) * 2 + u] + uref[u], -1.f), 1.f);
      action[((long)b * N + i) * 2 + u] = act[u];
    }
    dst[0] = src[0] + src[2] * dt;
    dst[1] = src[1] + src[3] * dt;
    dst[2] = fminf(fmaxf(src[2] + act[0] * inv_m * dt, -vmax), vmax);
    dst[3] = fminf(fmaxf(src[3] + act[1] * inv_m * dt, -vmax), vmax);
  }
}

__launch_bounds__(256) __global__
void di_loss_prep_bwd_kernel(const float* __restrict__ states, const float* __restrict__ raw,
                             const float* __restrict__ Kmat, const float* __restrict__ action,
                             const float* __restrict__ daction,  // (B,N,2)
                             const float* __restrict__ dbig,     // (2B,V,4)
                             float* __restrict__ draw,           // (B,N,2)
                             int B, int V, int N, float dt, float inv_m, float comm,
                             float vmax) {
  const long total = (long)B * N;
  for (long it = (long)blockIdx.x * blockDim.x + threadIdx.x; it < total;
       it += (long)gridDim.x * blockDim.x) {
    const int i = it % N;
    const int b = it / N;
    const float* src = states + ((long)b * V + i) * 4;
    const float* gl = states + ((long)b * V + N + i) * 4;
    const float* dnx = dbig + (((long)(B + b)) * V + i) * 4;
    // recompute u_ref for the pre-clamp action (clamp-mask needs it)
    float err[4], nrm = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      err[s] = gl[s] - src[s];
      nrm += err[s] * err[s];
    }
    nrm = fmaxf(sqrtf(nrm), 1e-9f);
    float e2[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const float emax = fabsf(err[s] / nrm * comm);
      e2[s] = fminf(fmaxf(err[s], -emax), emax);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      float uref = 0.f;
#pragma unroll
      for (int s = 0; s < 4; ++s) uref += Kmat[u * 4 + s] * e2[s];
      uref = fminf(fmaxf(uref, -1.f), 1.f);
      const float pre = 2.f * raw[it * 2 + u] + uref;
      const float m_act = (pre >= -1.f && pre <= 1.f) ? 1.f : 0.f;
      const float a = action[it * 2 + u];
      const float vel_pre = src[2 + u] + a * inv_m * dt;
      const float m_vel = (fabsf(vel_pre) <= vmax) ? 1.f : 0.f;
      const float dact = daction[it * 2 + u] + dnx[2 + u] * m_vel * inv_m * dt;
      draw[it * 2 + u] = 2.f * m_act * dact;
    }
  }
}

// ---------------------------------------------------------------------------
// CrazyFlie prologue (env/crazyflie.py u_ref + forward_graph):
//   action = 2*raw + u_ref, stored UNCLAMPED (the action loss sees it so)
//   next_agent = clip_state(RK4(x, clamp(action) * vel_targets_scale)), the
//                low-level LQR re-evaluated per stage
//   big = [ states ; next_states ]
// The dynamics are crazyflie_dyn.h, shared with the env step kernel: float
// for the values, CfDual (value + one tangent) for the backward, which
// recomputes the RK4 with the tangent seeded on one action component, so
// d x_next / d a[c] covers both df/dx (through the stage states) and df/du.
//   draw[c] = 2*daction[c] + 2 * m_act[c] * sum_s m_state[s] * dnext[s]
//             * d x_next[s] / d a[c]
// m_act / m_state are torch.clamp's inclusive pass-through masks.
// State and stage vectors are indexed by unrolled constants only (registers).
// ---------------------------------------------------------------------------
#include "crazyflie_dyn.h"

__launch_bounds__(256) __global__
void crazyflie_loss_prep_fwd_kernel(const float* __restrict__ states,  // (B,V,12)
                                    const float* __restrict__ raw,     // (B,N,4)
                                    const float* __restrict__ cst,     // (CF_NCONST,)
                                    float* __restrict__ action,        // (B,N,4)
                                    float* __restrict__ big,           // (2B,V,12)
                                    int B, int V, int N) {
  const long rows = (long)2 * B * V;
  for (long row = (long)blockIdx.x * blockDim.x + threadIdx.x; row < rows;
       row += (long)gridDim.x * blockDim.x) {
    const int v = row % V;
    const long bb = row / V;
    const int half = bb / B;     // 0: current, 1: next
    const int b = bb % B;
    const float4* src = (const float4*)(states + ((long)b * V + v) * 12);
    float4* dst = (float4*)(big + row * 12);
    const float4 s0 = src[0], s1 = src[1], s2 = src[2];
    if (half == 0 || v >= N) {
      dst[0] = s0;
      dst[1] = s1;
      dst[2] = s2;
      continue;
    }
    // next agent state for agent i = v
    const int i = v;
    CfState x;
    x.v[0] = s0.x, x.v[1] = s0.y, x.v[2] = s0.z, x.v[3] = s0.w;
    x.v[4] = s1.x, x.v[5] = s1.y, x.v[6] = s1.z, x.v[7] = s1.w;
    x.v[8] = s2.x, x.v[9] = s2.y, x.v[10] = s2.z, x.v[11] = s2.w;
    float err[12];
    crazyflie_goal_err(x, states + ((long)b * V + N + i) * 12, cst, err);
    const float4 rw = *(const float4*)(raw + ((long)b * N + i) * 4);
    const float r4[4] = {rw.x, rw.y, rw.z, rw.w};
    float act[4], vt[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      act[u] = 2.f * r4[u] + crazyflie_uref(err, u, cst);
      vt[u] = fminf(fmaxf(act[u], cst[CF_ALO + u]), cst[CF_AHI + u]) * cst[CF_VTS + u];
    }
    *(float4*)(action + ((long)b * N + i) * 4) = make_float4(act[0], act[1], act[2], act[3]);
    const CfState xn = crazyflie_rk4(x, vt, cst);
    float o[12];
#pragma unroll
    for (int s = 0; s < 12; ++s)
      o[s] = fminf(fmaxf(xn.v[s], cst[CF_SLO + s]), cst[CF_SHI + s]);
    dst[0] = make_float4(o[0], o[1], o[2], o[3]);
    dst[1] = make_float4(o[4], o[5], o[6], o[7]);
    dst[2] = make_float4(o[8], o[9], o[10], o[11]);
  }
}

// one thread per (b, i, c): the dual RK4 seeded on action component c
__launch_bounds__(256) __global__
void crazyflie_loss_prep_bwd_kernel(const float* __restrict__ states,   // (B,V,12)
                                    const float* __restrict__ cst,      // (CF_NCONST,)
                                    const float* __restrict__ action,   // (B,N,4) unclamped
                                    const float* __restrict__ daction,  // (B,N,4)
                                    const float* __restrict__ dbig,     // (2B,V,12)
                                    float* __restrict__ draw,           // (B,N,4)
                                    int B, int V, int N) {
  const long total = (long)B * N * 4;
  for (long it = (long)blockIdx.x * blockDim.x + threadIdx.x; it < total;
       it += (long)gridDim.x * blockDim.x) {
    const int c = it & 3;
    const long ag = it >> 2;  // b * N + i
    const int i = ag % N;
    const long b = ag / N;
    const float4 aw = *(const float4*)(action + ag * 4);
    const float a4[4] = {aw.x, aw.y, aw.z, aw.w};
    const float pre = action[it];
    const float two_da = 2.f * daction[it];
    if (!(pre >= cst[CF_ALO + c] && pre <= cst[CF_AHI + c])) {
      draw[it] = two_da;  // clamp active: nothing flows from the dynamics
      continue;
    }
    const float4* src = (const float4*)(states + (b * V + i) * 12);
    const float4 s0 = src[0], s1 = src[1], s2 = src[2];
    CfStateT<CfDual> x;
    x.v[0] = s0.x, x.v[1] = s0.y, x.v[2] = s0.z, x.v[3] = s0.w;
    x.v[4] = s1.x, x.v[5] = s1.y, x.v[6] = s1.z, x.v[7] = s1.w;
    x.v[8] = s2.x, x.v[9] = s2.y, x.v[10] = s2.z, x.v[11] = s2.w;
    CfDual vt[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float scale = cst[CF_VTS + u];
      vt[u] = CfDual(fminf(fmaxf(a4[u], cst[CF_ALO + u]), cst[CF_AHI + u]) * scale,
                     u == c ? scale : 0.f);
    }
    const CfStateT<CfDual> xn = crazyflie_rk4(x, vt, cst);
    const float4* dn = (const float4*)(dbig + ((B + b) * V + i) * 12);
    const float4 d0 = dn[0], d1 = dn[1], d2 = dn[2];
    const float g[12] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y,
                         d1.z, d1.w, d2.x, d2.y, d2.z, d2.w};
    float acc = 0.f;
#pragma unroll
    for (int s = 0; s < 12; ++s) {
      const bool pass = xn.v[s].v >= cst[CF_SLO + s] && xn.v[s].v <= cst[CF_SHI + s];
      acc += pass ? g[s] * xn.v[s].d : 0.f;
    }
    draw[it] = two_da + 2.f * acc;
  }
}

// ---------------------------------------------------------------------------
// DubinsCar / LinearDrone / SingleIntegrator prologue: one templated kernel
// pair over the per-env structs of loss_prep_envs.h (u_ref, step, jacobian in
// one place per env). Same contract as the CrazyFlie prologue above: action
// stored unclamped, dynamics on the clamped action, gradient to raw only.
// ---------------------------------------------------------------------------
#include "loss_prep_envs.h"

// Row moves use the widest vector the row stride keeps aligned on a 16-byte
// aligned base: 16 B for W % 4 == 0, 8 B for even W (24-byte S = 6 rows are
// only 8-byte aligned), scalars otherwise (NU = 3).
template <int W>
__device__ __forceinline__ void load_vec(const float* __restrict__ p, float* r) {
  if constexpr (W % 4 == 0) {
#pragma unroll
    for (int k = 0; k < W / 4; ++k) {
      const float4 t = ((const float4*)p)[k];
      r[4 * k] = t.x, r[4 * k + 1] = t.y, r[4 * k + 2] = t.z, r[4 * k + 3] = t.w;
    }
  } else if constexpr (W % 2 == 0) {
#pragma unroll
    for (int k = 0; k < W / 2; ++k) {
      const float2 t = ((const float2*)p)[k];
      r[2 * k] = t.x, r[2 * k + 1] = t.y;
    }
  } else {
#pragma unroll
    for (int k = 0; k < W; ++k) r[k] = p[k];
  }
}

template <int W>
__device__ __forceinline__ void store_vec(float* __restrict__ p, const float* r) {
  if constexpr (W % 4 == 0) {
#pragma unroll
    for (int k = 0; k < W / 4; ++k)
      ((float4*)p)[k] = make_float4(r[4 * k], r[4 * k + 1], r[4 * k + 2], r[4 * k + 3]);
  } else if constexpr (W % 2 == 0) {
#pragma unroll
    for (int k = 0; k < W / 2; ++k) ((float2*)p)[k] = make_float2(r[2 * k], r[2 * k + 1]);
  } else {
#pragma unroll
    for (int k = 0; k < W; ++k) p[k] = r[k];
  }
}

template <class E>
__launch_bounds__(256) __global__
void env_loss_prep_fwd_kernel(const float* __restrict__ states, const float* __restrict__ raw,
                              float* __restrict__ action, float* __restrict__ big,
                              int B, int V, int N, const typename E::Args p) {
  constexpr int S = E::S, NU = E::NU;
  const long rows = (long)2 * B * V;
  for (long row = (long)blockIdx.x * blockDim.x + threadIdx.x; row < rows;
       row += (long)gridDim.x * blockDim.x) {
    const int v = row % V;
    const long bb = row / V;
    const int half = bb / B;     // 0: current, 1: next
    const long b = bb % B;
    float x[S];
    load_vec<S>(states + (b * V + v) * S, x);
    float* dst = big + row * S;
    if (half == 0 || v >= N) {
      store_vec<S>(dst, x);
      continue;
    }
    // next agent state for agent i = v
    const long ag = b * N + v;
    float g[S], r[NU], u[NU], act[NU], ac[NU], pre[S];
    load_vec<S>(states + (b * V + N + v) * S, g);
    load_vec<NU>(raw + ag * NU, r);
    E::uref(x, g, p, u);
#pragma unroll
    for (int c = 0; c < NU; ++c) {
      act[c] = 2.f * r[c] + u[c];
      ac[c] = fminf(fmaxf(act[c], p.alo[c]), p.ahi[c]);
    }
    store_vec<NU>(action + ag * NU, act);
    E::step(x, g, ac, p, pre);
#pragma unroll
    for (int s = 0; s < S; ++s) pre[s] = fminf(fmaxf(pre[s], p.slo[s]), p.shi[s]);
    store_vec<S>(dst, pre);
  }
}

// one thread per (b, agent); no atomics, every draw element written once
template <class E>
__launch_bounds__(256) __global__
void env_loss_prep_bwd_kernel(const float* __restrict__ states,
                              const float* __restrict__ action,
                              const float* __restrict__ daction,
                              const float* __restrict__ dbig, float* __restrict__ draw,
                              int B, int V, int N, const typename E::Args p) {
  constexpr int S = E::S, NU = E::NU;
  const long total = (long)B * N;
  for (long ag = (long)blockIdx.x * blockDim.x + threadIdx.x; ag < total;
       ag += (long)gridDim.x * blockDim.x) {
    const int i = ag % N;
    const long b = ag / N;
    float x[S], g[S], act[NU], ac[NU], da[NU], dn[S], pre[S], J[S][NU], out[NU];
    load_vec<S>(states + (b * V + i) * S, x);
    load_vec<S>(states + (b * V + N + i) * S, g);
    load_vec<NU>(action + ag * NU, act);
    load_vec<NU>(daction + ag * NU, da);
    load_vec<S>(dbig + ((B + b) * V + i) * S, dn);
#pragma unroll
    for (int c = 0; c < NU; ++c) ac[c] = fminf(fmaxf(act[c], p.alo[c]), p.ahi[c]);
    // the pre-clip next state again: clip_state's mask
    E::step(x, g, ac, p, pre);
    E::jac(x, g, p, J);
#pragma unroll
    for (int c = 0; c < NU; ++c) {
      float acc = 0.f;
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const bool pass = pre[s] >= p.slo[s] && pre[s] <= p.shi[s] && J[s][c] != 0.f;
        acc += pass ? dn[s] * J[s][c] : 0.f;
      }
      const float two_da = 2.f * da[c];
      // clamp active: nothing flows from the dynamics
      out[c] = (act[c] >= p.alo[c] && act[c] <= p.ahi[c]) ? two_da + 2.f * acc : two_da;
    }
    store_vec<NU>(draw + ag * NU, out);
  }
}

#define INSTANTIATE_ENV_LOSS_PREP(E)                                                       \
  template __global__ void env_loss_prep_fwd_kernel<E>(const float*, const float*, float*, \
                                                       float*, int, int, int,              \
                                                       const E::Args);                     \
  template __global__ void env_loss_prep_bwd_kernel<E>(const float*, const float*,         \
                                                       const float*, const float*, float*, \
                                                       int, int, int, const E::Args);
INSTANTIATE_ENV_LOSS_PREP(SiPrep)
INSTANTIATE_ENV_LOSS_PREP(DronePrep)
INSTANTIATE_ENV_LOSS_PREP(DubinsPrep)
