// Per-environment math of the fused GCBF+ loss prologue for DubinsCar,
// LinearDrone and SingleIntegrator (kernels: env_loss_prep_{fwd,bwd}_kernel in
// loss_prep.hip, one instantiation per env struct below).
//
// Semantics are the eager branch of GCBFPlus._loss:
//   action = 2*raw + u_ref              stored UNCLAMPED
//   a_c    = clamp(action, action_lim)
//   next   = clip_state(pre),  pre = E::step(x, goal, a_c)
//   draw_c = 2*daction_c + 2 * m_act_c * sum_s m_state_s * J[s][c] * dnext_s
// with J = d pre / d a_c (pre is affine in a_c for all three envs) and
// m_act / m_state torch.clamp's inclusive pass-through masks.
//
// An env struct E provides S, NU and three device functions:
//   E::uref(x, g, p, u)      reference controller, env/<name>.py u_ref
//   E::step(x, g, ac, p, pre) pre-clip next state for the clamped action
//   E::jac(x, g, p, J)        J[s][c] = d pre[s] / d ac[c]
// All arrays are indexed by unrolled constants only (registers).
#pragma once
#include <hip/hip_runtime.h>

// By-value kernel argument. Limits are action_lim() / state_lim() of the env
// class (+-inf where a state component is unlimited: the clamp and its mask
// pass everything through), the rest its _params / tensors.
template <int S_, int NU_>
struct PrepArgs {
  float alo[NU_], ahi[NU_];  // action_lim()
  float slo[S_], shi[S_];    // state_lim()
  float dt;
  float comm;                // comm_radius
  float stop_r;              // Dubins: 0.5 * car_radius; < 0 with enable_stop off
  const float* K;            // (NU, S) LQR gain            (LQR family)
  const float* A;            // (S, S)  continuous dynamics (LinearDrone)
  const float* Bm;           // (S, NU) input matrix        (LinearDrone)
};

// u_ref of the clipped-error LQR family (env/double_integrator.py u_ref,
// env/single_integrator.py u_ref): err = goal - x, each component clipped to
// |err / ||err|| * comm|, times K^T, clipped to the action limits.
template <int S, int NU>
__device__ __forceinline__ void lqr_uref(const float* x, const float* g,
                                         const PrepArgs<S, NU>& p, float* u) {
  float err[S], nrm = 0.f;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    err[s] = g[s] - x[s];
    nrm += err[s] * err[s];
  }
  nrm = fmaxf(sqrtf(nrm), 1e-9f);
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const float emax = fabsf(err[s] / nrm * p.comm);
    err[s] = fminf(fmaxf(err[s], -emax), emax);
  }
#pragma unroll
  for (int c = 0; c < NU; ++c) {
    float acc = 0.f;
#pragma unroll
    for (int s = 0; s < S; ++s) acc += p.K[c * S + s] * err[s];
    u[c] = fminf(fmaxf(acc, p.alo[c]), p.ahi[c]);
  }
}

// ---- SingleIntegrator: state (x, y), action (vx, vy), xdot = a --------------
struct SiPrep {
  static constexpr int S = 2, NU = 2;
  typedef PrepArgs<2, 2> Args;
  static __device__ __forceinline__ void uref(const float* x, const float* g, const Args& p,
                                              float* u) {
    lqr_uref<2, 2>(x, g, p, u);
  }
  static __device__ __forceinline__ void step(const float* x, const float*, const float* ac,
                                              const Args& p, float* pre) {
    pre[0] = x[0] + ac[0] * p.dt;
    pre[1] = x[1] + ac[1] * p.dt;
  }
  static __device__ __forceinline__ void jac(const float*, const float*, const Args& p,
                                             float (*J)[2]) {
    J[0][0] = p.dt, J[0][1] = 0.f;
    J[1][0] = 0.f, J[1][1] = p.dt;
  }
};

// ---- LinearDrone: state (pos, vel) in 3D, xdot = A x + B a ------------------
struct DronePrep {
  static constexpr int S = 6, NU = 3;
  typedef PrepArgs<6, 3> Args;
  static __device__ __forceinline__ void uref(const float* x, const float* g, const Args& p,
                                              float* u) {
    lqr_uref<6, 3>(x, g, p, u);
  }
  static __device__ __forceinline__ void step(const float* x, const float*, const float* ac,
                                              const Args& p, float* pre) {
#pragma unroll
    for (int s = 0; s < 6; ++s) {
      float ax = 0.f, bu = 0.f;
#pragma unroll
      for (int j = 0; j < 6; ++j) ax += p.A[s * 6 + j] * x[j];
#pragma unroll
      for (int c = 0; c < 3; ++c) bu += p.Bm[s * 3 + c] * ac[c];
      pre[s] = x[s] + (ax + bu) * p.dt;
    }
  }
  static __device__ __forceinline__ void jac(const float*, const float*, const Args& p,
                                             float (*J)[3]) {
#pragma unroll
    for (int s = 0; s < 6; ++s)
#pragma unroll
      for (int c = 0; c < 3; ++c) J[s][c] = p.Bm[s * 3 + c] * p.dt;
  }
};

// ---- DubinsCar: state (x, y, theta, v), action (omega, acc) -----------------
// The PID gains, the omega clamp of 5 and the x20 on omega are literals in
// env/dubins_car.py too (u_ref, agent_xdot): change both places together.
struct DubinsPrep {
  static constexpr int S = 4, NU = 2;
  typedef PrepArgs<4, 2> Args;
  static constexpr float K_OMEGA = 1.f, K_V = 2.3f, K_A = 2.5f;  // u_ref gains
  static constexpr float OMEGA_MAX = 5.f;                       // u_ref omega clamp
  static constexpr float OMEGA_GAIN = 20.f;                     // agent_xdot theta row

  // python's x % (2 pi) for floats: exact fmod, shifted into [0, 2 pi)
  static __device__ __forceinline__ float mod_2pi(float x) {
    const float TWO_PI = 6.283185307179586f;
    const float r = fmodf(x, TWO_PI);
    return r < 0.f ? r + TWO_PI : r;
  }
  // 1 - stop of _step_states: 0 freezes an agent within stop_r of its goal
  static __device__ __forceinline__ float go(const float* x, const float* g, const Args& p) {
    const float dx = x[0] - g[0], dy = x[1] - g[1];
    return sqrtf(dx * dx + dy * dy) < p.stop_r ? 0.f : 1.f;
  }
  static __device__ __forceinline__ void uref(const float* x, const float* g, const Args& p,
                                              float* u) {
    const float PI = 3.14159265358979f;
    const float pdx = x[0] - g[0], pdy = x[1] - g[1];
    const float sq = pdx * pdx + pdy * pdy;
    const float dist = sqrtf(sq);
    const float theta_t = mod_2pi(atan2f(-pdy, -pdx));
    const float theta = mod_2pi(x[2]);
    const float theta_diff = theta_t - theta;
    const float inner = (-pdx * cosf(theta) - pdy * sinf(theta)) / (dist + 1e-4f);
    const float between = acosf(fminf(fmaxf(inner, -1.f), 1.f));
    const bool fwd = theta_diff < PI && theta_diff >= 0.f;
    const bool bwd = theta_diff > -PI && theta_diff <= 0.f;
    const float omega = theta <= PI ? (fwd ? K_OMEGA * between : -K_OMEGA * between)
                                    : (bwd ? -K_OMEGA * between : K_OMEGA * between);
    u[0] = fminf(fmaxf(omega, -OMEGA_MAX), OMEGA_MAX);
    const float nrm = sqrtf(1e-6f + sq);
    const float coef = nrm > p.comm ? p.comm / nrm : 1.f;
    const float qx = coef * pdx, qy = coef * pdy;
    u[1] = -K_A * x[3] + K_V * sqrtf(qx * qx + qy * qy);
  }
  static __device__ __forceinline__ void step(const float* x, const float* g, const float* ac,
                                              const Args& p, float* pre) {
    const float m = go(x, g, p);
    pre[0] = x[0] + cosf(x[2]) * x[3] * m * p.dt;
    pre[1] = x[1] + sinf(x[2]) * x[3] * m * p.dt;
    pre[2] = x[2] + ac[0] * OMEGA_GAIN * m * p.dt;
    pre[3] = x[3] + ac[1] * m * p.dt;
  }
  static __device__ __forceinline__ void jac(const float* x, const float* g, const Args& p,
                                             float (*J)[2]) {
    const float m = go(x, g, p);
    J[0][0] = 0.f, J[0][1] = 0.f;
    J[1][0] = 0.f, J[1][1] = 0.f;
    J[2][0] = OMEGA_GAIN * m * p.dt, J[2][1] = 0.f;
    J[3][0] = 0.f, J[3][1] = m * p.dt;
  }
};

template <class E>
__global__ void env_loss_prep_fwd_kernel(const float* __restrict__ states,  // (B,V,S)
                                         const float* __restrict__ raw,     // (B,N,NU)
                                         float* __restrict__ action,        // (B,N,NU)
                                         float* __restrict__ big,           // (2B,V,S)
                                         int B, int V, int N, const typename E::Args p);

template <class E>
__global__ void env_loss_prep_bwd_kernel(const float* __restrict__ states,   // (B,V,S)
                                         const float* __restrict__ action,   // (B,N,NU) unclamped
                                         const float* __restrict__ daction,  // (B,N,NU)
                                         const float* __restrict__ dbig,     // (2B,V,S)
                                         float* __restrict__ draw,           // (B,N,NU)
                                         int B, int V, int N, const typename E::Args p);
