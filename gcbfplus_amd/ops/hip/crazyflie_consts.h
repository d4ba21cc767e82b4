// CrazyFlie fused step: float offsets into the per-device constant block
// built by env/crazyflie.py::_fused_consts (same order; keep in sync), and
// the launch's LDS budget, shared by the kernel and its binding.
#pragma once
#include <cstddef>

enum {
  CF_KNOM = 0,       // (4, 12) nominal LQR gain
  CF_KLL = 48,       // (4, 9)  low-level LQR gain
  CF_MM = 84,        // (4, 4)  motor thrusts -> (w., p., q., r.)
  CF_UEQ = 100,      // (4,)    hover thrusts
  CF_VTS = 104,      // (4,)    velocity-target scale
  CF_INERTIA = 108,  // (3,)    Ixx, Iyy, Izz
  CF_GRAV = 111,
  CF_SLO = 112,      // (12,)   state lower limits
  CF_SHI = 124,      // (12,)   state upper limits
  CF_ALO = 136,      // (4,)    action lower limits
  CF_AHI = 140,      // (4,)    action upper limits
  CF_DRONE_R = 144,
  CF_COMM = 145,
  CF_DT = 146,
  CF_NCONST = 147
};

// dynamic LDS of crazyflie_step_kernel: next states [N][12], current
// positions [N][3], spheres [K][4], reward/collision/inside partials [4][3]
static inline size_t crazyflie_step_lds_bytes(long N, long K) {
  return (size_t)(N * 12 + N * 3 + K * 4 + 12) * sizeof(float);
}
// default per-workgroup LDS limit (no opt-in to the larger gfx950 LDS)
static const size_t CF_LDS_LIMIT = 64 * 1024;
