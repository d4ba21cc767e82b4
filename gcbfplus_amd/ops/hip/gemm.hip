// MFMA GEMM kernels for the GNN MLP stack.
//
// The networks are stacks of Dense layers with K, N in {16..384} and M up to
// ~3e5 rows (batch * agents * edge-slots), bf16 inputs / f32 accumulate.
// Kernel family (launcher picks by shape, bindings.hip):
//   gemm_bias_act_kernel      : Y = act(X @ W + b), 128x64 tile, BK=32;
//                               B staged once per block in a fragment-blocked
//                               LDS image, A staged per K-tile. Template
//                               <ACT, BT, ACTIN>: BT consumes W^T through a
//                               transposed B-stage (backward dX without a
//                               transpose copy); ACTIN folds the upstream
//                               activation backward into the A-stage.
//   gemm_bias_act_panel_kernel: row panel for M%128==0, K%64==0, K<=384: a
//                               workgroup keeps 128 rows of X in LDS and
//                               produces every output column; X, W by
//                               global_load_lds ("glds" / "glds_bt" paths).
//   gemm_bias_act_sm_kernel   : 32x64 tile so mid-size M still fills 256 CUs.
//   dot_bias_act_kernel       : N == 1 gate/head outputs, thread-per-row.
//   gemv_bias_act_kernel      : 2 <= N <= 16 outputs, wave-per-row, f32 out.
//   gemm_tn_partial + reduce  : dW = X^T @ dZ, deterministic split-M partials
//                               + fixed-order reduction (no atomics), with
//                               fused db and optional upstream-act fold.
//   ..._grouped_kernel        : the small-M (tn1) partial and the reduce for
//                               up to 16 independent problems per launch
//                               (deferred dW: gemm_tn_defer / dw_flush).
// Device row count: dot, gemv, sm, the 128x64 kernel, the row panel, tn1 and
// tn3 take a last argument m_dev (null, or one int32 in device memory) and
// work on min(*m_dev, M) rows: workgroups past it leave at entry, the dW
// kernels spread the live rows over their S slabs. Grids and plans stay those
// of the static M, so edge-compacted calls replay from a captured graph with
// any count (edge_compact.hip). With m_dev null nothing changes. Training
// gives tn1 / tn3 a row map instead (tn_map_row): the dense call's summation
// order over compact operands, so dW/db keep the dense call's bits. With a
// map tn3 runs gemm_tn_partial3_map_kernel, which stages the live rows only.
#include "common.h"
#include "dw_group.h"


// ---------------------------------------------------------------------------
// B-operand staging into the k-blocked LDS image sB[[K/8][BN=64][8]].
// BT=false: W is (K, N) row-major, stage cols n0..n0+63.
// BT=true:  W is the ORIGINAL forward weight (N_out, K) row-major and the
//           GEMM consumes W^T — stage rows n0..n0+63 transposed, so the
//           backward dX = dZ @ W^T needs NO materialized transpose copy.
// ---------------------------------------------------------------------------
template <bool BT>
__device__ __forceinline__ void stage_B_image(const bf16_t* __restrict__ W, bf16_t* sB,
                                              int N, int K, int n0, int tid) {
  constexpr int BN = 64;
  if constexpr (!BT) {
    for (int c = tid; c < K * 8; c += 256) {
      const int k = c >> 3;
      const int co = (c & 7) * 8;
      bf16_t v[8];
      // b128 loads need 16-B alignment: row base k*N is aligned only when
      // N % 8 == 0 (N = 20, 70, ... take the scalar path for every chunk)
      if (n0 + co + 7 < N && (N & 7) == 0) {
        *(bf16x8*)v = *(const bf16x8*)(W + (long)k * N + n0 + co);
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i)
          v[i] = (n0 + co + i < N) ? W[(long)k * N + n0 + co + i] : (bf16_t)0.f;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) sB[((k >> 3) * BN + (co + i)) * 8 + (k & 7)] = v[i];
    }
  } else {
    const int kch = K >> 3;  // K % 8 == 0 (launcher enforces)
    for (int c = tid; c < BN * kch; c += 256) {
      const int r = c / kch;
      const int kc = (c % kch) * 8;
      bf16_t v[8];
      if (n0 + r < N) {
        *(bf16x8*)v = *(const bf16x8*)(W + (long)(n0 + r) * K + kc);
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (bf16_t)0.f;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i)
        sB[(((kc + i) >> 3) * BN + r) * 8 + ((kc + i) & 7)] = v[i];
    }
  }
}

// ---------------------------------------------------------------------------
// Y[M,N] = act(X[M,K] @ W[K,N] + bias[N]);  K % 32 == 0 (launcher pads).
// grid: (ceil(M/128), ceil(N/64)); block: 256 threads (4 waves, 2x2).
// LDS: B-block [K/8][64][8] (k-blocked so B-fragments are single b128 reads)
//      + A-tile [128][40] (pad 32->40 kills b128 bank conflicts).
// ---------------------------------------------------------------------------
template <int ACT, bool BT, int ACTIN>
__launch_bounds__(256) __global__
void gemm_bias_act_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ W,
                          const float* __restrict__ bias, bf16_t* __restrict__ Y,
                          const bf16_t* __restrict__ Xact, int M, int N, int K,
                          const int* __restrict__ m_dev) {
  constexpr int BM = 128, BN = 64, BK = 32, APAD = 40;
  extern __shared__ char smem[];
  bf16_t* sB = (bf16_t*)smem;                    // [K/8][BN][8]
  bf16_t* sA = (bf16_t*)(smem + (K / 8) * BN * 8 * sizeof(bf16_t));  // [BM][APAD]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int wm = w >> 1, wn = w & 1;  // wave tile: 64(M) x 32(N)
  const int m0 = blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  M = live_rows(m_dev, M);
  if (m0 >= M) return;  // block-uniform, ahead of every barrier and LDS write

  // ---- preload W block n0..n0+63 into k-blocked LDS image ----------------
  // chunk c -> k = c>>3, col8 = (c&7)*8 ; threads cover K*8 chunks.
  stage_B_image<BT>(W, sB, N, K, n0, tid);

  f32x4 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int arow = tid >> 1;            // A-stage: 2 threads per row
  const int acol = (tid & 1) * 16;      // each stages 16 bf16 = 32 B
  for (int k0 = 0; k0 < K; k0 += BK) {
    __syncthreads();
    // stage A[m0..+128][k0..+32]
    bf16_t av[16];
    const long arow_g = (long)(m0 + arow);
    if (arow_g < M) {
      *(bf16x8*)av = *(const bf16x8*)(X + arow_g * K + k0 + acol);
      *(bf16x8*)(av + 8) = *(const bf16x8*)(X + arow_g * K + k0 + acol + 8);
      if constexpr (ACTIN != 0) {
        // X operand is dY of an activated layer: fold dZ = dY * act'(Y)
        bf16_t yv[16];
        *(bf16x8*)yv = *(const bf16x8*)(Xact + arow_g * K + k0 + acol);
        *(bf16x8*)(yv + 8) = *(const bf16x8*)(Xact + arow_g * K + k0 + acol + 8);
#pragma unroll
        for (int i = 0; i < 16; ++i)
          av[i] = (bf16_t)((float)av[i] * act_grad_from_out((float)yv[i], ACTIN));
      }
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) av[i] = (bf16_t)0.f;
    }
#pragma unroll
    for (int i = 0; i < 16; i += 8) *(bf16x8*)(sA + arow * APAD + acol + i) = *(bf16x8*)(av + i);
    __syncthreads();

    // fragments + MFMA
    bf16x8 afr[4];
#pragma unroll
    for (int mf = 0; mf < 4; ++mf)
      afr[mf] = *(const bf16x8*)(sA + (wm * 64 + mf * 16 + (lane & 15)) * APAD + (lane >> 4) * 8);
    bf16x8 bfr[2];
#pragma unroll
    for (int nf = 0; nf < 2; ++nf)
      bfr[nf] = *(const bf16x8*)(sB + (((k0 >> 3) + (lane >> 4)) * BN + wn * 32 + nf * 16 + (lane & 15)) * 8);
#pragma unroll
    for (int mf = 0; mf < 4; ++mf)
#pragma unroll
      for (int nf = 0; nf < 2; ++nf)
        acc[mf][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr[mf], bfr[nf], acc[mf][nf], 0, 0, 0);
  }

  // ---- epilogue: bias + activation + bf16 store --------------------------
#pragma unroll
  for (int mf = 0; mf < 4; ++mf) {
#pragma unroll
    for (int nf = 0; nf < 2; ++nf) {
      const int col = n0 + wn * 32 + nf * 16 + (lane & 15);
      if (col >= N) continue;
      const float bv = bias[col];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long row = m0 + wm * 64 + mf * 16 + (lane >> 4) * 4 + r;
        if (row < M) Y[row * N + col] = (bf16_t)apply_act(acc[mf][nf][r] + bv, ACT);
      }
    }
  }
}


// ---------------------------------------------------------------------------
// Small-M variant: BM=32 x BN=64 tile (4 waves as 2x2, wave 16x32) so
// mid-size rows (update/head layers, M ~ 2k) still fill all 256 CUs.
// ---------------------------------------------------------------------------
template <int ACT, bool BT, int ACTIN>
__launch_bounds__(256) __global__
void gemm_bias_act_sm_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ W,
                             const float* __restrict__ bias, bf16_t* __restrict__ Y,
                             const bf16_t* __restrict__ Xact, int M, int N, int K,
                             const int* __restrict__ m_dev) {
  constexpr int BM = 32, BN = 64, BK = 32, APAD = 40;
  extern __shared__ char smem[];
  bf16_t* sB = (bf16_t*)smem;                                        // [K/8][BN][8]
  bf16_t* sA = (bf16_t*)(smem + (K / 8) * BN * 8 * sizeof(bf16_t));  // [BM][APAD]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int wm = w >> 1, wn = w & 1;  // wave tile: 16(M) x 32(N)
  const int m0 = blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  M = live_rows(m_dev, M);
  if (m0 >= M) return;  // block-uniform, ahead of every barrier and LDS write

  stage_B_image<BT>(W, sB, N, K, n0, tid);

  f32x4 acc[1][2];
  acc[0][0] = f32x4{0.f, 0.f, 0.f, 0.f};
  acc[0][1] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int arow = tid >> 3;           // 32 rows x 8 threads per row
  const int acol = (tid & 7) * 4;      // 4 bf16 (8 B) per thread
  for (int k0 = 0; k0 < K; k0 += BK) {
    __syncthreads();
    bf16_t av[4];
    const long arow_g = (long)(m0 + arow);
    if (arow_g < M) {
      *(uint2*)av = *(const uint2*)(X + arow_g * K + k0 + acol);
      if constexpr (ACTIN != 0) {
        bf16_t yv[4];
        *(uint2*)yv = *(const uint2*)(Xact + arow_g * K + k0 + acol);
#pragma unroll
        for (int i = 0; i < 4; ++i)
          av[i] = (bf16_t)((float)av[i] * act_grad_from_out((float)yv[i], ACTIN));
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) av[i] = (bf16_t)0.f;
    }
    *(uint2*)(sA + arow * APAD + acol) = *(uint2*)av;
    __syncthreads();

    bf16x8 afr = *(const bf16x8*)(sA + (wm * 16 + (lane & 15)) * APAD + (lane >> 4) * 8);
    bf16x8 bfr[2];
#pragma unroll
    for (int nf = 0; nf < 2; ++nf)
      bfr[nf] = *(const bf16x8*)(sB + (((k0 >> 3) + (lane >> 4)) * BN + wn * 32 + nf * 16 + (lane & 15)) * 8);
#pragma unroll
    for (int nf = 0; nf < 2; ++nf)
      acc[0][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr, bfr[nf], acc[0][nf], 0, 0, 0);
  }

#pragma unroll
  for (int nf = 0; nf < 2; ++nf) {
    const int col = n0 + wn * 32 + nf * 16 + (lane & 15);
    if (col >= N) continue;
    const float bv = bias[col];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long row = m0 + wm * 16 + (lane >> 4) * 4 + r;
      if (row < M) Y[row * N + col] = (bf16_t)apply_act(acc[0][nf][r] + bv, ACT);
    }
  }
}

template __global__ void gemm_bias_act_sm_kernel<0, false, 0>(const bf16_t*, const bf16_t*, const float*, bf16_t*, const bf16_t*, int, int, int, const int*);
template __global__ void gemm_bias_act_sm_kernel<1, false, 0>(const bf16_t*, const bf16_t*, const float*, bf16_t*, const bf16_t*, int, int, int, const int*);
template __global__ void gemm_bias_act_sm_kernel<2, false, 0>(const bf16_t*, const bf16_t*, const float*, bf16_t*, const bf16_t*, int, int, int, const int*);
template __global__ void gemm_bias_act_sm_kernel<0, true, 0>(const bf16_t*, const bf16_t*, const float*, bf16_t*, const bf16_t*, int, int, int, const int*);
template __global__ void gemm_bias_act_sm_kernel<0, true, 1>(const bf16_t*, const bf16_t*, const float*, bf16_t*, const bf16_t*, int, int, int, const int*);
template __global__ void gemm_bias_act_sm_kernel<0, true, 2>(const bf16_t*, const bf16_t*, const float*, bf16_t*, const bf16_t*, int, int, int, const int*);

// ---------------------------------------------------------------------------
// N == 1 path (attention gate, CBF head): ONE THREAD per output row — the
// wave-per-row gemv dispatches M/4 tiny workgroups and is dispatch-bound at
// M ~ 3e5; here 256 rows share a workgroup and W (<= 384 values, uniform
// across the wave) comes from the scalar cache.
// ---------------------------------------------------------------------------
template <int ACT>
__launch_bounds__(256) __global__
void dot_bias_act_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ W,
                         const float* __restrict__ bias, float* __restrict__ Y,
                         long M, int K, const int* __restrict__ m_dev) {
  const long m = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (m_dev != nullptr) {
    const long md = *m_dev;
    M = md < M ? md : M;
  }
  if (m >= M) return;
  float a0 = 0.f, a1 = 0.f;
  const int kv = ((K & 7) == 0) ? (K / 16) * 16 : 0;  // b128 path needs 16-B
  int k = 0;                                          // aligned rows (K%8==0)
  for (; k < kv; k += 16) {  // two b128 loads in flight per iteration
    const bf16x8 x0 = *(const bf16x8*)(X + m * K + k);
    const bf16x8 x1 = *(const bf16x8*)(X + m * K + k + 8);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      a0 += (float)x0[i] * (float)W[k + i];
      a1 += (float)x1[i] * (float)W[k + 8 + i];
    }
  }
  for (; k < K; ++k) a0 += (float)X[m * K + k] * (float)W[k];
  Y[m] = apply_act(a0 + a1 + bias[0], ACT);
}

template __global__ void dot_bias_act_kernel<0>(const bf16_t*, const bf16_t*, const float*, float*, long, int, const int*);
template __global__ void dot_bias_act_kernel<1>(const bf16_t*, const bf16_t*, const float*, float*, long, int, const int*);
template __global__ void dot_bias_act_kernel<2>(const bf16_t*, const bf16_t*, const float*, float*, long, int, const int*);

// ---------------------------------------------------------------------------
// Small-N path (N <= 16): one wave per output row, W cached in LDS.
// grid: ceil(M/4); block 256 (4 waves).
// ---------------------------------------------------------------------------
template <int ACT, typename OutT>
__launch_bounds__(256) __global__
void gemv_bias_act_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ W,
                          const float* __restrict__ bias, OutT* __restrict__ Y,
                          int M, int N, int K, const int* __restrict__ m_dev) {
  extern __shared__ char smem[];
  bf16_t* sW = (bf16_t*)smem;  // [K][N]
  M = live_rows(m_dev, M);
  if ((long)blockIdx.x * 4 >= M) return;  // block-uniform, ahead of the barrier
  for (int i = threadIdx.x; i < K * N; i += 256) sW[i] = W[i];
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  float p[16];
#pragma unroll
  for (int n = 0; n < 16; ++n) p[n] = 0.f;
  const int kvec = ((K & 7) == 0) ? K : 0;  // b128 rows need K % 8 == 0
  for (int k8 = lane * 8; k8 < kvec; k8 += WAVE * 8) {  // b128 row loads
    const bf16x8 xv = *(const bf16x8*)(X + m * K + k8);
#pragma unroll
    for (int i = 0; i < 8; ++i)
      for (int n = 0; n < N; ++n) p[n] += (float)xv[i] * (float)sW[(k8 + i) * N + n];
  }
  for (int k = kvec + lane; k < K; k += WAVE) {  // ragged tail
    const float xv = (float)X[m * K + k];
    for (int n = 0; n < N; ++n) p[n] += xv * (float)sW[k * N + n];
  }
  for (int n = 0; n < N; ++n) {
    const float s = wave_reduce_sum(p[n]);
    if (lane == 0) Y[m * N + n] = (OutT)apply_act(s + bias[n], ACT);
  }
}

// ---------------------------------------------------------------------------
// act_bwd: dZ = dY * act'(Y), elementwise bf16.
// ---------------------------------------------------------------------------
__global__ void act_bwd_kernel(const bf16_t* __restrict__ dY, const bf16_t* __restrict__ Y,
                               bf16_t* __restrict__ dZ, long n, int act) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dZ[i] = (bf16_t)((float)dY[i] * act_grad_from_out((float)Y[i], act));
}

// ---------------------------------------------------------------------------
// dW = X^T @ dZ  (deterministic split-M).  Stage 1: partials[s][K][N].
// grid: (ceil(K/64), ceil(N/64), S); block 256 (4 waves 2x2, wave 32x32).
// A-operand = X^T staged transposed in LDS (scalar transpose writes),
// B-operand = dZ staged k-blocked like the forward GEMM.
// ---------------------------------------------------------------------------
// LDS of one tn1 block. The kernels own it and hand it to the body, so the
// grouped kernel's three inlined ACT instantiations share one copy.
struct Tn1Lds {
  bf16_t sXT[64][72];    // [k][m] transposed X tile, pad >= BMR + 8
  bf16_t sB[8][64][8];   // dZ tile, m-blocked
  float sDb[4][64];      // db tree reduce (k0==0 blocks)
};

// XCD-aware placement (1-D launch, S % 8 == 0): all gk*gn blocks of one
// split-M slab s get ids with id%8 == s%8 -> same XCD (dispatch places
// block b on XCD b%8), so the X and dZ slab reads of the 2nd..24th block
// hit that XCD's L2 instead of re-reading HBM from 6 different XCDs.
// `id` is the block's id within its problem (the grouped kernel starts every
// problem at a multiple of 8, which keeps id%8 the XCD there too).
__device__ __forceinline__ void tn1_decode_remap(int id, int K, int N, int& kb, int& nb, int& s) {
  const int gk = (K + 63) / 64, gn = (N + 63) / 64;
  const int per = gk * gn;
  const int rest = id >> 3;
  s = (id & 7) + 8 * (rest / per);
  const int j = rest % per;
  kb = j / gn;
  nb = j % gn;
}

// Optional row map of the dW kernels (edge compaction): the reduction runs
// over the M = numel(row_map) DENSE slot rows, slab and tile boundaries and the
// position of every row in its MFMA step as in the dense call, but row m is
// read from row row_map[m] of the compact operands (X, dZ, Yact, rowgate;
// xrows rows) and is zero where row_map[m] < 0. A masked slot's dZ row is
// exactly zero in the dense call, so every partial keeps the dense call's bits.
__device__ __forceinline__ void tn_map_row(const int* __restrict__ row_map, int xrows, long& mr,
                                           bool& live) {
  if (row_map == nullptr || !live) return;
  const int j = row_map[mr];
  live = j >= 0 && j < xrows;
  mr = live ? j : 0;
}

// One block of the tn1 partial: output tile (kb, nb) of split-M slab s.
template <int ACT>
__device__ __forceinline__
void gemm_tn_partial_body(const bf16_t* __restrict__ X, const bf16_t* __restrict__ dZ,
                          const bf16_t* __restrict__ Yact,
                          const bool* __restrict__ rowgate,  // null or (M,):
                          // rows with gate=false contribute NOTHING to
                          // dW/db (the dX path elsewhere stays ungated) —
                          // implements per-sample stop-gradient of the
                          // parameters (GCBF+ unlabeled h_dot rows)
                          float* __restrict__ partial, float* __restrict__ db_partial,
                          int M, int N, int K, int S, int kb, int nb, int s, Tn1Lds& lds,
                          const int* __restrict__ row_map = nullptr, int xrows = 0) {
  // 64x64 output tile, BMR=64 reduction steps with register-prefetch
  // staging (load tile t+1 into registers while tile t computes).
  constexpr int BKDIM = 64, BN = 64, BMR = 64;
  auto& sXT = lds.sXT;
  auto& sB = lds.sB;
  auto& sDb = lds.sDb;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int wk = w >> 1, wn = w & 1;  // wave tile 32(K) x 32(N)
  const int k0 = kb * BKDIM;
  const int n0 = nb * BN;

  const long m_per = ((long)M + S - 1) / S;
  const long ms = (long)s * m_per;
  const long me = (ms + m_per < (long)M) ? ms + m_per : (long)M;

  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float db_acc = 0.f;
  const int db_c = tid & 63, db_q = tid >> 6;

  // per-thread staging assignments (2 chunks each for X and dZ)
  //   X: chunk c -> row m0 + (c>>3), k-chunk (c&7)*8 (64 rows x 8 chunks)
  //   dZ: chunk c -> row m0 + (c>>3), n-chunk (c&7)*8
  bf16_t xv[2][8], zv[2][8];

  auto load_tile = [&](long m0) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = tid + h * 256;
      long mr = m0 + (c >> 3);
      const int kc = (c & 7) * 8;
      bool live = mr < me;
      tn_map_row(row_map, xrows, mr, live);
      // b128 loads need 16-B alignment: row base mr*K is aligned only when
      // K % 8 == 0 (misaligned b128 at a segment end page-faults)
      if (live && k0 + kc + 7 < K && (K & 7) == 0) {
        *(bf16x8*)xv[h] = *(const bf16x8*)(X + mr * K + k0 + kc);
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i)
          xv[h][i] = (live && k0 + kc + i < K) ? X[mr * K + k0 + kc + i] : (bf16_t)0.f;
      }
      const bool gated = rowgate != nullptr && live && !rowgate[mr];
      if (gated) {
#pragma unroll
        for (int i = 0; i < 8; ++i) zv[h][i] = (bf16_t)0.f;
      } else if (live && n0 + kc + 7 < N && (N & 7) == 0) {
        *(bf16x8*)zv[h] = *(const bf16x8*)(dZ + mr * N + n0 + kc);
        if constexpr (ACT != 0) {
          // dZ operand is dY here: fold dZ = dY * act'(Y) into the stage
          bf16x8 yv = *(const bf16x8*)(Yact + mr * N + n0 + kc);
#pragma unroll
          for (int i = 0; i < 8; ++i)
            zv[h][i] = (bf16_t)((float)zv[h][i] * act_grad_from_out((float)yv[i], ACT));
        }
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const bool ok = live && n0 + kc + i < N;
          float z = ok ? (float)dZ[mr * N + n0 + kc + i] : 0.f;
          if constexpr (ACT != 0)
            if (ok) z *= act_grad_from_out((float)Yact[mr * N + n0 + kc + i], ACT);
          zv[h][i] = (bf16_t)z;
        }
      }
    }
  };

  auto write_tile = [&]() {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = tid + h * 256;
      const int mr = c >> 3;
      const int kc = (c & 7) * 8;
#pragma unroll
      for (int i = 0; i < 8; ++i) sXT[kc + i][mr] = xv[h][i];
#pragma unroll
      for (int i = 0; i < 8; ++i) sB[mr >> 3][kc + i][mr & 7] = zv[h][i];
    }
  };

  load_tile(ms);
  for (long m0 = ms; m0 < me; m0 += BMR) {
    __syncthreads();
    write_tile();
    __syncthreads();
    if (m0 + BMR < me) load_tile(m0 + BMR);  // overlap with the MFMA below

    if (kb == 0) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const bf16x8 v = *(const bf16x8*)(&sB[db_q * 2 + q][db_c][0]);
#pragma unroll
        for (int i = 0; i < 8; ++i) db_acc += (float)v[i];
      }
    }
#pragma unroll
    for (int mm = 0; mm < 2; ++mm) {  // two 32-deep reduction steps
      bf16x8 afr[2], bfr[2];
#pragma unroll
      for (int kf = 0; kf < 2; ++kf)
        afr[kf] = *(const bf16x8*)(&sXT[wk * 32 + kf * 16 + (lane & 15)][mm * 32 + (lane >> 4) * 8]);
#pragma unroll
      for (int nf = 0; nf < 2; ++nf)
        bfr[nf] = *(const bf16x8*)(&sB[mm * 4 + (lane >> 4)][wn * 32 + nf * 16 + (lane & 15)][0]);
#pragma unroll
      for (int kf = 0; kf < 2; ++kf)
#pragma unroll
        for (int nf = 0; nf < 2; ++nf)
          acc[kf][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr[kf], bfr[nf], acc[kf][nf], 0, 0, 0);
    }
  }

  if (kb == 0) {
    // db_acc covers rows {db_q*16..+16} interleaved (q pairs): tree-reduce
    sDb[db_q][db_c] = db_acc;
    __syncthreads();
    if (db_q == 0 && n0 + db_c < N)
      db_partial[(long)s * N + n0 + db_c] =
          (sDb[0][db_c] + sDb[1][db_c]) + (sDb[2][db_c] + sDb[3][db_c]);
  }
  float* out = partial + (long)s * K * N;
#pragma unroll
  for (int kf = 0; kf < 2; ++kf)
#pragma unroll
    for (int nf = 0; nf < 2; ++nf) {
      const int col = n0 + wn * 32 + nf * 16 + (lane & 15);
      if (col >= N) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int krow = k0 + wk * 32 + kf * 16 + (lane >> 4) * 4 + r;
        if (krow < K) out[(long)krow * N + col] = acc[kf][nf][r];
      }
    }
}

template <int ACT>
__launch_bounds__(256) __global__
void gemm_tn_partial_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ dZ,
                            const bf16_t* __restrict__ Yact, const bool* __restrict__ rowgate,
                            float* __restrict__ partial, float* __restrict__ db_partial,
                            int M, int N, int K, int S, int remap,
                            const int* __restrict__ m_dev, const int* __restrict__ row_map,
                            int xrows) {
  __shared__ Tn1Lds lds;
  // a device row count moves the slab boundaries (m_per below); every slab
  // still writes its partial, the empty ones zeros
  M = live_rows(m_dev, M);
  int kb, nb, s;
  if (remap) {
    tn1_decode_remap(blockIdx.x, K, N, kb, nb, s);
  } else {
    kb = blockIdx.x;
    nb = blockIdx.y;
    s = blockIdx.z;
  }
  gemm_tn_partial_body<ACT>(X, dZ, Yact, rowgate, partial, db_partial, M, N, K, S, kb, nb, s, lds,
                            row_map, xrows);
}

// Several independent tn1 problems in one launch (deferred-dW flush). A block
// finds its problem by a uniform scan of the start table and runs the body
// with its local id; per problem nothing changes (same tiles, slab ranges,
// MFMA order), so every partial keeps its bits. Without the 1-D remap the
// local id decodes x-fastest like the 3-D grid it replaces.
__launch_bounds__(256) __global__
void gemm_tn_partial_grouped_kernel(const TnPartialGroup g) {
  __shared__ Tn1Lds lds;
  const int bid = blockIdx.x;
  int gi = 0;
  for (int i = 1; i < g.n; ++i)
    if (bid >= g.start[i]) gi = i;
  const int id = bid - g.start[gi];
  if (id >= g.nblk[gi]) return;  // alignment padding between problems
  const TnPartialProblem& p = g.p[gi];
  const int M = p.M, N = p.N, K = p.K, S = p.S;
  int kb, nb, s;
  if (p.remap) {
    tn1_decode_remap(id, K, N, kb, nb, s);
  } else {
    kb = id % p.gk;
    nb = (id / p.gk) % p.gn;
    s = id / (p.gk * p.gn);
  }
  const bf16_t* X = (const bf16_t*)p.X;
  const bf16_t* dZ = (const bf16_t*)p.dZ;
  const bf16_t* Yact = (const bf16_t*)p.Yact;
  if (p.act == 1)
    gemm_tn_partial_body<1>(X, dZ, Yact, p.rowgate, p.partial, p.db_partial, M, N, K, S, kb, nb, s, lds);
  else if (p.act == 2)
    gemm_tn_partial_body<2>(X, dZ, Yact, p.rowgate, p.partial, p.db_partial, M, N, K, S, kb, nb, s, lds);
  else
    gemm_tn_partial_body<0>(X, dZ, Yact, p.rowgate, p.partial, p.db_partial, M, N, K, S, kb, nb, s, lds);
}

template __global__ void gemm_tn_partial_kernel<0>(const bf16_t*, const bf16_t*, const bf16_t*, const bool*, float*, float*, int, int, int, int, int, const int*, const int*, int);
template __global__ void gemm_tn_partial_kernel<1>(const bf16_t*, const bf16_t*, const bf16_t*, const bool*, float*, float*, int, int, int, int, int, const int*, const int*, int);
template __global__ void gemm_tn_partial_kernel<2>(const bf16_t*, const bf16_t*, const bf16_t*, const bool*, float*, float*, int, int, int, int, int, const int*, const int*, int);

// ---------------------------------------------------------------------------
// dW computed TRANSPOSED: dW^T[n,k] = sum_m dZ[m,n] X[m,k]. With i=n, j=k,
// p=m both MFMA operands contract over m, the ROW index of both row-major
// inputs. Both tiles are staged row-major ([m][64 cols], b128 global load ->
// one b128 LDS store per chunk, like the fwd kernels) and transposed on the
// read: every operand fragment is two ds_read_b64_tr_b16 (gfx950), each
// handing a 4(m) x 16(col) block to its 16-lane group column-major. The
// m -> operand-slot map is the one of the m-blocked images this replaces
// (lane group g holds rows 32*mm + 8*g + 0..7), so with the same MFMA and the
// same order over substeps and tiles every slab partial keeps its bits.
//
// LDS image: 128-byte rows, 16-byte chunk ch of row m stored at chunk
// ch ^ tn3_swz(m). Bank check (a/4 mod 64 per 32-lane half for the transposed
// read, a/4 mod 32 per 8 lanes for the b128 store):
//   operand read: a half takes rows b+q and b+8+q (q = 0..3) of one 32-byte
//     column pair. Rows of equal parity share a 128-byte bank half; their
//     (bit 1, bit 3) differ, so the XOR puts the four pairs in four distinct
//     32-byte slots: conflict-free. (Plain rows: rows m and m+2 collide.)
//   db read: a half takes rows b+q of two column pairs that differ in chunk
//     bit 1, which the XOR of rows q and q+2 swaps: 2-way, 4 reads per tile in
//     the kb == 0 blocks only.
//   store: 8 lanes write the 8 chunks of one row, permuted: conflict-free.
// The transposed read needs EXEC all ones and 8-byte-aligned addresses: no
// lane-dependent branch surrounds one, trip counts are block-uniform, and
// ragged tiles are zero-filled, never masked.
// One tile buffer, two barriers per tile, the next tile's global loads in
// flight under the MFMAs: a second buffer (one barrier per tile) measured no
// faster. Block 64(n) x 64(k), 4 waves 2x2 of 32x32, BMR=64.
// ---------------------------------------------------------------------------
typedef short tn3_s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) tn3_s16x4 tn3_lds_s16x4;

__device__ __forceinline__ int tn3_swz(int row) { return (row & 2) | ((row >> 1) & 4); }

// element offset of 16-byte chunk ch (0..7) of row `row` in a [64][64] tile
__device__ __forceinline__ int tn3_off(int row, int ch) {
  return row * 64 + ((ch ^ tn3_swz(row)) << 3);
}

// two transposed reads, rows r0..r0+3 and r0+4..r0+7 -> one 8-deep operand;
// `a` is the lane's address for the block at r0 (4 rows = 256 elements on)
__device__ __forceinline__ bf16x8 tn3_read_frag(const bf16_t* a) {
  const tn3_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tn3_lds_s16x4*)a);
  const tn3_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tn3_lds_s16x4*)(a + 4 * 64));
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, v);
}

template <int ACT>
__launch_bounds__(256) __global__
void gemm_tn_partial3_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ dZ,
                             const bf16_t* __restrict__ Yact,
                             const bool* __restrict__ rowgate,
                             float* __restrict__ partial, float* __restrict__ db_partial,
                             int M, int N, int K, int S, int remap,
                             const int* __restrict__ m_dev, const int* __restrict__ row_map,
                             int xrows) {
  constexpr int BNR = 64, BKD = 64, BMR = 64;
  constexpr int TILE = BMR * 64;  // elements of one row-major tile
  // a device row count moves the slab boundaries (m_per below): the live rows
  // spread over all S slabs, and an empty slab still writes a zero partial
  M = live_rows(m_dev, M);
  // one array for all LDS: dZ tile | X tile | db exchange
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * TILE * 2 + 4 * BNR * 4];
  bf16_t* const sZ = (bf16_t*)smem;
  float* const sDb = (float*)(smem + 2 * TILE * 2);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int wi = w >> 1, wj = w & 1;  // wave tile 32(n) x 32(k)
  int kb, nb, s;
  if (remap) {
    const int gk = (K + BKD - 1) / BKD, gn = (N + BNR - 1) / BNR;
    const int per = gk * gn;
    const int id = blockIdx.x;
    const int rest = id >> 3;
    s = (id & 7) + 8 * (rest / per);
    const int j = rest % per;
    kb = j / gn;
    nb = j % gn;
  } else {
    kb = blockIdx.x;
    nb = blockIdx.y;
    s = blockIdx.z;
  }
  const int k0 = kb * BKD;
  const int n0 = nb * BNR;

  const long m_per = ((long)M + S - 1) / S;
  const long ms = (long)s * m_per;
  const long me = (ms + m_per < (long)M) ? ms + m_per : (long)M;

  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float db_acc = 0.f;
  const int db_c = tid & 63, db_q = tid >> 6;

  // b128 loads need 16-B alignment: the row base is aligned only when the
  // row length is a multiple of 8 and the tensor itself starts aligned
  const bool xvec = (K & 7) == 0 && ((size_t)X & 15) == 0;
  const bool zvec = (N & 7) == 0 && ((size_t)dZ & 15) == 0 &&
                    (ACT == 0 || ((size_t)Yact & 15) == 0);

  // staging, 2 chunks per thread and tile, both tiles row-wise
  // (row = c >> 3, 8 cols = (c & 7) * 8); act fold and row gate in registers
  bf16_t xv[2][8], zv[2][8];

  auto load_tile = [&](long m0) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = tid + h * 256;
      long mr = m0 + (c >> 3);
      const int cc = (c & 7) * 8;
      bool live = mr < me;
      tn_map_row(row_map, xrows, mr, live);
      if (live && xvec && k0 + cc + 7 < K) {
        *(bf16x8*)xv[h] = *(const bf16x8*)(X + mr * K + k0 + cc);
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i)
          xv[h][i] = (live && k0 + cc + i < K) ? X[mr * K + k0 + cc + i] : (bf16_t)0.f;
      }
      const bool zgated = rowgate != nullptr && live && !rowgate[mr];
      if (zgated) {
#pragma unroll
        for (int i = 0; i < 8; ++i) zv[h][i] = (bf16_t)0.f;
      } else if (live && zvec && n0 + cc + 7 < N) {
        *(bf16x8*)zv[h] = *(const bf16x8*)(dZ + mr * N + n0 + cc);
        if constexpr (ACT != 0) {
          bf16x8 yv = *(const bf16x8*)(Yact + mr * N + n0 + cc);
#pragma unroll
          for (int i = 0; i < 8; ++i)
            zv[h][i] = (bf16_t)((float)zv[h][i] * act_grad_from_out((float)yv[i], ACT));
        }
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const bool ok = live && n0 + cc + i < N;
          float z = ok ? (float)dZ[mr * N + n0 + cc + i] : 0.f;
          if constexpr (ACT != 0)
            if (ok) z *= act_grad_from_out((float)Yact[mr * N + n0 + cc + i], ACT);
          zv[h][i] = (bf16_t)z;
        }
      }
    }
  };

  auto write_tile = [&]() {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = tid + h * 256;
      const int o = tn3_off(c >> 3, c & 7);
      *(bf16x8*)(sZ + o) = *(bf16x8*)zv[h];
      *(bf16x8*)(sZ + TILE + o) = *(bf16x8*)xv[h];
    }
  };

  // per-lane addresses of the transposed reads: lane 4q+p of a 16-lane group
  // points at row q, columns 4p..4p+3 of its block. tn3_swz of an operand
  // row 32*mm + 8*g + 4*r + q does not depend on mm or r, so those are
  // constant offsets from one address per fragment.
  const int g = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
  int aoff[2], boff[2], doff[4];
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    aoff[f] = tn3_off(8 * g + tq, wi * 4 + f * 2 + (tp >> 1)) + 4 * (tp & 1);
    boff[f] = TILE + tn3_off(8 * g + tq, wj * 4 + f * 2 + (tp >> 1)) + 4 * (tp & 1);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
    doff[r] = tn3_off(16 * db_q + 4 * r + tq, g * 2 + (tp >> 1)) + 4 * (tp & 1);

  load_tile(ms);
  for (long m0 = ms; m0 < me; m0 += BMR) {
    __syncthreads();
    write_tile();
    __syncthreads();
    if (m0 + BMR < me) load_tile(m0 + BMR);  // overlap with the MFMA below

    if (kb == 0) {
      // column db_c, rows 16*db_q + 0..15 in increasing order
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const tn3_s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tn3_lds_s16x4*)(sZ + doff[r]));
        typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
        const bf16x4 bv = __builtin_bit_cast(bf16x4, v);
#pragma unroll
        for (int i = 0; i < 4; ++i) db_acc += (float)bv[i];
      }
    }
#pragma unroll
    for (int mm = 0; mm < 2; ++mm) {  // two 32-deep reduction substeps
      bf16x8 afr[2], bfr[2];
#pragma unroll
      for (int nf = 0; nf < 2; ++nf) afr[nf] = tn3_read_frag(sZ + aoff[nf] + mm * 32 * 64);
#pragma unroll
      for (int kf = 0; kf < 2; ++kf) bfr[kf] = tn3_read_frag(sZ + boff[kf] + mm * 32 * 64);
#pragma unroll
      for (int nf = 0; nf < 2; ++nf)
#pragma unroll
        for (int kf = 0; kf < 2; ++kf)
          acc[nf][kf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr[nf], bfr[kf], acc[nf][kf], 0, 0, 0);
    }
  }

  if (kb == 0) {
    sDb[db_q * BNR + db_c] = db_acc;
    __syncthreads();
    if (db_q == 0 && n0 + db_c < N)
      db_partial[(long)s * N + n0 + db_c] =
          (sDb[db_c] + sDb[BNR + db_c]) + (sDb[2 * BNR + db_c] + sDb[3 * BNR + db_c]);
  }

  // C frag: lane holds C[row = n-frag][col = k-frag]; write transposed into
  // partial[s][k][n] (4-float runs are contiguous in n? no: row=n varies by
  // r -> stride 1 writes along n for fixed k = per-lane column)
  float* out = partial + (long)s * K * N;
#pragma unroll
  for (int nf = 0; nf < 2; ++nf) {
#pragma unroll
    for (int kf = 0; kf < 2; ++kf) {
      const int krow = k0 + wj * 32 + kf * 16 + (lane & 15);
      if (krow >= K) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ncol = n0 + wi * 32 + nf * 16 + (lane >> 4) * 4 + r;
        if (ncol < N) out[(long)krow * N + ncol] = acc[nf][kf][r];
      }
    }
  }
}

template __global__ void gemm_tn_partial3_kernel<0>(const bf16_t*, const bf16_t*, const bf16_t*, const bool*, float*, float*, int, int, int, int, int, const int*, const int*, int);
template __global__ void gemm_tn_partial3_kernel<1>(const bf16_t*, const bf16_t*, const bf16_t*, const bool*, float*, float*, int, int, int, int, int, const int*, const int*, int);
template __global__ void gemm_tn_partial3_kernel<2>(const bf16_t*, const bf16_t*, const bf16_t*, const bool*, float*, float*, int, int, int, int, int, const int*, const int*, int);

// ---------------------------------------------------------------------------
// gemm_tn_partial3_kernel for a call with a row map, staged sparse. With a map
// nine in ten rows of every dense tile are zeros, and the tile loop above is a
// latency chain (map load -> operand load -> barrier -> LDS write -> barrier).
// Here a block takes its slab in chunks of whole 64-row dense tiles: it reads
// the chunk's map segment, numbers the in-range entries in order of
// appearance (one wave ballot per tile), loads only those operand rows, all
// at once, into a COMPACT LDS image, and then runs the dense call's MFMA
// steps with no barrier and no global access: in ds_read_b64_tr_b16 every
// lane supplies its own row address, so a lane whose dense row is live points
// at that row's compact copy and a lane whose dense row is masked points at
// one shared all-zero row. A 16-bit table holds the LDS row slot of every
// dense row of the chunk, the two entries a lane needs in one step adjacent.
//
// The partials are bit-equal to gemm_tn_partial3_kernel's because
//  1. the launch geometry is the same: plan (gk, gn, S, remap) from the 64x64
//     tiling of the dense M = numel(row_map), the same XCD remap of the block
//     id, the same slab bounds m_per = ceil(M/S), ms, me; an empty slab writes
//     a zero partial and a zero db_partial;
//  2. the MFMA work is the same: per output element one
//     v_mfma_f32_16x16x32_bf16 per 32 dense rows, in increasing order from ms,
//     the zero-filled tail of the last 64-row tile included, from a zero
//     accumulator. No masked row is dropped and no row moves inside its step;
//  3. the operand positions are the same: dense row ms + 64t + 32mm + 8g + e
//     is element e of lane group g in both operands (tn3_read_frag);
//  4. the staged values are the same: a live row holds the bits load_tile
//     produces (dZ folded with act_grad_from_out(Yact) in f32 and rounded to
//     bf16, zeroed where rowgate[j] is false; ragged K/N columns zero-filled,
//     never masked; b128 loads only under xvec / zvec, scalar otherwise); a map
//     entry < 0 or >= xrows is a masked row;
//  5. the db order is the same: thread (db_q, db_c) adds the rows with
//     ((m - ms) % 64) / 16 == db_q in increasing m into one f32 that starts at
//     +0, and the four sums combine as (s0+s1)+(s2+s3). Masked rows are read
//     from the zero row here; they could as well be skipped, since adding +0
//     to an accumulator that is never -0 is exact.
// A chunk takes as many tiles (<= TN3MAP_TILES) as its live rows fit
// TN3MAP_ROWS slots, at least one (ROWS >= 64), so any density runs, 100%
// included. The numbering does not need a monotonic map. Image rows use the
// swizzle of the dense tile (tn3_off) on the slot number: consecutive slots,
// which is what a half-wave's live rows mostly are, spread like consecutive
// dense rows. EXEC is full around every transposed read (all trip counts are
// block-uniform) and every address is 8-byte aligned.
// ---------------------------------------------------------------------------
template <int ACT>
__launch_bounds__(256) __global__
void gemm_tn_partial3_map_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ dZ,
                                 const bf16_t* __restrict__ Yact,
                                 const bool* __restrict__ rowgate,
                                 float* __restrict__ partial, float* __restrict__ db_partial,
                                 int M, int N, int K, int S, int remap,
                                 const int* __restrict__ row_map, int xrows) {
  constexpr int BNR = 64, BKD = 64, BMR = 64;
  constexpr int C = TN3MAP_ROWS, TT = TN3MAP_TILES;
  constexpr int IMG = (C + 1) * 64;  // elements of one compact image, zero row last
  __shared__ __attribute__((aligned(16))) unsigned char smem[TN3MAP_LDS];
  bf16_t* const sZ = (bf16_t*)smem;
  bf16_t* const sX = sZ + IMG;
  unsigned short* const sTab = (unsigned short*)(sX + IMG);
  int* const sSrc = (int*)(sTab + (2 * TT + 1) * 32);
  int* const sCnt = sSrc + C;
  float* const sDb = (float*)(sCnt + TT);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int wi = w >> 1, wj = w & 1;  // wave tile 32(n) x 32(k)
  int kb, nb, s;
  if (remap) {
    const int gk = (K + BKD - 1) / BKD, gn = (N + BNR - 1) / BNR;
    const int per = gk * gn;
    const int id = blockIdx.x;
    const int rest = id >> 3;
    s = (id & 7) + 8 * (rest / per);
    const int j = rest % per;
    kb = j / gn;
    nb = j % gn;
  } else {
    kb = blockIdx.x;
    nb = blockIdx.y;
    s = blockIdx.z;
  }
  const int k0 = kb * BKD;
  const int n0 = nb * BNR;

  const long m_per = ((long)M + S - 1) / S;
  const long ms = (long)s * m_per;
  const long me = (ms + m_per < (long)M) ? ms + m_per : (long)M;
  const int ntiles = me > ms ? (int)((me - ms + BMR - 1) / BMR) : 0;

  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float db_acc = 0.f;
  const int db_c = tid & 63, db_q = tid >> 6;

  const bool xvec = (K & 7) == 0 && ((size_t)X & 15) == 0;
  const bool zvec = (N & 7) == 0 && ((size_t)dZ & 15) == 0 &&
                    (ACT == 0 || ((size_t)Yact & 15) == 0);

  // the zero row; the chunk barriers order it before the first read
  if (tid < 16) {
    bf16x8 z;
#pragma unroll
    for (int i = 0; i < 8; ++i) z[i] = (bf16_t)0.f;
    *(bf16x8*)((tid < 8 ? sZ : sX) + C * 64 + (tid & 7) * 8) = z;
  }

  // lane 4q+p of a 16-lane group points at row q, columns 4p..4p+3 of its
  // block, as in gemm_tn_partial3_kernel; the row is now a slot from the table
  const int g = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
  const int tl = g * 4 + tq;  // the lane's pair of table entries in a step
  const int e4 = 4 * (tp & 1);
  const int cha = wi * 4 + (tp >> 1), chb = wj * 4 + (tp >> 1), chd = g * 2 + (tp >> 1);
  const unsigned* const tab32 = (const unsigned*)sTab;
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  auto read_frag = [&](const bf16_t* img, int s0, int s1, int ch) {
    const tn3_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tn3_lds_s16x4*)(img + tn3_off(s0, ch) + e4));
    const tn3_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tn3_lds_s16x4*)(img + tn3_off(s1, ch) + e4));
    const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
  };

  for (int t0 = 0; t0 < ntiles;) {
    const int tleft = ntiles - t0 < TT ? ntiles - t0 : TT;
    const long mc = ms + (long)t0 * BMR;

    // map segment: wave w takes tiles w, w+4, ..; a tile is one ballot
    int jrow[TT / 4], within[TT / 4];
#pragma unroll
    for (int i = 0; i < TT / 4; ++i) {
      const int tile = 4 * i + w;
      const long m = mc + (long)tile * BMR + lane;
      int j = -1;
      if (tile < tleft && m < me) j = row_map[m];
      const bool live = j >= 0 && j < xrows;
      const unsigned long long mask = __ballot(live);
      within[i] = __popcll(mask & ((1ull << lane) - 1ull));
      jrow[i] = live ? j : -1;
      if (lane == 0) sCnt[tile] = __popcll(mask);
    }
    __syncthreads();  // counts visible; every wave has left the previous chunk

    // tiles of this chunk: the longest prefix whose live rows fit C slots
    int run = 0, nt = 0, pre[TT / 4];
    bool open = true;
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      const int c = sCnt[t];
      open = open && t < tleft && run + c <= C;
      if ((t & 3) == w) pre[t >> 2] = run;
      if (open) {
        run += c;
        nt = t + 1;
      }
    }
    const int nrows = run;
#pragma unroll
    for (int i = 0; i < TT / 4; ++i) {
      const int tile = 4 * i + w;
      if (tile < nt) {
        // dense row 32*step + 8*g + 4*h + q of the chunk -> entry
        // 32*step + 2*(4*g + q) + h: one 32-bit read gives a lane both rows
        const int slot = jrow[i] >= 0 ? pre[i] + within[i] : C;
        const int r32 = lane & 31;
        const int e = (tile * 2 + (lane >> 5)) * 32 + (((r32 >> 3) * 4 + (r32 & 3)) << 1) +
                      ((r32 >> 2) & 1);
        sTab[e] = (unsigned short)slot;
        if (jrow[i] >= 0) sSrc[slot] = jrow[i];
      }
    }
    __syncthreads();

    // operand rows of the chunk, 16-byte chunk c & 7 of slot c >> 3: all
    // addresses are known, so the loads go out together; act fold and row
    // gate in registers as in load_tile
    constexpr int NH = C * 8 / 256;
    bf16_t xv[NH][8], zv[NH][8];
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const int c = tid + h * 256;
      const int slot = c >> 3;
      const int cc = (c & 7) * 8;
      const bool live = slot < nrows;
      const long mr = live ? sSrc[slot] : 0;
      if (live && xvec && k0 + cc + 7 < K) {
        *(bf16x8*)xv[h] = *(const bf16x8*)(X + mr * K + k0 + cc);
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i)
          xv[h][i] = (live && k0 + cc + i < K) ? X[mr * K + k0 + cc + i] : (bf16_t)0.f;
      }
      const bool zgated = rowgate != nullptr && live && !rowgate[mr];
      if (zgated) {
#pragma unroll
        for (int i = 0; i < 8; ++i) zv[h][i] = (bf16_t)0.f;
      } else if (live && zvec && n0 + cc + 7 < N) {
        *(bf16x8*)zv[h] = *(const bf16x8*)(dZ + mr * N + n0 + cc);
        if constexpr (ACT != 0) {
          bf16x8 yv = *(const bf16x8*)(Yact + mr * N + n0 + cc);
#pragma unroll
          for (int i = 0; i < 8; ++i)
            zv[h][i] = (bf16_t)((float)zv[h][i] * act_grad_from_out((float)yv[i], ACT));
        }
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const bool ok = live && n0 + cc + i < N;
          float z = ok ? (float)dZ[mr * N + n0 + cc + i] : 0.f;
          if constexpr (ACT != 0)
            if (ok) z *= act_grad_from_out((float)Yact[mr * N + n0 + cc + i], ACT);
          zv[h][i] = (bf16_t)z;
        }
      }
    }
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const int c = tid + h * 256;
      if ((c >> 3) < nrows) {
        const int o = tn3_off(c >> 3, c & 7);
        *(bf16x8*)(sZ + o) = *(bf16x8*)zv[h];
        *(bf16x8*)(sX + o) = *(bf16x8*)xv[h];
      }
    }
    __syncthreads();

    // the dense call's steps over the chunk; table read one step ahead (the
    // table has one spare step, so the last read-ahead stays inside it)
    unsigned nxt = tab32[tl];
    for (int t = 0; t < nt; ++t) {
      if (kb == 0) {
        // column db_c, dense rows 16*db_q + 0..15 of the tile in increasing order
        const unsigned* dp = tab32 + (2 * t + (db_q >> 1)) * 16 + (db_q & 1) * 8 + tq;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const unsigned p = dp[(r >> 1) * 4];
          const int slot = (r & 1) ? (int)(p >> 16) : (int)(p & 0xffffu);
          const tn3_s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (tn3_lds_s16x4*)(sZ + tn3_off(slot, chd) + e4));
          typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
          const bf16x4 bv = __builtin_bit_cast(bf16x4, v);
#pragma unroll
          for (int i = 0; i < 4; ++i) db_acc += (float)bv[i];
        }
      }
#pragma unroll
      for (int mm = 0; mm < 2; ++mm) {
        const unsigned cur = nxt;
        nxt = tab32[(2 * t + mm + 1) * 16 + tl];
        const int s0 = (int)(cur & 0xffffu), s1 = (int)(cur >> 16);
        bf16x8 afr[2], bfr[2];
#pragma unroll
        for (int nf = 0; nf < 2; ++nf) afr[nf] = read_frag(sZ, s0, s1, cha + nf * 2);
#pragma unroll
        for (int kf = 0; kf < 2; ++kf) bfr[kf] = read_frag(sX, s0, s1, chb + kf * 2);
#pragma unroll
        for (int nf = 0; nf < 2; ++nf)
#pragma unroll
          for (int kf = 0; kf < 2; ++kf)
            acc[nf][kf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr[nf], bfr[kf], acc[nf][kf], 0, 0, 0);
      }
    }
    t0 += nt;
  }

  if (kb == 0) {
    sDb[db_q * BNR + db_c] = db_acc;
    __syncthreads();
    if (db_q == 0 && n0 + db_c < N)
      db_partial[(long)s * N + n0 + db_c] =
          (sDb[db_c] + sDb[BNR + db_c]) + (sDb[2 * BNR + db_c] + sDb[3 * BNR + db_c]);
  }

  // as gemm_tn_partial3_kernel: transposed into partial[s][k][n]
  float* out = partial + (long)s * K * N;
#pragma unroll
  for (int nf = 0; nf < 2; ++nf) {
#pragma unroll
    for (int kf = 0; kf < 2; ++kf) {
      const int krow = k0 + wj * 32 + kf * 16 + (lane & 15);
      if (krow >= K) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ncol = n0 + wi * 32 + nf * 16 + (lane >> 4) * 4 + r;
        if (ncol < N) out[(long)krow * N + ncol] = acc[nf][kf][r];
      }
    }
  }
}

template __global__ void gemm_tn_partial3_map_kernel<0>(const bf16_t*, const bf16_t*, const bf16_t*, const bool*, float*, float*, int, int, int, int, int, const int*, int);
template __global__ void gemm_tn_partial3_map_kernel<1>(const bf16_t*, const bf16_t*, const bf16_t*, const bool*, float*, float*, int, int, int, int, int, const int*, int);
template __global__ void gemm_tn_partial3_map_kernel<2>(const bf16_t*, const bf16_t*, const bf16_t*, const bool*, float*, float*, int, int, int, int, int, const int*, int);

// ---------------------------------------------------------------------------
// dW^T orientation at 128x128 block / 64x64 wave tile: same vector-only
// staging as kernel3, 4x fragment reuse (0.5 LDS loads per MFMA).
// Requires K >= 128 and N >= 128 (guards handle ragged edges).
// ---------------------------------------------------------------------------
template <int ACT>
__launch_bounds__(256) __global__
void gemm_tn_partial4_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ dZ,
                             const bf16_t* __restrict__ Yact,
                             float* __restrict__ partial, float* __restrict__ db_partial,
                             int M, int N, int K, int S, int remap) {
  constexpr int BNR = 128, BKD = 128, BMR = 64;
  __shared__ bf16_t sZ[BMR / 8][BNR][8];  // 16 KB
  __shared__ bf16_t sX[BMR / 8][BKD][8];  // 16 KB
  __shared__ float sDb[2][BNR];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int wi = w >> 1, wj = w & 1;  // wave tile 64(n) x 64(k)
  int kb, nb, s;
  if (remap) {
    const int gk = (K + BKD - 1) / BKD, gn = (N + BNR - 1) / BNR;
    const int per = gk * gn;
    const int id = blockIdx.x;
    const int rest = id >> 3;
    s = (id & 7) + 8 * (rest / per);
    const int j = rest % per;
    kb = j / gn;
    nb = j % gn;
  } else {
    kb = blockIdx.x;
    nb = blockIdx.y;
    s = blockIdx.z;
  }
  const int k0 = kb * BKD;
  const int n0 = nb * BNR;

  const long m_per = ((long)M + S - 1) / S;
  const long ms = (long)s * m_per;
  const long me = (ms + m_per < (long)M) ? ms + m_per : (long)M;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float db_acc = 0.f;
  const int db_c = tid & 127, db_h = tid >> 7;

  // staging: 1024 col-chunks each (128 cols x 8 m-blocks); 4 per thread
  bf16_t xv[4][8], zv[4][8];

  auto load_tile = [&](long m0) {
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int c = tid + h * 256;
      const int col = c & 127;
      const long mr0 = m0 + (c >> 7) * 8;
      const bool kin = k0 + col < K;
      const bool nin = n0 + col < N;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const long mr = mr0 + i;
        xv[h][i] = (mr < me && kin) ? X[mr * K + k0 + col] : (bf16_t)0.f;
        float z = (mr < me && nin) ? (float)dZ[mr * N + n0 + col] : 0.f;
        if constexpr (ACT != 0)
          if (mr < me && nin) z *= act_grad_from_out((float)Yact[mr * N + n0 + col], ACT);
        zv[h][i] = (bf16_t)z;
      }
    }
  };

  auto write_tile = [&]() {
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int c = tid + h * 256;
      const int col = c & 127;
      const int mb = c >> 7;
      *(bf16x8*)(&sX[mb][col][0]) = *(bf16x8*)xv[h];
      *(bf16x8*)(&sZ[mb][col][0]) = *(bf16x8*)zv[h];
    }
  };

  load_tile(ms);
  for (long m0 = ms; m0 < me; m0 += BMR) {
    __syncthreads();
    write_tile();
    __syncthreads();
    if (m0 + BMR < me) load_tile(m0 + BMR);

    if (kb == 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const bf16x8 v = *(const bf16x8*)(&sZ[db_h * 4 + q][db_c][0]);
#pragma unroll
        for (int i = 0; i < 8; ++i) db_acc += (float)v[i];
      }
    }
#pragma unroll
    for (int mm = 0; mm < 2; ++mm) {
      bf16x8 afr[4], bfr[4];
#pragma unroll
      for (int nf = 0; nf < 4; ++nf)
        afr[nf] = *(const bf16x8*)(&sZ[mm * 4 + (lane >> 4)][wi * 64 + nf * 16 + (lane & 15)][0]);
#pragma unroll
      for (int kf = 0; kf < 4; ++kf)
        bfr[kf] = *(const bf16x8*)(&sX[mm * 4 + (lane >> 4)][wj * 64 + kf * 16 + (lane & 15)][0]);
#pragma unroll
      for (int nf = 0; nf < 4; ++nf)
#pragma unroll
        for (int kf = 0; kf < 4; ++kf)
          acc[nf][kf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr[nf], bfr[kf], acc[nf][kf], 0, 0, 0);
    }
  }

  if (kb == 0) {
    sDb[db_h][db_c] = db_acc;
    __syncthreads();
    if (db_h == 0 && n0 + db_c < N)
      db_partial[(long)s * N + n0 + db_c] = sDb[0][db_c] + sDb[1][db_c];
  }

  float* out = partial + (long)s * K * N;
#pragma unroll
  for (int nf = 0; nf < 4; ++nf) {
#pragma unroll
    for (int kf = 0; kf < 4; ++kf) {
      const int krow = k0 + wj * 64 + kf * 16 + (lane & 15);
      if (krow >= K) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ncol = n0 + wi * 64 + nf * 16 + (lane >> 4) * 4 + r;
        if (ncol < N) out[(long)krow * N + ncol] = acc[nf][kf][r];
      }
    }
  }
}

template __global__ void gemm_tn_partial4_kernel<0>(const bf16_t*, const bf16_t*, const bf16_t*, float*, float*, int, int, int, int, int);
template __global__ void gemm_tn_partial4_kernel<1>(const bf16_t*, const bf16_t*, const bf16_t*, float*, float*, int, int, int, int, int);
template __global__ void gemm_tn_partial4_kernel<2>(const bf16_t*, const bf16_t*, const bf16_t*, float*, float*, int, int, int, int, int);

// ---------------------------------------------------------------------------
// dW = X^T dZ, 128x128 output tile / 64x64 wave tile (K >= 128, N >= 128).
// The 64x64 kernel above is LDS-load bound (1 b128 fragment read per MFMA,
// measured 121 TF); the 64x64 WAVE tile reuses each fragment 4x -> 0.5
// loads/MFMA. Same split-M partial + fused-db scheme, same XCD-aware 1-D
// placement decode.
// ---------------------------------------------------------------------------
template <int ACT>
__launch_bounds__(256) __global__
void gemm_tn_partial2_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ dZ,
                             const bf16_t* __restrict__ Yact,
                             float* __restrict__ partial, float* __restrict__ db_partial,
                             int M, int N, int K, int S, int remap) {
  constexpr int BK2 = 128, BN2 = 128, BMR = 64, TPAD = 72;
  __shared__ bf16_t sXT[BK2][TPAD];      // [k][m] transposed X tile (18.4 KB)
  __shared__ bf16_t sB[BMR / 8][BN2][8]; // dZ tile, m-blocked (16.4 KB)
  __shared__ float sDb[2][BN2];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int wk = w >> 1, wn = w & 1;  // wave tile 64(K) x 64(N)
  int kb, nb, s;
  if (remap) {
    const int gk = (K + BK2 - 1) / BK2, gn = (N + BN2 - 1) / BN2;
    const int per = gk * gn;
    const int id = blockIdx.x;
    const int rest = id >> 3;
    s = (id & 7) + 8 * (rest / per);
    const int j = rest % per;
    kb = j / gn;
    nb = j % gn;
  } else {
    kb = blockIdx.x;
    nb = blockIdx.y;
    s = blockIdx.z;
  }
  const int k0 = kb * BK2;
  const int n0 = nb * BN2;

  const long m_per = ((long)M + S - 1) / S;
  const long ms = (long)s * m_per;
  const long me = (ms + m_per < (long)M) ? ms + m_per : (long)M;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float db_acc = 0.f;
  const int db_c = tid & 127, db_h = tid >> 7;

  // staging: 1024 8-elem chunks each for X and dZ -> 4 chunks per thread
  //   chunk c: local row mr = c >> 4 (64 rows), 8-col group (c & 15) * 8
  bf16_t xv[4][8], zv[4][8];

  auto load_tile = [&](long m0) {
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int c = tid + h * 256;
      const long mr = m0 + (c >> 4);
      const int kc = (c & 15) * 8;
      if (mr < me && k0 + kc + 7 < K && (K & 7) == 0) {
        *(bf16x8*)xv[h] = *(const bf16x8*)(X + mr * K + k0 + kc);
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i)
          xv[h][i] = (mr < me && k0 + kc + i < K) ? X[mr * K + k0 + kc + i] : (bf16_t)0.f;
      }
      if (mr < me && n0 + kc + 7 < N && (N & 7) == 0) {
        *(bf16x8*)zv[h] = *(const bf16x8*)(dZ + mr * N + n0 + kc);
        if constexpr (ACT != 0) {
          bf16x8 yv = *(const bf16x8*)(Yact + mr * N + n0 + kc);
#pragma unroll
          for (int i = 0; i < 8; ++i)
            zv[h][i] = (bf16_t)((float)zv[h][i] * act_grad_from_out((float)yv[i], ACT));
        }
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const bool ok = mr < me && n0 + kc + i < N;
          float z = ok ? (float)dZ[mr * N + n0 + kc + i] : 0.f;
          if constexpr (ACT != 0)
            if (ok) z *= act_grad_from_out((float)Yact[mr * N + n0 + kc + i], ACT);
          zv[h][i] = (bf16_t)z;
        }
      }
    }
  };

  auto write_tile = [&]() {
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int c = tid + h * 256;
      const int mr = c >> 4;
      const int kc = (c & 15) * 8;
#pragma unroll
      for (int i = 0; i < 8; ++i) sXT[kc + i][mr] = xv[h][i];
#pragma unroll
      for (int i = 0; i < 8; ++i) sB[mr >> 3][kc + i][mr & 7] = zv[h][i];
    }
  };

  load_tile(ms);
  for (long m0 = ms; m0 < me; m0 += BMR) {
    __syncthreads();
    write_tile();
    __syncthreads();
    if (m0 + BMR < me) load_tile(m0 + BMR);  // overlap with the MFMA below

    if (kb == 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const bf16x8 v = *(const bf16x8*)(&sB[db_h * 4 + q][db_c][0]);
#pragma unroll
        for (int i = 0; i < 8; ++i) db_acc += (float)v[i];
      }
    }
#pragma unroll
    for (int mm = 0; mm < 2; ++mm) {  // two 32-deep reduction substeps
      bf16x8 afr[4], bfr[4];
#pragma unroll
      for (int kf = 0; kf < 4; ++kf)
        afr[kf] = *(const bf16x8*)(&sXT[wk * 64 + kf * 16 + (lane & 15)][mm * 32 + (lane >> 4) * 8]);
#pragma unroll
      for (int nf = 0; nf < 4; ++nf)
        bfr[nf] = *(const bf16x8*)(&sB[mm * 4 + (lane >> 4)][wn * 64 + nf * 16 + (lane & 15)][0]);
#pragma unroll
      for (int kf = 0; kf < 4; ++kf)
#pragma unroll
        for (int nf = 0; nf < 4; ++nf)
          acc[kf][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr[kf], bfr[nf], acc[kf][nf], 0, 0, 0);
    }
  }

  if (kb == 0) {
    sDb[db_h][db_c] = db_acc;
    __syncthreads();
    if (db_h == 0 && n0 + db_c < N)
      db_partial[(long)s * N + n0 + db_c] = sDb[0][db_c] + sDb[1][db_c];
  }

  float* out = partial + (long)s * K * N;
#pragma unroll
  for (int kf = 0; kf < 4; ++kf) {
#pragma unroll
    for (int nf = 0; nf < 4; ++nf) {
      const int col = n0 + wn * 64 + nf * 16 + (lane & 15);
      if (col >= N) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int krow = k0 + wk * 64 + kf * 16 + (lane >> 4) * 4 + r;
        if (krow < K) out[(long)krow * N + col] = acc[kf][nf][r];
      }
    }
  }
}

template __global__ void gemm_tn_partial2_kernel<0>(const bf16_t*, const bf16_t*, const bf16_t*, float*, float*, int, int, int, int, int);
template __global__ void gemm_tn_partial2_kernel<1>(const bf16_t*, const bf16_t*, const bf16_t*, float*, float*, int, int, int, int, int);
template __global__ void gemm_tn_partial2_kernel<2>(const bf16_t*, const bf16_t*, const bf16_t*, float*, float*, int, int, int, int, int);

// (dw_partial (S,K,N), db_partial (S,N)) -> (dW, db) in ONE launch.
// Fixed summation order per output (deterministic):
//   a_j = sum of src[s], s = j (mod 4), s < 4*(S/4), increasing s;
//   the remaining s are added to a_0 in order; r = (a0 + a1) + (a2 + a3).
// The four chains of an output run in parallel, one wave of the block per
// chain (j = tid >> 6), so a thread's S/4 loads are independent and stay in
// flight together; chains 1..3 hand their sums to wave 0 through LDS. With
// vec != 0 a thread of a dW block takes four consecutive outputs as 16-byte
// loads and stores (launcher: K*N % 4 == 0 and both pointers 16-B aligned).
// Blocks [0, nbw) cover dW, 64 * (vec ? 4 : 1) outputs each; the rest cover
// db, 64 outputs each, always scalar.
// acc != 0 accumulates (+=) into dW/db — used to write straight into the
// optimizer's flat-gradient views, skipping autograd's AccumulateGrad adds.
// `bid` is the block's id within its problem; sA is the block's LDS.
__device__ __forceinline__
void reduce_dw_db_body(const float* __restrict__ pw, const float* __restrict__ pb,
                       float* __restrict__ dW, float* __restrict__ db,
                       float* __restrict__ db2,
                       long KN, int N, int S, int acc, int vec, int nbw, int bid,
                       f32x4 (&sA)[3][64]) {
  const int lane = threadIdx.x & 63, j = threadIdx.x >> 6;
  const bool is_db = bid >= nbw;  // block-uniform
  const bool v4 = !is_db && vec;
  const float* src = is_db ? pb : pw;
  const long stride = is_db ? N : KN;
  const long blk = is_db ? (long)bid - nbw : (long)bid;
  const long off = (blk * 64 + lane) * (v4 ? 4 : 1);
  const bool live = off < stride;
  const int S4 = S & ~3;
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    if (v4) {
#pragma unroll 8
      for (int s = j; s < S4; s += 4) a += *(const f32x4*)(src + (long)s * stride + off);
    } else {
#pragma unroll 8
      for (int s = j; s < S4; s += 4) a[0] += src[(long)s * stride + off];
    }
  }
  if (j != 0) sA[j - 1][lane] = a;
  __syncthreads();
  if (j != 0 || !live) return;
  if (v4) {
    for (int s = S4; s < S; ++s) a += *(const f32x4*)(src + (long)s * stride + off);
    const f32x4 r = (a + sA[0][lane]) + (sA[1][lane] + sA[2][lane]);
    f32x4* dst = (f32x4*)(dW + off);
    *dst = acc ? (*dst + r) : r;
    return;
  }
  for (int s = S4; s < S; ++s) a[0] += src[(long)s * stride + off];
  const float r = (a[0] + sA[0][lane][0]) + (sA[1][lane][0] + sA[2][lane][0]);
  float* dst = is_db ? db + off : dW + off;
  *dst = acc ? (*dst + r) : r;
  // optional second db accumulation target (one-hot bias fold: the same db
  // flows into both bias.grad and kernel.grad[oh_row])
  if (is_db && db2 != nullptr) db2[off] += r;
}

__launch_bounds__(256) __global__
void reduce_dw_db_kernel(const float* __restrict__ pw, const float* __restrict__ pb,
                         float* __restrict__ dW, float* __restrict__ db,
                         float* __restrict__ db2,
                         long KN, int N, int S, int acc, int vec, int nbw) {
  __shared__ f32x4 sA[3][64];
  reduce_dw_db_body(pw, pb, dW, db, db2, KN, N, S, acc, vec, nbw, (int)blockIdx.x, sA);
}

// The reduces of several layers in one launch (deferred-dW flush): same table
// scheme as gemm_tn_partial_grouped_kernel, the 16-byte or scalar variant
// chosen per problem, the four summation chains of an output unchanged.
__launch_bounds__(256) __global__
void reduce_dw_db_grouped_kernel(const DwReduceGroup g) {
  __shared__ f32x4 sA[3][64];
  const int bid = blockIdx.x;
  int gi = 0;
  for (int i = 1; i < g.n; ++i)
    if (bid >= g.start[i]) gi = i;
  const int id = bid - g.start[gi];
  if (id >= g.nblk[gi]) return;
  const DwReduceProblem& p = g.p[gi];
  reduce_dw_db_body(p.pw, p.pb, p.dW, p.db, p.db2, p.KN, p.N, p.S, p.acc, p.vec, p.nbw, id, sA);
}

// ---------------------------------------------------------------------------
// host-visible launchers (called from bindings.cpp)
// ---------------------------------------------------------------------------
template __global__ void gemm_bias_act_kernel<0, false, 0>(const bf16_t*, const bf16_t*, const float*, bf16_t*, const bf16_t*, int, int, int, const int*);
template __global__ void gemm_bias_act_kernel<1, false, 0>(const bf16_t*, const bf16_t*, const float*, bf16_t*, const bf16_t*, int, int, int, const int*);
template __global__ void gemm_bias_act_kernel<2, false, 0>(const bf16_t*, const bf16_t*, const float*, bf16_t*, const bf16_t*, int, int, int, const int*);
template __global__ void gemm_bias_act_kernel<0, true, 0>(const bf16_t*, const bf16_t*, const float*, bf16_t*, const bf16_t*, int, int, int, const int*);
template __global__ void gemm_bias_act_kernel<0, true, 1>(const bf16_t*, const bf16_t*, const float*, bf16_t*, const bf16_t*, int, int, int, const int*);
template __global__ void gemm_bias_act_kernel<0, true, 2>(const bf16_t*, const bf16_t*, const float*, bf16_t*, const bf16_t*, int, int, int, const int*);
template __global__ void gemv_bias_act_kernel<0, bf16_t>(const bf16_t*, const bf16_t*, const float*, bf16_t*, int, int, int, const int*);
template __global__ void gemv_bias_act_kernel<1, bf16_t>(const bf16_t*, const bf16_t*, const float*, bf16_t*, int, int, int, const int*);
template __global__ void gemv_bias_act_kernel<2, bf16_t>(const bf16_t*, const bf16_t*, const float*, bf16_t*, int, int, int, const int*);
template __global__ void gemv_bias_act_kernel<0, float>(const bf16_t*, const bf16_t*, const float*, float*, int, int, int, const int*);
template __global__ void gemv_bias_act_kernel<1, float>(const bf16_t*, const bf16_t*, const float*, float*, int, int, int, const int*);
template __global__ void gemv_bias_act_kernel<2, float>(const bf16_t*, const bf16_t*, const float*, float*, int, int, int, const int*);

// ---------------------------------------------------------------------------
// Row-panel GEMM (dispatch names "glds" / "glds_bt"): one workgroup owns 128
// rows of X and produces EVERY output column for them, so X is read from
// memory once per call, not once per 64-column tile. Needs M % 128 == 0 and
// K % 64 == 0 (global_load_lds has no per-lane predicate); grid M/128.
//
// LDS, all filled by 16-byte global_load_lds (1 KiB per wave instruction,
// lane-linear destination, swizzle applied to the per-lane SOURCE address):
//   panel  [K/64][128][64]  the X slice, staged once; 16-byte granule g of a
//          row sits at granule g ^ ((row >> 1) & 7), A fragments are b128 reads
//   W tile (x nbuf, 1 or 2), the slice of W for one 64-column n-tile:
//     BT   W is (Nout, K) row-major; image [K/64][64 n][64 k], the panel's
//          swizzle; a B fragment is 8 consecutive k of one row: one b128 read
//     fwd  W is (K, N) row-major; image [K][64 n] in the row-major layout of
//          the dW tiles (tn3_off); B fragments by ds_read_b64_tr_b16
//   bias   [ceil(N/64)*64] f32, zero past N
//   256*K + nbuf*128*K bytes + bias. With two buffers the DMA of tile t+1 is
//   issued before the MFMAs of tile t; with one (K = 384) it follows them.
// A tile whose DMA would touch bytes outside W (last tile of N % 64 != 0) or
// whose rows are not 16-byte aligned (wvec == 0: forward N % 8 != 0, or an
// unaligned W) is staged through registers into the same image, predicated
// and zero-filled.
// The epilogue of tile t is issued after the DMA of tile t+1 and ahead of the
// MFMAs of tile t+1 (two-buffer case), so the barrier's wait for that DMA,
// which also waits for outstanding stores, finds both long done.
// While a DMA is in flight the compiler puts s_waitcnt vmcnt(0) in front of
// every LDS read it can see (the DMA may alias it) and of every use of a
// global load, which would drain the DMA and the stores ahead of the MFMAs.
// So the fragment reads are inline assembly with their own s_waitcnt lgkmcnt,
// the k loop is unrolled in full (NCH = K/64 is a template argument: no read
// is pending over a back edge, where a register copy could be placed), and
// the bias of a tile is read from LDS before the next DMA is issued. The
// barrier discipline, not the compiler, orders DMA and fragment reads.
// MFMA, k -> operand-slot map (lane group lane>>4 holds k = 32*step + 8*group
// + 0..7, steps ascending) and acc + bias -> act -> bf16 are those of
// gemm_bias_act_kernel: outputs are bit-identical to it.
// The transposed reads need EXEC all ones: no lane-dependent branch surrounds
// the k loop, and ragged tiles are zero-filled, never masked.
// ---------------------------------------------------------------------------
template <bool BT>
__device__ __forceinline__ void panel_stage_w(const bf16_t* __restrict__ W, bf16_t* buf,
                                              int N, int K, int n0, bool dma, bool wvec,
                                              int tid) {
  const int lane = tid & 63, w = tid >> 6;
  if (dma) {
    if constexpr (BT) {
      // per 64-wide k chunk: 64 rows x 128 B = 8 wave instructions
      for (int j = w; j < (K >> 6) * 8; j += 4) {
        const int c = j >> 3;
        const int idx = (j & 7) * 64 + lane;
        const int row = idx >> 3;
        const int gsrc = (idx & 7) ^ ((row >> 1) & 7);
        const bf16_t* src = W + (long)(n0 + row) * K + c * 64 + gsrc * 8;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) uint32_t*)src,
                                         (__attribute__((address_space(3))) uint32_t*)(buf + (long)j * 512),
                                         16, 0, 0);
      }
    } else {
      // 8 rows of k x 128 B per wave instruction
      for (int j = w; j < (K >> 3); j += 4) {
        const int row = j * 8 + (lane >> 3);
        const int csrc = (lane & 7) ^ tn3_swz(row);
        const bf16_t* src = W + (long)row * N + n0 + csrc * 8;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) uint32_t*)src,
                                         (__attribute__((address_space(3))) uint32_t*)(buf + (long)j * 512),
                                         16, 0, 0);
      }
    }
    return;
  }
  if constexpr (BT) {
    const int kch = K >> 3;
    for (int c = tid; c < 64 * kch; c += 256) {
      const int r = c / kch;
      const int kg = c % kch;  // 16-byte granule along K
      bf16x8 v;
      if (n0 + r < N) {
        v = *(const bf16x8*)(W + (long)(n0 + r) * K + kg * 8);
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (bf16_t)0.f;
      }
      *(bf16x8*)(buf + (kg >> 3) * 4096 + r * 64 + (((kg & 7) ^ ((r >> 1) & 7)) << 3)) = v;
    }
  } else {
    for (int c = tid; c < K * 8; c += 256) {
      const int k = c >> 3;
      const int ch = c & 7;
      const int co = ch * 8;
      bf16x8 v;
      if (wvec && n0 + co + 7 < N) {
        v = *(const bf16x8*)(W + (long)k * N + n0 + co);
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i)
          v[i] = (n0 + co + i < N) ? W[(long)k * N + n0 + co + i] : (bf16_t)0.f;
      }
      *(bf16x8*)(buf + tn3_off(k, ch)) = v;
    }
  }
}

typedef int panel_i32x4 __attribute__((ext_vector_type(4)));
typedef int panel_i32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned panel_lds_addr(const void* p) {
  return (unsigned)(size_t)(const __attribute__((address_space(3))) char*)p;
}

// fragments of one 32-deep step, as issued (not yet waited for)
template <bool BT>
struct PanelFrags {
  panel_i32x4 a[4];
  panel_i32x4 b[2];       // BT: one b128 per n fragment
  panel_i32x2 blo[2], bhi[2];  // fwd: two transposed 64-bit reads per n fragment
};

// `hold`: the fragments of the step whose MFMAs follow. They pass through the
// statement so that those MFMAs cannot be scheduled ahead of these reads
// (which would let one register set serve both steps and serialize them).
#define PANEL_A_READS(A)                 \
  "ds_read_b128 %0, %" A "\n\t"            \
  "ds_read_b128 %1, %" A " offset:2048\n\t" \
  "ds_read_b128 %2, %" A " offset:4096\n\t" \
  "ds_read_b128 %3, %" A " offset:6144\n\t"
template <bool BT>
__device__ __forceinline__ void panel_issue(PanelFrags<BT>& f, unsigned aaddr, unsigned b0addr,
                                            unsigned b1addr, PanelFrags<BT>* hold) {
  if constexpr (BT) {
    if (hold != nullptr) {
      asm volatile(PANEL_A_READS("12")
                   "ds_read_b128 %4, %13\n\t"
                   "ds_read_b128 %5, %14"
                   : "=&v"(f.a[0]), "=&v"(f.a[1]), "=&v"(f.a[2]), "=&v"(f.a[3]), "=&v"(f.b[0]),
                     "=&v"(f.b[1]), "+v"(hold->a[0]), "+v"(hold->a[1]), "+v"(hold->a[2]),
                     "+v"(hold->a[3]), "+v"(hold->b[0]), "+v"(hold->b[1])
                   : "v"(aaddr), "v"(b0addr), "v"(b1addr));
    } else {
      asm volatile(PANEL_A_READS("6")
                   "ds_read_b128 %4, %7\n\t"
                   "ds_read_b128 %5, %8"
                   : "=&v"(f.a[0]), "=&v"(f.a[1]), "=&v"(f.a[2]), "=&v"(f.a[3]), "=&v"(f.b[0]),
                     "=&v"(f.b[1])
                   : "v"(aaddr), "v"(b0addr), "v"(b1addr));
    }
  } else {
    if (hold != nullptr) {
      asm volatile(PANEL_A_READS("14")
                   "ds_read_b64_tr_b16 %4, %15\n\t"
                   "ds_read_b64_tr_b16 %5, %15 offset:512\n\t"
                   "ds_read_b64_tr_b16 %6, %16\n\t"
                   "ds_read_b64_tr_b16 %7, %16 offset:512"
                   : "=&v"(f.a[0]), "=&v"(f.a[1]), "=&v"(f.a[2]), "=&v"(f.a[3]), "=&v"(f.blo[0]),
                     "=&v"(f.bhi[0]), "=&v"(f.blo[1]), "=&v"(f.bhi[1]), "+v"(hold->a[0]),
                     "+v"(hold->a[1]), "+v"(hold->a[2]), "+v"(hold->a[3]), "+v"(hold->b[0]),
                     "+v"(hold->b[1])
                   : "v"(aaddr), "v"(b0addr), "v"(b1addr));
    } else {
      asm volatile(PANEL_A_READS("8")
                   "ds_read_b64_tr_b16 %4, %9\n\t"
                   "ds_read_b64_tr_b16 %5, %9 offset:512\n\t"
                   "ds_read_b64_tr_b16 %6, %10\n\t"
                   "ds_read_b64_tr_b16 %7, %10 offset:512"
                   : "=&v"(f.a[0]), "=&v"(f.a[1]), "=&v"(f.a[2]), "=&v"(f.a[3]), "=&v"(f.blo[0]),
                     "=&v"(f.bhi[0]), "=&v"(f.blo[1]), "=&v"(f.bhi[1])
                   : "v"(aaddr), "v"(b0addr), "v"(b1addr));
    }
  }
}
#undef PANEL_A_READS

// wait for every issued read; the fragments pass through the statement so no
// use of them can be scheduled ahead of it
template <bool BT>
__device__ __forceinline__ void panel_wait(PanelFrags<BT>& f) {
  if constexpr (BT) {
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(f.a[0]), "+v"(f.a[1]), "+v"(f.a[2]), "+v"(f.a[3]), "+v"(f.b[0]),
                   "+v"(f.b[1]));
  } else {
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(f.a[0]), "+v"(f.a[1]), "+v"(f.a[2]), "+v"(f.a[3]), "+v"(f.blo[0]),
                   "+v"(f.bhi[0]), "+v"(f.blo[1]), "+v"(f.bhi[1]));
    f.b[0] = panel_i32x4{f.blo[0][0], f.blo[0][1], f.bhi[0][0], f.bhi[0][1]};
    f.b[1] = panel_i32x4{f.blo[1][0], f.blo[1][1], f.bhi[1][0], f.bhi[1][1]};
  }
}

template <int ACT, bool BT, int NCH>
__launch_bounds__(256) __global__
void gemm_bias_act_panel_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ W,
                                const float* __restrict__ bias, bf16_t* __restrict__ Y,
                                int M, int N, int nbuf, int wvec,
                                const int* __restrict__ m_dev) {
  constexpr int BM = 128, BN = 64, K = NCH * 64;
  // a device row count is a multiple of 128 here (the caller hands the padded
  // count): panels past it leave ahead of every DMA, barrier and LDS write
  if ((int)blockIdx.x * BM >= live_rows(m_dev, M)) return;
  extern __shared__ char smem[];
  bf16_t* const sA = (bf16_t*)smem;  // [NCH][128][64]
  bf16_t* const sW = sA + BM * K;    // nbuf x (64 * K)
  float* const sBias = (float*)(sW + nbuf * (BN * K));

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int wm = w >> 1, wn = w & 1;  // wave tile: 64(M) x 32(N)
  const int m0 = blockIdx.x * BM;
  const int ntiles = (N + BN - 1) / BN;

  // ---- bias first: no global load may be waited for under a DMA ----------
  for (int i = tid; i < ntiles * BN; i += 256) sBias[i] = i < N ? bias[i] : 0.f;

  // ---- the X panel: 16 wave instructions per 64-wide k chunk --------------
#pragma unroll
  for (int it = 0; it < NCH * 4; ++it) {
    const int j = it * 4 + w;
    const int c = j >> 4;
    const int idx = (j & 15) * 64 + lane;  // 16-byte granule index in the chunk
    const int row = idx >> 3;
    const int gsrc = (idx & 7) ^ ((row >> 1) & 7);
    const bf16_t* src = X + (long)(m0 + row) * K + c * 64 + gsrc * 8;
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) uint32_t*)src,
                                     (__attribute__((address_space(3))) uint32_t*)(sA + (long)j * 512),
                                     16, 0, 0);
  }
  auto tile_dma = [&](int t) { return wvec != 0 && (t + 1) * BN <= N; };
  panel_stage_w<BT>(W, sW, N, K, 0, tile_dma(0), wvec != 0, tid);

  // ---- per-lane fragment addresses (LDS bytes) ----------------------------
  const int g = lane >> 4;
  const int sw = (lane >> 1) & 7;  // (row >> 1) & 7 of every fragment row
  unsigned aaddr[2];               // A fragment mf = 0, k step parity 0/1
#pragma unroll
  for (int kk = 0; kk < 2; ++kk)
    aaddr[kk] = panel_lds_addr(sA) +
                2 * ((wm * 64 + (lane & 15)) * 64 + (((kk * 4 + g) ^ sw) << 3));
  unsigned boff[2][2];  // BT: [nf][kk] in a k chunk; fwd: [nf][0] in a 32-deep step
  if constexpr (BT) {
#pragma unroll
    for (int nf = 0; nf < 2; ++nf)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
        boff[nf][kk] = 2 * ((wn * 32 + nf * 16 + (lane & 15)) * 64 + (((kk * 4 + g) ^ sw) << 3));
  } else {
    const int tq = (lane >> 2) & 3, tp = lane & 3;
#pragma unroll
    for (int nf = 0; nf < 2; ++nf) {
      boff[nf][0] = 2 * (tn3_off(8 * g + tq, wn * 4 + nf * 2 + (tp >> 1)) + 4 * (tp & 1));
      boff[nf][1] = 0;
    }
  }

  // issue the fragment reads of 32-deep step s (chunk s >> 1, half s & 1)
  auto issue = [&](PanelFrags<BT>& f, unsigned wbase, int s, PanelFrags<BT>* hold) {
    const unsigned a = aaddr[s & 1] + (s >> 1) * (BM * 64 * 2);
    if constexpr (BT)
      panel_issue<BT>(f, a, wbase + (s >> 1) * 8192 + boff[0][s & 1],
                      wbase + (s >> 1) * 8192 + boff[1][s & 1], hold);
    else
      panel_issue<BT>(f, a, wbase + s * 4096 + boff[0][0], wbase + s * 4096 + boff[1][0], hold);
  };

  auto read_bias = [&](float (&bv)[2], int n0) {
#pragma unroll
    for (int nf = 0; nf < 2; ++nf) bv[nf] = sBias[n0 + wn * 32 + nf * 16 + (lane & 15)];
  };

  auto epilogue = [&](const f32x4 (&acc)[4][2], const float (&bv)[2], int n0) {
#pragma unroll
    for (int mf = 0; mf < 4; ++mf) {
#pragma unroll
      for (int nf = 0; nf < 2; ++nf) {
        const int col = n0 + wn * 32 + nf * 16 + (lane & 15);
        if (col >= N) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const long row = m0 + wm * 64 + mf * 16 + (lane >> 4) * 4 + r;
          Y[row * N + col] = (bf16_t)apply_act(acc[mf][nf][r] + bv[nf], ACT);
        }
      }
    }
  };

  f32x4 acc[4][2], prev[4][2];
  float bv[2];
  for (int t = 0; t < ntiles; ++t) {
    __syncthreads();  // W tile t (and at t == 0 the panel and the bias) has landed
    const bf16_t* wb = sW + ((nbuf == 2) ? (t & 1) : 0) * (BN * K);
    if (nbuf == 2) {
      if (t > 0) read_bias(bv, (t - 1) * BN);  // ahead of the DMA
      if (t + 1 < ntiles)
        panel_stage_w<BT>(W, sW + ((t + 1) & 1) * (BN * K), N, K, (t + 1) * BN, tile_dma(t + 1),
                          wvec != 0, tid);
      if (t > 0) epilogue(prev, bv, (t - 1) * BN);
    }

#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const unsigned wbase = panel_lds_addr(wb);
    PanelFrags<BT> f[2];
    issue(f[0], wbase, 0, nullptr);
#pragma unroll
    for (int s = 0; s < 2 * NCH; ++s) {  // reads of step s+1 issue under the MFMAs of step s
      PanelFrags<BT>& cur = f[s & 1];
      panel_wait<BT>(cur);
      if (s + 1 < 2 * NCH) issue(f[(s + 1) & 1], wbase, s + 1, &cur);
#pragma unroll
      for (int mf = 0; mf < 4; ++mf)
#pragma unroll
        for (int nf = 0; nf < 2; ++nf)
          acc[mf][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              __builtin_bit_cast(bf16x8, cur.a[mf]), __builtin_bit_cast(bf16x8, cur.b[nf]),
              acc[mf][nf], 0, 0, 0);
      // keep the next step's wait behind these MFMAs
      __builtin_amdgcn_sched_barrier(0);
    }

    if (nbuf == 2) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) prev[i][j] = acc[i][j];
    } else {
      read_bias(bv, t * BN);
      if (t + 1 < ntiles) {
        __syncthreads();  // every wave is done reading the one W buffer
        panel_stage_w<BT>(W, sW, N, K, (t + 1) * BN, tile_dma(t + 1), wvec != 0, tid);
      }
      epilogue(acc, bv, t * BN);  // stores go out while the DMA is in flight
    }
  }
  if (nbuf == 2) {
    read_bias(bv, (ntiles - 1) * BN);
    epilogue(prev, bv, (ntiles - 1) * BN);
  }
}

#define PANEL_INST(ACT, BT)                                                                          \
  template __global__ void gemm_bias_act_panel_kernel<ACT, BT, 1>(const bf16_t*, const bf16_t*, const float*, bf16_t*, int, int, int, int, const int*); \
  template __global__ void gemm_bias_act_panel_kernel<ACT, BT, 2>(const bf16_t*, const bf16_t*, const float*, bf16_t*, int, int, int, int, const int*); \
  template __global__ void gemm_bias_act_panel_kernel<ACT, BT, 3>(const bf16_t*, const bf16_t*, const float*, bf16_t*, int, int, int, int, const int*); \
  template __global__ void gemm_bias_act_panel_kernel<ACT, BT, 4>(const bf16_t*, const bf16_t*, const float*, bf16_t*, int, int, int, int, const int*); \
  template __global__ void gemm_bias_act_panel_kernel<ACT, BT, 5>(const bf16_t*, const bf16_t*, const float*, bf16_t*, int, int, int, int, const int*); \
  template __global__ void gemm_bias_act_panel_kernel<ACT, BT, 6>(const bf16_t*, const bf16_t*, const float*, bf16_t*, int, int, int, int, const int*);
PANEL_INST(0, false)
PANEL_INST(1, false)
PANEL_INST(2, false)
PANEL_INST(0, true)
#undef PANEL_INST
