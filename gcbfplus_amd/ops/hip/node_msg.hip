// Fused GNN input of layer >= 1 (deep path, gnn_layers >= 2): a pure gather.
//
// fwd: X0 (B,N,D,KP0) bf16 (the layer-0 input of edge_msg.hip; its first E
// columns are the edge features in every mode), xa (B,N,F) bf16 agent
// features of the previous layer, c (2,F) f32 = features of a goal / a lidar
// hit node (they never receive a message, so they are two constant rows)
//   -> X1 (B,N,D,KP1) bf16, row (b,i,d) =
//      [ X0[b,i,d,0:E] | s (F) | xa[b,i] (F) | 0 pad ]
//      s = xa[b,d] for d < N, bf16(c[0]) for d == N, bf16(c[1]) for d > N
// the column order of the eager cat([edge_feats, sender, recv]).
//
// The feature blocks start at byte 2E of a 16 B-aligned row, so source and
// destination of a feature chunk differ in alignment by 2E mod 16: one thread
// assembles one 16 B chunk of the output from 4 B loads (E even: every column
// pair has a single 4 B-aligned source, the block boundaries E, E+F, E+2F are
// all even) or 2 B loads (E odd) and issues ONE aligned 16 B store. No 16 B
// access is made at an address that is not 16 B aligned. xa and c are small
// and L2-resident; consecutive threads read consecutive dwords.
//
// bwd: dX1 -> dX0 (columns [0,E) copied, the rest zero), dxa (B,N,F) f32,
// dc (2,F) f32, ATOMIC-FREE and in a fixed order (DP ranks stay bitwise in
// sync): see the kernels.
#include "common.h"

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned bf_bits(bf16_t v) {
  return (unsigned)__builtin_bit_cast(unsigned short, v);
}

// W consecutive bf16 as raw bits in the low 16*W bits (W = 2 needs p 4 B aligned)
template <int W>
__device__ __forceinline__ unsigned load_bits(const bf16_t* __restrict__ p) {
  if (W == 2) return *(const unsigned*)p;
  return (unsigned)*(const unsigned short*)p;
}

// the same for W f32 constants, rounded to bf16 (round to nearest even, as
// Tensor.to(torch.bfloat16))
template <int W>
__device__ __forceinline__ unsigned const_bits(const float* __restrict__ p) {
  unsigned v = bf_bits((bf16_t)p[0]);
  if (W == 2) v |= bf_bits((bf16_t)p[1]) << 16;
  return v;
}

__device__ __forceinline__ float bits_to_f32(unsigned lo16) {
  return __uint_as_float(lo16 << 16);
}

// acc[0..W) += the W bf16 at p
template <int W>
__device__ __forceinline__ void add_bits(float* acc, const bf16_t* __restrict__ p) {
  const unsigned v = load_bits<W>(p);
  acc[0] += bits_to_f32(v & 0xffffu);
  if (W == 2) acc[1] += bits_to_f32(v >> 16);
}

// one thread per (row, 16 B output chunk)
template <int W>
__launch_bounds__(256) __global__
void node_msg_in_fwd_kernel(const bf16_t* __restrict__ X0, const bf16_t* __restrict__ xa,
                            const float* __restrict__ c, bf16_t* __restrict__ X1, long rows,
                            int N, int D, int E, int F, int KP0, int KP1) {
  const int CH = KP1 / 8;
  const long total = rows * CH;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (long)gridDim.x * blockDim.x) {
    const int ch = t % CH;
    const long row = t / CH;
    const int d = row % D;
    const long bi = row / D;  // b * N + i
    const long b = bi / N;
    // sender features of this slot: an agent row of xa, or a constant row
    const bf16_t* send = (d < N) ? xa + (b * N + d) * F : nullptr;
    const float* cst = c + (d == N ? 0 : F);
    unsigned e[8];
#pragma unroll
    for (int p = 0; p < 8; p += W) {
      const int col = ch * 8 + p;
      unsigned v = 0u;  // pad
      if (col < E) {
        v = load_bits<W>(X0 + row * KP0 + col);
      } else if (col < E + F) {
        v = send ? load_bits<W>(send + (col - E)) : const_bits<W>(cst + (col - E));
      } else if (col < E + 2 * F) {
        v = load_bits<W>(xa + bi * F + (col - E - F));
      }
      e[p] = v;
    }
    u32x4 o;
    if (W == 2) {
      o = u32x4{e[0], e[2], e[4], e[6]};
    } else {
      o = u32x4{e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16),
                e[6] | (e[7] << 16)};
    }
    *(u32x4*)(X1 + row * KP1 + ch * 8) = o;
  }
}

// dX0: one thread per (row, 16 B chunk of the KP0-wide row)
template <int W>
__launch_bounds__(256) __global__
void node_msg_in_bwd_dx0_kernel(const bf16_t* __restrict__ dX1, bf16_t* __restrict__ dX0,
                                long rows, int E, int KP0, int KP1) {
  const int CH = KP0 / 8;
  const long total = rows * CH;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (long)gridDim.x * blockDim.x) {
    const int ch = t % CH;
    const long row = t / CH;
    unsigned e[8];
#pragma unroll
    for (int p = 0; p < 8; p += W) {
      const int col = ch * 8 + p;
      e[p] = (col < E) ? load_bits<W>(dX1 + row * KP1 + col) : 0u;
    }
    u32x4 o;
    if (W == 2) {
      o = u32x4{e[0], e[2], e[4], e[6]};
    } else {
      o = u32x4{e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16),
                e[6] | (e[7] << 16)};
    }
    *(u32x4*)(dX0 + row * KP0 + ch * 8) = o;
  }
}

// dxa and the per-(b,j) partials of dc. One thread per (b, j, W features)
// walks its N sender rows and D receiver rows serially, f32, in this order:
//   dxa[b,j,f] = sum_{i=0..N-1} dX1[b,i,j,E+f] + sum_{d=0..D-1} dX1[b,j,d,E+F+f]
// then the goal / hit sender columns of receiver j's own rows:
//   part[b,j,0,f] = dX1[b,j,N,E+f]    part[b,j,1,f] = sum_{d>N} dX1[b,j,d,E+f]
// Serial N + 2D row walk per thread: fine at training sizes (N + D <= ~100,
// B*N*F/W threads keep the device busy); a swarm-sized N would want a block
// per (b, j) with a row-parallel fixed-order tree instead.
template <int W>
__launch_bounds__(256) __global__
void node_msg_in_bwd_gather_kernel(const bf16_t* __restrict__ dX1, float* __restrict__ dxa,
                                   float* __restrict__ part, long BN, int N, int D, int E,
                                   int F, int KP1) {
  const int FC = F / W;
  const long total = BN * FC;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (long)gridDim.x * blockDim.x) {
    const int f = (int)(t % FC) * W;
    const long bj = t / FC;
    const int j = bj % N;
    const long b = bj / N;
    const bf16_t* base = dX1 + b * N * D * KP1;
    const bf16_t* own = base + (long)j * D * KP1;  // receiver j's D rows
    float acc[2] = {0.f, 0.f};
    for (int i = 0; i < N; ++i) add_bits<W>(acc, base + ((long)i * D + j) * KP1 + E + f);
    for (int d = 0; d < D; ++d) add_bits<W>(acc, own + (long)d * KP1 + E + F + f);
    float goal[2] = {0.f, 0.f}, hit[2] = {0.f, 0.f};
    add_bits<W>(goal, own + (long)N * KP1 + E + f);
    for (int d = N + 1; d < D; ++d) add_bits<W>(hit, own + (long)d * KP1 + E + f);
#pragma unroll
    for (int w = 0; w < W; ++w) {
      dxa[bj * F + f + w] = acc[w];
      part[(bj * 2 + 0) * F + f + w] = goal[w];
      part[(bj * 2 + 1) * F + f + w] = hit[w];
    }
  }
}

// dc[col] = sum over the BN partial rows, col in [0, C = 2F). A block owns 16
// columns; its 16 row lanes each sum rows lane, lane+16, ... in order, then
// lane 0 adds the 16 lane sums in lane order: the order depends on the shapes
// only.
__launch_bounds__(256) __global__
void node_msg_in_dc_reduce_kernel(const float* __restrict__ part, float* __restrict__ dc,
                                  long BN, int C) {
  __shared__ float s[16][16];
  const int cl = threadIdx.x & 15;
  const int lane = threadIdx.x >> 4;
  const int col = blockIdx.x * 16 + cl;
  float acc = 0.f;
  if (col < C)
    for (long r = lane; r < BN; r += 16) acc += part[r * C + col];
  s[lane][cl] = acc;
  __syncthreads();
  if (lane == 0 && col < C) {
    float sum = 0.f;
#pragma unroll
    for (int l = 0; l < 16; ++l) sum += s[l][cl];
    dc[col] = sum;
  }
}

template __global__ void node_msg_in_fwd_kernel<1>(const bf16_t*, const bf16_t*, const float*,
                                                   bf16_t*, long, int, int, int, int, int, int);
template __global__ void node_msg_in_fwd_kernel<2>(const bf16_t*, const bf16_t*, const float*,
                                                   bf16_t*, long, int, int, int, int, int, int);
template __global__ void node_msg_in_bwd_dx0_kernel<1>(const bf16_t*, bf16_t*, long, int, int,
                                                       int);
template __global__ void node_msg_in_bwd_dx0_kernel<2>(const bf16_t*, bf16_t*, long, int, int,
                                                       int);
template __global__ void node_msg_in_bwd_gather_kernel<1>(const bf16_t*, float*, float*, long,
                                                          int, int, int, int, int);
template __global__ void node_msg_in_bwd_gather_kernel<2>(const bf16_t*, float*, float*, long,
                                                          int, int, int, int, int);
