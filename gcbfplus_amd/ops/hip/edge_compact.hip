// Edge compaction: run the edge-level GNN kernels on the ACTIVE edge slots.
//
// A slot whose mask is false gets attention 0 in the masked softmax, adds 0 to
// aggr, and receives dmsg = dgate = 0: no output and no gradient depends on
// its row. The kernels here pack the active slots of a (B, N, D) mask into a
// dense prefix of "compact rows", in ascending slot order, so that a
// receiver's active slots stay contiguous:
//
//   edge_compact         mask -> rows / inv / off / cnt, an ordered scan
//                        (per-receiver counts, one-block prefix sum, ordered
//                        fill by wave ballot): deterministic, no atomics
//   gather_rows(_bwd)    dense (M, K) rows <-> compact (cap, K) rows
//   softmax_aggr_c_*     the masked softmax-aggregate on compact gate / msg
//   add_rows_bf16        a + b over the live compact rows
//
// The row count never leaves the device (the minibatch is a captured graph):
// every buffer has the static capacity cap = ceil128(M) rows, grids are sized
// for it, and kernels read cnt = {count, ceil128(count), prefix count,
// ceil128(prefix count)} and leave early. Rows [count, count_pad) are padding
// for the row-panel GEMM (whole 128-row panels): gather writes zeros there
// and the softmax backward writes zero gradients, which keeps them out of
// every dW. Rows >= count_pad are never read or written by these kernels.
//
// The compact softmax is bit-equal to softmax_aggr.hip: reductions that
// depend on the lane a slot sits in (sum of exp, t) run over the same
// D-slot LDS image with zeros in the masked slots, and the channel sums walk
// the active slots in slot order (the dense kernel adds +0 for the others).
#include "common.h"

// per-receiver active count; one wave per receiver, block 256
__launch_bounds__(256) __global__
void edge_count_kernel(const bool* __restrict__ mask, int* __restrict__ cnt_r, int R, int D) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= R) return;
  int c = 0;
  for (int d0 = 0; d0 < D; d0 += WAVE) {
    const int d = d0 + lane;
    const bool a = d < D && mask[(long)r * D + d];
    c += __popcll(__ballot(a));
  }
  if (lane == 0) cnt_r[r] = c;
}

// off[0..R] = exclusive prefix of cnt_r; cnt[0..3]. One block of 1024.
__launch_bounds__(1024) __global__
void edge_scan_kernel(const int* __restrict__ cnt_r, int* __restrict__ off,
                      int* __restrict__ cnt, int R, int prefix_recv, int align) {
  __shared__ int wsum[16];
  __shared__ int carry_s;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (int base = 0; base < R; base += 1024) {
    const int i = base + tid;
    const int v = i < R ? cnt_r[i] : 0;
    int inc = v;  // inclusive scan within the wave
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
      const int t = __shfl_up(inc, o, WAVE);
      if (lane >= o) inc += t;
    }
    if (lane == WAVE - 1) wsum[w] = inc;
    __syncthreads();
    int wbase = carry_s;
    for (int j = 0; j < w; ++j) wbase += wsum[j];
    if (i < R) off[i] = wbase + inc - v;
    __syncthreads();
    if (tid == 1023) carry_s = wbase + inc;
    __syncthreads();
  }
  if (tid == 0) {
    const int total = carry_s;
    off[R] = total;
    cnt[0] = total;
    cnt[1] = (total + align - 1) / align * align;
  }
  __syncthreads();
  if (tid == 0) {
    // off[prefix_recv] was written above by this block (or is the total)
    const int p = prefix_recv >= R ? carry_s : off[prefix_recv];
    cnt[2] = p;
    cnt[3] = (p + align - 1) / align * align;
  }
}

// rows / inv (/ gate_c = gate[receiver]) in ascending slot order; one wave per
// receiver, block 256
__launch_bounds__(256) __global__
void edge_fill_kernel(const bool* __restrict__ mask, const int* __restrict__ off,
                      const bool* __restrict__ gate, int* __restrict__ rows,
                      int* __restrict__ inv, bool* __restrict__ gate_c, int R, int D) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= R) return;
  int j = off[r];
  const bool gv = gate != nullptr ? gate[r] : true;
  for (int d0 = 0; d0 < D; d0 += WAVE) {
    const int d = d0 + lane;
    const bool a = d < D && mask[(long)r * D + d];
    const unsigned long long b = __ballot(a);
    if (d < D) {
      const int slot = r * D + d;
      const int jj = j + __popcll(b & ((1ull << lane) - 1ull));
      if (a) {
        rows[jj] = slot;
        if (gate_c != nullptr) gate_c[jj] = gv;
      }
      inv[slot] = a ? jj : -1;
    }
    j += __popcll(b);
  }
}

// Xc[j] = X[rows[j]] for j < count, zeros for count <= j < count_pad; rows of
// `chunks` 16-byte pieces, one thread per piece
__global__ void gather_rows_kernel(const uint4* __restrict__ X, const int* __restrict__ rows,
                                   const int* __restrict__ cnt, uint4* __restrict__ Xc,
                                   long M, long cap, int chunks) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long j = i / chunks;
  const int c = (int)(i % chunks);
  if (j >= cap || j >= cnt[1]) return;
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (j < cnt[0]) {
    const long r = rows[j];
    if (r >= 0 && r < M) v = X[r * chunks + c];  // always, for rows of this X's mask
  }
  Xc[j * chunks + c] = v;
}

// dX[m] = dXc[inv[m]], or zeros where inv[m] < 0
__global__ void gather_rows_bwd_kernel(const uint4* __restrict__ dXc, const int* __restrict__ inv,
                                       uint4* __restrict__ dX, long M, long cap,
                                       int chunks) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long m = i / chunks;
  const int c = (int)(i % chunks);
  if (m >= M) return;
  const int j = inv[m];
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (j >= 0 && j < cap) v = dXc[(long)j * chunks + c];
  dX[m * chunks + c] = v;
}

// out = a + b over rows < count_pad: the add in f32, one rounding to bf16 (what
// the elementwise bf16 add of the tensor library computes); 8 elements a thread
__global__ void add_rows_bf16_kernel(const bf16x8* __restrict__ a, const bf16x8* __restrict__ b,
                                     const int* __restrict__ cnt, bf16x8* __restrict__ out,
                                     long cap, int chunks) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long j = i / chunks;
  if (j >= cap || j >= cnt[1]) return;
  const bf16x8 x = a[i], y = b[i];
  bf16x8 o;
#pragma unroll
  for (int k = 0; k < 8; ++k) o[k] = (bf16_t)((float)x[k] + (float)y[k]);
  out[i] = o;
}

extern __shared__ char sac_smem[];

// slot -> compact row j of a receiver whose rows are [j0, j0 + nact)
__device__ __forceinline__ bool sac_live(int j, int j0, int nact) {
  return j >= j0 && j < j0 + nact;
}

// one workgroup per receiver, as softmax_aggr_fwd_kernel; gate_c / msg_c /
// attn_c are compact, inv maps a slot to its compact row
__launch_bounds__(256) __global__
void softmax_aggr_c_fwd_kernel(const float* __restrict__ gate_c, const bf16_t* __restrict__ msg_c,
                               const int* __restrict__ off, const int* __restrict__ inv,
                               bf16_t* __restrict__ aggr, float* __restrict__ attn_c, int D,
                               int C, int cap) {
  const long row = blockIdx.x;
  const int* iv = inv + row * D;
  const int j0 = off[row];
  int nact = off[row + 1] - j0;
  // off / inv of one mask always pass; anything else must not leave the buffers
  if (j0 < 0 || nact < 0 || nact > D || j0 + nact > cap) nact = 0;
  float* attn = (float*)sac_smem;  // [D] by slot, 0 in masked slots
  float* attn_j = attn + D;        // [nact] by compact row
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6;

  float mx = -3.0e38f;
  for (int d = tid; d < D; d += 256) {
    const int j = iv[d];
    mx = fmaxf(mx, sac_live(j, j0, nact) ? gate_c[j] : -3.0e38f);
  }
  mx = wave_reduce_max(mx);
  if (lane == 0) red[w] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));

  float sm = 0.f;
  for (int d = tid; d < D; d += 256) {
    const int j = iv[d];
    const float e = sac_live(j, j0, nact) ? __expf(gate_c[j] - mx) : 0.f;
    attn[d] = e;
    sm += e;
  }
  sm = wave_reduce_sum(sm);
  __syncthreads();
  if (lane == 0) red[w] = sm;
  __syncthreads();
  sm = red[0] + red[1] + red[2] + red[3];
  const float inv_sm = 1.f / fmaxf(sm, 1e-20f);
  for (int d = tid; d < D; d += 256) {
    const int j = iv[d];
    const float a = attn[d] * inv_sm;
    if (sac_live(j, j0, nact)) {
      attn_c[j] = a;
      attn_j[j - j0] = a;
    }
  }
  __syncthreads();

  const bf16_t* m = msg_c + (long)j0 * C;
  for (int c = tid; c < C; c += 256) {
    float a = 0.f;
    for (int jj = 0; jj < nact; ++jj) a += attn_j[jj] * (float)m[(long)jj * C + c];
    aggr[row * C + c] = (bf16_t)a;
  }
}

// blocks [0, R): one receiver each, as softmax_aggr_bwd_kernel; block R zeroes
// the gradients of the padding rows [count, count_pad)
__launch_bounds__(256) __global__
void softmax_aggr_c_bwd_kernel(const bf16_t* __restrict__ daggr, const float* __restrict__ attn_c,
                               const bf16_t* __restrict__ msg_c, const int* __restrict__ off,
                               const int* __restrict__ rows, const int* __restrict__ cnt,
                               float* __restrict__ dgate_c, bf16_t* __restrict__ dmsg_c,
                               int R, int D, int C, int cap) {
  const int tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6;
  if ((int)blockIdx.x == R) {
    long lo = cnt[0], hi = cnt[1];
    if (lo < 0 || hi > cap) lo = hi = 0;
    for (long j = lo + tid; j < hi; j += 256) dgate_c[j] = 0.f;
    for (long i = lo * C + tid; i < hi * C; i += 256) dmsg_c[i] = (bf16_t)0.f;
    return;
  }
  const long row = blockIdx.x;
  const int j0 = off[row];
  int nact = off[row + 1] - j0;
  if (j0 < 0 || nact < 0 || nact > D || j0 + nact > cap) nact = 0;
  const bf16_t* da = daggr + row * C;
  const bf16_t* m = msg_c + (long)j0 * C;
  float* sv = (float*)sac_smem;  // [D] s-values by slot, 0 in masked slots
  float* at = sv + D;            // [D] attention by slot, 0 in masked slots
  int* slot = (int*)(at + D);    // [nact] slot of a compact row
  __shared__ float red[4];

  for (int d = tid; d < D; d += 256) {
    sv[d] = 0.f;
    at[d] = 0.f;
  }
  __syncthreads();
  for (int jj = tid; jj < nact; jj += 256) {
    int d = rows[j0 + jj] - (int)(row * D);
    d = d < 0 ? 0 : (d >= D ? D - 1 : d);  // in range for rows of this mask
    slot[jj] = d;
    at[d] = attn_c[j0 + jj];
  }
  __syncthreads();
  for (int jj = w; jj < nact; jj += 4) {
    float p = 0.f;
    for (int c = lane; c < C; c += WAVE) p += (float)da[c] * (float)m[(long)jj * C + c];
    p = wave_reduce_sum(p);
    if (lane == 0) sv[slot[jj]] = p;
  }
  __syncthreads();

  float t = 0.f;
  for (int d = tid; d < D; d += 256) t += at[d] * sv[d];
  t = wave_reduce_sum(t);
  if (lane == 0) red[w] = t;
  __syncthreads();
  t = red[0] + red[1] + red[2] + red[3];

  for (int jj = tid; jj < nact; jj += 256) {
    const int d = slot[jj];
    dgate_c[j0 + jj] = at[d] * (sv[d] - t);
  }
  bf16_t* dm = dmsg_c + (long)j0 * C;
  for (int jj = w; jj < nact; jj += 4) {
    const float a = at[slot[jj]];
    for (int c = lane; c < C; c += WAVE) dm[(long)jj * C + c] = (bf16_t)(a * (float)da[c]);
  }
}
