// Problem tables of the grouped dW kernels (gemm.hip), filled on the host by
// the deferred-dW queue (bindings.hip). A table travels BY VALUE in the
// kernel arguments: no device-side descriptor buffer and no host-to-device
// copy, so a grouped launch is valid inside a stream capture. bf16 pointers
// are spelled `const void*` so that both translation units share one layout.
#pragma once

#define DW_GROUP_MAX 16  // problems per grouped launch (G)

// one split-M partial problem of the `tn1` kernel (gemm_tn_partial_kernel)
struct TnPartialProblem {
  const void* X;         // (M, K) bf16
  const void* dZ;        // (M, N) bf16
  const void* Yact;      // (M, N) bf16 when act != 0
  const bool* rowgate;   // null or (M,)
  float* partial;        // (S, K, N)
  float* db_partial;     // (S, N)
  int M, N, K, S;
  int remap;             // XCD-aware 1-D decode of the local block id
  int act;               // 0 / 1 / 2: upstream activation folded into the dZ stage
  int gk, gn;            // output tile grid, ceil(K/64) x ceil(N/64)
};

// one reduce problem (reduce_dw_db_kernel)
struct DwReduceProblem {
  const float* pw;  // (S, K, N)
  const float* pb;  // (S, N)
  float* dW;
  float* db;
  float* db2;       // null or second db accumulation target
  long KN;
  int N, S, acc, vec, nbw;
  int pad_;
};

// start[i] is the first block of problem i, start[n] the grid size; block b
// with start[i] <= b < start[i] + nblk[i] runs local block b - start[i] of
// problem i, blocks past nblk[i] (alignment padding) do nothing.
struct TnPartialGroup {
  int n;
  int start[DW_GROUP_MAX + 1];
  int nblk[DW_GROUP_MAX];
  TnPartialProblem p[DW_GROUP_MAX];
};

struct DwReduceGroup {
  int n;
  int start[DW_GROUP_MAX + 1];
  int nblk[DW_GROUP_MAX];
  DwReduceProblem p[DW_GROUP_MAX];
};

// Geometry of the sparse-staged dW kernel (gemm_tn_partial3_map_kernel): a
// chunk holds up to TN3MAP_ROWS live operand rows and spans up to
// TN3MAP_TILES dense 64-row tiles. LDS: two compact images of ROWS + 1 rows
// (the last is the shared zero row) of 128 bytes, the row table (one 16-bit
// entry per dense row plus one step of read-ahead), the source row of every
// slot, the per-tile counts and the db exchange.
#define TN3MAP_ROWS 128
#define TN3MAP_TILES 16
#define TN3MAP_LDS                                                                  \
  (2 * (TN3MAP_ROWS + 1) * 128 + (2 * TN3MAP_TILES + 1) * 32 * 2 + TN3MAP_ROWS * 4 + \
   TN3MAP_TILES * 4 + 4 * 64 * 4)
static_assert(TN3MAP_ROWS >= 64 && TN3MAP_ROWS < 65535, "a chunk must hold one full tile");
static_assert(TN3MAP_TILES % 4 == 0, "one wave numbers one tile per pass");

static_assert(sizeof(TnPartialGroup) <= 2048, "grouped partial table must stay under 2 KB");
static_assert(sizeof(DwReduceGroup) <= 2048, "grouped reduce table must stay under 2 KB");
