// Per-class traffic accounting: the 12 features of every live flow summed per
// predicted class, with a flow count, in f64.
//
//   class_traffic_partial_kernel  one [(C + 1) * 13] f64 partial per block
//   class_traffic_finish_kernel   one block sums the partials in block order
//
// totals[g, 0] counts the rows of group g and totals[g, 1 + j] sums X[r, j]
// over them; g is the row's label, or C ("unknown") for a label outside
// 0..C-1 and for a confidence below min_conf.  Both kernels run on the
// caller's stream and write every cell on every launch, so a replayed graph
// never shows an earlier poll's totals.
//
// Bit-identical for the same inputs, n and grid: there is no atomic, and
// every sum is formed by one lane in an order that only n and the grid fix.
//
// The partial kernel gives a wave 64 consecutive rows at a time.
//   * Lane l reads the label and confidence of row base + l (coalesced
//     dwords) and forms that row's group once.
//   * For the features, lane (s, j) = (l / 16, l % 16) owns COLUMN j of the
//     rows base + 4 k + s, k = 0..15: a wave-wide load reads 4 consecutive
//     rows, 192 contiguous bytes, and all 16 loads are issued before the
//     first use.  Lane j = 12 carries the constant 1 of the flow count, lanes
//     13..15 idle.  (A lane that loaded its own row as three float4 would
//     need 13 accumulators per group: 117 doubles per lane, in registers or
//     LDS, which neither holds at a useful occupancy.)
//   * The row's group reaches the 16 lanes of its row through a wave shuffle
//     and selects one of the lane's C + 1 accumulators, acc[g][thread] in
//     LDS: a read, an f64 add and a write by the one lane that owns the word.
//     [g][thread] puts the 32 lanes of an LDS access group on 64 different
//     banks whatever their g.  A NaN or infinity therefore reaches the one
//     cell of its row's group and column, and a label never indexes anything
//     unchecked.
// After the block's last tile, thread c < (C + 1) * 13 adds the 16 lanes
// that own (group, column) of cell c, in lane order.
//
// n_live is read from memory once per lane (null: all n rows), so a captured
// launch over `capacity` rows follows the live count; rows at or past it are
// neither loaded nor counted.
//
// Bytes read per row: 48 of features, 4 of label, 4 of confidence if given.

#include "common.h"
#include "launchers.h"

#define TRAFFIC_BLOCK 256
#define TRAFFIC_COLS 13        // flow count + 12 features
#define TRAFFIC_MAX_GROUPS 9   // 8 classes + unknown
#define TRAFFIC_FIN_SLICES 8
#define TRAFFIC_FIN_CELLS 128  // >= TRAFFIC_MAX_GROUPS * TRAFFIC_COLS
#define TRAFFIC_FIN_BATCH 32

__launch_bounds__(TRAFFIC_BLOCK) __global__ void class_traffic_partial_kernel(
    const float* __restrict__ X, const int* __restrict__ labels,
    const float* __restrict__ conf, const int* __restrict__ n_live,
    float min_conf, int C, double* __restrict__ partial, long long n) {
  __shared__ double acc[TRAFFIC_MAX_GROUPS * TRAFFIC_BLOCK];
  long long live = n;
  if (n_live) {
    const long long v = *n_live;
    live = v < n ? v : n;
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = lane >> 4, j = lane & 15;
  // the lane's own words: nobody else touches them before the barrier
  for (int g = 0; g <= C; ++g) acc[g * TRAFFIC_BLOCK + tid] = 0.0;

  const long long stride = (long long)gridDim.x * TRAFFIC_BLOCK;
  for (long long base = ((long long)blockIdx.x * 4 + wave) * WAVE; base < live;
       base += stride) {
    // Every load is unconditional and 32-bit indexed from the tile's first
    // row, so that all 18 are in flight together: a row past the live ones
    // reads the tile's last live row instead (base < live here) and is
    // dropped by its group of -1; lanes 12..15 read column 0.
    const long long left = live - base;
    const int last = left < WAVE ? (int)left - 1 : WAVE - 1;
    const float* xt = X + base * 12 + (j < 12 ? j : 0);
    float x[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int row = 4 * k + s;
      x[k] = xt[(row < last ? row : last) * 12];
    }
    const int rl = lane < last ? lane : last;
    const int lab = labels[base + rl];
    const float cv = conf ? conf[base + rl] : 0.f;
    const bool low = conf && cv < min_conf;  // false for a NaN
    int g = ((unsigned)lab < (unsigned)C && !low) ? lab : C;
    g = lane <= last ? g : -1;  // past the live rows: counted nowhere
#pragma unroll
    for (int k = 0; k < 16; ++k) x[k] = j < 12 ? x[k] : 1.0f;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int gk = __shfl(g, 4 * k + s, WAVE);
      if (gk >= 0 && j <= 12) acc[gk * TRAFFIC_BLOCK + tid] += (double)x[k];
    }
  }
  __syncthreads();

  const int cells = (C + 1) * TRAFFIC_COLS;
  if (tid < cells) {
    const int g = tid / TRAFFIC_COLS, col = tid % TRAFFIC_COLS;
    const int jj = col ? col - 1 : 12;
    double t = 0.0;
    for (int slot = 0; slot < TRAFFIC_BLOCK / 16; ++slot)
      t += acc[g * TRAFFIC_BLOCK + slot * 16 + jj];
    partial[(long long)blockIdx.x * cells + tid] = t;
  }
}

// Sums the nb partials per cell: slice p of 8 adds its ceil(nb / 8) blocks in
// block order, then one lane per cell adds the 8 slices in slice order.
__launch_bounds__(TRAFFIC_FIN_SLICES * TRAFFIC_FIN_CELLS) __global__
void class_traffic_finish_kernel(const double* __restrict__ partial, int nb,
                                 int cells, double* __restrict__ totals) {
  __shared__ double sl[TRAFFIC_FIN_SLICES * TRAFFIC_FIN_CELLS];
  const int c = threadIdx.x % TRAFFIC_FIN_CELLS, p = threadIdx.x / TRAFFIC_FIN_CELLS;
  const int per = (nb + TRAFFIC_FIN_SLICES - 1) / TRAFFIC_FIN_SLICES;
  if (c < cells) {
    const int b0 = p * per, b1 = b0 + per < nb ? b0 + per : nb;
    double t = 0.0;
    // TRAFFIC_FIN_BATCH loads in flight, then their adds in block order: one
    // load per add would pay a memory latency for each of up to 256 blocks.
    // A block past the slice reads the slice's last one and adds 0 instead.
    for (int b = b0; b < b1; b += TRAFFIC_FIN_BATCH) {
      double v[TRAFFIC_FIN_BATCH];
#pragma unroll
      for (int i = 0; i < TRAFFIC_FIN_BATCH; ++i) {
        const int bi = b + i < b1 ? b + i : b1 - 1;
        v[i] = partial[(long long)bi * cells + c];
      }
#pragma unroll
      for (int i = 0; i < TRAFFIC_FIN_BATCH; ++i) t += b + i < b1 ? v[i] : 0.0;
    }
    sl[p * TRAFFIC_FIN_CELLS + c] = t;
  }
  __syncthreads();
  if (threadIdx.x < cells) {
    double t = sl[c];
    for (int q = 1; q < TRAFFIC_FIN_SLICES; ++q) t += sl[q * TRAFFIC_FIN_CELLS + c];
    totals[c] = t;
  }
}

// Blocks of the partial kernel for n rows: the grid of the row-per-lane
// probability kernels, so TCSDN_PROBA_BLOCKS (read per call) caps it too.
// The caller sizes `partial` with it and hands the same number to the launcher.
extern "C" int class_traffic_blocks(long long n) {
  return ts_grid(n, TRAFFIC_BLOCK, env_block_cap("TCSDN_PROBA_BLOCKS", 2048));
}

// `conf` and `n_live` may be null.  `partial` holds nb * (C + 1) * 13 doubles.
// Returns nonzero, and launches nothing, for C outside 2..8 or nb < 1.  n <= 0
// still launches: the totals are written, as zeros.
extern "C" int launch_class_traffic(const float* X, const int* labels,
                                    const float* conf, const int* n_live,
                                    float min_conf, double* partial,
                                    double* totals, long long n, int C, int nb,
                                    hipStream_t stream) {
  if (C < 2 || C > 8 || nb < 1) return 1;
  hipLaunchKernelGGL(class_traffic_partial_kernel, dim3(nb), dim3(TRAFFIC_BLOCK),
                     0, stream, X, labels, conf, n_live, min_conf, C, partial,
                     n < 0 ? 0 : n);
  hipLaunchKernelGGL(class_traffic_finish_kernel, dim3(1),
                     dim3(TRAFFIC_FIN_SLICES * TRAFFIC_FIN_CELLS), 0, stream,
                     partial, nb, (C + 1) * TRAFFIC_COLS, totals);
  return 0;
}
