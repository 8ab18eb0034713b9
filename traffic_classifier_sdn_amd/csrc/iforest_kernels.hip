// Isolation forest novelty score on device: per row the anomaly score, the
// novelty flag and, optionally, the row's class label masked by the flag.
//
// Packed tables (ops/cpu.py iforest_pack): `nodes` is the uint2 layout of the
// classifier forest's table,
//   inner node: word0 = f32 threshold bits, word1 = right_GLOBAL << 8 | feature
//   leaf:       word0 = f32 bits of h = depth + c(n_node_samples), word1 = 0xff
// and `roots` the T root indices.  The left child of an inner node is the next
// entry.  A leaf carries its whole contribution, so the walk keeps no depth
// counter and reads no leaf table.
//
// Per row
//   psum  = sum over the T trees of h_t(x)      (f64)
//   score = (float)exp2(-psum * inv_denom)      inv_denom = 1 / (T c(psi))
//   novel = psum < depth_cut                    depth_cut = -log2(thr) T c(psi)
//
// Every h is 0 or an f32 in [1, 64), hence a multiple of 2^-23, and at most
// 4096 of them sum to less than 2^18: every partial sum is a multiple of
// 2^-23 below 2^18, which f64 holds exactly.  The sum therefore does not
// depend on its order: both kernels below and the CPU oracle give the same
// psum bit for bit, and the flag, which compares psum and never the rounded
// score, is the same everywhere too.
//
// `x <= thr` is false for a NaN x, so a NaN feature goes right.

#include <cstdlib>
#include <cstring>

#include "common.h"
#include "launchers.h"

// What a launch needs besides X and the tables.
struct IForestOut {
  const int* labels_in;   // [n] or null (null exactly when labels_out is)
  float* score;           // [n]
  double* psum;           // [n] or null
  int* labels_out;        // [n] or null
  unsigned char* flags;   // [n]
  double inv_denom;
  double depth_cut;
};

DEV void iforest_store(const IForestOut& o, long long row, double psum) {
  const bool novel = psum < o.depth_cut;
  o.score[row] = (float)exp2(-psum * o.inv_denom);
  o.flags[row] = novel ? 1 : 0;
  if (o.psum) o.psum[row] = psum;
  if (o.labels_out) o.labels_out[row] = novel ? -1 : o.labels_in[row];
}

// ---------------------------------------------------------------------------
// Wave-per-row (serve batch sizes): the 64 lanes load the same row and lane
// `lane` walks trees lane, lane + 64, ... as rf_wave_scores does; the f64
// partial sums are reduced with wave_sum and lane 0 stores.
// ---------------------------------------------------------------------------
__launch_bounds__(256) __global__ void iforest_wave_kernel(
    const float* __restrict__ X, const uint2* __restrict__ nodes,
    const int* __restrict__ roots, IForestOut o, long long n, int T) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long long row = (long long)blockIdx.x * (blockDim.x / WAVE) +
                        (threadIdx.x >> 6);
  if (row >= n) return;  // wave-uniform
  const Row12 x = load_row12(X, row);  // broadcast load
  double acc = 0.0;
  for (int t = lane; t < T; t += WAVE) {
    int idx = roots[t];
    while (true) {
      const uint2 node = nodes[idx];
      const unsigned feat = node.y & 0xffu;
      if (feat == 0xffu) {
        acc += (double)__uint_as_float(node.x);
        break;
      }
      const float thr = __uint_as_float(node.x);
      idx = (sel12(x, feat) <= thr) ? idx + 1 : (int)(node.y >> 8);
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) iforest_store(o, row, acc);
}

// ---------------------------------------------------------------------------
// Row-per-lane (bulk scoring): each lane's 12 features in LDS at pitch 13,
// node table in L2, as rf_scores_lane_kernel places them.  No barrier in the
// row loop, hence a plain grid-stride loop.
// ---------------------------------------------------------------------------
#define IFOREST_BLOCK 512

__launch_bounds__(IFOREST_BLOCK) __global__ void iforest_lane_kernel(
    const float* __restrict__ X, const uint2* __restrict__ nodes,
    const int* __restrict__ roots, IForestOut o, long long n, int T) {
  __shared__ float s_feat[IFOREST_BLOCK * 13];
  float* my_feat = s_feat + (int)threadIdx.x * 13;

  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x; row < n;
       row += stride) {
    const Row12 x = load_row12(X, row);
#pragma unroll
    for (int j = 0; j < 12; ++j) my_feat[j] = x.v[j];
    double acc = 0.0;
    for (int t = 0; t < T; ++t) {
      int idx = roots[t];
      while (true) {
        const uint2 node = nodes[idx];
        const unsigned feat = node.y & 0xffu;
        if (feat == 0xffu) {
          acc += (double)__uint_as_float(node.x);
          break;
        }
        const float thr = __uint_as_float(node.x);
        idx = (my_feat[feat] <= thr) ? idx + 1 : (int)(node.y >> 8);
      }
    }
    iforest_store(o, row, acc);
  }
}

// Returns 0, or nonzero when T is outside 1..4096 (nothing is launched and
// the outputs stay unwritten: the caller must turn that into an error).
// `psum` may be null; `labels_in` and `labels_out` are null together.
//
// Read per launch, like TCSDN_RF_PROBA_MODE:
//   TCSDN_IFOREST_MODE=wave|lane  force one kernel at any n (default:
//       wave-per-row up to IFOREST_WAVE_MAX_ROWS, where the two were measured
//       to cross with 100 trees: profiles/novelty.md)
//   TCSDN_IFOREST_BLOCKS=<n>      cap on the row-per-lane grid, so small
//       inputs make each block loop over several tiles
// No sync and no allocation: safe under stream capture.
#define IFOREST_WAVE_MAX_ROWS 163840

extern "C" int launch_iforest_score(const float* X, const unsigned* nodes,
                                    const int* roots, const int* labels_in,
                                    float* score, double* psum, int* labels_out,
                                    unsigned char* flags, double inv_denom,
                                    double depth_cut, long long n, int T,
                                    hipStream_t stream) {
  if (T < 1 || T > 4096) return 1;
  if ((labels_in == nullptr) != (labels_out == nullptr)) return 1;
  if (n <= 0) return 0;
  bool wave = n <= IFOREST_WAVE_MAX_ROWS;
  if (const char* e = getenv("TCSDN_IFOREST_MODE")) {
    if (!strcmp(e, "wave")) wave = true;
    else if (!strcmp(e, "lane")) wave = false;
  }
  const uint2* nd = reinterpret_cast<const uint2*>(nodes);
  const IForestOut o{labels_in, score, psum, labels_out, flags, inv_denom, depth_cut};
  if (wave) {
    hipLaunchKernelGGL(iforest_wave_kernel, dim3((unsigned)((n + 3) / 4)),
                       dim3(256), 0, stream, X, nd, roots, o, n, T);
  } else {
    const int grid = ts_grid(n, IFOREST_BLOCK,
                             env_block_cap("TCSDN_IFOREST_BLOCKS", 4096));
    hipLaunchKernelGGL(iforest_lane_kernel, dim3(grid), dim3(IFOREST_BLOCK), 0,
                       stream, X, nd, roots, o, n, T);
  }
  return 0;
}
