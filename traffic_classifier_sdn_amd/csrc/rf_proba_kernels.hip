// Random forest class scores on device: per row the full probability vector,
// the label and the confidence (the top probability).
//
// Same packed tables as the predict kernels (ops/gpu.py rf_pack: `nodes`,
// `roots`, `leaf_proba`) and the same leaf encoding: a pure leaf adds one to
// its class's 10-bit field of a packed u64 counter, a mixed leaf adds its
// f32 distribution row to acc[].  What differs from rf_predict_*: EVERY tree
// counts (no early majority exit — a probability needs all T terms), and
// per row the kernels write
//
//   sum[c]    = acc[c] + pure count[c]
//   proba[c]  = sum[c] / (float)T        (IEEE division; optional store)
//   label     = first-maximum argmax of sum[c]   (rf_predict_kernel's rule)
//   conf      = max_c sum[c] / (float)T
//
// conf is the maximum of the proba row bit for bit: division by a positive
// constant is monotone, so the largest sum gives the largest quotient.

#include <cstdlib>
#include <cstring>

#include "common.h"
#include "launchers.h"

// Label and confidence from the C sums.
template <int C>
DEV void rf_scores_finish(const float (&sc)[C], float fT, int& label, float& conf) {
  const ArgMax m = first_max<C>(sc);
  label = m.idx;
  conf = m.val / fT;
}

// ---------------------------------------------------------------------------
// Wave-per-row (serve batch sizes): the sums come from rf_wave_scores
// (common.h), the body rf_predict_wave_kernel calls too, and lane 0 stores —
// so below the cutover the sums, and with them the labels, are those of
// rf_argmax bit for bit.
// ---------------------------------------------------------------------------
template <int C, bool WANT_PROBA>
__launch_bounds__(256) __global__ void rf_scores_wave_kernel(
    const float* __restrict__ X, const uint2* __restrict__ nodes,
    const int* __restrict__ roots, const float* __restrict__ leaf_proba,
    float* __restrict__ proba, int* __restrict__ labels,
    float* __restrict__ conf, long long n, int T) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long long row = (long long)blockIdx.x * (blockDim.x / WAVE) +
                        (threadIdx.x >> 6);
  if (row >= n) return;  // wave-uniform
  float sc[C];
  rf_wave_scores<C>(X, row, lane, nodes, roots, leaf_proba, T, sc);
  if (lane == 0) {
    const float fT = (float)T;
    int bi;
    float cf;
    rf_scores_finish<C>(sc, fT, bi, cf);
    labels[row] = bi;
    conf[row] = cf;
    if (WANT_PROBA) {
#pragma unroll
      for (int c = 0; c < C; ++c) proba[row * C + c] = sc[c] / fT;
    }
  }
}

// ---------------------------------------------------------------------------
// Row-per-lane (large batches): the mode-2 placement of rf_predict_kernel —
// each lane's 12 features in LDS at pitch 13, node table in L2.  (gcd(13,32)
// = 1 keeps a 32-lane group on distinct banks only while its lanes pick the
// same feature, which lanes at different depths of a tree do not: the pick
// does pay bank conflicts, see rf_predict_kernel.)
//
// Output: labels and conf are one dword per lane, coalesced as they are.  A
// lane also stores its own C probabilities: C dword stores of stride 4C
// bytes across the wave.  Passing the wave's [64, C] tile through the lanes'
// (by then free) feature rows and writing it out as C coalesced 256-byte
// stores was built and measured level with this at 1M rows and 0.1 % behind
// at 4M (profiles/rf_proba.md): the store is 2 % of a kernel that spends its
// time in ~1000 dependent node fetches per row, so the simpler form stays.
// No barrier in the row loop, hence a plain grid-stride loop.
// ---------------------------------------------------------------------------
#define RF_SCORES_BLOCK 512

template <int C, bool WANT_PROBA>
__launch_bounds__(RF_SCORES_BLOCK) __global__ void rf_scores_lane_kernel(
    const float* __restrict__ X, const uint2* __restrict__ nodes,
    const int* __restrict__ roots, const float* __restrict__ leaf_proba,
    float* __restrict__ proba, int* __restrict__ labels,
    float* __restrict__ conf, long long n, int T) {
  __shared__ float s_feat[RF_SCORES_BLOCK * 13];
  float* my_feat = s_feat + (int)threadIdx.x * 13;
  const float fT = (float)T;

  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x; row < n;
       row += stride) {
    Row12 x = load_row12(X, row);
#pragma unroll
    for (int j = 0; j < 12; ++j) my_feat[j] = x.v[j];
    float acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.f;
    unsigned long long votes = 0ull;  // 10-bit packed per-class pure counts
    for (int t = 0; t < T; ++t) {
      int idx = roots[t];
      while (true) {
        uint2 node = nodes[idx];
        unsigned feat = node.y & 0xffu;
        if (feat >= 0xf0u) {
          if (feat == 0xffu) {  // mixed leaf: read the distribution
            int pr = (int)node.x * C;
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += leaf_proba[pr + c];
          } else {  // pure leaf: class in the low nibble
            votes += 1ull << ((feat & 0xfu) * 10);
          }
          break;
        }
        float thr = __uint_as_float(node.x);
        idx = (my_feat[feat] <= thr) ? idx + 1 : (int)(node.y >> 8);
      }
    }
    float sc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) sc[c] = acc[c] + vote_count(votes, c);
    int bi;
    float cf;
    rf_scores_finish<C>(sc, fT, bi, cf);
    labels[row] = bi;
    conf[row] = cf;
    if (WANT_PROBA) {
#pragma unroll
      for (int c = 0; c < C; ++c) proba[row * C + c] = sc[c] / fT;
    }
  }
}

// Returns 0, or nonzero when C is outside 2..8 (nothing is launched and the
// outputs stay unwritten: the caller must turn that into an error).
// `proba` may be null: then only labels and conf are written.
//
// Read per launch, like TCSDN_RF_MODE:
//   TCSDN_RF_PROBA_MODE=wave|lane  force one kernel at any n (default:
//       wave-per-row up to the 131072 rows of launch_rf_predict's cutover)
//   TCSDN_RF_PROBA_BLOCKS=<n>      cap on the row-per-lane grid, so small
//       inputs make each block loop over several tiles
// No sync and no allocation: safe under stream capture.
extern "C" int launch_rf_scores(const float* X, const unsigned* nodes,
                                const int* roots, const float* leaf_proba,
                                float* proba, int* labels, float* conf,
                                long long n, int T, int C,
                                hipStream_t stream) {
  if (C < 2 || C > 8) return 1;
  if (n <= 0) return 0;
  bool wave = n <= 131072;
  if (const char* e = getenv("TCSDN_RF_PROBA_MODE")) {
    if (!strcmp(e, "wave")) wave = true;
    else if (!strcmp(e, "lane")) wave = false;
  }
  const uint2* nd = reinterpret_cast<const uint2*>(nodes);
  const dim3 grid = wave ? dim3((unsigned)((n + 3) / 4))
                         : dim3(ts_grid(n, RF_SCORES_BLOCK,
                                        env_block_cap("TCSDN_RF_PROBA_BLOCKS", 4096)));
  const dim3 block(wave ? 256 : RF_SCORES_BLOCK);
  return !dispatch_int<2, 3, 4, 5, 6, 7, 8>(C, [&](auto c) {
    constexpr int CV = decltype(c)::value;
    auto* kernel = wave ? (proba ? rf_scores_wave_kernel<CV, true>
                                 : rf_scores_wave_kernel<CV, false>)
                        : (proba ? rf_scores_lane_kernel<CV, true>
                                 : rf_scores_lane_kernel<CV, false>);
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, X, nd, roots,
                       leaf_proba, proba, labels, conf, n, T);
  });
}
