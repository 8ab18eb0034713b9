// Why a forest gave a row its class: per row the 12 per-feature contributions
// to the probability of one class (the Saabas / "treeinterpreter"
// decomposition), the feature that speaks most for it and that feature's
// share.
//
// Tables: `nodes` and `roots` are the classifier forest's (ops/gpu.py
// rf_pack: inner node word0 = f32 threshold bits, word1 = right_GLOBAL << 8 |
// feature; a leaf has a feature byte >= 0xf0; the left child is the next
// entry).  `delta` (ops/cpu.py rf_explain_flatten) is int32 [n_nodes, C]: row
// w holds, for every class, the step of the class probability from w's parent
// to w, times 2^30 and rounded to an integer; a root's row is zero.
//
// Per row, with c = labels[row]:
//   S[f]      = sum over the T trees and the edges v -> w of the row's path
//               with feature(v) = f, of delta[w, c]            (int64)
//   contrib   = (float)((double)S[f] / (2^30 T))               (one f64 division)
//   why       = first-maximum argmax of S[f] if that maximum is > 0, else -1
//   why_value = contrib[why], or 0 when why is -1
// A label outside [0, C) gives zeros, why = -1 and why_value = 0, and walks
// nothing.
//
// The sums are integers: at most T * depth < 2^22 terms below 2^30 each stay
// below 2^52, so S does not depend on the order of the additions and both
// kernels and the CPU oracle agree on it bit for bit, hence on everything
// derived from it.  Every tree counts: there is no early exit.
//
// `x <= thr` is false for a NaN x, so a NaN feature goes right.
//
// The accumulators.  S[f] is picked by a runtime feature id; twelve 64-bit
// registers indexed by it would go to scratch.  Each lane therefore keeps its
// twelve sums in a strip of LDS of its own, sum f of thread t at
// s_acc[f * PITCH + t]: a wave's lanes are 8 bytes apart when they pick the
// same f and the rows of two f 16 bytes apart in the banks, so the 64-bit add
// meets at most a two-way bank conflict.  The add is an LDS
// atomic whose result nobody reads (ds_add_u64): it hangs off the walk's
// dependent chain, which stays the one of rf_scores — node fetch, compare,
// next address.  The delta row's address is known when the next node's is,
// so the two loads issue together.  The other form, twelve 64-bit registers
// behind a chain of selects, was built and measured 1.2x slower in the
// wave-per-row kernel and 2.2x slower in the row-per-lane kernel
// (profiles/rf_explain.md): 36 more vector instructions in every step.

#include <cstdlib>
#include <cstring>

#include "common.h"
#include "launchers.h"

#define RF_EXPLAIN_BLOCK 256
// u64 entries between the sums of two features: two more than a block's
// threads, which puts the twelve rows 16 bytes apart in the LDS banks for the
// wave kernel's column sums
#define RF_EXPLAIN_PITCH (RF_EXPLAIN_BLOCK + 2)

// What a launch needs besides X and the tables.
struct ExplainOut {
  const int* labels;   // [n]
  float* contrib;      // [n,12] or null
  int* why;            // [n]
  float* why_value;    // [n]
  long long* sums;     // [n,12] or null
  double denom;        // 2^30 T
};

// One thread's twelve sums in its LDS strip.
struct LaneSums {
  unsigned long long* s;  // s_acc + threadIdx.x

  DEV explicit LaneSums(unsigned long long* strip) : s(strip) {}
  DEV void clear() {
#pragma unroll
    for (int f = 0; f < 12; ++f) s[f * RF_EXPLAIN_PITCH] = 0ull;
  }
  // non-returning: nothing waits for it
  DEV void add(unsigned feat, int d) {
    atomicAdd(&s[feat * RF_EXPLAIN_PITCH], (unsigned long long)(long long)d);
  }
  DEV unsigned long long get(int f) const { return s[f * RF_EXPLAIN_PITCH]; }
};

// One step of a path, the same in both kernels: from inner node `node` at
// the child `idx` chosen by the caller, add delta[idx, c] to the sum of the
// node's feature and fetch the child.  The two loads depend on idx alone.
DEV void explain_step(const uint2* __restrict__ nodes,
                      const int* __restrict__ delta, int idx, int C, int c,
                      unsigned feat, uint2& node, LaneSums& acc) {
  const int d = delta[(long long)idx * C + c];
  node = nodes[idx];
  acc.add(feat, d);
}

DEV float explain_share(long long s, double denom) {
  return (float)((double)s / denom);
}

DEV void explain_store(const ExplainOut& o, long long row,
                       const long long (&S)[12]) {
  long long best = 0;
  int why = -1;
#pragma unroll
  for (int f = 0; f < 12; ++f) {
    if (S[f] > best) { best = S[f]; why = f; }
  }
  o.why[row] = why;
  // best is S[why], or 0 when no feature speaks for the class
  o.why_value[row] = explain_share(best, o.denom);
  if (o.contrib) {
    float4* p = reinterpret_cast<float4*>(o.contrib + row * 12);
#pragma unroll
    for (int q = 0; q < 3; ++q)
      p[q] = make_float4(explain_share(S[4 * q], o.denom),
                         explain_share(S[4 * q + 1], o.denom),
                         explain_share(S[4 * q + 2], o.denom),
                         explain_share(S[4 * q + 3], o.denom));
  }
  if (o.sums) {
#pragma unroll
    for (int f = 0; f < 12; ++f) o.sums[row * 12 + f] = S[f];
  }
}

// ---------------------------------------------------------------------------
// Wave-per-row (serve batch sizes): the 64 lanes load the same row and lane
// `lane` walks trees lane, lane + 64, ... as rf_wave_scores does; the twelve
// partial sums are added up in LDS, where they are, and lane 0 stores.
// ---------------------------------------------------------------------------
__launch_bounds__(RF_EXPLAIN_BLOCK) __global__ void rf_explain_wave_kernel(
    const float* __restrict__ X, const uint2* __restrict__ nodes,
    const int* __restrict__ roots, const int* __restrict__ delta, ExplainOut o,
    long long n, int T, int C) {
  __shared__ __attribute__((aligned(16))) unsigned long long s_acc[12 * RF_EXPLAIN_PITCH];
  const int lane = threadIdx.x & (WAVE - 1);
  const long long row = (long long)blockIdx.x * (RF_EXPLAIN_BLOCK / WAVE) +
                        (threadIdx.x >> 6);
  if (row >= n) return;  // wave-uniform
  long long S[12];
  const int c = o.labels[row];  // wave-uniform
  if (c >= 0 && c < C) {
    const Row12 x = load_row12(X, row);  // broadcast load
    LaneSums acc(s_acc + threadIdx.x);
    acc.clear();
    for (int t = lane; t < T; t += WAVE) {
      int idx = roots[t];
      uint2 node = nodes[idx];
      while (true) {
        const unsigned feat = node.y & 0xffu;
        if (feat >= 0xf0u) break;  // a leaf, pure or mixed
        const float thr = __uint_as_float(node.x);
        idx = (sel12(x, feat) <= thr) ? idx + 1 : (int)(node.y >> 8);
        explain_step(nodes, delta, idx, C, c, feat, node, acc);
      }
    }
    // The wave's 12 x 64 partial sums lie in LDS already: lane f adds up
    // feature f's 64 as 32 16-byte reads and leaves the total in the wave's
    // first slot of that row, from where lane 0 takes all twelve.  (Twelve
    // wave_sum(unsigned long long) calls cost 144 full-width cross-lane LDS
    // operations per row and were most of the kernel: profiles/rf_explain.md.)
    unsigned long long* wave_row = s_acc + (threadIdx.x & ~(WAVE - 1));
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane < 12) {
      unsigned long long* mine = wave_row + lane * RF_EXPLAIN_PITCH;
      const ulonglong2* p = reinterpret_cast<const ulonglong2*>(mine);
      unsigned long long a = 0ull, b = 0ull;
#pragma unroll 8
      for (int k = 0; k < WAVE / 2; ++k) {
        const ulonglong2 v = p[k];
        a += v.x;
        b += v.y;
      }
      mine[0] = a + b;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int f = 0; f < 12; ++f) S[f] = (long long)wave_row[f * RF_EXPLAIN_PITCH];
  } else {
#pragma unroll
    for (int f = 0; f < 12; ++f) S[f] = 0;
  }
  if (lane == 0) explain_store(o, row, S);
}

// ---------------------------------------------------------------------------
// Row-per-lane (bulk): each lane's 12 features in LDS at pitch 13, node and
// delta tables in L2, as rf_scores_lane_kernel places them.  No barrier in
// the row loop, hence a plain grid-stride loop.
// ---------------------------------------------------------------------------
__launch_bounds__(RF_EXPLAIN_BLOCK) __global__ void rf_explain_lane_kernel(
    const float* __restrict__ X, const uint2* __restrict__ nodes,
    const int* __restrict__ roots, const int* __restrict__ delta, ExplainOut o,
    long long n, int T, int C) {
  __shared__ __attribute__((aligned(16))) unsigned long long s_acc[12 * RF_EXPLAIN_PITCH];
  __shared__ float s_feat[RF_EXPLAIN_BLOCK * 13];
  float* my_feat = s_feat + (int)threadIdx.x * 13;
  LaneSums acc(s_acc + threadIdx.x);

  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x; row < n;
       row += stride) {
    long long S[12];
    const int c = o.labels[row];
    if (c >= 0 && c < C) {
      const Row12 x = load_row12(X, row);
#pragma unroll
      for (int j = 0; j < 12; ++j) my_feat[j] = x.v[j];
      acc.clear();
      for (int t = 0; t < T; ++t) {
        int idx = roots[t];
        uint2 node = nodes[idx];
        while (true) {
          const unsigned feat = node.y & 0xffu;
          if (feat >= 0xf0u) break;  // a leaf, pure or mixed
          const float thr = __uint_as_float(node.x);
          idx = (my_feat[feat] <= thr) ? idx + 1 : (int)(node.y >> 8);
          explain_step(nodes, delta, idx, C, c, feat, node, acc);
        }
      }
#pragma unroll
      for (int f = 0; f < 12; ++f) S[f] = (long long)acc.get(f);
    } else {
#pragma unroll
      for (int f = 0; f < 12; ++f) S[f] = 0;
    }
    explain_store(o, row, S);
  }
}

// Returns 0, or nonzero when C is outside 2..8 or T outside 1..4096 (nothing
// is launched and the outputs stay unwritten: the caller must turn that into
// an error).  `contrib` and `sums` may be null.
//
// Read per launch, like TCSDN_IFOREST_MODE:
//   TCSDN_RF_EXPLAIN_MODE=wave|lane  force one kernel at any n (default:
//       wave-per-row up to RF_EXPLAIN_WAVE_MAX_ROWS, where the two were
//       measured to cross on the shipped forest: profiles/rf_explain.md)
//   TCSDN_RF_EXPLAIN_BLOCKS=<n>      cap on the row-per-lane grid, so small
//       inputs make each block loop over several tiles
// No sync and no allocation: safe under stream capture.
#define RF_EXPLAIN_WAVE_MAX_ROWS 65536

extern "C" int launch_rf_explain(const float* X, const unsigned* nodes,
                                 const int* roots, const int* delta,
                                 const int* labels, float* contrib, int* why,
                                 float* why_value, long long* sums, long long n,
                                 int T, int C, hipStream_t stream) {
  if (C < 2 || C > 8) return 1;
  if (T < 1 || T > 4096) return 1;
  if (n <= 0) return 0;
  bool wave = n <= RF_EXPLAIN_WAVE_MAX_ROWS;
  if (const char* e = getenv("TCSDN_RF_EXPLAIN_MODE")) {
    if (!strcmp(e, "wave")) wave = true;
    else if (!strcmp(e, "lane")) wave = false;
  }
  const uint2* nd = reinterpret_cast<const uint2*>(nodes);
  const ExplainOut o{labels, contrib, why, why_value, sums,
                     1073741824.0 * (double)T};
  if (wave) {
    hipLaunchKernelGGL(rf_explain_wave_kernel,
                       dim3((unsigned)((n + 3) / 4)), dim3(RF_EXPLAIN_BLOCK), 0,
                       stream, X, nd, roots, delta, o, n, T, C);
  } else {
    const int grid = ts_grid(n, RF_EXPLAIN_BLOCK,
                             env_block_cap("TCSDN_RF_EXPLAIN_BLOCKS", 8192));
    hipLaunchKernelGGL(rf_explain_lane_kernel, dim3(grid),
                       dim3(RF_EXPLAIN_BLOCK), 0, stream, X, nd, roots, delta,
                       o, n, T, C);
  }
  return 0;
}
