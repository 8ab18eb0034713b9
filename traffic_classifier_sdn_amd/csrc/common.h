// Common device helpers for the CDNA4 (gfx950) kernels.
// Target: MI355X only — wave64, 256 CUs / 8 XCDs, 160 KiB LDS per CU.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdlib>
#include <type_traits>

#define WAVE 64
#define DEV __device__ __forceinline__

// Grid sizing for memory-bound grid-stride kernels (guide G11):
// cap blocks, grid-stride the rest.
static inline int ts_grid(long long work, int block, int cap = 2048) {
  long long b = (work + block - 1) / block;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

// A grid cap that the environment variable `name` (read per launch) may
// lower, never raise: tests set it so that small inputs make each block
// loop over several row tiles and end on a partial one.
static inline int env_block_cap(const char* name, int cap) {
  if (const char* e = getenv(name)) {
    const int v = atoi(e);
    if (v >= 1 && v < cap) cap = v;
  }
  return cap;
}

// Host-side dispatch of a runtime integer onto a list of compile-time ones:
// calls f(std::integral_constant<int, V>{}) for the V that equals v and
// returns true, or calls nothing and returns false.  A launcher turns false
// into its nonzero "nothing was launched" return.
template <int... Vs, class F>
static inline bool dispatch_int(int v, F&& f) {
  return ((v == Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...);
}

// 12-float feature row load: rows are 48 B, so every row is 16-B aligned
// when the base pointer is. 3x float4 per row.
struct Row12 {
  float v[12];
};

DEV Row12 load_row12(const float* __restrict__ X, long long row) {
  Row12 r;
  const float4* p = reinterpret_cast<const float4*>(X + row * 12);
  float4 a = p[0], b = p[1], c = p[2];
  r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w;
  r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
  r.v[8] = c.x; r.v[9] = c.y; r.v[10] = c.z; r.v[11] = c.w;
  return r;
}

// wave-level f32/f64 sum over all 64 lanes
DEV float wave_sum(float x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  return x;
}

DEV double wave_sum(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  return x;
}

DEV unsigned long long wave_sum(unsigned long long x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  return x;
}

// Forest traversal helpers shared by predict_kernels.hip and
// rf_proba_kernels.hip.  The row-per-lane kernels (rf_predict_kernel,
// rf_predict_stream_kernel, rf_scores_lane_kernel) keep their own walks: a
// shared body cost them registers (profiles/kernel_bodies.md).

// select v[f] for runtime f in [0,12) with compile-time register indices:
// two levels — pick r = f&3 within each quad, then the quad q = f>>2.
DEV float sel12(const Row12& x, unsigned f) {
  unsigned r = f & 3u, q = f >> 2;
  float a = (r & 1u) ? x.v[1] : x.v[0];
  float b = (r & 2u) ? ((r & 1u) ? x.v[3] : x.v[2]) : a;
  float q0 = b;
  float c = (r & 1u) ? x.v[5] : x.v[4];
  float d = (r & 2u) ? ((r & 1u) ? x.v[7] : x.v[6]) : c;
  float q1 = d;
  float e = (r & 1u) ? x.v[9] : x.v[8];
  float g = (r & 2u) ? ((r & 1u) ? x.v[11] : x.v[10]) : e;
  float q2 = g;
  float lo = (q & 1u) ? q1 : q0;
  return (q & 2u) ? q2 : lo;
}

// Pure-leaf votes of class c out of the packed register (10 bits per class).
// Only classes 0..5 have a field: rf_pack gives a forest with more classes
// no pure leaves, and a shift past bit 63 must not even be formed (c is a
// compile-time constant in every caller's unrolled loop).  The u32 cast
// keeps the convert a single instruction.
DEV float vote_count(unsigned long long votes, int c) {
  return c * 10 + 10 <= 64 ? (float)(unsigned)((votes >> (c * 10)) & 1023ull)
                           : 0.f;
}

// Wave-per-row forest scores, the one statement of what rf_predict_wave_kernel
// and rf_scores_wave_kernel compute: the wave's 64 lanes load the same row
// and lane `lane` walks trees lane, lane+64, ...  Nodes are read from global
// memory (the packed forest, tens of KB, stays L2-resident); per lane the
// mixed leaves are added in tree order, then the packed counter and the C
// partial sums are reduced with wave_sum.  On return
//   sc[c] = acc[c] + pure count[c]
// holds the row's class sums in lane 0 (other lanes hold partial values).
template <int C>
DEV void rf_wave_scores(const float* __restrict__ X, long long row, int lane,
                        const uint2* __restrict__ nodes,
                        const int* __restrict__ roots,
                        const float* __restrict__ leaf_proba, int T,
                        float (&sc)[C]) {
  Row12 x = load_row12(X, row);  // broadcast load
  float acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.f;
  unsigned long long votes = 0ull;  // 10-bit packed per-class pure counts
  for (int t = lane; t < T; t += WAVE) {
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
      idx = (sel12(x, feat) <= thr) ? idx + 1 : (int)(node.y >> 8);
    }
  }
  votes = wave_sum(votes);  // per-field sums stay < 1024: no cross-field carry
#pragma unroll
  for (int c = 0; c < C; ++c) sc[c] = wave_sum(acc[c]) + vote_count(votes, c);
}

// First-maximum argmax of the C scores (sklearn's tie rule; compared with >,
// so a NaN never wins).  Only compile-time indices into sc[].
struct ArgMax {
  int idx;
  float val;
};

template <int C>
DEV ArgMax first_max(const float (&sc)[C]) {
  float best = -INFINITY;
  int bi = 0;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    if (sc[c] > best) { best = sc[c]; bi = c; }
  }
  return {bi, best};
}
