// Common device helpers for the CDNA4 (gfx950) kernels.
// Target: MI355X only — wave64, 256 CUs / 8 XCDs, 160 KiB LDS per CU.
#pragma once

#include <hip/hip_runtime.h>

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
// rf_proba_kernels.hip.

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
