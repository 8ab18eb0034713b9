// SVC class probabilities for gfx950 (C = 2..6, F = 12): the one-vs-one
// decision values of every row, then Platt sigmoids coupled by the method of
// Wu, Lin and Weng (libsvm's multiclass_probability; sklearn's
// SVC(probability=True)).
//
//   svc_decision_kernel<C>, svc_decision_wave_kernel<C>
//       f64 [n, C(C-1)/2] decision values, pair order (0,1),(0,2)..(C-2,C-1)
//       as ops.cpu.svc_ovo_decision.  Each RE-STATES the accumulation of its
//       svc_predict* counterpart in predict_kernels.hip operation for
//       operation (SV tile of 128, per-tile f32 partials folded into f64,
//       __expf, the same wave reduction), so every decision has the sign the
//       label kernel votes with and a label is the same with and without
//       probabilities.  The label kernels stay where they are: they are on
//       the serve and bench path.  Change one side only together with the
//       other (tests/test_svc_proba_kernels.py compares the votes exactly).
//   svc_couple_kernel<C>
//       one row per lane: sigmoids, the coupling iteration, the vote.
//
// As in predict_kernels.hip, every per-lane array is sized by the template
// parameter and indexed only inside fully unrolled loops, so nothing is
// indexed at run time and nothing goes to scratch.
//
// No kernel here syncs or allocates: all are safe under stream capture.

#include <cstdlib>

#include "common.h"

#define SVCP_TILE 128  // = SVC_TILE of predict_kernels.hip
#define SVCP_BLOCK 256

template <int C>
__global__ void svc_decision_kernel(const float* __restrict__ X,
                                    const float* __restrict__ SV,    // [nsv,F]
                                    const float* __restrict__ dual,  // [C-1,nsv]
                                    const unsigned char* __restrict__ svclass,
                                    const float* __restrict__ intercept,
                                    double* __restrict__ out,  // [n,NPAIR]
                                    long long n, int nsv, float gamma) {
  constexpr int F = 12;
  constexpr int CR = C - 1;
  constexpr int NPAIR = C * (C - 1) / 2;
  __shared__ __attribute__((aligned(16))) float s_sv[SVCP_TILE * F];
  __shared__ float s_dual[CR * SVCP_TILE];
  __shared__ unsigned char s_cls[SVCP_TILE];
  __shared__ float s_b[NPAIR];

  for (int i = threadIdx.x; i < NPAIR; i += blockDim.x) s_b[i] = intercept[i];

  long long stride = (long long)gridDim.x * blockDim.x;
  // lock-step row tiles so the SV staging loop stays uniform per block
  for (long long base = (long long)blockIdx.x * blockDim.x; base < n;
       base += stride) {
    long long row = base + threadIdx.x;
    Row12 x;
    if (row < n) x = load_row12(X, row);
    double acc[C * CR];
#pragma unroll
    for (int i = 0; i < C * CR; ++i) acc[i] = 0.0;

    for (int tile = 0; tile < nsv; tile += SVCP_TILE) {
      int cnt = min(SVCP_TILE, nsv - tile);
      __syncthreads();
      for (int i = threadIdx.x; i < cnt * F; i += blockDim.x)
        s_sv[i] = SV[(long long)tile * F + i];
#pragma unroll
      for (int r = 0; r < CR; ++r)
        for (int i = threadIdx.x; i < cnt; i += blockDim.x)
          s_dual[r * SVCP_TILE + i] = dual[(long long)r * nsv + tile + i];
      for (int i = threadIdx.x; i < cnt; i += blockDim.x)
        s_cls[i] = svclass[tile + i];
      __syncthreads();
      if (row < n) {
        float accT[C * CR];
#pragma unroll
        for (int i = 0; i < C * CR; ++i) accT[i] = 0.f;
        for (int s = 0; s < cnt; ++s) {
          float d = 0.f;
#pragma unroll
          for (int j = 0; j < F; ++j) {
            float t = x.v[j] - s_sv[s * F + j];
            d = fmaf(t, t, d);
          }
          float kv = __expf(-gamma * d);
          int c = s_cls[s];  // wave-uniform
#pragma unroll
          for (int cc = 0; cc < C; ++cc) {
            if (c == cc) {
#pragma unroll
              for (int r = 0; r < CR; ++r)
                accT[cc * CR + r] =
                    fmaf(s_dual[r * SVCP_TILE + s], kv, accT[cc * CR + r]);
            }
          }
        }
#pragma unroll
        for (int i = 0; i < C * CR; ++i) acc[i] += (double)accT[i];
      }
    }
    if (row >= n) continue;
    double* o = out + row * NPAIR;
    int p = 0;
#pragma unroll
    for (int i = 0; i < C; ++i)
#pragma unroll
      for (int j = i + 1; j < C; ++j, ++p)
        o[p] = acc[i * CR + (j - 1)] + acc[j * CR + i] + (double)s_b[p];
  }
}

// One wave per row, SVs split across lanes (svc_predict_wave_kernel's
// accumulation); lane 0 writes the row's decisions.
template <int C>
__launch_bounds__(256) __global__ void svc_decision_wave_kernel(
    const float* __restrict__ X, const float* __restrict__ SV,
    const float* __restrict__ dual, const unsigned char* __restrict__ svclass,
    const float* __restrict__ intercept, double* __restrict__ out, long long n,
    int nsv, float gamma) {
  constexpr int F = 12;
  constexpr int CR = C - 1;
  constexpr int NPAIR = C * (C - 1) / 2;
  const int lane = threadIdx.x & (WAVE - 1);
  const long long row = (long long)blockIdx.x * (blockDim.x / WAVE) +
                        (threadIdx.x >> 6);
  if (row >= n) return;
  Row12 x = load_row12(X, row);  // broadcast load, all lanes same row
  double acc[C * CR];
#pragma unroll
  for (int i = 0; i < C * CR; ++i) acc[i] = 0.0;
  for (int s = lane; s < nsv; s += WAVE) {
    Row12 sv = load_row12(SV, s);
    float d = 0.f;
#pragma unroll
    for (int j = 0; j < F; ++j) {
      float t = x.v[j] - sv.v[j];
      d = fmaf(t, t, d);
    }
    float kv = __expf(-gamma * d);
    int c = svclass[s];
#pragma unroll
    for (int cc = 0; cc < C; ++cc) {
      if (c == cc) {
#pragma unroll
        for (int r = 0; r < CR; ++r)
          acc[cc * CR + r] += (double)(dual[(long long)r * nsv + s] * kv);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < C * CR; ++i) acc[i] = wave_sum(acc[i]);
  if (lane == 0) {
    double* o = out + row * NPAIR;
    int p = 0;
#pragma unroll
    for (int i = 0; i < C; ++i)
#pragma unroll
      for (int j = i + 1; j < C; ++j, ++p)
        o[p] = acc[i * CR + (j - 1)] + acc[j * CR + i] + (double)intercept[p];
  }
}

// Returns 0, or nonzero when C is outside 2..6 (nothing is launched and the
// output stays unwritten: the caller must turn that into an error).
// TCSDN_SVC_DEC_MODE (read per launch, like TCSDN_RF_MODE) forces a variant
// at any n: 1 = wave per row, 2 = tiled row per lane.  Default: wave per row
// up to the 131072 rows of launch_svc_predict's cutover.
extern "C" int launch_svc_decision(const float* X, const float* SV,
                                   const float* dual,
                                   const unsigned char* svclass,
                                   const float* intercept, double* out,
                                   long long n, int nsv, int C, float gamma,
                                   hipStream_t stream) {
  if (C < 2 || C > 6) return 1;
  if (n <= 0) return 0;
  bool wave = n <= 131072;
  if (const char* e = getenv("TCSDN_SVC_DEC_MODE")) {
    const int v = atoi(e);
    if (v == 1) wave = true;
    else if (v == 2) wave = false;
  }
  if (n > (1ll << 30)) wave = false;  // one wave per row: 4 rows per block
  if (wave) {
    dim3 wgrid((unsigned)((n + 3) / 4));
#define SVCD_WCASE(CV)                                                       \
  case CV:                                                                   \
    hipLaunchKernelGGL((svc_decision_wave_kernel<CV>), wgrid,                \
                       dim3(SVCP_BLOCK), 0, stream, X, SV, dual, svclass,    \
                       intercept, out, n, nsv, gamma);                       \
    return 0;
    switch (C) {
      SVCD_WCASE(2) SVCD_WCASE(3) SVCD_WCASE(4) SVCD_WCASE(5) SVCD_WCASE(6)
      default: return 1;
    }
#undef SVCD_WCASE
  }
  dim3 grid(ts_grid(n, SVCP_BLOCK));
#define SVCD_CASE(CV)                                                        \
  case CV:                                                                   \
    hipLaunchKernelGGL((svc_decision_kernel<CV>), grid, dim3(SVCP_BLOCK), 0, \
                       stream, X, SV, dual, svclass, intercept, out, n, nsv, \
                       gamma);                                               \
    return 0;
  switch (C) {
    SVCD_CASE(2) SVCD_CASE(3) SVCD_CASE(4) SVCD_CASE(5) SVCD_CASE(6)
    default: return 1;
  }
#undef SVCD_CASE
}

// ---------------------------------------------------------------------------
// Pairwise coupling.  A transcription of libsvm (svm.cpp: sigmoid_predict,
// svm_predict_probability, multiclass_probability), all in f64 and in its
// operation order, with contraction off so that a*b+c rounds twice as it
// does there:
//   r[i][j] = clamp(sigmoid(dec[p]*A[p] + B[p]), 1e-7, 1-1e-7), r[j][i] = 1-r[i][j]
//   Q[t][t] = sum_{j!=t} r[j][t]^2,   Q[t][j] = -r[j][t]*r[t][j]
//   p = 1/C; up to max(100, C) sweeps, each preceded by a fresh Qp, pQp and
//   the test max_t |Qp[t] - pQp| < 0.005/C; a sweep updates p[t] one t at a
//   time with the incremental Qp/pQp formulas; no final renormalisation.
// A lane that has met the test idles until its wave's last lane has.
// The vote is ops.cpu.svc_vote's: dec > 0 votes for the pair's first class,
// the first maximum wins ties.  conf is the coupled probability of the VOTED
// class, which need not be the row's largest.
// ---------------------------------------------------------------------------
template <int C>
__launch_bounds__(SVCP_BLOCK) __global__ void svc_couple_kernel(
    const double* __restrict__ dec, const double* __restrict__ probA,
    const double* __restrict__ probB, float* __restrict__ proba,
    int* __restrict__ idx, float* __restrict__ conf, long long n) {
#pragma clang fp contract(off)
  constexpr int NPAIR = C * (C - 1) / 2;
  constexpr int MAX_ITER = C > 100 ? C : 100;
  const double eps = 0.005 / C;
  long long stride = (long long)gridDim.x * blockDim.x;
  for (long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       row < n; row += stride) {
    const double* d = dec + row * NPAIR;
    double r[C * C];
    int votes[C];
#pragma unroll
    for (int c = 0; c < C; ++c) votes[c] = 0;
    {
      int p = 0;
#pragma unroll
      for (int i = 0; i < C; ++i)
#pragma unroll
        for (int j = i + 1; j < C; ++j, ++p) {
          const double dv = d[p];
          if (dv > 0.0) votes[i]++; else votes[j]++;
          const double fApB = dv * probA[p] + probB[p];
          double s;
          if (fApB >= 0) {
            const double e = exp(-fApB);
            s = e / (1.0 + e);
          } else {
            s = 1.0 / (1 + exp(fApB));
          }
          s = fmin(fmax(s, 1e-7), 1 - 1e-7);
          r[i * C + j] = s;
          r[j * C + i] = 1 - s;
        }
    }
    double Q[C * C], Qp[C], pr[C], pQp;
#pragma unroll
    for (int t = 0; t < C; ++t) {
      pr[t] = 1.0 / C;
      Qp[t] = 0;
      double q = 0;
#pragma unroll
      for (int j = 0; j < t; ++j) {
        q += r[j * C + t] * r[j * C + t];
        Q[t * C + j] = Q[j * C + t];
      }
#pragma unroll
      for (int j = t + 1; j < C; ++j) {
        q += r[j * C + t] * r[j * C + t];
        Q[t * C + j] = -r[j * C + t] * r[t * C + j];
      }
      Q[t * C + t] = q;
    }
    for (int iter = 0; iter < MAX_ITER; ++iter) {
      // stopping condition; Qp and pQp recomputed for numerical accuracy
      pQp = 0;
#pragma unroll
      for (int t = 0; t < C; ++t) {
        double a = 0;
#pragma unroll
        for (int j = 0; j < C; ++j) a += Q[t * C + j] * pr[j];
        Qp[t] = a;
        pQp += pr[t] * a;
      }
      double max_error = 0;
#pragma unroll
      for (int t = 0; t < C; ++t) {
        const double error = fabs(Qp[t] - pQp);
        if (error > max_error) max_error = error;
      }
      if (max_error < eps) break;
#pragma unroll
      for (int t = 0; t < C; ++t) {
        const double diff = (-Qp[t] + pQp) / Q[t * C + t];
        pr[t] += diff;
        pQp = (pQp + diff * (diff * Q[t * C + t] + 2 * Qp[t])) / (1 + diff) /
              (1 + diff);
#pragma unroll
        for (int j = 0; j < C; ++j) {
          Qp[j] = (Qp[j] + diff * Q[t * C + j]) / (1 + diff);
          pr[j] /= (1 + diff);
        }
      }
    }
    int best = -1, bi = 0;
#pragma unroll
    for (int c = 0; c < C; ++c)
      if (votes[c] > best) { best = votes[c]; bi = c; }
    float cf = 0.f;
    float* o = proba + row * C;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float pf = (float)pr[c];
      o[c] = pf;
      if (c == bi) cf = pf;
    }
    idx[row] = bi;
    conf[row] = cf;
  }
}

// Returns 0, or nonzero when C is outside 2..6.  TCSDN_PROBA_BLOCKS=<n>
// (read per launch) caps the grid as it does for ensemble_kernels.hip, so
// small inputs make each block loop over several row tiles.
extern "C" int launch_svc_couple(const double* dec, const double* probA,
                                 const double* probB, float* proba, int* idx,
                                 float* conf, long long n, int C,
                                 hipStream_t stream) {
  if (C < 2 || C > 6) return 1;
  if (n <= 0) return 0;
  int cap = 2048;
  if (const char* e = getenv("TCSDN_PROBA_BLOCKS")) {
    const int v = atoi(e);
    if (v >= 1 && v < cap) cap = v;
  }
  dim3 grid(ts_grid(n, SVCP_BLOCK, cap));
#define SVCC_CASE(CV)                                                        \
  case CV:                                                                   \
    hipLaunchKernelGGL((svc_couple_kernel<CV>), grid, dim3(SVCP_BLOCK), 0,   \
                       stream, dec, probA, probB, proba, idx, conf, n);      \
    return 0;
  switch (C) {
    SVCC_CASE(2) SVCC_CASE(3) SVCC_CASE(4) SVCC_CASE(5) SVCC_CASE(6)
    default: return 1;
  }
#undef SVCC_CASE
}
