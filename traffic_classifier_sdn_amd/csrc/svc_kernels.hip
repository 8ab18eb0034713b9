// RBF SVC for gfx950 (C = 2..6, F = 12): one-vs-one labels (SURVEY.md §2.2
// N2), the f64 decision values of every row, and class probabilities from
// Platt sigmoids coupled by the method of Wu, Lin and Weng (libsvm's
// multiclass_probability; sklearn's SVC(probability=True)).
//
//   svc_predict_kernel<C>, svc_predict_wave_kernel<C>
//       i32 [n] labels: majority vote of the pair decisions, first maximum.
//   svc_decision_kernel<C>, svc_decision_wave_kernel<C>
//       f64 [n, C(C-1)/2] decision values, pair order (0,1),(0,2)..(C-2,C-1)
//       as ops.cpu.svc_ovo_decision.
//   svc_couple_kernel<C>
//       one row per lane: sigmoids, the coupling iteration, the vote.
//
// The accumulation is written once per variant, svc_tiled_rows and
// svc_wave_row.  A body hands each pair's decision value to a SINK as soon
// as it is formed: the label sink votes on its sign, the decision sink
// stores it.  svc_predict_wave_kernel and svc_decision_wave_kernel are one
// body with two sinks, so every stored decision has the sign the label
// kernel votes with and a label is the same with and without probabilities;
// svc_decision_kernel is svc_tiled_rows with the storing sink, and
// svc_predict_kernel states the same loop itself (why: at the kernel).
// (A body that first filled dec[NPAIR] and then handed the array over put
// the tiled kernels, which sit at the 128-VGPR cap at C = 6, into scratch:
// profiles/kernel_bodies.md.)
//
// As in predict_kernels.hip, every per-lane array is sized by the template
// parameter and indexed only inside fully unrolled loops, so nothing is
// indexed at run time and nothing goes to scratch.
//
// No kernel here syncs or allocates: all are safe under stream capture.

#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "launchers.h"

#define SVC_TILE 128
#define SVC_BLOCK 256
// Up to this many rows the wave-per-row kernels run, above it the tiled ones:
// at 65K rows the wave-per-row label kernel beats the tiled one (serve 34.5
// -> 39.6M flows/s), so the cutover sits at 131072 (as for the forest).
#define SVC_WAVE_MAX_ROWS 131072

// Label sink: one-vs-one vote, dec > 0 votes for the pair's first class and
// the first maximum wins ties (libsvm semantics; ops.cpu.svc_vote).
template <int C>
struct SvcLabelSink {
  int* __restrict__ out;  // [n]
  int votes[C];
  DEV void begin() {
#pragma unroll
    for (int c = 0; c < C; ++c) votes[c] = 0;
  }
  DEV void pair(long long, int i, int j, int, double dec) {
    if (dec > 0.0) votes[i]++; else votes[j]++;
  }
  DEV int winner() const {
    int best = -1, bi = 0;
#pragma unroll
    for (int c = 0; c < C; ++c)
      if (votes[c] > best) { best = votes[c]; bi = c; }
    return bi;
  }
  DEV void end(long long row) { out[row] = winner(); }
};

// Decision sink: pair p of the row goes to out[row, p].
template <int C>
struct SvcDecisionSink {
  double* __restrict__ out;  // [n, NPAIR]
  DEV void begin() {}
  DEV void pair(long long row, int, int, int p, double dec) {
    out[row * (C * (C - 1) / 2) + p] = dec;
  }
  DEV void end(long long) {}
};

// ---------------------------------------------------------------------------
// Row per lane (large batches).  SV tiles (features, libsvm dual rows, class
// ids) stream through LDS; each lane keeps C*(C-1) accumulators
//   acc[c][r] = sum over SVs of class c of dual[r][sv] * exp(-gamma*d2(x,sv))
// then dec(i<j) = acc[i][j-1] + acc[j][i] + b[pair].
// The per-SV class branch is wave-UNIFORM (the sv index is uniform across
// the block), so only the matching unrolled branch executes and all
// accumulator indices stay compile-time.
// ---------------------------------------------------------------------------
template <int C, class Sink>
DEV void svc_tiled_rows(const float* __restrict__ X,
                        const float* __restrict__ SV,    // [nsv,F]
                        const float* __restrict__ dual,  // [C-1,nsv]
                        const unsigned char* __restrict__ svclass,
                        const float* __restrict__ intercept,
                        long long n, int nsv, float gamma, Sink sink) {
  constexpr int F = 12;
  constexpr int CR = C - 1;
  constexpr int NPAIR = C * (C - 1) / 2;
  __shared__ __attribute__((aligned(16))) float s_sv[SVC_TILE * F];
  __shared__ float s_dual[CR * SVC_TILE];
  __shared__ unsigned char s_cls[SVC_TILE];
  __shared__ float s_b[NPAIR];

  for (int i = threadIdx.x; i < NPAIR; i += blockDim.x) s_b[i] = intercept[i];

  long long stride = (long long)gridDim.x * blockDim.x;
  // lock-step row tiles so the SV staging loop stays uniform per block
  for (long long base = (long long)blockIdx.x * blockDim.x; base < n;
       base += stride) {
    long long row = base + threadIdx.x;
    Row12 x;
    if (row < n) x = load_row12(X, row);
    // f64 running accumulators + per-tile f32 partials: a single f32 chain
    // over tens of thousands of SIGNED near-unit dual terms (thousands of
    // alphas at the C bound in a non-separable fit) loses the O(1) decision
    // value to rounding (measured: 24% wrong votes at 35K SVs); a 128-term
    // f32 partial folded into f64 per tile is exact to ~1e-5 at any nsv
    double acc[C * CR];
#pragma unroll
    for (int i = 0; i < C * CR; ++i) acc[i] = 0.0;

    for (int tile = 0; tile < nsv; tile += SVC_TILE) {
      int cnt = min(SVC_TILE, nsv - tile);
      __syncthreads();
      for (int i = threadIdx.x; i < cnt * F; i += blockDim.x)
        s_sv[i] = SV[(long long)tile * F + i];
#pragma unroll
      for (int r = 0; r < CR; ++r)
        for (int i = threadIdx.x; i < cnt; i += blockDim.x)
          s_dual[r * SVC_TILE + i] = dual[(long long)r * nsv + tile + i];
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
                    fmaf(s_dual[r * SVC_TILE + s], kv, accT[cc * CR + r]);
            }
          }
        }
#pragma unroll
        for (int i = 0; i < C * CR; ++i) acc[i] += (double)accT[i];
      }
    }
    if (row >= n) continue;
    sink.begin();
    int p = 0;
#pragma unroll
    for (int i = 0; i < C; ++i)
#pragma unroll
      for (int j = i + 1; j < C; ++j, ++p)
        sink.pair(row, i, j, p,
                  acc[i * CR + (j - 1)] + acc[j * CR + i] + (double)s_b[p]);
    sink.end(row);
  }
}

// ---------------------------------------------------------------------------
// Small batches: ONE WAVE PER ROW, SVs split across lanes.  At serve batch
// sizes (thousands of rows) the row-per-lane body leaves most of the chip
// idle and each lane walks all nsv SVs serially; here n waves fill the 1024
// SIMDs and the per-row latency drops ~100x (serve-path profile:
// profiles/serve_kernel_trace_r01.md).  SV rows stream from global memory —
// the working set (nsv * 69 B) stays L2-resident and is shared by every
// wave.  The per-SV class is NOT wave-uniform here, so the accumulator
// update is an unrolled compile-time switch on the class id.  Lane 0 feeds
// the sink.
// ---------------------------------------------------------------------------
template <int C, class Sink>
DEV void svc_wave_row(const float* __restrict__ X, const float* __restrict__ SV,
                      const float* __restrict__ dual,
                      const unsigned char* __restrict__ svclass,
                      const float* __restrict__ intercept, long long n, int nsv,
                      float gamma, Sink sink) {
  constexpr int F = 12;
  constexpr int CR = C - 1;
  const int lane = threadIdx.x & (WAVE - 1);
  const long long row = (long long)blockIdx.x * (blockDim.x / WAVE) +
                        (threadIdx.x >> 6);
  if (row >= n) return;
  Row12 x = load_row12(X, row);  // broadcast load, all lanes same row
  // f64 per-lane accumulators: the 64-way split already conditions the sum,
  // but signed bounded-alpha duals at large nsv still overwhelm f32 (same
  // hazard as the tiled body — see comment there)
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
  // cross-lane reduction of the C*(C-1) partial sums
#pragma unroll
  for (int i = 0; i < C * CR; ++i) acc[i] = wave_sum(acc[i]);
  if (lane == 0) {
    sink.begin();
    int p = 0;
#pragma unroll
    for (int i = 0; i < C; ++i)
#pragma unroll
      for (int j = i + 1; j < C; ++j, ++p)
        sink.pair(row, i, j, p,
                  acc[i * CR + (j - 1)] + acc[j * CR + i] + (double)intercept[p]);
    sink.end(row);
  }
}

#define SVC_KERNEL_ARGS(OUT_T)                                               \
  const float* __restrict__ X, const float* __restrict__ SV,                 \
      const float* __restrict__ dual,                                        \
      const unsigned char* __restrict__ svclass,                             \
      const float* __restrict__ intercept, OUT_T* __restrict__ out,          \
      long long n, int nsv, float gamma

// The tiled label kernel is the one kernel here that does NOT call its body:
// it states svc_tiled_rows' loop and SvcLabelSink's vote itself.  Built as
// svc_tiled_rows + SvcLabelSink it had the same registers, LDS and, modulo
// scalar register numbers, the same instructions in the SV loop, but the
// shorter prologue moved that loop in the code and 2^20 rows of the shipped
// model took 2.90 ms instead of 2.83 ms, in every round of every run
// (profiles/kernel_bodies.md).  It is on the bench path, so it keeps the
// text that measures 2.83 ms.  Change it only together with svc_tiled_rows
// (tests/test_svc_proba_kernels.py compares its labels with the votes of
// svc_decision_kernel's decisions exactly).
template <int C>
__global__ void svc_predict_kernel(const float* __restrict__ X,
                                   const float* __restrict__ SV,    // [nsv,F]
                                   const float* __restrict__ dual,  // [C-1,nsv]
                                   const unsigned char* __restrict__ svclass,
                                   const float* __restrict__ intercept,
                                   int* __restrict__ out,
                                   long long n, int nsv, float gamma) {
  constexpr int F = 12;
  constexpr int CR = C - 1;
  constexpr int NPAIR = C * (C - 1) / 2;
  __shared__ __attribute__((aligned(16))) float s_sv[SVC_TILE * F];
  __shared__ float s_dual[CR * SVC_TILE];
  __shared__ unsigned char s_cls[SVC_TILE];
  __shared__ float s_b[NPAIR];

  for (int i = threadIdx.x; i < NPAIR; i += blockDim.x) s_b[i] = intercept[i];

  long long stride = (long long)gridDim.x * blockDim.x;
  // lock-step row tiles so the SV staging loop stays uniform per block
  for (long long base = (long long)blockIdx.x * blockDim.x; base < n;
       base += stride) {
    long long row = base + threadIdx.x;
    Row12 x;
    if (row < n) x = load_row12(X, row);
    double acc[C * CR];  // f64 folds of f32 tile partials: see svc_tiled_rows
#pragma unroll
    for (int i = 0; i < C * CR; ++i) acc[i] = 0.0;

    for (int tile = 0; tile < nsv; tile += SVC_TILE) {
      int cnt = min(SVC_TILE, nsv - tile);
      __syncthreads();
      for (int i = threadIdx.x; i < cnt * F; i += blockDim.x)
        s_sv[i] = SV[(long long)tile * F + i];
#pragma unroll
      for (int r = 0; r < CR; ++r)
        for (int i = threadIdx.x; i < cnt; i += blockDim.x)
          s_dual[r * SVC_TILE + i] = dual[(long long)r * nsv + tile + i];
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
                    fmaf(s_dual[r * SVC_TILE + s], kv, accT[cc * CR + r]);
            }
          }
        }
#pragma unroll
        for (int i = 0; i < C * CR; ++i) acc[i] += (double)accT[i];
      }
    }
    if (row >= n) continue;
    // SvcLabelSink's vote
    int votes[C];
#pragma unroll
    for (int c = 0; c < C; ++c) votes[c] = 0;
    int p = 0;
#pragma unroll
    for (int i = 0; i < C; ++i)
#pragma unroll
      for (int j = i + 1; j < C; ++j, ++p) {
        double dec = acc[i * CR + (j - 1)] + acc[j * CR + i] + (double)s_b[p];
        if (dec > 0.0) votes[i]++; else votes[j]++;
      }
    int best = -1, bi = 0;
#pragma unroll
    for (int c = 0; c < C; ++c)
      if (votes[c] > best) { best = votes[c]; bi = c; }
    out[row] = bi;
  }
}

template <int C>
__launch_bounds__(256) __global__ void svc_predict_wave_kernel(SVC_KERNEL_ARGS(int)) {
  svc_wave_row<C>(X, SV, dual, svclass, intercept, n, nsv, gamma,
                  SvcLabelSink<C>{out});
}

template <int C>
__global__ void svc_decision_kernel(SVC_KERNEL_ARGS(double)) {
  svc_tiled_rows<C>(X, SV, dual, svclass, intercept, n, nsv, gamma,
                    SvcDecisionSink<C>{out});
}

template <int C>
__launch_bounds__(256) __global__ void svc_decision_wave_kernel(SVC_KERNEL_ARGS(double)) {
  svc_wave_row<C>(X, SV, dual, svclass, intercept, n, nsv, gamma,
                  SvcDecisionSink<C>{out});
}
#undef SVC_KERNEL_ARGS

// Wave per row or tiled, for labels and decisions alike: wave per row up to
// SVC_WAVE_MAX_ROWS.  TCSDN_SVC_DEC_MODE (read per launch, like
// TCSDN_RF_MODE) forces a variant at any n: 1 = wave per row, 2 = tiled.
static bool svc_use_wave(long long n) {
  bool wave = n <= SVC_WAVE_MAX_ROWS;
  if (const char* e = getenv("TCSDN_SVC_DEC_MODE")) {
    const int v = atoi(e);
    if (v == 1) wave = true;
    else if (v == 2) wave = false;
  }
  if (n > (1ll << 30)) wave = false;  // one wave per row: 4 rows per block
  return wave;
}

// Launches the label kernels (Out = int) or the decision kernels (Out =
// double).  Returns 0, or nonzero when C is outside 2..6 (nothing is launched
// and the output stays unwritten: the caller must turn that into an error).
// TCSDN_PROBA_BLOCKS caps the tiled grid as it does svc_couple_kernel's.
template <class Out>
static int svc_launch(const float* X, const float* SV, const float* dual,
                      const unsigned char* svclass, const float* intercept,
                      Out* out, long long n, int nsv, int C, float gamma,
                      hipStream_t stream) {
  if (C < 2 || C > 6) return 1;
  if (n <= 0) return 0;
  const bool wave = svc_use_wave(n);
  const dim3 grid = wave ? dim3((unsigned)((n + 3) / 4))
                         : dim3(ts_grid(n, SVC_BLOCK,
                                        env_block_cap("TCSDN_PROBA_BLOCKS", 2048)));
  return !dispatch_int<2, 3, 4, 5, 6>(C, [&](auto c) {
    constexpr int CV = decltype(c)::value;
    void (*kernel)(const float*, const float*, const float*,
                   const unsigned char*, const float*, Out*, long long, int,
                   float);
    if constexpr (std::is_same_v<Out, int>)
      kernel = wave ? svc_predict_wave_kernel<CV> : svc_predict_kernel<CV>;
    else
      kernel = wave ? svc_decision_wave_kernel<CV> : svc_decision_kernel<CV>;
    hipLaunchKernelGGL(kernel, grid, dim3(SVC_BLOCK), 0, stream, X, SV, dual,
                       svclass, intercept, out, n, nsv, gamma);
  });
}

extern "C" int launch_svc_predict(const float* X, const float* SV,
                                  const float* dual,
                                  const unsigned char* svclass,
                                  const float* intercept, int* out,
                                  long long n, int nsv, int C, float gamma,
                                  hipStream_t stream) {
  return svc_launch(X, SV, dual, svclass, intercept, out, n, nsv, C, gamma, stream);
}

extern "C" int launch_svc_decision(const float* X, const float* SV,
                                   const float* dual,
                                   const unsigned char* svclass,
                                   const float* intercept, double* out,
                                   long long n, int nsv, int C, float gamma,
                                   hipStream_t stream) {
  return svc_launch(X, SV, dual, svclass, intercept, out, n, nsv, C, gamma, stream);
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
__launch_bounds__(SVC_BLOCK) __global__ void svc_couple_kernel(
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
    SvcLabelSink<C> vote{idx};  // the label kernels' vote, on the loaded values
    vote.begin();
    {
      int p = 0;
#pragma unroll
      for (int i = 0; i < C; ++i)
#pragma unroll
        for (int j = i + 1; j < C; ++j, ++p) {
          const double dv = d[p];
          vote.pair(row, i, j, p, dv);
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
    const int bi = vote.winner();
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
  dim3 grid(ts_grid(n, SVC_BLOCK, env_block_cap("TCSDN_PROBA_BLOCKS", 2048)));
  return !dispatch_int<2, 3, 4, 5, 6>(C, [&](auto c) {
    hipLaunchKernelGGL((svc_couple_kernel<decltype(c)::value>), grid,
                       dim3(SVC_BLOCK), 0, stream, dec, probA, probB, proba,
                       idx, conf, n);
  });
}
