// Class probabilities of the non-forest models on device, and the soft vote
// that combines the members' probabilities into one label and confidence.
//
//   gnb_proba_kernel       softmax of the Gaussian NB joint log-likelihoods
//   linear_proba_kernel    softmax of the logistic logits
//   knn_vote_proba_kernel  neighbour vote fractions from a top-k index list
//   ensemble_vote_kernel   weighted average of up to 8 members' probabilities
//   proba_smooth_kernel    per-flow moving average of a probability row
//                          across polls, with a margin for switching labels
//
// Conventions of predict_kernels.hip: 12 features and load_row12, parameters
// broadcast through LDS, grid-stride loops, per-lane arrays sized by a
// template parameter and indexed only in fully unrolled loops.  No sync and
// no allocation in any launcher: all of them capture into a graph.
//
// The two softmax kernels work in f64 from the models' own f64/f32
// parameters: a probability is exp of a DIFFERENCE of scores, so an absolute
// score error e becomes a relative probability error e, and f32 scores of
// magnitude 1e5 (the shipped logistic model on flow counters) would leave
// no digit of it.  One row per lane; the outputs are f32.

#include <cstdlib>

#include "common.h"
#include "launchers.h"

#define PROBA_BLOCK 256

// Grid of the row-per-lane kernels here.  TCSDN_PROBA_BLOCKS=<n> (read per
// launch) caps it, so small inputs make each block loop over several row
// tiles with a partial last one.
static int proba_grid(long long n) {
  return ts_grid(n, PROBA_BLOCK, env_block_cap("TCSDN_PROBA_BLOCKS", 2048));
}

// The softmax kernels read up to 2 * 8 * 12 f64 parameters from LDS per row.
// They do not change between rows, so the compiler would lift them all out
// of the grid-stride loop into registers: 256 VGPRs plus AGPR spills and one
// wave per SIMD.  A compiler-level memory barrier at the top of the loop
// keeps the reads where they are (it emits no instruction).
#define PROBA_NO_HOIST() asm volatile("" ::: "memory")

// A lane's row of CN floats at p + row * CN, in the widest accesses its
// alignment allows: rows of a 16-B aligned base are 16-B aligned when CN is
// a multiple of 4 and 8-B aligned when it is even.
template <int CN>
DEV void load_probs(const float* __restrict__ p, long long row, float (&v)[CN]) {
  const float* r = p + row * CN;
  if (CN % 4 == 0) {
#pragma unroll
    for (int i = 0; i < CN / 4; ++i) {
      const float4 q = reinterpret_cast<const float4*>(r)[i];
      v[4 * i] = q.x; v[4 * i + 1] = q.y; v[4 * i + 2] = q.z; v[4 * i + 3] = q.w;
    }
  } else if (CN % 2 == 0) {
#pragma unroll
    for (int i = 0; i < CN / 2; ++i) {
      const float2 q = reinterpret_cast<const float2*>(r)[i];
      v[2 * i] = q.x; v[2 * i + 1] = q.y;
    }
  } else {
#pragma unroll
    for (int i = 0; i < CN; ++i) v[i] = r[i];
  }
}

template <int CN>
DEV void store_probs(float* __restrict__ p, long long row, const float (&v)[CN]) {
  float* r = p + row * CN;
  if (CN % 4 == 0) {
#pragma unroll
    for (int i = 0; i < CN / 4; ++i)
      reinterpret_cast<float4*>(r)[i] =
          make_float4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
  } else if (CN % 2 == 0) {
#pragma unroll
    for (int i = 0; i < CN / 2; ++i)
      reinterpret_cast<float2*>(r)[i] = make_float2(v[2 * i], v[2 * i + 1]);
  } else {
#pragma unroll
    for (int i = 0; i < CN; ++i) r[i] = v[i];
  }
}

// Max-subtracted softmax in f64, stored as f32.
template <int C>
DEV void softmax_store(const double (&s)[C], float* __restrict__ proba, long long row) {
  double mx = s[0];
#pragma unroll
  for (int c = 1; c < C; ++c) mx = s[c] > mx ? s[c] : mx;
  double e[C];
  double sum = 0.0;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    e[c] = exp(s[c] - mx);
    sum += e[c];
  }
  float out[C];
#pragma unroll
  for (int c = 0; c < C; ++c) out[c] = (float)(e[c] / sum);
  store_probs<C>(proba, row, out);
}

// ---------------------------------------------------------------------------
// Gaussian NB:  ll[c] = const[c] - 0.5 * sum_j (x_j - theta[c,j])^2 * inv_var[c,j]
// const and inv_var are derived on the host in f64 (ops/gpu.py).
// ---------------------------------------------------------------------------
template <int C>
__launch_bounds__(PROBA_BLOCK) __global__ void gnb_proba_kernel(
    const float* __restrict__ X, const double* __restrict__ theta,
    const double* __restrict__ inv_var, const double* __restrict__ cconst,
    float* __restrict__ proba, long long n) {
  constexpr int F = 12;
  __shared__ double s_theta[C * F];
  __shared__ double s_ivar[C * F];
  __shared__ double s_const[C];
  for (int i = threadIdx.x; i < C * F; i += blockDim.x) {
    s_theta[i] = theta[i];
    s_ivar[i] = inv_var[i];
  }
  for (int i = threadIdx.x; i < C; i += blockDim.x) s_const[i] = cconst[i];
  __syncthreads();

  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x; row < n;
       row += stride) {
    PROBA_NO_HOIST();
    const Row12 x = load_row12(X, row);
    double ll[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      double q = 0.0;
#pragma unroll
      for (int j = 0; j < F; ++j) {
        const double d = (double)x.v[j] - s_theta[c * F + j];
        q = fma(d * d, s_ivar[c * F + j], q);
      }
      ll[c] = s_const[c] - 0.5 * q;
    }
    softmax_store<C>(ll, proba, row);
  }
}

// ---------------------------------------------------------------------------
// Logistic:  z[c] = b[c] + sum_j x_j * w[c,j], the f32 parameters upcast.
// ---------------------------------------------------------------------------
template <int C>
__launch_bounds__(PROBA_BLOCK) __global__ void linear_proba_kernel(
    const float* __restrict__ X, const float* __restrict__ W,
    const float* __restrict__ b, float* __restrict__ proba, long long n) {
  constexpr int F = 12;
  __shared__ double s_w[C * F];
  __shared__ double s_b[C];
  for (int i = threadIdx.x; i < C * F; i += blockDim.x) s_w[i] = (double)W[i];
  for (int i = threadIdx.x; i < C; i += blockDim.x) s_b[i] = (double)b[i];
  __syncthreads();

  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x; row < n;
       row += stride) {
    PROBA_NO_HOIST();
    const Row12 x = load_row12(X, row);
    double z[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      double a = s_b[c];
#pragma unroll
      for (int j = 0; j < F; ++j) a = fma((double)x.v[j], s_w[c * F + j], a);
      z[c] = a;
    }
    softmax_store<C>(z, proba, row);
  }
}

// ---------------------------------------------------------------------------
// KNN vote fractions:  proba[c] = count[c] / k_valid  (IEEE f32 division).
// An entry outside 0 <= idx < nr is not counted: idx < 0 is the top-k
// kernels' padding when the reference set has fewer than k rows, and nothing
// past the label array is ever read.  The contract is k_valid >= 1.
// ---------------------------------------------------------------------------
template <int C>
__launch_bounds__(PROBA_BLOCK) __global__ void knn_vote_proba_kernel(
    const int* __restrict__ idx, const unsigned char* __restrict__ y,
    float* __restrict__ proba, long long n, int k, long long nr) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x; row < n;
       row += stride) {
    const int* r = idx + row * k;
    int count[C];
#pragma unroll
    for (int c = 0; c < C; ++c) count[c] = 0;
    int valid = 0;
    for (int i = 0; i < k; ++i) {
      const int ri = r[i];
      if (ri >= 0 && (long long)ri < nr) {
        const int lab = y[ri];
        ++valid;
#pragma unroll
        for (int c = 0; c < C; ++c) count[c] += lab == c ? 1 : 0;
      }
    }
    const float fk = (float)valid;
    float out[C];
#pragma unroll
    for (int c = 0; c < C; ++c) out[c] = (float)count[c] / fk;
    store_probs<C>(proba, row, out);
  }
}

// ---------------------------------------------------------------------------
// Soft vote.  Per row: avg[c] = 0, then in member order
//   avg[map_m[j]] = fmaf(w_m, p_m[row, j], avg[map_m[j]])   for j < C_m
// so a class a member lacks gets nothing from it; label = first-maximum
// argmax of avg (compared with >, so a NaN never wins), conf = that maximum,
// bit for bit the maximum of the stored avg row.
//
// The member table arrives by value in the kernel arguments and one lane
// puts it into LDS, from where the runtime member index reads it (a runtime
// index into the argument block itself would send it through scratch).  The
// member's class count picks a load_probs instantiation under a
// block-uniform switch; the ensemble column of a member column is a runtime
// value, so each fmaf is applied under a select over the C compile-time
// accumulators instead of indexing avg[] with it.
//
// Traffic per row is sum_m 4 C_m bytes in and 4 C (optional) + 8 bytes out,
// every byte touched once: a lane moves its rows as float4 / float2 where
// the row pitch keeps them aligned, and the instructions of one row together
// use every byte of the lines they touch.
// ---------------------------------------------------------------------------
template <int C, int CM>
DEV void ens_add(const float* __restrict__ p, long long row, float w,
                 const unsigned char* map, float (&avg)[C]) {
  float v[CM];
  load_probs<CM>(p, row, v);
#pragma unroll
  for (int j = 0; j < CM; ++j) {
    const int col = map[j];
#pragma unroll
    for (int c = 0; c < C; ++c) avg[c] = col == c ? fmaf(w, v[j], avg[c]) : avg[c];
  }
}

template <int C, bool WANT_PROBA>
__launch_bounds__(PROBA_BLOCK) __global__ void ensemble_vote_kernel(
    const EnsembleArgs args, float* __restrict__ avg_out,
    int* __restrict__ labels, float* __restrict__ conf, long long n) {
  __shared__ EnsembleArgs s;
  if (threadIdx.x == 0) s = args;
  __syncthreads();
  const int M = args.M;

  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x; row < n;
       row += stride) {
    float avg[C];
#pragma unroll
    for (int c = 0; c < C; ++c) avg[c] = 0.f;
    for (int m = 0; m < M; ++m) {
      const float* __restrict__ p = s.p[m];
      const float w = s.w[m];
      const unsigned char* map = &s.map[m * ENS_MAX_C];
      switch (s.cm[m]) {  // block-uniform
        case 2: ens_add<C, 2>(p, row, w, map, avg); break;
        case 3: ens_add<C, 3>(p, row, w, map, avg); break;
        case 4: ens_add<C, 4>(p, row, w, map, avg); break;
        case 5: ens_add<C, 5>(p, row, w, map, avg); break;
        case 6: ens_add<C, 6>(p, row, w, map, avg); break;
        case 7: ens_add<C, 7>(p, row, w, map, avg); break;
        case 8: ens_add<C, 8>(p, row, w, map, avg); break;
        default: break;  // the launcher admits 2..8 only
      }
    }
    float best = -INFINITY;
    int bi = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if (avg[c] > best) { best = avg[c]; bi = c; }
    }
    labels[row] = bi;
    conf[row] = best;
    if (WANT_PROBA) store_probs<C>(avg_out, row, avg);
  }
}

// ---------------------------------------------------------------------------
// Per-flow smoothing of a probability row across polls.  `state` [cap, C] and
// `held` [cap] belong to the flow slots; per row r < n, with a and b = 1 - a
// formed by the caller in f32:
//   r >= *n_live     state[r] = 0, held[r] = -1; label and conf are the
//                    first-maximum argmax of proba[r] and that maximum
//   held[r] < 0      s = proba[r], bit for bit (first sighting)
//   otherwise        s[c] = fmaf(a, proba[r,c], b * state[r,c]), the product
//                    rounded once and the fused add once
// then top = first-maximum argmax of s, and the held label stays unless
// s[top] - s[held] > margin (an exact tie keeps it, also against a lower
// class index).  state[r] = s, held[r] = labels[r] = label, conf[r] =
// s[label]: the smoothed probability of the REPORTED class.
//
// The held class is a runtime index: s[held] is a select over the C
// registers (as ens_add applies its fmaf), which yields -inf for a value
// outside 0..C-1, so such a row switches to top and nothing is read out of
// bounds.  n_live is read from memory once per lane, so a captured graph
// over all cap rows follows a live count that the host changes between
// replays; null means all n rows are live.  One lane owns a row's state and
// held entry: no other lane reads or writes them.
//
// Traffic per row: 8 C + 4 bytes in (proba, state, held), 4 C + 12 bytes out
// (state, held, label, conf); a first sighting skips the state read.
// ---------------------------------------------------------------------------
template <int C>
__launch_bounds__(PROBA_BLOCK) __global__ void proba_smooth_kernel(
    const float* __restrict__ proba, float* __restrict__ state,
    int* __restrict__ held, const int* __restrict__ n_live, float a, float b,
    float margin, int* __restrict__ labels, float* __restrict__ conf,
    long long n) {
  const long long live = n_live ? (long long)*n_live : n;

  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x; row < n;
       row += stride) {
    float s[C];
    load_probs<C>(proba, row, s);
    if (row >= live) {
      const ArgMax m = first_max<C>(s);
      labels[row] = m.idx;
      conf[row] = m.val;
#pragma unroll
      for (int c = 0; c < C; ++c) s[c] = 0.f;
      store_probs<C>(state, row, s);
      held[row] = -1;
      continue;
    }
    const int h = held[row];
    if (h >= 0) {
      float old[C];
      load_probs<C>(state, row, old);
#pragma unroll
      for (int c = 0; c < C; ++c) s[c] = fmaf(a, s[c], __fmul_rn(b, old[c]));
    }
    const ArgMax m = first_max<C>(s);
    float sh = -INFINITY;
#pragma unroll
    for (int c = 0; c < C; ++c) sh = h == c ? s[c] : sh;
    const bool keep = h >= 0 && !(m.val - sh > margin);
    const int label = keep ? h : m.idx;
    store_probs<C>(state, row, s);
    held[row] = label;
    labels[row] = label;
    conf[row] = keep ? sh : m.val;
  }
}

// ---------------------------------------------------------------------------
// Launchers.  Each returns 0, or nonzero when a class or member count is out
// of range (nothing is launched and the outputs stay unwritten: the caller
// must turn that into an error).
// ---------------------------------------------------------------------------
template <class F>
static int proba_dispatch(int C, F&& launch) {
  return !dispatch_int<2, 3, 4, 5, 6, 7, 8>(C, launch);
}

extern "C" int launch_gnb_proba(const float* X, const double* theta,
                                const double* inv_var, const double* cconst,
                                float* proba, long long n, int C,
                                hipStream_t stream) {
  if (C < 2 || C > 8) return 1;
  if (n <= 0) return 0;
  dim3 grid(proba_grid(n));
  return proba_dispatch(C, [&](auto c) {
    hipLaunchKernelGGL((gnb_proba_kernel<decltype(c)::value>), grid,
                       dim3(PROBA_BLOCK), 0, stream, X, theta, inv_var, cconst,
                       proba, n);
  });
}

extern "C" int launch_linear_proba(const float* X, const float* W,
                                   const float* b, float* proba, long long n,
                                   int C, hipStream_t stream) {
  if (C < 2 || C > 8) return 1;
  if (n <= 0) return 0;
  dim3 grid(proba_grid(n));
  return proba_dispatch(C, [&](auto c) {
    hipLaunchKernelGGL((linear_proba_kernel<decltype(c)::value>), grid,
                       dim3(PROBA_BLOCK), 0, stream, X, W, b, proba, n);
  });
}

extern "C" int launch_knn_vote_proba(const int* idx, const unsigned char* y,
                                     float* proba, long long n, int k,
                                     long long nr, int C, hipStream_t stream) {
  if (C < 2 || C > 8 || k < 1) return 1;
  if (n <= 0) return 0;
  dim3 grid(proba_grid(n));
  return proba_dispatch(C, [&](auto c) {
    hipLaunchKernelGGL((knn_vote_proba_kernel<decltype(c)::value>), grid,
                       dim3(PROBA_BLOCK), 0, stream, idx, y, proba, n, k, nr);
  });
}

// `avg` may be null: then only labels and conf are written.
extern "C" int launch_ensemble_vote(const EnsembleArgs* args, float* avg,
                                    int* labels, float* conf, long long n,
                                    int C, hipStream_t stream) {
  if (C < 2 || C > ENS_MAX_C) return 1;
  if (args->M < 1 || args->M > ENS_MAX_M) return 1;
  for (int m = 0; m < args->M; ++m) {
    if (args->cm[m] < 2 || args->cm[m] > ENS_MAX_C) return 1;
    for (int j = 0; j < args->cm[m]; ++j)
      if (args->map[m * ENS_MAX_C + j] >= C) return 1;
  }
  if (n <= 0) return 0;
  dim3 grid(proba_grid(n));
  return proba_dispatch(C, [&](auto c) {
    constexpr int CV = decltype(c)::value;
    auto* kernel = avg ? ensemble_vote_kernel<CV, true> : ensemble_vote_kernel<CV, false>;
    hipLaunchKernelGGL(kernel, grid, dim3(PROBA_BLOCK), 0, stream, *args, avg,
                       labels, conf, n);
  });
}

// `n_live` may be null: then all n rows are live.  `state` and `held` have
// at least n rows; `a` is in (0, 1] and `margin` finite and >= 0.
extern "C" int launch_proba_smooth(const float* proba, float* state, int* held,
                                   const int* n_live, float a, float margin,
                                   int* labels, float* conf, long long n, int C,
                                   hipStream_t stream) {
  if (C < 2 || C > 8) return 1;
  if (!(a > 0.f && a <= 1.f) || !(margin >= 0.f) || margin == INFINITY) return 1;
  if (n <= 0) return 0;
  const float b = 1.0f - a;
  dim3 grid(proba_grid(n));
  return proba_dispatch(C, [&](auto c) {
    hipLaunchKernelGGL((proba_smooth_kernel<decltype(c)::value>), grid,
                       dim3(PROBA_BLOCK), 0, stream, proba, state, held, n_live,
                       a, b, margin, labels, conf, n);
  });
}
