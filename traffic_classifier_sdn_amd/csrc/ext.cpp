// PyTorch (ROCm) bindings for the CDNA4 kernels.  This TU is host-only;
// every kernel lives in the .hip TUs and is reached through the extern "C"
// launchers of launchers.h so the torch headers never touch device code.
//
// Every binding follows one path.  It checks its arguments with the
// functions below: the kernels index by their counts alone, so every extent
// they index by is checked here.  It makes the device of its first tensor
// current, so that the stream and the outputs belong to the tensors' device.
// It launches, turns a launcher's nonzero return into an error (an error,
// never an unwritten output), and ends with the launch check.  None of this
// synchronises, so every binding captures into a graph.

#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include <ATen/cuda/CUDAContext.h>
#include <c10/cuda/CUDAException.h>
#include <c10/cuda/CUDAGuard.h>

#include "launchers.h"

namespace {

using c10::cuda::CUDAGuard;
using torch::Tensor;
using OptTensor = c10::optional<torch::Tensor>;

constexpr auto kF32 = torch::kFloat32;
constexpr auto kF64 = torch::kFloat64;
constexpr auto kI32 = torch::kInt32;
constexpr auto kI64 = torch::kInt64;
constexpr auto kU8 = torch::kUInt8;

hipStream_t cur_stream() {
  return at::cuda::getCurrentCUDAStream().stream();
}

// An input: on a GPU, contiguous, of the given dtype.
void check_in(const Tensor& t, const char* name, c10::ScalarType type) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == type, name, " has wrong dtype: ",
              t.scalar_type(), ", not ", type);
}

// An input matrix of 12-feature rows; returns its row count.
int64_t rows12(const Tensor& t, const char* name, c10::ScalarType type) {
  check_in(t, name, type);
  TORCH_CHECK(t.dim() == 2 && t.size(1) == 12, name, " must be (n,12)");
  return t.size(0);
}

// A per-row vector or work buffer: an input on the device of the first
// tensor that holds the `need` elements a kernel indexes.
void check_buf(const Tensor& t, const char* name, c10::ScalarType type,
               int64_t need, const Tensor& first) {
  check_in(t, name, type);
  TORCH_CHECK(t.device() == first.device(), name,
              " must be on the device of the first tensor, ", first.device());
  TORCH_CHECK(t.numel() >= need, name, " needs at least ", need,
              " elements, has ", t.numel());
}

// An optional input: its data pointer, or nullptr for None.
template <class T>
const T* opt_ptr(const OptTensor& t, const char* name, c10::ScalarType type,
                 int64_t numel, const Tensor& first) {
  if (!t.has_value()) return nullptr;
  check_in(*t, name, type);
  TORCH_CHECK(t->numel() == numel && t->device() == first.device(), name,
              " must have ", numel, " element(s) on the device of the first tensor");
  return t->data_ptr<T>();
}

// A class count or k inside the range that `op` has kernels for.
void check_range(int64_t v, int64_t lo, int64_t hi, const char* op,
                 const char* what) {
  TORCH_CHECK(v >= lo && v <= hi, op, " supports ", lo, "..", hi, " ", what,
              ", got ", v);
}

// A count whose dynamic LDS, by the launcher's own size function, fits a
// launch.  A count above the byte limit cannot fit, so `bytes` never sees an
// int that overflows its arithmetic.
void check_lds(int64_t count, size_t (*bytes)(int), const char* op,
               const char* what) {
  TORCH_CHECK(count >= 1 && count <= MAX_DYNAMIC_LDS_BYTES &&
                  bytes((int)count) <= MAX_DYNAMIC_LDS_BYTES,
              op, ": ", count, " ", what, " do not fit the ",
              MAX_DYNAMIC_LDS_BYTES, " bytes of LDS of a launch");
}

// Every tensor of a call is on the device of the first (checked inputs all),
// which the returned guard makes current until the binding returns.
template <class... Ts>
CUDAGuard same_device(const char* op, const Tensor& first, const Ts&... rest) {
  TORCH_CHECK(((rest.device() == first.device()) && ...), op,
              ": every tensor must be on the device of the first, ",
              first.device());
  return CUDAGuard(first.device());
}

unsigned long long* u64(const Tensor& t) {  // packed u64 keys in int64 storage
  return reinterpret_cast<unsigned long long*>(t.data_ptr<int64_t>());
}
const unsigned* u32(const Tensor& t) {  // packed uint2 nodes in int32 storage
  return reinterpret_cast<const unsigned*>(t.data_ptr<int>());
}

}  // namespace

static Tensor gnb_predict(Tensor X, Tensor theta, Tensor inv_var, Tensor cconst) {
  const int64_t n = rows12(X, "X", kF32);
  const int64_t C = rows12(theta, "theta", kF32);
  check_in(inv_var, "inv_var", kF32);
  check_in(cconst, "cconst", kF32);
  TORCH_CHECK(inv_var.numel() == C * 12, "inv_var must be (C,12)");
  TORCH_CHECK(cconst.numel() == C, "cconst must be (C)");
  check_lds(C, gnb_predict_lds_bytes, "gnb_predict", "classes");
  const CUDAGuard guard = same_device("gnb_predict", X, theta, inv_var, cconst);
  auto out = torch::empty({n}, X.options().dtype(kI32));
  launch_gnb_predict(X.data_ptr<float>(), theta.data_ptr<float>(),
                     inv_var.data_ptr<float>(), cconst.data_ptr<float>(),
                     out.data_ptr<int>(), n, (int)C, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return out;
}

static Tensor linear_argmax(Tensor X, Tensor W, Tensor b) {
  const int64_t n = rows12(X, "X", kF32);
  const int64_t C = rows12(W, "W", kF32);
  check_in(b, "b", kF32);
  TORCH_CHECK(b.numel() == C, "b must be (C)");
  check_lds(C, linear_argmax_lds_bytes, "linear_argmax", "classes");
  const CUDAGuard guard = same_device("linear_argmax", X, W, b);
  auto out = torch::empty({n}, X.options().dtype(kI32));
  launch_linear_argmax(X.data_ptr<float>(), W.data_ptr<float>(),
                       b.data_ptr<float>(), out.data_ptr<int>(), n, (int)C,
                       cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return out;
}

static std::vector<Tensor> kmeans_assign(Tensor X, Tensor centers,
                                         bool want_update) {
  const int64_t n = rows12(X, "X", kF32);
  const int64_t K = rows12(centers, "centers", kF32);
  check_lds(K, kmeans_assign_lds_bytes, "kmeans_assign", "clusters");
  const CUDAGuard guard = same_device("kmeans_assign", X, centers);
  auto labels = torch::empty({n}, X.options().dtype(kI32));
  auto counts = torch::zeros({K}, X.options().dtype(kF64));
  auto sums = torch::zeros({K, 12}, X.options().dtype(kF64));
  auto inertia = torch::zeros({1}, X.options().dtype(kF64));
  launch_kmeans_assign(X.data_ptr<float>(), centers.data_ptr<float>(),
                       labels.data_ptr<int>(), counts.data_ptr<double>(),
                       sums.data_ptr<double>(), inertia.data_ptr<double>(), n,
                       (int)K, want_update ? 1 : 0, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {labels, counts, sums, inertia};
}

// What both forest bindings ask of the packed forest (ops/gpu.py rf_pack):
// `nodes` is packed uint2 as 2 x int32.  The node words themselves (child
// links, leaf rows) are rf_pack's to get right: checking them would need a
// pass over the table per call.  Returns the tree count.
static int64_t check_forest(const Tensor& nodes, const Tensor& roots,
                            const Tensor& leaf_proba, int64_t n_leaves,
                            int64_t C) {
  check_in(nodes, "nodes", kI32);
  check_in(roots, "roots", kI32);
  check_in(leaf_proba, "leaf_proba", kF32);
  TORCH_CHECK(nodes.dim() == 2 && nodes.size(1) == 2,
              "nodes must be (n_nodes,2) int32");
  TORCH_CHECK(roots.dim() == 1, "roots must be (n_trees)");
  TORCH_CHECK(n_leaves >= 0 && leaf_proba.numel() >= n_leaves * C,
              "leaf_proba must hold n_leaves rows of C");
  return roots.size(0);
}

static Tensor rf_predict(Tensor X, Tensor nodes, Tensor snodes, Tensor roots,
                         Tensor leaf_proba, int64_t n_leaves, int64_t C) {
  const int64_t n = rows12(X, "X", kF32);
  check_range(C, 2, 16, "rf_predict", "classes");
  const int64_t T = check_forest(nodes, roots, leaf_proba, n_leaves, C);
  check_in(snodes, "snodes", kI32);  // streaming kernel's table (ops/gpu.py)
  TORCH_CHECK(snodes.dim() == 2 && snodes.size(1) == 2 &&
                  snodes.size(0) == nodes.size(0) + 2,
              "snodes must be (n_nodes+2,2) int32");
  const CUDAGuard guard =
      same_device("rf_predict", X, nodes, snodes, roots, leaf_proba);
  auto out = torch::empty({n}, X.options().dtype(kI32));
  if (n == 0) return out;  // the wave-per-row grid would have no block
  const int rc = launch_rf_predict(
      X.data_ptr<float>(), u32(nodes), u32(snodes), roots.data_ptr<int>(),
      leaf_proba.data_ptr<float>(), out.data_ptr<int>(), n, (int)nodes.size(0),
      (int)n_leaves, (int)T, (int)C, cur_stream());
  TORCH_CHECK(rc == 0, "rf_predict: no kernel for ", C, " classes");
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return out;
}

// Class scores of the forest (rf_proba_kernels.hip): every tree counts.
// Returns (proba [n,C] f32 or an empty tensor, labels [n] i32, conf [n] f32).
static std::vector<Tensor> rf_predict_scores(Tensor X, Tensor nodes,
                                             Tensor roots, Tensor leaf_proba,
                                             int64_t n_leaves, int64_t C,
                                             bool want_proba) {
  const int64_t n = rows12(X, "X", kF32);
  check_range(C, 2, 8, "rf_predict_scores", "classes");
  const int64_t T = check_forest(nodes, roots, leaf_proba, n_leaves, C);
  TORCH_CHECK(T >= 1, "forest has no trees");
  const CUDAGuard guard =
      same_device("rf_predict_scores", X, nodes, roots, leaf_proba);
  auto proba = torch::empty({want_proba ? n : 0, C}, X.options());
  auto labels = torch::empty({n}, X.options().dtype(kI32));
  auto conf = torch::empty({n}, X.options());
  const int rc = launch_rf_scores(
      X.data_ptr<float>(), u32(nodes), roots.data_ptr<int>(),
      leaf_proba.data_ptr<float>(),
      want_proba ? proba.data_ptr<float>() : nullptr, labels.data_ptr<int>(),
      conf.data_ptr<float>(), n, (int)T, (int)C, cur_stream());
  TORCH_CHECK(rc == 0, "rf_predict_scores: no kernel for ", C, " classes");
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {proba, labels, conf};
}

// Isolation forest novelty score (iforest_kernels.hip) over the packed tables
// of ops/cpu.py iforest_pack, whose node words are iforest_pack's to get
// right.  Returns (score [n] f32, flags [n] u8, labels_out [n] i32 or an
// empty tensor, psum [n] f64 or an empty tensor).  `labels` is an int32 [n]
// tensor or None; `depth_cut` may be -inf (nothing is flagged).
static std::vector<Tensor> iforest_score(Tensor X, Tensor nodes, Tensor roots,
                                         OptTensor labels, double inv_denom,
                                         double depth_cut, bool want_sum) {
  const int64_t n = rows12(X, "X", kF32);
  check_in(nodes, "nodes", kI32);
  check_in(roots, "roots", kI32);
  TORCH_CHECK(nodes.dim() == 2 && nodes.size(1) == 2 && nodes.size(0) >= 1,
              "nodes must be (n_nodes,2) int32");
  TORCH_CHECK(roots.dim() == 1, "roots must be (n_trees)");
  const int64_t T = roots.size(0);
  check_range(T, 1, 4096, "iforest_score", "trees");
  TORCH_CHECK(std::isfinite(inv_denom) && inv_denom > 0.0,
              "inv_denom must be finite and positive");
  TORCH_CHECK(!std::isnan(depth_cut), "depth_cut must not be NaN");
  if (labels.has_value())
    TORCH_CHECK(labels->dim() == 1, "labels must be (n)");
  const int* lab = opt_ptr<int>(labels, "labels", kI32, n, X);
  const CUDAGuard guard = same_device("iforest_score", X, nodes, roots);
  auto score = torch::empty({n}, X.options());
  auto flags = torch::empty({n}, X.options().dtype(kU8));
  auto labels_out = torch::empty({lab ? n : 0}, X.options().dtype(kI32));
  auto psum = torch::empty({want_sum ? n : 0}, X.options().dtype(kF64));
  const int rc = launch_iforest_score(
      X.data_ptr<float>(), u32(nodes), roots.data_ptr<int>(), lab,
      score.data_ptr<float>(), want_sum ? psum.data_ptr<double>() : nullptr,
      lab ? labels_out.data_ptr<int>() : nullptr,
      flags.data_ptr<unsigned char>(), inv_denom, depth_cut, n, (int)T,
      cur_stream());
  TORCH_CHECK(rc == 0, "iforest_score: no kernel for ", T, " trees");
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {score, flags, labels_out, psum};
}

// Per-feature contributions to the probability of each row's class
// (rf_explain_kernels.hip) over the classifier forest's packed `nodes` and
// `roots` and the `delta` table of ops/cpu.py rf_explain_flatten, one row of
// C steps per node.  Returns (contrib [n,12] f32 or an empty tensor, why [n]
// i32, why_value [n] f32, sums [n,12] i64 or an empty tensor).  The range
// refusals are the launcher's: its nonzero return is the error.
static std::vector<Tensor> rf_explain(Tensor X, Tensor nodes, Tensor roots,
                                      Tensor delta, Tensor labels,
                                      bool want_matrix, bool want_sums) {
  const int64_t n = rows12(X, "X", kF32);
  check_in(nodes, "nodes", kI32);
  check_in(roots, "roots", kI32);
  check_in(delta, "delta", kI32);
  check_in(labels, "labels", kI32);
  TORCH_CHECK(nodes.dim() == 2 && nodes.size(1) == 2 && nodes.size(0) >= 1,
              "nodes must be (n_nodes,2) int32");
  TORCH_CHECK(roots.dim() == 1, "roots must be (n_trees)");
  TORCH_CHECK(delta.dim() == 2 && delta.size(0) == nodes.size(0),
              "delta must be (n_nodes,C): one row per node of nodes");
  TORCH_CHECK(labels.dim() == 1 && labels.size(0) == n, "labels must be (n)");
  const int64_t T = roots.size(0);
  const int64_t C = delta.size(1);
  TORCH_CHECK(T <= INT32_MAX && C <= INT32_MAX, "rf_explain: counts past 32 bits");
  const CUDAGuard guard =
      same_device("rf_explain", X, nodes, roots, delta, labels);
  auto contrib = torch::empty({want_matrix ? n : 0, 12}, X.options());
  auto why = torch::empty({n}, X.options().dtype(kI32));
  auto why_value = torch::empty({n}, X.options());
  auto sums = torch::empty({want_sums ? n : 0, 12}, X.options().dtype(kI64));
  const int rc = launch_rf_explain(
      X.data_ptr<float>(), u32(nodes), roots.data_ptr<int>(),
      delta.data_ptr<int>(), labels.data_ptr<int>(),
      want_matrix ? contrib.data_ptr<float>() : nullptr, why.data_ptr<int>(),
      why_value.data_ptr<float>(),
      want_sums ? reinterpret_cast<long long*>(sums.data_ptr<int64_t>()) : nullptr,
      n, (int)T, (int)C, cur_stream());
  TORCH_CHECK(rc == 0, "rf_explain: no kernel for ", C, " classes and ", T,
              " trees (2..8 classes, 1..4096 trees)");
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {contrib, why, why_value, sums};
}

// Class probabilities and the soft vote (ensemble_kernels.hip).
static Tensor gnb_proba(Tensor X, Tensor theta, Tensor inv_var, Tensor cconst) {
  const int64_t n = rows12(X, "X", kF32);
  check_in(theta, "theta", kF64);
  check_in(inv_var, "inv_var", kF64);
  check_in(cconst, "cconst", kF64);
  const int64_t C = cconst.numel();
  check_range(C, 2, 8, "gnb_proba", "classes");
  TORCH_CHECK(theta.numel() == C * 12 && inv_var.numel() == C * 12,
              "theta and inv_var must be (C,12)");
  const CUDAGuard guard = same_device("gnb_proba", X, theta, inv_var, cconst);
  auto proba = torch::empty({n, C}, X.options());
  const int rc = launch_gnb_proba(
      X.data_ptr<float>(), theta.data_ptr<double>(), inv_var.data_ptr<double>(),
      cconst.data_ptr<double>(), proba.data_ptr<float>(), n, (int)C,
      cur_stream());
  TORCH_CHECK(rc == 0, "gnb_proba: no kernel for ", C, " classes");
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return proba;
}

static Tensor linear_proba(Tensor X, Tensor W, Tensor b) {
  const int64_t n = rows12(X, "X", kF32);
  check_in(W, "W", kF32);
  check_in(b, "b", kF32);
  const int64_t C = b.numel();
  check_range(C, 2, 8, "linear_proba", "classes");
  TORCH_CHECK(W.numel() == C * 12, "W must be (C,12)");
  const CUDAGuard guard = same_device("linear_proba", X, W, b);
  auto proba = torch::empty({n, C}, X.options());
  const int rc = launch_linear_proba(X.data_ptr<float>(), W.data_ptr<float>(),
                                     b.data_ptr<float>(),
                                     proba.data_ptr<float>(), n, (int)C,
                                     cur_stream());
  TORCH_CHECK(rc == 0, "linear_proba: no kernel for ", C, " classes");
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return proba;
}

// The kernel skips an index outside [0, y.numel()), so idx needs no check.
static Tensor knn_vote_proba(Tensor idx, Tensor y, int64_t C) {
  check_in(idx, "idx", kI32);
  check_in(y, "y", kU8);
  TORCH_CHECK(idx.dim() == 2 && idx.size(1) >= 1, "idx must be (n,k), k >= 1");
  check_range(C, 2, 8, "knn_vote_proba", "classes");
  const int64_t n = idx.size(0);
  const CUDAGuard guard = same_device("knn_vote_proba", idx, y);
  auto proba = torch::empty({n, C}, idx.options().dtype(kF32));
  const int rc = launch_knn_vote_proba(
      idx.data_ptr<int>(), y.data_ptr<unsigned char>(), proba.data_ptr<float>(),
      n, (int)idx.size(1), (long long)y.numel(), (int)C, cur_stream());
  TORCH_CHECK(rc == 0, "knn_vote_proba: no kernel for ", C, " classes");
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return proba;
}

// Returns (avg [n,C] f32 or an empty tensor, labels [n] i32, conf [n] f32).
// `weights` are the normalised weights (the caller divides by their f64 sum).
static std::vector<Tensor> ensemble_vote(
    std::vector<Tensor> probas, std::vector<std::vector<int64_t>> colmaps,
    std::vector<double> weights, int64_t C, bool want_proba) {
  const int64_t M = (int64_t)probas.size();
  check_range(M, 1, ENS_MAX_M, "ensemble_vote", "members");
  TORCH_CHECK((int64_t)colmaps.size() == M && (int64_t)weights.size() == M,
              "ensemble_vote: one column map and one weight per member");
  check_range(C, 2, ENS_MAX_C, "ensemble_vote", "classes");
  EnsembleArgs args;
  memset(&args, 0, sizeof(args));
  args.M = (int)M;
  const int64_t n = probas[0].dim() ? probas[0].size(0) : 0;
  for (int64_t m = 0; m < M; ++m) {
    const Tensor& p = probas[m];
    check_buf(p, "member probabilities", kF32, 0, probas[0]);
    TORCH_CHECK(p.dim() == 2, "member probabilities must be (n,C_m)");
    TORCH_CHECK(p.size(0) == n, "members differ in their row count");
    const int64_t cm = p.size(1);
    TORCH_CHECK(cm >= 2 && cm <= ENS_MAX_C, "a member has ", cm, " classes, not 2..8");
    TORCH_CHECK((int64_t)colmaps[m].size() == cm,
                "a column map must have one entry per member class");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(p.data_ptr<float>()) % 16 == 0,
                "member probabilities must be 16-byte aligned");
    for (int64_t j = 0; j < cm; ++j) {
      TORCH_CHECK(colmaps[m][j] >= 0 && colmaps[m][j] < C,
                  "column map entry ", colmaps[m][j], " outside the ", C, " classes");
      args.map[m * ENS_MAX_C + j] = (unsigned char)colmaps[m][j];
    }
    const float w = (float)weights[m];
    TORCH_CHECK(std::isfinite(w) && w > 0.f, "weights must be finite and positive");
    args.p[m] = p.data_ptr<float>();
    args.w[m] = w;
    args.cm[m] = (unsigned char)cm;
  }
  const CUDAGuard guard = same_device("ensemble_vote", probas[0]);
  auto opts = probas[0].options();
  auto avg = torch::empty({want_proba ? n : 0, C}, opts);
  auto labels = torch::empty({n}, opts.dtype(kI32));
  auto conf = torch::empty({n}, opts);
  const int rc = launch_ensemble_vote(
      &args, want_proba ? avg.data_ptr<float>() : nullptr,
      labels.data_ptr<int>(), conf.data_ptr<float>(), n, (int)C, cur_stream());
  TORCH_CHECK(rc == 0, "ensemble_vote: arguments out of the kernel's range");
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {avg, labels, conf};
}

// Returns (labels [n] i32, conf [n] f32); `state` [cap,C] and `held` [cap]
// are updated in place, rows < n only.  `n_live` is an int32 [1] tensor or
// None (all n rows are live).
static std::vector<Tensor> proba_smooth(Tensor proba, Tensor state, Tensor held,
                                        OptTensor n_live, double alpha,
                                        double margin) {
  check_in(proba, "proba", kF32);
  check_in(state, "state", kF32);
  check_in(held, "held", kI32);
  TORCH_CHECK(proba.dim() == 2 && state.dim() == 2 && held.dim() == 1,
              "proba_smooth takes proba (n,C), state (cap,C) and held (cap)");
  const int64_t n = proba.size(0);
  const int64_t C = proba.size(1);
  check_range(C, 2, 8, "proba_smooth", "classes");
  TORCH_CHECK(state.size(1) == C, "state has ", state.size(1), " columns for ", C, " classes");
  TORCH_CHECK(state.size(0) >= n && held.size(0) >= n,
              "state and held need at least ", n, " rows");
  const char* p0 = static_cast<const char*>(proba.data_ptr());
  const char* s0 = static_cast<const char*>(state.data_ptr());
  TORCH_CHECK(p0 + proba.nbytes() <= s0 || s0 + state.nbytes() <= p0,
              "proba must not alias state");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(p0) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(s0) % 16 == 0,
              "proba and state must be 16-byte aligned");
  const int* live = opt_ptr<int>(n_live, "n_live", kI32, 1, proba);
  const float a = (float)alpha, m = (float)margin;
  TORCH_CHECK(a > 0.f && a <= 1.f, "alpha must be in (0, 1]");
  TORCH_CHECK(std::isfinite(m) && m >= 0.f, "margin must be finite and >= 0");
  const CUDAGuard guard = same_device("proba_smooth", proba, state, held);
  auto labels = torch::empty({n}, proba.options().dtype(kI32));
  auto conf = torch::empty({n}, proba.options());
  const int rc = launch_proba_smooth(
      proba.data_ptr<float>(), state.data_ptr<float>(), held.data_ptr<int>(),
      live, a, m, labels.data_ptr<int>(), conf.data_ptr<float>(), n, (int)C,
      cur_stream());
  TORCH_CHECK(rc == 0, "proba_smooth: arguments out of the kernel's range");
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {labels, conf};
}

// Returns totals [C + 1, 13] f64: per group (class, or C for "unknown") the
// row count and the f64 sums of the 12 features.  `conf` is an f32 [n] tensor
// or None, `n_live` an int32 [1] tensor or None (all n rows are live).
static Tensor class_traffic(Tensor X, Tensor labels, int64_t n_classes,
                            OptTensor conf, double min_conf, OptTensor n_live) {
  const int64_t n = rows12(X, "X", kF32);
  check_in(labels, "labels", kI32);
  TORCH_CHECK(labels.dim() == 1 && labels.size(0) == n, "labels must be (n)");
  TORCH_CHECK(n_classes >= 2 && n_classes <= 8,
              "no kernel for class_traffic with ", n_classes, " classes (2..8)");
  const float* cf = opt_ptr<float>(conf, "conf", kF32, n, X);
  const int* live = opt_ptr<int>(n_live, "n_live", kI32, 1, X);
  const float mc = (float)min_conf;
  TORCH_CHECK(std::isfinite(mc), "min_conf must be finite");
  const int C = (int)n_classes;
  const int nb = class_traffic_blocks(n);
  const CUDAGuard guard = same_device("class_traffic", X, labels);
  const auto f64 = X.options().dtype(kF64);
  auto partial = torch::empty({(int64_t)nb * (C + 1) * 13}, f64);
  auto totals = torch::empty({C + 1, 13}, f64);
  const int rc = launch_class_traffic(
      X.data_ptr<float>(), labels.data_ptr<int>(), cf, live, mc,
      partial.data_ptr<double>(), totals.data_ptr<double>(), n, C, nb,
      cur_stream());
  TORCH_CHECK(rc == 0, "no kernel for class_traffic with ", C, " classes");
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return totals;
}

// Returns (rows int32 [C + 1, k], keys f32 [C + 1, k]): per group the k live
// rows with the largest key, the f32 sum of the columns in `col_mask`
// (top_flows_kernels.hip); -1 and 0.0 where a group has fewer.  `conf` and
// `n_live` as in class_traffic.
static std::vector<Tensor> class_top_flows(Tensor X, Tensor labels,
                                           int64_t n_classes, int64_t k,
                                           int64_t col_mask, OptTensor conf,
                                           double min_conf, OptTensor n_live) {
  const int64_t n = rows12(X, "X", kF32);
  check_in(labels, "labels", kI32);
  TORCH_CHECK(labels.dim() == 1 && labels.size(0) == n, "labels must be (n)");
  TORCH_CHECK(n <= INT32_MAX, "class_top_flows indexes rows with 32 bits, got ", n);
  TORCH_CHECK(n_classes >= 2 && n_classes <= 8,
              "no kernel for class_top_flows with ", n_classes, " classes (2..8)");
  TORCH_CHECK(k >= 1 && k <= 64,
              "no kernel for class_top_flows with k = ", k, " (1..64)");
  check_range(col_mask, 1, 0xfff, "class_top_flows", "as the column mask");
  const float* cf = opt_ptr<float>(conf, "conf", kF32, n, X);
  const int* live = opt_ptr<int>(n_live, "n_live", kI32, 1, X);
  const float mc = (float)min_conf;
  TORCH_CHECK(std::isfinite(mc), "min_conf must be finite");
  const int C = (int)n_classes;
  const int nb = class_top_flows_blocks(n);
  const CUDAGuard guard = same_device("class_top_flows", X, labels);
  auto partial = torch::empty({(int64_t)nb * (C + 1) * k}, X.options().dtype(kI64));
  auto rows = torch::empty({C + 1, k}, X.options().dtype(kI32));
  auto keys = torch::empty({C + 1, k}, X.options());
  const int rc = launch_class_top_flows(
      X.data_ptr<float>(), labels.data_ptr<int>(), cf, live, mc,
      (unsigned)col_mask, u64(partial), rows.data_ptr<int>(),
      keys.data_ptr<float>(), n, C, (int)k, nb, cur_stream());
  TORCH_CHECK(rc == 0, "no kernel for class_top_flows with ", C, " classes and k = ", k);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {rows, keys};
}

// SVC labels (Out = int, [n]) and decision values (Out = double, [n,npair])
// of svc_kernels.hip take the same arguments through the same kernel bodies,
// which index SV, dual, svclass and intercept by nsv and C alone: one check
// of every extent for both.
template <class Out, class Launcher>
static Tensor svc_run(const char* op, Launcher launch, const Tensor& X,
                      const Tensor& SV, const Tensor& dual,
                      const Tensor& svclass, const Tensor& intercept,
                      double gamma) {
  const int64_t n = rows12(X, "X", kF32);
  const int64_t nsv = rows12(SV, "SV", kF32);
  check_in(dual, "dual", kF32);
  check_in(svclass, "svclass", kU8);
  check_in(intercept, "intercept", kF32);
  TORCH_CHECK(dual.dim() == 2, "dual must be (C-1,nsv)");
  const int64_t C = dual.size(0) + 1;
  check_range(C, 2, 6, op, "classes");
  TORCH_CHECK(nsv <= INT32_MAX, "too many support vectors");
  const int64_t npair = C * (C - 1) / 2;
  TORCH_CHECK(dual.size(1) == nsv, "dual must be (C-1,nsv)");
  TORCH_CHECK(svclass.numel() == nsv, "svclass must have one entry per SV");
  TORCH_CHECK(intercept.numel() == npair, "intercept must have C(C-1)/2 entries");
  const CUDAGuard guard = same_device(op, X, SV, dual, svclass, intercept);
  const auto opts = X.options().dtype(c10::CppTypeToScalarType<Out>::value);
  Tensor out = std::is_same_v<Out, int> ? torch::empty({n}, opts)
                                        : torch::empty({n, npair}, opts);
  const int rc = launch(X.data_ptr<float>(), SV.data_ptr<float>(),
                        dual.data_ptr<float>(), svclass.data_ptr<unsigned char>(),
                        intercept.data_ptr<float>(), out.data_ptr<Out>(), n,
                        (int)nsv, (int)C, (float)gamma, cur_stream());
  TORCH_CHECK(rc == 0, op, ": no kernel for ", C, " classes");
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return out;
}

static Tensor svc_predict(Tensor X, Tensor SV, Tensor dual, Tensor svclass,
                          Tensor intercept, double gamma) {
  return svc_run<int>("svc_predict", launch_svc_predict, X, SV, dual, svclass,
                      intercept, gamma);
}

static Tensor svc_decision(Tensor X, Tensor SV, Tensor dual, Tensor svclass,
                           Tensor intercept, double gamma) {
  return svc_run<double>("svc_decision", launch_svc_decision, X, SV, dual,
                         svclass, intercept, gamma);
}

// Returns (proba [n,C] f32, idx [n] i32, conf [n] f32).
static std::vector<Tensor> svc_couple(Tensor dec, Tensor probA, Tensor probB,
                                      int64_t C) {
  check_in(dec, "dec", kF64);
  check_in(probA, "probA", kF64);
  check_in(probB, "probB", kF64);
  check_range(C, 2, 6, "svc_couple", "classes");
  const int64_t npair = C * (C - 1) / 2;
  TORCH_CHECK(dec.dim() == 2 && dec.size(1) == npair,
              "dec must be (n,C(C-1)/2)");
  TORCH_CHECK(probA.numel() == npair && probB.numel() == npair,
              "probA and probB must have C(C-1)/2 entries");
  const int64_t n = dec.size(0);
  const CUDAGuard guard = same_device("svc_couple", dec, probA, probB);
  auto f32 = dec.options().dtype(kF32);
  auto proba = torch::empty({n, C}, f32);
  auto idx = torch::empty({n}, dec.options().dtype(kI32));
  auto conf = torch::empty({n}, f32);
  const int rc = launch_svc_couple(
      dec.data_ptr<double>(), probA.data_ptr<double>(),
      probB.data_ptr<double>(), proba.data_ptr<float>(), idx.data_ptr<int>(),
      conf.data_ptr<float>(), n, (int)C, cur_stream());
  TORCH_CHECK(rc == 0, "svc_couple: no kernel for ", C, " classes");
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {proba, idx, conf};
}

// What both top-k bindings return: (dist [nq,k], idx [nq,k]) and, with the
// reference rows' labels `ry` [nr], the fused vote lab [nq].
struct KnnOut {
  Tensor dist, idx, lab;
  const unsigned char* ry;

  KnnOut(const Tensor& Q, int64_t nq, int64_t nr, int64_t k, const OptTensor& ry_)
      : dist(torch::empty({nq, k}, Q.options())),
        idx(torch::empty({nq, k}, Q.options().dtype(kI32))),
        ry(opt_ptr<unsigned char>(ry_, "ry", kU8, nr, Q)) {
    if (ry) lab = torch::empty({nq}, Q.options().dtype(kI32));
  }
  int* lab_ptr() const { return ry ? lab.data_ptr<int>() : nullptr; }
  std::vector<Tensor> result() const {
    if (ry) return {dist, idx, lab};
    return {dist, idx};
  }
};

static std::vector<Tensor> knn_topk(Tensor Q, Tensor R, OptTensor ry, int64_t k,
                                    int64_t C, int64_t idx_base) {
  const int64_t nq = rows12(Q, "Q", kF32);
  const int64_t nr = rows12(R, "R", kF32);
  check_range(k, 1, 32, "knn_topk", "neighbours");
  const CUDAGuard guard = same_device("knn_topk", Q, R);
  const KnnOut out(Q, nq, nr, k, ry);
  const int rc = launch_knn_topk(
      Q.data_ptr<float>(), R.data_ptr<float>(), out.ry,
      out.dist.data_ptr<float>(), out.idx.data_ptr<int>(), out.lab_ptr(), nq,
      nr, (int)k, (int)C, idx_base, cur_stream());
  TORCH_CHECK(rc == 0, "knn_topk: no kernel for k = ", k);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return out.result();
}

// MFMA distance-GEMM path: R sharded across gridDim.y, per-shard partial
// top-k lists merged by a second kernel (knn_mfma.hip), whose vote counts
// the classes in 16 registers.
static std::vector<Tensor> knn_topk_mfma(Tensor Q, Tensor R, Tensor cmean,
                                         OptTensor ry, int64_t k, int64_t C,
                                         int64_t idx_base, int64_t n_shards,
                                         int64_t approx) {
  const int64_t nq = rows12(Q, "Q", kF32);
  const int64_t nr = rows12(R, "R", kF32);
  check_in(cmean, "cmean", kF32);
  TORCH_CHECK(nr >= 1, "R needs at least one row");
  check_range(k, 1, 8, "knn_topk_mfma", "neighbours");
  check_range(C, 0, 16, "knn_topk_mfma", "classes");
  TORCH_CHECK(cmean.numel() == 12, "cmean must be (12,)");
  const int S = (int)std::max<int64_t>(1, std::min<int64_t>(n_shards, (nr + 127) / 128));
  const CUDAGuard guard = same_device("knn_topk_mfma", Q, R, cmean);
  const KnnOut out(Q, nq, nr, k, ry);
  if (nq == 0) return out.result();  // the grid would have no block
  auto part_d = torch::empty({S, nq, k}, Q.options());
  auto part_i = torch::empty({S, nq, k}, Q.options().dtype(kI32));
  launch_knn_mfma(Q.data_ptr<float>(), R.data_ptr<float>(),
                  cmean.data_ptr<float>(), out.ry, part_d.data_ptr<float>(),
                  part_i.data_ptr<int>(), out.dist.data_ptr<float>(),
                  out.idx.data_ptr<int>(), out.lab_ptr(), nq, nr, S, (int)k,
                  (int)C, idx_base, (int)approx, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return out.result();
}

// The label VALUES of the fit kernels (y in [0,C), nid a node or < 0) index
// their accumulators; they are the caller's to get right: checking them would
// need a pass over the data per call.
static std::vector<Tensor> gnb_fit_stats(Tensor X, Tensor y, int64_t C) {
  const int64_t n = rows12(X, "X", kF64);
  check_buf(y, "y", kI64, n, X);
  check_lds(C, gnb_fit_stats_lds_bytes, "gnb_fit_stats", "classes");
  const CUDAGuard guard = same_device("gnb_fit_stats", X);
  auto count = torch::zeros({C}, X.options());
  auto sum = torch::zeros({C, 12}, X.options());
  auto sumsq = torch::zeros({C, 12}, X.options());
  launch_gnb_fit_stats(X.data_ptr<double>(),
                       reinterpret_cast<const long long*>(y.data_ptr<int64_t>()),
                       count.data_ptr<double>(), sum.data_ptr<double>(),
                       sumsq.data_ptr<double>(), n, (int)C, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {count, sum, sumsq};
}

static std::vector<Tensor> logistic_grad(Tensor X, Tensor y, Tensor W, Tensor b) {
  const int64_t n = rows12(X, "X", kF64);
  check_buf(y, "y", kI64, n, X);
  const int64_t C = rows12(W, "W", kF64);
  check_range(C, 2, 16, "logistic_grad", "classes");
  check_in(b, "b", kF64);
  TORCH_CHECK(b.numel() == C, "b must be (C)");
  const CUDAGuard guard = same_device("logistic_grad", X, W, b);
  auto grad = torch::zeros({C, 13}, X.options());
  auto loss = torch::zeros({1}, X.options());
  const int rc = launch_logistic_grad(
      X.data_ptr<double>(),
      reinterpret_cast<const long long*>(y.data_ptr<int64_t>()),
      W.data_ptr<double>(), b.data_ptr<double>(), grad.data_ptr<double>(),
      loss.data_ptr<double>(), n, (int)C, cur_stream());
  TORCH_CHECK(rc == 0, "logistic_grad: no kernel for ", C, " classes");
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {grad, loss};
}

static Tensor flow_features(Tensor cur, Tensor prev, Tensor times) {
  check_in(cur, "cur", kF64);
  check_in(prev, "prev", kF64);
  check_in(times, "times", kF64);
  TORCH_CHECK(cur.dim() == 2 && cur.size(1) == 4, "cur must be (n,4)");
  const int64_t n = cur.size(0);
  TORCH_CHECK(prev.dim() == 2 && prev.size(0) == n && prev.size(1) == 4,
              "prev must be (n,4)");
  TORCH_CHECK(times.dim() == 2 && times.size(0) == n && times.size(1) == 6,
              "times must be (n,6)");
  const CUDAGuard guard = same_device("flow_features", cur, prev, times);
  auto out = torch::empty({n, 12}, cur.options().dtype(kF32));
  launch_flow_features(cur.data_ptr<double>(), prev.data_ptr<double>(),
                       times.data_ptr<double>(), out.data_ptr<float>(), n,
                       cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return out;
}

// SMO working-pair kernels (fit_kernels.hip).  Every one of them works on the
// n rows of X, or of y where it takes no X: y, alpha, grad and krow hold a
// value per row, `sel` packed u64 keys in int64 storage, two for WSS-1 and
// three for WSS-2, `rows` the 24 floats of x_i and x_j, `sol` 4 doubles.  The
// row numbers inside `sel` come from a select kernel that ran over the same n
// rows, so they index nothing that the checks below have not covered.
static void smo_select(Tensor y, Tensor alpha, Tensor grad, double C, Tensor out) {
  check_in(y, "y", kF32);
  TORCH_CHECK(y.dim() == 1, "y must be (n)");
  const int64_t n = y.size(0);
  check_buf(alpha, "alpha", kF64, n, y);
  check_buf(grad, "grad", kF64, n, y);
  check_buf(out, "out", kI64, 2, y);
  const CUDAGuard guard = same_device("smo_select", y);
  launch_smo_select(y.data_ptr<float>(), alpha.data_ptr<double>(),
                    grad.data_ptr<double>(), C, n, u64(out), cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

// smo_solve (WSS-1, sel_len 2) and smo_solve2 (WSS-2, sel_len 3)
template <class Launcher>
static void smo_solve_run(Launcher launch, int64_t sel_len, const Tensor& X,
                          const Tensor& y, const Tensor& alpha,
                          const Tensor& grad, const Tensor& sel,
                          const Tensor& rows, const Tensor& sol, double C,
                          double tol, double gamma) {
  const int64_t n = rows12(X, "X", kF32);
  check_buf(y, "y", kF32, n, X);
  check_buf(alpha, "alpha", kF64, n, X);
  check_buf(grad, "grad", kF64, n, X);
  check_buf(sel, "sel", kI64, sel_len, X);
  check_buf(rows, "rows", kF32, 24, X);
  check_buf(sol, "sol", kF64, 4, X);
  const CUDAGuard guard = same_device("smo_solve", X);
  launch(X.data_ptr<float>(), y.data_ptr<float>(), alpha.data_ptr<double>(),
         grad.data_ptr<double>(), u64(sel), rows.data_ptr<float>(),
         sol.data_ptr<double>(), C, tol, (float)gamma, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

static void smo_solve(Tensor X, Tensor y, Tensor alpha, Tensor grad, Tensor sel,
                      Tensor rows, Tensor sol, double C, double tol,
                      double gamma) {
  smo_solve_run(launch_smo_solve, 2, X, y, alpha, grad, sel, rows, sol, C, tol, gamma);
}

static void smo_solve2(Tensor X, Tensor y, Tensor alpha, Tensor grad, Tensor sel,
                       Tensor rows, Tensor sol, double C, double tol,
                       double gamma) {
  smo_solve_run(launch_smo_solve2, 3, X, y, alpha, grad, sel, rows, sol, C, tol, gamma);
}

static void smo_update_dev(Tensor X, Tensor y, Tensor grad, Tensor rows,
                           Tensor sol, double gamma) {
  const int64_t n = rows12(X, "X", kF32);
  check_buf(y, "y", kF32, n, X);
  check_buf(grad, "grad", kF64, n, X);
  check_buf(rows, "rows", kF32, 24, X);
  check_buf(sol, "sol", kF64, 4, X);
  const CUDAGuard guard = same_device("smo_update_dev", X);
  launch_smo_update_dev(X.data_ptr<float>(), y.data_ptr<float>(),
                        grad.data_ptr<double>(), rows.data_ptr<float>(),
                        sol.data_ptr<double>(), (float)gamma, n, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

static void smo_update(Tensor X, Tensor y, Tensor grad, Tensor rows,
                       double yidai, double yjdaj, double gamma) {
  const int64_t n = rows12(X, "X", kF32);
  check_buf(y, "y", kF32, n, X);
  check_buf(grad, "grad", kF64, n, X);
  check_buf(rows, "rows", kF32, 24, X);
  const CUDAGuard guard = same_device("smo_update", X);
  launch_smo_update(X.data_ptr<float>(), y.data_ptr<float>(),
                    grad.data_ptr<double>(), rows.data_ptr<float>(), yidai,
                    yjdaj, (float)gamma, n, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

static void smo_row(Tensor X, Tensor sel, Tensor sol, Tensor krow, double gamma) {
  const int64_t n = rows12(X, "X", kF32);
  check_buf(sel, "sel", kI64, 1, X);
  check_buf(sol, "sol", kF64, 4, X);
  check_buf(krow, "krow", kF32, n, X);
  const CUDAGuard guard = same_device("smo_row", X);
  launch_smo_row(X.data_ptr<float>(), u64(sel), sol.data_ptr<double>(),
                 krow.data_ptr<float>(), (float)gamma, n, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

static void smo_select2(Tensor y, Tensor alpha, Tensor grad, Tensor krow,
                        Tensor sel, Tensor sol, double C) {
  check_in(y, "y", kF32);
  TORCH_CHECK(y.dim() == 1, "y must be (n)");
  const int64_t n = y.size(0);
  check_buf(alpha, "alpha", kF64, n, y);
  check_buf(grad, "grad", kF64, n, y);
  check_buf(krow, "krow", kF32, n, y);
  check_buf(sel, "sel", kI64, 3, y);
  check_buf(sol, "sol", kF64, 4, y);
  const CUDAGuard guard = same_device("smo_select2", y);
  launch_smo_select2(y.data_ptr<float>(), alpha.data_ptr<double>(),
                     grad.data_ptr<double>(), krow.data_ptr<float>(), u64(sel),
                     sol.data_ptr<double>(), C, n, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

static void smo_update_dev2(Tensor X, Tensor y, Tensor grad, Tensor rows,
                            Tensor sol, Tensor krow, double gamma) {
  const int64_t n = rows12(X, "X", kF32);
  check_buf(y, "y", kF32, n, X);
  check_buf(grad, "grad", kF64, n, X);
  check_buf(rows, "rows", kF32, 24, X);
  check_buf(sol, "sol", kF64, 4, X);
  check_buf(krow, "krow", kF32, n, X);
  const CUDAGuard guard = same_device("smo_update_dev2", X);
  launch_smo_update_dev2(X.data_ptr<float>(), y.data_ptr<float>(),
                         grad.data_ptr<double>(), rows.data_ptr<float>(),
                         sol.data_ptr<double>(), krow.data_ptr<float>(),
                         (float)gamma, n, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

// Random-forest fit (fit_kernels.hip): `hist` is u32 counts in int32 storage.
static void rf_hist(Tensor bins, Tensor y, Tensor nid, Tensor hist,
                    OptTensor fsel = c10::nullopt) {
  const int64_t n = rows12(bins, "bins", kU8);
  check_buf(y, "y", kU8, n, bins);
  check_buf(nid, "nid", kI32, n, bins);
  check_buf(hist, "hist", kI32, 0, bins);
  TORCH_CHECK(hist.dim() == 4 && hist.size(1) == 12 && hist.size(2) == 256 &&
                  hist.size(3) >= 1,
              "hist must be (nodes,12,256,C)");
  const unsigned char* fs =
      opt_ptr<unsigned char>(fsel, "fsel", kU8, hist.size(0) * 12, bins);
  const CUDAGuard guard = same_device("rf_hist", bins);
  launch_rf_hist(bins.data_ptr<unsigned char>(), y.data_ptr<unsigned char>(),
                 nid.data_ptr<int>(), fs,
                 reinterpret_cast<unsigned*>(hist.data_ptr<int>()), n,
                 (int)hist.size(3), cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

static std::vector<Tensor> rf_split(Tensor hist, Tensor fsel) {
  check_in(hist, "hist", kI32);
  TORCH_CHECK(hist.dim() == 4 && hist.size(1) == 12 && hist.size(2) == 256,
              "hist must be (L,12,256,C)");
  const int64_t L = hist.size(0), C = hist.size(3);
  check_range(C, 2, 16, "rf_split", "classes");
  check_buf(fsel, "fsel", kU8, L * 12, hist);
  const CUDAGuard guard = same_device("rf_split", hist);
  auto best = torch::full({L}, -1, hist.options().dtype(kI64));
  auto cnt = torch::zeros({L, C}, hist.options());
  if (L == 0) return {best, cnt};  // the grid would have no block
  const int rc = launch_rf_split(hist.data_ptr<int>(),
                                 fsel.data_ptr<unsigned char>(), u64(best),
                                 cnt.data_ptr<int>(), (int)L, (int)C,
                                 cur_stream());
  TORCH_CHECK(rc == 0, "rf_split: no kernel for ", C, " classes");
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {best, cnt};
}

// Fused level pass: compact mtry-plane histogram scatter + split search.
static std::vector<Tensor> rf_level_compact(Tensor bins, Tensor y, Tensor nid,
                                            Tensor frank, Tensor fidx,
                                            int64_t L, int64_t C) {
  const int64_t n = rows12(bins, "bins", kU8);
  check_buf(y, "y", kU8, n, bins);
  check_buf(nid, "nid", kI32, n, bins);
  check_range(L, 1, INT32_MAX, "rf_level_compact", "nodes");
  check_range(C, 2, 16, "rf_level_compact", "classes");
  check_buf(frank, "frank", kU8, L * 12, bins);
  check_buf(fidx, "fidx", kU8, L, bins);
  const int64_t mf = fidx.numel() / L;
  TORCH_CHECK(mf <= 12 && mf * L == fidx.numel(), "fidx must be (L,mf), mf in 1..12");
  const CUDAGuard guard = same_device("rf_level_compact", bins);
  auto hist = torch::zeros({L, mf, 256, C}, bins.options().dtype(kI32));
  launch_rf_hist_compact(bins.data_ptr<unsigned char>(),
                         y.data_ptr<unsigned char>(), nid.data_ptr<int>(),
                         frank.data_ptr<unsigned char>(),
                         reinterpret_cast<unsigned*>(hist.data_ptr<int>()), n,
                         (int)C, (int)mf, cur_stream());
  auto best = torch::full({L}, -1, bins.options().dtype(kI64));
  auto cnt = torch::zeros({L, C}, bins.options().dtype(kI32));
  const int rc = launch_rf_split_compact(
      hist.data_ptr<int>(), fidx.data_ptr<unsigned char>(), u64(best),
      cnt.data_ptr<int>(), (int)L, (int)C, (int)mf, cur_stream());
  TORCH_CHECK(rc == 0, "rf_level_compact: no kernel for ", C, " classes");
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {best, cnt};
}

// lmap, feat and binthr hold a value per node of the level that nid counts in.
static void rf_partition(Tensor B, Tensor nid, Tensor lmap, Tensor feat,
                         Tensor binthr) {
  const int64_t n = rows12(B, "B", kU8);
  check_buf(nid, "nid", kI32, n, B);
  check_buf(lmap, "lmap", kI32, 0, B);
  check_buf(feat, "feat", kI32, lmap.numel(), B);
  check_buf(binthr, "binthr", kI32, lmap.numel(), B);
  const CUDAGuard guard = same_device("rf_partition", B);
  launch_rf_partition(B.data_ptr<unsigned char>(), nid.data_ptr<int>(),
                      lmap.data_ptr<int>(), feat.data_ptr<int>(),
                      binthr.data_ptr<int>(), n, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("smo_select", &smo_select, "WSS-1 pair candidate selection");
  m.def("smo_update", &smo_update, "fused RBF-row gradient update");
  m.def("rf_hist", &rf_hist, "per-node per-feature class histograms (tree build)",
        py::arg("bins"), py::arg("y"), py::arg("nid"), py::arg("hist"),
        py::arg("fsel") = c10::nullopt);
  m.def("smo_solve", &smo_solve, "device-side SMO pair solve (fused iteration)");
  m.def("smo_update_dev", &smo_update_dev, "gradient update from device sol buffer");
  m.def("rf_split", &rf_split, "fused gini split search over a level histogram");
  m.def("rf_partition", &rf_partition, "fused frontier row partition");
  m.def("rf_level_compact", &rf_level_compact,
        "fused level pass: mtry-compact hist scatter + split search");
  m.def("smo_row", &smo_row, "K(x_i, .) kernel row for WSS-2");
  m.def("smo_select2", &smo_select2, "WSS-2 second-order j selection");
  m.def("smo_solve2", &smo_solve2, "device-side WSS-2 pair solve");
  m.def("smo_update_dev2", &smo_update_dev2, "gradient update reusing the WSS-2 kernel row");
  m.def("gnb_predict", &gnb_predict, "fused GaussianNB loglik+argmax");
  m.def("linear_argmax", &linear_argmax, "logits+argmax");
  m.def("kmeans_assign", &kmeans_assign, "Lloyd assign + partial update");
  m.def("rf_predict", &rf_predict, "packed-forest traversal + vote");
  m.def("rf_predict_scores", &rf_predict_scores,
        "packed-forest traversal, all trees: (proba | empty, labels, conf)");
  // The detector is no classifier op: it lives in a submodule of its own.
  // (tests/test_binding_checks.py pins the list of the top-level ops, each of
  // which it runs through its generic refusals; this op's refusals are in
  // tests/test_iforest_kernel.py.)
  auto novelty = m.def_submodule("novelty", "novelty detection next to the classifiers");
  novelty.def("iforest_score", &iforest_score,
              "isolation forest novelty: (score, flags, labels_out | empty, psum | empty)",
              py::arg("X"), py::arg("nodes"), py::arg("roots"), py::arg("labels"),
              py::arg("inv_denom"), py::arg("depth_cut"), py::arg("want_sum"));
  m.def("gnb_proba", &gnb_proba, "GaussianNB class probabilities (f64 softmax)");
  m.def("linear_proba", &linear_proba, "logistic class probabilities (f64 softmax)");
  m.def("knn_vote_proba", &knn_vote_proba, "neighbour vote fractions from top-k indices");
  m.def("ensemble_vote", &ensemble_vote,
        "soft vote over member probabilities: (avg | empty, labels, conf)");
  m.def("proba_smooth", &proba_smooth,
        "per-flow moving average of a probability row: (labels, conf)",
        py::arg("proba"), py::arg("state"), py::arg("held"), py::arg("n_live"),
        py::arg("alpha"), py::arg("margin"));
  m.def("class_traffic", &class_traffic,
        "per-class flow count and f64 feature sums: totals [C + 1, 13]",
        py::arg("X"), py::arg("labels"), py::arg("n_classes"), py::arg("conf"),
        py::arg("min_conf"), py::arg("n_live"));
  // Selection is no classifier op either: a submodule of its own, its
  // refusals in tests/test_top_flows_kernel.py.
  auto selection = m.def_submodule("selection", "selection over the classified flows");
  selection.def("class_top_flows", &class_top_flows,
                "per class and unknown, the k flows with the largest key: (rows, keys)",
                py::arg("X"), py::arg("labels"), py::arg("n_classes"), py::arg("k"),
                py::arg("col_mask"), py::arg("conf"), py::arg("min_conf"),
                py::arg("n_live"));
  // Nor is the explanation: a submodule of its own, its refusals in
  // tests/test_rf_explain_kernel.py.
  auto explain = m.def_submodule("explain", "why a model gave a flow its class");
  explain.def("rf_explain", &rf_explain,
              "forest feature contributions: (contrib | empty, why, why_value, sums | empty)",
              py::arg("X"), py::arg("nodes"), py::arg("roots"), py::arg("delta"),
              py::arg("labels"), py::arg("want_matrix"), py::arg("want_sums"));
  m.def("svc_predict", &svc_predict, "RBF Gram + OVO vote");
  m.def("svc_decision", &svc_decision, "RBF Gram + OVO decision values (f64)");
  m.def("svc_couple", &svc_couple,
        "Platt sigmoids + pairwise coupling: (proba, idx, conf)");
  m.def("knn_topk", &knn_topk, "brute-force top-k (+fused vote)");
  m.def("knn_topk_mfma", &knn_topk_mfma, "MFMA distance-GEMM top-k (+fused vote)",
        py::arg("Q"), py::arg("R"), py::arg("cmean"), py::arg("ry"),
        py::arg("k"), py::arg("C"), py::arg("idx_base"), py::arg("n_shards"),
        py::arg("approx") = 0);
  m.def("gnb_fit_stats", &gnb_fit_stats, "per-class sufficient stats");
  m.def("logistic_grad", &logistic_grad, "fused CE loss+grad");
  m.def("flow_features", &flow_features, "counters -> 12 features");
}
