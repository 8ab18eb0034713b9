// PyTorch (ROCm) bindings for the CDNA4 kernels.  This TU is host-only;
// every kernel lives in the .hip TUs and is reached through the extern "C"
// launchers so the torch headers never touch device code.

#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include <ATen/cuda/CUDAContext.h>

#include "ensemble.h"

namespace {

#define CHECK_IN(t, type)                                         \
  TORCH_CHECK((t).is_cuda(), #t " must be a GPU tensor");         \
  TORCH_CHECK((t).is_contiguous(), #t " must be contiguous");     \
  TORCH_CHECK((t).scalar_type() == type, #t " has wrong dtype");

hipStream_t cur_stream() {
  return at::cuda::getCurrentCUDAStream().stream();
}

}  // namespace

extern "C" {
void launch_gnb_predict(const float*, const float*, const float*, const float*,
                        int*, long long, int, hipStream_t);
void launch_linear_argmax(const float*, const float*, const float*, int*,
                          long long, int, hipStream_t);
void launch_kmeans_assign(const float*, const float*, int*, double*, double*,
                          double*, long long, int, int, hipStream_t);
int launch_rf_predict(const float*, const unsigned*, const unsigned*,
                      const int*, const float*, int*, long long, int, int,
                      int, int, hipStream_t);
int launch_rf_scores(const float*, const unsigned*, const int*, const float*,
                     float*, int*, float*, long long, int, int, hipStream_t);
int launch_gnb_proba(const float*, const double*, const double*,
                     const double*, float*, long long, int, hipStream_t);
int launch_linear_proba(const float*, const float*, const float*, float*,
                        long long, int, hipStream_t);
int launch_knn_vote_proba(const int*, const unsigned char*, float*, long long,
                          int, long long, int, hipStream_t);
int launch_ensemble_vote(const EnsembleArgs*, float*, int*, float*, long long,
                         int, hipStream_t);
int launch_proba_smooth(const float*, float*, int*, const int*, float, float,
                        int*, float*, long long, int, hipStream_t);
int class_traffic_blocks(long long);
int launch_class_traffic(const float*, const int*, const float*, const int*,
                         float, double*, double*, long long, int, int,
                         hipStream_t);
int launch_svc_predict(const float*, const float*, const float*,
                       const unsigned char*, const float*, int*, long long,
                       int, int, float, hipStream_t);
int launch_svc_decision(const float*, const float*, const float*,
                        const unsigned char*, const float*, double*, long long,
                        int, int, float, hipStream_t);
int launch_svc_couple(const double*, const double*, const double*, float*,
                      int*, float*, long long, int, hipStream_t);
int launch_knn_topk(const float*, const float*, const unsigned char*, float*,
                    int*, int*, long long, long long, int, int, long long,
                    hipStream_t);
void launch_knn_mfma(const float*, const float*, const float*,
                     const unsigned char*, float*, int*, float*, int*, int*,
                     long long, long long, int, int, int, long long, int,
                     hipStream_t);
void launch_gnb_fit_stats(const double*, const long long*, double*, double*,
                          double*, long long, int, hipStream_t);
void launch_logistic_grad(const double*, const long long*, const double*,
                          const double*, double*, double*, long long, int,
                          hipStream_t);
void launch_flow_features(const double*, const double*, const double*, float*,
                          long long, hipStream_t);
void launch_smo_select(const float*, const double*, const double*, double,
                       long long, unsigned long long*, hipStream_t);
void launch_rf_hist(const unsigned char*, const unsigned char*, const int*,
                    const unsigned char*, unsigned*, long long, int,
                    hipStream_t);
void launch_smo_solve(const float*, const float*, double*, const double*,
                      unsigned long long*, float*, double*, double, double,
                      float, hipStream_t);
void launch_smo_update_dev(const float*, const float*, double*, const float*,
                           const double*, float, long long, hipStream_t);
void launch_smo_row(const float*, const unsigned long long*, const double*,
                    float*, float, long long, hipStream_t);
void launch_rf_split(const int*, const unsigned char*, unsigned long long*,
                     int*, int, int, hipStream_t);
void launch_rf_partition(const unsigned char*, int*, const int*, const int*,
                         const int*, long long, hipStream_t);
void launch_rf_hist_compact(const unsigned char*, const unsigned char*,
                            const int*, const unsigned char*, unsigned*,
                            long long, int, int, hipStream_t);
void launch_rf_split_compact(const int*, const unsigned char*,
                             unsigned long long*, int*, int, int, int,
                             hipStream_t);
void launch_smo_select2(const float*, const double*, const double*,
                        const float*, unsigned long long*, const double*,
                        double, long long, hipStream_t);
void launch_smo_solve2(const float*, const float*, double*, const double*,
                       unsigned long long*, float*, double*, double, double,
                       float, hipStream_t);
void launch_smo_update_dev2(const float*, const float*, double*, const float*,
                            const double*, const float*, float, long long,
                            hipStream_t);
void launch_smo_update(const float*, const float*, double*, const float*,
                       double, double, float, long long, hipStream_t);
}

static torch::Tensor gnb_predict(torch::Tensor X, torch::Tensor theta,
                                 torch::Tensor inv_var, torch::Tensor cconst) {
  CHECK_IN(X, torch::kFloat32);
  CHECK_IN(theta, torch::kFloat32);
  CHECK_IN(inv_var, torch::kFloat32);
  CHECK_IN(cconst, torch::kFloat32);
  TORCH_CHECK(X.size(1) == 12, "X must be (n,12)");
  const long long n = X.size(0);
  const int C = theta.size(0);
  auto out = torch::empty({n}, X.options().dtype(torch::kInt32));
  launch_gnb_predict(X.data_ptr<float>(), theta.data_ptr<float>(),
                     inv_var.data_ptr<float>(), cconst.data_ptr<float>(),
                     out.data_ptr<int>(), n, C, cur_stream());
  return out;
}

static torch::Tensor linear_argmax(torch::Tensor X, torch::Tensor W,
                                   torch::Tensor b) {
  CHECK_IN(X, torch::kFloat32);
  CHECK_IN(W, torch::kFloat32);
  CHECK_IN(b, torch::kFloat32);
  TORCH_CHECK(X.size(1) == 12, "X must be (n,12)");
  const long long n = X.size(0);
  const int C = W.size(0);
  auto out = torch::empty({n}, X.options().dtype(torch::kInt32));
  launch_linear_argmax(X.data_ptr<float>(), W.data_ptr<float>(),
                       b.data_ptr<float>(), out.data_ptr<int>(), n, C,
                       cur_stream());
  return out;
}

static std::vector<torch::Tensor> kmeans_assign(torch::Tensor X,
                                                torch::Tensor centers,
                                                bool want_update) {
  CHECK_IN(X, torch::kFloat32);
  CHECK_IN(centers, torch::kFloat32);
  TORCH_CHECK(X.size(1) == 12, "X must be (n,12)");
  const long long n = X.size(0);
  const int K = centers.size(0);
  auto labels = torch::empty({n}, X.options().dtype(torch::kInt32));
  auto counts = torch::zeros({K}, X.options().dtype(torch::kFloat64));
  auto sums = torch::zeros({K, 12}, X.options().dtype(torch::kFloat64));
  auto inertia = torch::zeros({1}, X.options().dtype(torch::kFloat64));
  launch_kmeans_assign(X.data_ptr<float>(), centers.data_ptr<float>(),
                       labels.data_ptr<int>(), counts.data_ptr<double>(),
                       sums.data_ptr<double>(), inertia.data_ptr<double>(), n,
                       K, want_update ? 1 : 0, cur_stream());
  return {labels, counts, sums, inertia};
}

static torch::Tensor rf_predict(torch::Tensor X, torch::Tensor nodes,
                                torch::Tensor snodes, torch::Tensor roots,
                                torch::Tensor leaf_proba, int64_t n_leaves,
                                int64_t C) {
  CHECK_IN(X, torch::kFloat32);
  CHECK_IN(nodes, torch::kInt32);   // packed uint2 as 2x int32
  CHECK_IN(snodes, torch::kInt32);  // streaming kernel's table (ops/gpu.py)
  CHECK_IN(roots, torch::kInt32);
  CHECK_IN(leaf_proba, torch::kFloat32);
  TORCH_CHECK(X.size(1) == 12, "X must be (n,12)");
  TORCH_CHECK(nodes.size(1) == 2, "nodes must be (n_nodes,2) int32");
  TORCH_CHECK(snodes.dim() == 2 && snodes.size(1) == 2 &&
                  snodes.size(0) == nodes.size(0) + 2,
              "snodes must be (n_nodes+2,2) int32");
  TORCH_CHECK(leaf_proba.numel() >= n_leaves * C,
              "leaf_proba must hold n_leaves rows of C");
  const long long n = X.size(0);
  const int n_nodes = nodes.size(0);
  const int T = roots.size(0);
  auto out = torch::empty({n}, X.options().dtype(torch::kInt32));
  const int rc = launch_rf_predict(
      X.data_ptr<float>(),
      reinterpret_cast<const unsigned*>(nodes.data_ptr<int>()),
      reinterpret_cast<const unsigned*>(snodes.data_ptr<int>()),
      roots.data_ptr<int>(), leaf_proba.data_ptr<float>(), out.data_ptr<int>(),
      n, n_nodes, (int)n_leaves, T, (int)C, cur_stream());
  TORCH_CHECK(rc == 0, "rf_predict: no kernel for ", C, " classes");
  return out;
}

// Class scores of the forest (rf_proba_kernels.hip): every tree counts.
// Returns (proba [n,C] f32 or an empty tensor, labels [n] i32, conf [n] f32).
static std::vector<torch::Tensor> rf_predict_scores(
    torch::Tensor X, torch::Tensor nodes, torch::Tensor roots,
    torch::Tensor leaf_proba, int64_t n_leaves, int64_t C, bool want_proba) {
  CHECK_IN(X, torch::kFloat32);
  CHECK_IN(nodes, torch::kInt32);  // packed uint2 as 2x int32
  CHECK_IN(roots, torch::kInt32);
  CHECK_IN(leaf_proba, torch::kFloat32);
  TORCH_CHECK(X.dim() == 2 && X.size(1) == 12, "X must be (n,12)");
  TORCH_CHECK(nodes.dim() == 2 && nodes.size(1) == 2,
              "nodes must be (n_nodes,2) int32");
  TORCH_CHECK(C >= 2 && C <= 8, "rf_predict_scores supports 2..8 classes, got ", C);
  TORCH_CHECK(n_leaves >= 0 && leaf_proba.numel() >= n_leaves * C,
              "leaf_proba must hold n_leaves rows of C");
  const long long n = X.size(0);
  const int T = roots.size(0);
  TORCH_CHECK(T >= 1, "forest has no trees");
  auto proba = torch::empty({want_proba ? n : 0, C}, X.options());
  auto labels = torch::empty({n}, X.options().dtype(torch::kInt32));
  auto conf = torch::empty({n}, X.options());
  const int rc = launch_rf_scores(
      X.data_ptr<float>(),
      reinterpret_cast<const unsigned*>(nodes.data_ptr<int>()),
      roots.data_ptr<int>(), leaf_proba.data_ptr<float>(),
      want_proba ? proba.data_ptr<float>() : nullptr, labels.data_ptr<int>(),
      conf.data_ptr<float>(), n, T, (int)C, cur_stream());
  TORCH_CHECK(rc == 0, "rf_predict_scores: no kernel for ", C, " classes");
  return {proba, labels, conf};
}

// Class probabilities and the soft vote (ensemble_kernels.hip).  Class counts
// are 2..8; anything else is an error here, never an unwritten output.
static torch::Tensor gnb_proba(torch::Tensor X, torch::Tensor theta,
                               torch::Tensor inv_var, torch::Tensor cconst) {
  CHECK_IN(X, torch::kFloat32);
  CHECK_IN(theta, torch::kFloat64);
  CHECK_IN(inv_var, torch::kFloat64);
  CHECK_IN(cconst, torch::kFloat64);
  TORCH_CHECK(X.dim() == 2 && X.size(1) == 12, "X must be (n,12)");
  const int64_t C = cconst.numel();
  TORCH_CHECK(C >= 2 && C <= 8, "gnb_proba supports 2..8 classes, got ", C);
  TORCH_CHECK(theta.numel() == C * 12 && inv_var.numel() == C * 12,
              "theta and inv_var must be (C,12)");
  const long long n = X.size(0);
  auto proba = torch::empty({n, C}, X.options());
  const int rc = launch_gnb_proba(
      X.data_ptr<float>(), theta.data_ptr<double>(), inv_var.data_ptr<double>(),
      cconst.data_ptr<double>(), proba.data_ptr<float>(), n, (int)C,
      cur_stream());
  TORCH_CHECK(rc == 0, "gnb_proba: no kernel for ", C, " classes");
  return proba;
}

static torch::Tensor linear_proba(torch::Tensor X, torch::Tensor W,
                                  torch::Tensor b) {
  CHECK_IN(X, torch::kFloat32);
  CHECK_IN(W, torch::kFloat32);
  CHECK_IN(b, torch::kFloat32);
  TORCH_CHECK(X.dim() == 2 && X.size(1) == 12, "X must be (n,12)");
  const int64_t C = b.numel();
  TORCH_CHECK(C >= 2 && C <= 8, "linear_proba supports 2..8 classes, got ", C);
  TORCH_CHECK(W.numel() == C * 12, "W must be (C,12)");
  const long long n = X.size(0);
  auto proba = torch::empty({n, C}, X.options());
  const int rc = launch_linear_proba(X.data_ptr<float>(), W.data_ptr<float>(),
                                     b.data_ptr<float>(),
                                     proba.data_ptr<float>(), n, (int)C,
                                     cur_stream());
  TORCH_CHECK(rc == 0, "linear_proba: no kernel for ", C, " classes");
  return proba;
}

static torch::Tensor knn_vote_proba(torch::Tensor idx, torch::Tensor y,
                                    int64_t C) {
  CHECK_IN(idx, torch::kInt32);
  CHECK_IN(y, torch::kUInt8);
  TORCH_CHECK(idx.dim() == 2 && idx.size(1) >= 1, "idx must be (n,k), k >= 1");
  TORCH_CHECK(C >= 2 && C <= 8, "knn_vote_proba supports 2..8 classes, got ", C);
  const long long n = idx.size(0);
  auto proba = torch::empty({n, C}, idx.options().dtype(torch::kFloat32));
  const int rc = launch_knn_vote_proba(
      idx.data_ptr<int>(), y.data_ptr<unsigned char>(), proba.data_ptr<float>(),
      n, (int)idx.size(1), (long long)y.numel(), (int)C, cur_stream());
  TORCH_CHECK(rc == 0, "knn_vote_proba: no kernel for ", C, " classes");
  return proba;
}

// Returns (avg [n,C] f32 or an empty tensor, labels [n] i32, conf [n] f32).
// `weights` are the normalised weights (the caller divides by their f64 sum).
static std::vector<torch::Tensor> ensemble_vote(
    std::vector<torch::Tensor> probas,
    std::vector<std::vector<int64_t>> colmaps, std::vector<double> weights,
    int64_t C, bool want_proba) {
  const int64_t M = (int64_t)probas.size();
  TORCH_CHECK(M >= 1 && M <= ENS_MAX_M, "ensemble_vote takes 1..8 members, got ", M);
  TORCH_CHECK((int64_t)colmaps.size() == M && (int64_t)weights.size() == M,
              "ensemble_vote: one column map and one weight per member");
  TORCH_CHECK(C >= 2 && C <= ENS_MAX_C, "ensemble_vote supports 2..8 classes, got ", C);
  EnsembleArgs args;
  memset(&args, 0, sizeof(args));
  args.M = (int)M;
  const long long n = probas[0].size(0);
  for (int64_t m = 0; m < M; ++m) {
    const torch::Tensor& p = probas[m];
    CHECK_IN(p, torch::kFloat32);
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
  auto opts = probas[0].options();
  auto avg = torch::empty({want_proba ? n : 0, C}, opts);
  auto labels = torch::empty({n}, opts.dtype(torch::kInt32));
  auto conf = torch::empty({n}, opts);
  const int rc = launch_ensemble_vote(
      &args, want_proba ? avg.data_ptr<float>() : nullptr,
      labels.data_ptr<int>(), conf.data_ptr<float>(), n, (int)C, cur_stream());
  TORCH_CHECK(rc == 0, "ensemble_vote: arguments out of the kernel's range");
  return {avg, labels, conf};
}

// Returns (labels [n] i32, conf [n] f32); `state` [cap,C] and `held` [cap]
// are updated in place, rows < n only.  `n_live` is an int32 [1] tensor or
// None (all n rows are live).
static std::vector<torch::Tensor> proba_smooth(
    torch::Tensor proba, torch::Tensor state, torch::Tensor held,
    c10::optional<torch::Tensor> n_live, double alpha, double margin) {
  CHECK_IN(proba, torch::kFloat32);
  CHECK_IN(state, torch::kFloat32);
  CHECK_IN(held, torch::kInt32);
  TORCH_CHECK(proba.dim() == 2 && state.dim() == 2 && held.dim() == 1,
              "proba_smooth takes proba (n,C), state (cap,C) and held (cap)");
  const long long n = proba.size(0);
  const int64_t C = proba.size(1);
  TORCH_CHECK(C >= 2 && C <= 8, "proba_smooth supports 2..8 classes, got ", C);
  TORCH_CHECK(state.size(1) == C, "state has ", state.size(1), " columns for ", C, " classes");
  TORCH_CHECK(state.size(0) >= n && held.size(0) >= n,
              "state and held need at least ", n, " rows");
  TORCH_CHECK(proba.get_device() == state.get_device() &&
                  proba.get_device() == held.get_device(),
              "proba, state and held must be on one device");
  const char* p0 = static_cast<const char*>(proba.data_ptr());
  const char* s0 = static_cast<const char*>(state.data_ptr());
  TORCH_CHECK(p0 + proba.nbytes() <= s0 || s0 + state.nbytes() <= p0,
              "proba must not alias state");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(p0) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(s0) % 16 == 0,
              "proba and state must be 16-byte aligned");
  const int* live = nullptr;
  if (n_live.has_value()) {
    const torch::Tensor& n_live_t = n_live.value();
    CHECK_IN(n_live_t, torch::kInt32);
    TORCH_CHECK(n_live_t.numel() == 1 && n_live_t.get_device() == proba.get_device(),
                "n_live must be an int32 [1] tensor on proba's device");
    live = n_live_t.data_ptr<int>();
  }
  const float a = (float)alpha, m = (float)margin;
  TORCH_CHECK(a > 0.f && a <= 1.f, "alpha must be in (0, 1]");
  TORCH_CHECK(std::isfinite(m) && m >= 0.f, "margin must be finite and >= 0");
  auto labels = torch::empty({n}, proba.options().dtype(torch::kInt32));
  auto conf = torch::empty({n}, proba.options());
  const int rc = launch_proba_smooth(
      proba.data_ptr<float>(), state.data_ptr<float>(), held.data_ptr<int>(),
      live, a, m, labels.data_ptr<int>(), conf.data_ptr<float>(), n, (int)C,
      cur_stream());
  TORCH_CHECK(rc == 0, "proba_smooth: arguments out of the kernel's range");
  return {labels, conf};
}

// Returns totals [C + 1, 13] f64: per group (class, or C for "unknown") the
// row count and the f64 sums of the 12 features.  `conf` is an f32 [n] tensor
// or None, `n_live` an int32 [1] tensor or None (all n rows are live).
static torch::Tensor class_traffic(torch::Tensor X, torch::Tensor labels,
                                   int64_t n_classes,
                                   c10::optional<torch::Tensor> conf,
                                   double min_conf,
                                   c10::optional<torch::Tensor> n_live) {
  CHECK_IN(X, torch::kFloat32);
  CHECK_IN(labels, torch::kInt32);
  TORCH_CHECK(X.dim() == 2 && X.size(1) == 12, "X must be (n,12)");
  const long long n = X.size(0);
  TORCH_CHECK(labels.dim() == 1 && labels.size(0) == n, "labels must be (n)");
  TORCH_CHECK(labels.get_device() == X.get_device(),
              "X and labels must be on one device");
  TORCH_CHECK(n_classes >= 2 && n_classes <= 8,
              "no kernel for class_traffic with ", n_classes, " classes (2..8)");
  const float* cf = nullptr;
  if (conf.has_value()) {
    const torch::Tensor& conf_t = conf.value();
    CHECK_IN(conf_t, torch::kFloat32);
    TORCH_CHECK(conf_t.dim() == 1 && conf_t.size(0) == n &&
                    conf_t.get_device() == X.get_device(),
                "conf must be an f32 (n) tensor on X's device");
    cf = conf_t.data_ptr<float>();
  }
  const int* live = nullptr;
  if (n_live.has_value()) {
    const torch::Tensor& n_live_t = n_live.value();
    CHECK_IN(n_live_t, torch::kInt32);
    TORCH_CHECK(n_live_t.numel() == 1 && n_live_t.get_device() == X.get_device(),
                "n_live must be an int32 [1] tensor on X's device");
    live = n_live_t.data_ptr<int>();
  }
  const float mc = (float)min_conf;
  TORCH_CHECK(std::isfinite(mc), "min_conf must be finite");
  const int C = (int)n_classes;
  const int nb = class_traffic_blocks(n);
  const auto f64 = X.options().dtype(torch::kFloat64);
  auto partial = torch::empty({(int64_t)nb * (C + 1) * 13}, f64);
  auto totals = torch::empty({C + 1, 13}, f64);
  const int rc = launch_class_traffic(
      X.data_ptr<float>(), labels.data_ptr<int>(), cf, live, mc,
      partial.data_ptr<double>(), totals.data_ptr<double>(), n, C, nb,
      cur_stream());
  TORCH_CHECK(rc == 0, "no kernel for class_traffic with ", C, " classes");
  return totals;
}

static torch::Tensor svc_predict(torch::Tensor X, torch::Tensor SV,
                                 torch::Tensor dual, torch::Tensor svclass,
                                 torch::Tensor intercept, double gamma) {
  CHECK_IN(X, torch::kFloat32);
  CHECK_IN(SV, torch::kFloat32);
  CHECK_IN(dual, torch::kFloat32);
  CHECK_IN(svclass, torch::kUInt8);
  CHECK_IN(intercept, torch::kFloat32);
  TORCH_CHECK(X.size(1) == 12, "X must be (n,12)");
  const long long n = X.size(0);
  const int nsv = SV.size(0);
  const int C = dual.size(0) + 1;
  TORCH_CHECK(C >= 2 && C <= 6, "svc kernel supports 2..6 classes");
  auto out = torch::empty({n}, X.options().dtype(torch::kInt32));
  const int rc = launch_svc_predict(
      X.data_ptr<float>(), SV.data_ptr<float>(), dual.data_ptr<float>(),
      svclass.data_ptr<unsigned char>(), intercept.data_ptr<float>(),
      out.data_ptr<int>(), n, nsv, C, (float)gamma, cur_stream());
  TORCH_CHECK(rc == 0, "svc_predict: no kernel for ", C, " classes");
  return out;
}

// SVC class probabilities (svc_kernels.hip).  The decision kernels
// index SV, dual, svclass and intercept by nsv and C alone, so every extent
// is checked here.
static torch::Tensor svc_decision(torch::Tensor X, torch::Tensor SV,
                                  torch::Tensor dual, torch::Tensor svclass,
                                  torch::Tensor intercept, double gamma) {
  CHECK_IN(X, torch::kFloat32);
  CHECK_IN(SV, torch::kFloat32);
  CHECK_IN(dual, torch::kFloat32);
  CHECK_IN(svclass, torch::kUInt8);
  CHECK_IN(intercept, torch::kFloat32);
  TORCH_CHECK(X.dim() == 2 && X.size(1) == 12, "X must be (n,12)");
  TORCH_CHECK(SV.dim() == 2 && SV.size(1) == 12, "SV must be (nsv,12)");
  TORCH_CHECK(dual.dim() == 2, "dual must be (C-1,nsv)");
  const long long n = X.size(0);
  const int64_t nsv = SV.size(0);
  const int64_t C = dual.size(0) + 1;
  TORCH_CHECK(C >= 2 && C <= 6, "svc_decision supports 2..6 classes, got ", C);
  TORCH_CHECK(nsv <= INT32_MAX, "too many support vectors");
  const int64_t npair = C * (C - 1) / 2;
  TORCH_CHECK(dual.size(1) == nsv, "dual must be (C-1,nsv)");
  TORCH_CHECK(svclass.numel() == nsv, "svclass must have one entry per SV");
  TORCH_CHECK(intercept.numel() == npair, "intercept must have C(C-1)/2 entries");
  auto out = torch::empty({n, npair}, X.options().dtype(torch::kFloat64));
  const int rc = launch_svc_decision(
      X.data_ptr<float>(), SV.data_ptr<float>(), dual.data_ptr<float>(),
      svclass.data_ptr<unsigned char>(), intercept.data_ptr<float>(),
      out.data_ptr<double>(), n, (int)nsv, (int)C, (float)gamma, cur_stream());
  TORCH_CHECK(rc == 0, "svc_decision: no kernel for ", C, " classes");
  return out;
}

// Returns (proba [n,C] f32, idx [n] i32, conf [n] f32).
static std::vector<torch::Tensor> svc_couple(torch::Tensor dec,
                                             torch::Tensor probA,
                                             torch::Tensor probB, int64_t C) {
  CHECK_IN(dec, torch::kFloat64);
  CHECK_IN(probA, torch::kFloat64);
  CHECK_IN(probB, torch::kFloat64);
  TORCH_CHECK(C >= 2 && C <= 6, "svc_couple supports 2..6 classes, got ", C);
  const int64_t npair = C * (C - 1) / 2;
  TORCH_CHECK(dec.dim() == 2 && dec.size(1) == npair,
              "dec must be (n,C(C-1)/2)");
  TORCH_CHECK(probA.numel() == npair && probB.numel() == npair,
              "probA and probB must have C(C-1)/2 entries");
  const long long n = dec.size(0);
  auto f32 = dec.options().dtype(torch::kFloat32);
  auto proba = torch::empty({n, C}, f32);
  auto idx = torch::empty({n}, dec.options().dtype(torch::kInt32));
  auto conf = torch::empty({n}, f32);
  const int rc = launch_svc_couple(
      dec.data_ptr<double>(), probA.data_ptr<double>(),
      probB.data_ptr<double>(), proba.data_ptr<float>(), idx.data_ptr<int>(),
      conf.data_ptr<float>(), n, (int)C, cur_stream());
  TORCH_CHECK(rc == 0, "svc_couple: no kernel for ", C, " classes");
  return {proba, idx, conf};
}

static std::vector<torch::Tensor> knn_topk(torch::Tensor Q, torch::Tensor R,
                                           c10::optional<torch::Tensor> ry,
                                           int64_t k, int64_t C,
                                           int64_t idx_base) {
  CHECK_IN(Q, torch::kFloat32);
  CHECK_IN(R, torch::kFloat32);
  TORCH_CHECK(Q.size(1) == 12 && R.size(1) == 12, "rows must be (n,12)");
  TORCH_CHECK(k <= 32, "k <= 32");
  const long long nq = Q.size(0);
  const long long nr = R.size(0);
  auto dist = torch::empty({nq, k}, Q.options());
  auto idx = torch::empty({nq, k}, Q.options().dtype(torch::kInt32));
  const unsigned char* ry_ptr = nullptr;
  torch::Tensor lab;
  int* lab_ptr = nullptr;
  if (ry.has_value()) {
    CHECK_IN(ry.value(), torch::kUInt8);
    ry_ptr = ry.value().data_ptr<unsigned char>();
    lab = torch::empty({nq}, Q.options().dtype(torch::kInt32));
    lab_ptr = lab.data_ptr<int>();
  }
  const int rc = launch_knn_topk(
      Q.data_ptr<float>(), R.data_ptr<float>(), ry_ptr, dist.data_ptr<float>(),
      idx.data_ptr<int>(), lab_ptr, nq, nr, (int)k, (int)C, idx_base,
      cur_stream());
  TORCH_CHECK(rc == 0, "knn_topk: no kernel for k = ", k);
  if (ry.has_value()) return {dist, idx, lab};
  return {dist, idx};
}

// MFMA distance-GEMM path: R sharded across gridDim.y, per-shard partial
// top-k lists merged by a second kernel (knn_mfma.hip).
static std::vector<torch::Tensor> knn_topk_mfma(torch::Tensor Q,
                                                torch::Tensor R,
                                                torch::Tensor cmean,
                                                c10::optional<torch::Tensor> ry,
                                                int64_t k, int64_t C,
                                                int64_t idx_base,
                                                int64_t n_shards,
                                                int64_t approx) {
  CHECK_IN(Q, torch::kFloat32);
  CHECK_IN(R, torch::kFloat32);
  CHECK_IN(cmean, torch::kFloat32);
  TORCH_CHECK(Q.size(1) == 12 && R.size(1) == 12, "rows must be (n,12)");
  TORCH_CHECK(k >= 1 && k <= 8, "MFMA path supports k <= 8");
  TORCH_CHECK(cmean.numel() == 12, "cmean must be (12,)");
  const long long nq = Q.size(0);
  const long long nr = R.size(0);
  int S = (int)n_shards;
  if (S < 1) S = 1;
  if ((long long)S > (nr + 127) / 128) S = (int)((nr + 127) / 128);
  auto part_d = torch::empty({S, nq, k}, Q.options());
  auto part_i = torch::empty({S, nq, k}, Q.options().dtype(torch::kInt32));
  auto dist = torch::empty({nq, k}, Q.options());
  auto idx = torch::empty({nq, k}, Q.options().dtype(torch::kInt32));
  const unsigned char* ry_ptr = nullptr;
  torch::Tensor lab;
  int* lab_ptr = nullptr;
  if (ry.has_value()) {
    CHECK_IN(ry.value(), torch::kUInt8);
    ry_ptr = ry.value().data_ptr<unsigned char>();
    lab = torch::empty({nq}, Q.options().dtype(torch::kInt32));
    lab_ptr = lab.data_ptr<int>();
  }
  launch_knn_mfma(Q.data_ptr<float>(), R.data_ptr<float>(),
                  cmean.data_ptr<float>(), ry_ptr, part_d.data_ptr<float>(),
                  part_i.data_ptr<int>(), dist.data_ptr<float>(),
                  idx.data_ptr<int>(), lab_ptr, nq, nr, S, (int)k, (int)C,
                  idx_base, (int)approx, cur_stream());
  if (ry.has_value()) return {dist, idx, lab};
  return {dist, idx};
}

static std::vector<torch::Tensor> gnb_fit_stats(torch::Tensor X,
                                                torch::Tensor y, int64_t C) {
  CHECK_IN(X, torch::kFloat64);
  CHECK_IN(y, torch::kInt64);
  TORCH_CHECK(X.size(1) == 12, "X must be (n,12)");
  const long long n = X.size(0);
  auto count = torch::zeros({C}, X.options());
  auto sum = torch::zeros({C, 12}, X.options());
  auto sumsq = torch::zeros({C, 12}, X.options());
  launch_gnb_fit_stats(X.data_ptr<double>(), reinterpret_cast<const long long*>(y.data_ptr<int64_t>()),
                       count.data_ptr<double>(), sum.data_ptr<double>(),
                       sumsq.data_ptr<double>(), n, (int)C, cur_stream());
  return {count, sum, sumsq};
}

static std::vector<torch::Tensor> logistic_grad(torch::Tensor X,
                                                torch::Tensor y,
                                                torch::Tensor W,
                                                torch::Tensor b) {
  CHECK_IN(X, torch::kFloat64);
  CHECK_IN(y, torch::kInt64);
  CHECK_IN(W, torch::kFloat64);
  CHECK_IN(b, torch::kFloat64);
  const long long n = X.size(0);
  const int C = W.size(0);
  auto grad = torch::zeros({C, 13}, X.options());
  auto loss = torch::zeros({1}, X.options());
  launch_logistic_grad(X.data_ptr<double>(), reinterpret_cast<const long long*>(y.data_ptr<int64_t>()),
                       W.data_ptr<double>(), b.data_ptr<double>(),
                       grad.data_ptr<double>(), loss.data_ptr<double>(), n, C,
                       cur_stream());
  return {grad, loss};
}

static torch::Tensor flow_features(torch::Tensor cur, torch::Tensor prev,
                                   torch::Tensor times) {
  CHECK_IN(cur, torch::kFloat64);
  CHECK_IN(prev, torch::kFloat64);
  CHECK_IN(times, torch::kFloat64);
  const long long n = cur.size(0);
  auto out = torch::empty({n, 12}, cur.options().dtype(torch::kFloat32));
  launch_flow_features(cur.data_ptr<double>(), prev.data_ptr<double>(),
                       times.data_ptr<double>(), out.data_ptr<float>(), n,
                       cur_stream());
  return out;
}

static void smo_select(torch::Tensor y, torch::Tensor alpha,
                       torch::Tensor grad, double C, torch::Tensor out) {
  CHECK_IN(y, torch::kFloat32);
  CHECK_IN(alpha, torch::kFloat64);
  CHECK_IN(grad, torch::kFloat64);
  CHECK_IN(out, torch::kInt64);  // reinterpreted as u64 packed keys, len 2
  launch_smo_select(y.data_ptr<float>(), alpha.data_ptr<double>(),
                    grad.data_ptr<double>(), C, y.size(0),
                    reinterpret_cast<unsigned long long*>(out.data_ptr<int64_t>()),
                    cur_stream());
}

static void rf_hist(torch::Tensor bins, torch::Tensor y, torch::Tensor nid,
                    torch::Tensor hist,
                    c10::optional<torch::Tensor> fsel = c10::nullopt) {
  CHECK_IN(bins, torch::kUInt8);
  CHECK_IN(y, torch::kUInt8);
  CHECK_IN(nid, torch::kInt32);
  CHECK_IN(hist, torch::kInt32);  // u32 atomics on int32 storage
  TORCH_CHECK(bins.size(1) == 12, "bins must be (n,12)");
  TORCH_CHECK(hist.dim() == 4 && hist.size(1) == 12 && hist.size(2) == 256,
              "hist must be (nodes,12,256,C)");
  const unsigned char* fs = nullptr;
  if (fsel.has_value()) {
    CHECK_IN(fsel.value(), torch::kUInt8);
    TORCH_CHECK(fsel.value().numel() == hist.size(0) * 12,
                "fsel must be (nodes,12)");
    fs = fsel.value().data_ptr<unsigned char>();
  }
  launch_rf_hist(bins.data_ptr<unsigned char>(), y.data_ptr<unsigned char>(),
                 nid.data_ptr<int>(), fs,
                 reinterpret_cast<unsigned*>(hist.data_ptr<int>()),
                 bins.size(0), hist.size(3), cur_stream());
}

static void smo_solve(torch::Tensor X, torch::Tensor y, torch::Tensor alpha,
                      torch::Tensor grad, torch::Tensor sel, torch::Tensor rows,
                      torch::Tensor sol, double C, double tol, double gamma) {
  CHECK_IN(X, torch::kFloat32);
  CHECK_IN(y, torch::kFloat32);
  CHECK_IN(alpha, torch::kFloat64);
  CHECK_IN(grad, torch::kFloat64);
  CHECK_IN(sel, torch::kInt64);
  CHECK_IN(rows, torch::kFloat32);
  CHECK_IN(sol, torch::kFloat64);
  launch_smo_solve(X.data_ptr<float>(), y.data_ptr<float>(),
                   alpha.data_ptr<double>(), grad.data_ptr<double>(),
                   reinterpret_cast<unsigned long long*>(sel.data_ptr<int64_t>()),
                   rows.data_ptr<float>(), sol.data_ptr<double>(), C, tol,
                   (float)gamma, cur_stream());
}

static void smo_update_dev(torch::Tensor X, torch::Tensor y, torch::Tensor grad,
                           torch::Tensor rows, torch::Tensor sol, double gamma) {
  CHECK_IN(X, torch::kFloat32);
  CHECK_IN(y, torch::kFloat32);
  CHECK_IN(grad, torch::kFloat64);
  CHECK_IN(rows, torch::kFloat32);
  CHECK_IN(sol, torch::kFloat64);
  launch_smo_update_dev(X.data_ptr<float>(), y.data_ptr<float>(),
                        grad.data_ptr<double>(), rows.data_ptr<float>(),
                        sol.data_ptr<double>(), (float)gamma, X.size(0),
                        cur_stream());
}

static std::vector<torch::Tensor> rf_level_compact(torch::Tensor bins,
                                                   torch::Tensor y,
                                                   torch::Tensor nid,
                                                   torch::Tensor frank,
                                                   torch::Tensor fidx, int64_t L,
                                                   int64_t C) {
  // fused level pass: compact mtry-plane histogram scatter + split search
  CHECK_IN(bins, torch::kUInt8);
  CHECK_IN(y, torch::kUInt8);
  CHECK_IN(nid, torch::kInt32);
  CHECK_IN(frank, torch::kUInt8);
  CHECK_IN(fidx, torch::kUInt8);
  TORCH_CHECK(bins.size(1) == 12, "bins must be (n,12)");
  TORCH_CHECK(frank.numel() == L * 12, "frank must be (L,12)");
  int mf = (int)(fidx.numel() / L);
  TORCH_CHECK(mf >= 1 && (int64_t)mf * L == fidx.numel(), "fidx must be (L,mf)");
  auto hist = torch::zeros({L, mf, 256, C},
                           bins.options().dtype(torch::kInt32));
  launch_rf_hist_compact(bins.data_ptr<unsigned char>(),
                         y.data_ptr<unsigned char>(), nid.data_ptr<int>(),
                         frank.data_ptr<unsigned char>(),
                         reinterpret_cast<unsigned*>(hist.data_ptr<int>()),
                         bins.size(0), (int)C, mf, cur_stream());
  auto best = torch::full({L}, -1, bins.options().dtype(torch::kInt64));
  auto cnt = torch::zeros({L, C}, bins.options().dtype(torch::kInt32));
  launch_rf_split_compact(hist.data_ptr<int>(),
                          fidx.data_ptr<unsigned char>(),
                          reinterpret_cast<unsigned long long*>(best.data_ptr<int64_t>()),
                          cnt.data_ptr<int>(), (int)L, (int)C, mf,
                          cur_stream());
  return {best, cnt};
}

static void rf_partition(torch::Tensor B, torch::Tensor nid,
                         torch::Tensor lmap, torch::Tensor feat,
                         torch::Tensor binthr) {
  CHECK_IN(B, torch::kUInt8);
  CHECK_IN(nid, torch::kInt32);
  CHECK_IN(lmap, torch::kInt32);
  CHECK_IN(feat, torch::kInt32);
  CHECK_IN(binthr, torch::kInt32);
  TORCH_CHECK(B.size(1) == 12, "B must be (n,12)");
  launch_rf_partition(B.data_ptr<unsigned char>(), nid.data_ptr<int>(),
                      lmap.data_ptr<int>(), feat.data_ptr<int>(),
                      binthr.data_ptr<int>(), B.size(0), cur_stream());
}

static std::vector<torch::Tensor> rf_split(torch::Tensor hist,
                                           torch::Tensor fsel) {
  CHECK_IN(hist, torch::kInt32);
  CHECK_IN(fsel, torch::kUInt8);
  TORCH_CHECK(hist.dim() == 4 && hist.size(1) == 12 && hist.size(2) == 256,
              "hist must be (L,12,256,C)");
  int L = (int)hist.size(0);
  int C = (int)hist.size(3);
  auto best = torch::full({L}, -1, hist.options().dtype(torch::kInt64));
  auto cnt = torch::zeros({L, C}, hist.options());
  launch_rf_split(hist.data_ptr<int>(), fsel.data_ptr<unsigned char>(),
                  reinterpret_cast<unsigned long long*>(best.data_ptr<int64_t>()),
                  cnt.data_ptr<int>(), L, C, cur_stream());
  return {best, cnt};
}

static void smo_row(torch::Tensor X, torch::Tensor sel, torch::Tensor sol,
                    torch::Tensor krow, double gamma) {
  CHECK_IN(X, torch::kFloat32);
  CHECK_IN(sel, torch::kInt64);
  CHECK_IN(sol, torch::kFloat64);
  CHECK_IN(krow, torch::kFloat32);
  launch_smo_row(X.data_ptr<float>(),
                 reinterpret_cast<unsigned long long*>(sel.data_ptr<int64_t>()),
                 sol.data_ptr<double>(), krow.data_ptr<float>(), (float)gamma,
                 X.size(0), cur_stream());
}

static void smo_select2(torch::Tensor y, torch::Tensor alpha,
                        torch::Tensor grad, torch::Tensor krow,
                        torch::Tensor sel, torch::Tensor sol, double C) {
  CHECK_IN(y, torch::kFloat32);
  CHECK_IN(alpha, torch::kFloat64);
  CHECK_IN(grad, torch::kFloat64);
  CHECK_IN(krow, torch::kFloat32);
  CHECK_IN(sel, torch::kInt64);
  CHECK_IN(sol, torch::kFloat64);
  launch_smo_select2(y.data_ptr<float>(), alpha.data_ptr<double>(),
                     grad.data_ptr<double>(), krow.data_ptr<float>(),
                     reinterpret_cast<unsigned long long*>(sel.data_ptr<int64_t>()),
                     sol.data_ptr<double>(), C, y.size(0), cur_stream());
}

static void smo_solve2(torch::Tensor X, torch::Tensor y, torch::Tensor alpha,
                       torch::Tensor grad, torch::Tensor sel, torch::Tensor rows,
                       torch::Tensor sol, double C, double tol, double gamma) {
  CHECK_IN(X, torch::kFloat32);
  CHECK_IN(y, torch::kFloat32);
  CHECK_IN(alpha, torch::kFloat64);
  CHECK_IN(grad, torch::kFloat64);
  CHECK_IN(sel, torch::kInt64);
  CHECK_IN(rows, torch::kFloat32);
  CHECK_IN(sol, torch::kFloat64);
  TORCH_CHECK(sel.numel() >= 3, "WSS-2 sel buffer must be u64[3]");
  launch_smo_solve2(X.data_ptr<float>(), y.data_ptr<float>(),
                    alpha.data_ptr<double>(), grad.data_ptr<double>(),
                    reinterpret_cast<unsigned long long*>(sel.data_ptr<int64_t>()),
                    rows.data_ptr<float>(), sol.data_ptr<double>(), C, tol,
                    (float)gamma, cur_stream());
}

static void smo_update_dev2(torch::Tensor X, torch::Tensor y, torch::Tensor grad,
                            torch::Tensor rows, torch::Tensor sol,
                            torch::Tensor krow, double gamma) {
  CHECK_IN(X, torch::kFloat32);
  CHECK_IN(y, torch::kFloat32);
  CHECK_IN(grad, torch::kFloat64);
  CHECK_IN(rows, torch::kFloat32);
  CHECK_IN(sol, torch::kFloat64);
  CHECK_IN(krow, torch::kFloat32);
  launch_smo_update_dev2(X.data_ptr<float>(), y.data_ptr<float>(),
                         grad.data_ptr<double>(), rows.data_ptr<float>(),
                         sol.data_ptr<double>(), krow.data_ptr<float>(),
                         (float)gamma, X.size(0), cur_stream());
}

static void smo_update(torch::Tensor X, torch::Tensor y, torch::Tensor grad,
                       torch::Tensor rows, double yidai, double yjdaj,
                       double gamma) {
  CHECK_IN(X, torch::kFloat32);
  CHECK_IN(y, torch::kFloat32);
  CHECK_IN(grad, torch::kFloat64);
  CHECK_IN(rows, torch::kFloat32);
  launch_smo_update(X.data_ptr<float>(), y.data_ptr<float>(),
                    grad.data_ptr<double>(), rows.data_ptr<float>(), yidai,
                    yjdaj, (float)gamma, X.size(0), cur_stream());
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
