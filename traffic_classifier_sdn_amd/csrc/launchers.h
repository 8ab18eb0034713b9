// The one declaration of every kernel launcher.  The binding TU (ext.cpp)
// and every .hip TU that defines a launcher include this header, so a
// definition that differs from its declaration is a compile error
// ("conflicting types" for a C function) and not a silent swap of two
// pointers at run time.
//
// Return convention.  A launcher that returns `int` returns 0 after it has
// enqueued its kernels and nonzero when it launched NOTHING (a class, member
// or k count with no instantiation): the outputs are then unwritten and the
// caller must turn that into an error.  A `void` launcher always launches.
// Either way the caller checks the launch itself afterwards
// (hipGetLastError); no launcher synchronises or allocates, so all of them
// capture into a graph.
//
// Shapes are row-major and written as the kernels write them; X, Q, R, SV
// and B are 12-feature rows.  "or null" marks an optional pointer.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

// Kernel-argument block of ensemble_vote_kernel.  Everything a launch needs
// about its members is in here BY VALUE: there is no device-side pointer
// array to fill, so the launch needs no copy and no allocation.
#define ENS_MAX_M 8  // members
#define ENS_MAX_C 8  // classes, of a member and of the ensemble

struct EnsembleArgs {
  const float* p[ENS_MAX_M];                    // [n, cm[m]] f32, 16-B aligned
  float w[ENS_MAX_M];                           // normalised weights
  unsigned char cm[ENS_MAX_M];                  // member class counts
  unsigned char map[ENS_MAX_M * ENS_MAX_C];     // member column -> ensemble column
  int M;
};

// Dynamic LDS of a launch made without hipFuncSetAttribute: the launchers
// below whose LDS grows with a runtime count size their launch with the
// *_lds_bytes function, and the binding rejects a count whose bytes exceed
// this limit with the same function, so the two cannot disagree.
#define MAX_DYNAMIC_LDS_BYTES (64 * 1024)

static inline size_t gnb_predict_lds_bytes(int C) {  // theta, inv_var [C,12]; const [C]
  return (size_t)(2 * C * 12 + C) * sizeof(float);
}
static inline size_t linear_argmax_lds_bytes(int C) {  // W [C,12]; b [C]
  return (size_t)(C * 12 + C) * sizeof(float);
}
static inline size_t kmeans_assign_lds_bytes(int K) {  // f64 sums [K,12], counts [K]; f32 centers [K,12]
  return (size_t)(K * 12 + K) * sizeof(double) + (size_t)(K * 12) * sizeof(float);
}
static inline size_t gnb_fit_stats_lds_bytes(int C) {  // f64 sum, sumsq [C,12]; count [C]
  return (size_t)(2 * C * 12 + C) * sizeof(double);
}

extern "C" {

// --- predict_kernels.hip ---------------------------------------------------
void launch_gnb_predict(const float* X,        // [n,12]
                        const float* theta,    // [C,12]
                        const float* inv_var,  // [C,12]
                        const float* cconst,   // [C]
                        int* out,              // [n]
                        long long n, int C, hipStream_t stream);
void launch_linear_argmax(const float* X,  // [n,12]
                          const float* W,  // [C,12]
                          const float* b,  // [C]
                          int* out,        // [n]
                          long long n, int C, hipStream_t stream);
void launch_kmeans_assign(const float* X,        // [n,12]
                          const float* centers,  // [K,12]
                          int* labels,           // [n]
                          double* counts,        // [K], added to
                          double* sums,          // [K,12], added to
                          double* inertia,       // [1], added to
                          long long n, int K, int want_update,
                          hipStream_t stream);
// nonzero: no kernel for C classes
int launch_rf_predict(const float* X,           // [n,12]
                      const unsigned* nodes,    // [n_nodes,2] packed uint2
                      const unsigned* snodes,   // [n_nodes+2,2] packed uint2
                      const int* roots,         // [T]
                      const float* leaf_proba,  // [n_leaves,C]
                      int* out,                 // [n]
                      long long n, int n_nodes, int n_leaves, int T, int C,
                      hipStream_t stream);
// nonzero: no kernel for this k
int launch_knn_topk(const float* Q,           // [nq,12]
                    const float* R,           // [nr,12]
                    const unsigned char* ry,  // [nr] or null
                    float* out_d,             // [nq,k]
                    int* out_i,               // [nq,k]
                    int* out_lab,             // [nq] or null
                    long long nq, long long nr, int k, int C,
                    long long idx_base, hipStream_t stream);

// --- rf_proba_kernels.hip --------------------------------------------------
// nonzero: C outside 2..8
int launch_rf_scores(const float* X,           // [n,12]
                     const unsigned* nodes,    // [n_nodes,2] packed uint2
                     const int* roots,         // [T]
                     const float* leaf_proba,  // [n_leaves,C]
                     float* proba,             // [n,C] or null
                     int* labels,              // [n]
                     float* conf,              // [n]
                     long long n, int T, int C, hipStream_t stream);

// --- iforest_kernels.hip ---------------------------------------------------
// nonzero: T outside 1..4096, or only one of labels_in and labels_out given
int launch_iforest_score(const float* X,         // [n,12]
                         const unsigned* nodes,  // [n_nodes,2] packed uint2
                         const int* roots,       // [T]
                         const int* labels_in,   // [n] or null
                         float* score,           // [n]
                         double* psum,           // [n] or null
                         int* labels_out,        // [n] or null, with labels_in
                         unsigned char* flags,   // [n]
                         double inv_denom, double depth_cut, long long n, int T,
                         hipStream_t stream);

// --- rf_explain_kernels.hip ------------------------------------------------
// nonzero: C outside 2..8 or T outside 1..4096
int launch_rf_explain(const float* X,         // [n,12]
                      const unsigned* nodes,  // [n_nodes,2] packed uint2
                      const int* roots,       // [T]
                      const int* delta,       // [n_nodes,C]
                      const int* labels,      // [n]
                      float* contrib,         // [n,12] or null, 16-B aligned
                      int* why,               // [n]
                      float* why_value,       // [n]
                      long long* sums,        // [n,12] or null
                      long long n, int T, int C, hipStream_t stream);

// --- ensemble_kernels.hip --------------------------------------------------
// each nonzero for a class or member count out of range
int launch_gnb_proba(const float* X,         // [n,12]
                     const double* theta,    // [C,12]
                     const double* inv_var,  // [C,12]
                     const double* cconst,   // [C]
                     float* proba,           // [n,C]
                     long long n, int C, hipStream_t stream);
int launch_linear_proba(const float* X,  // [n,12]
                        const float* W,  // [C,12]
                        const float* b,  // [C]
                        float* proba,    // [n,C]
                        long long n, int C, hipStream_t stream);
int launch_knn_vote_proba(const int* idx,          // [n,k], entries outside [0,nr) are skipped
                          const unsigned char* y,  // [nr]
                          float* proba,            // [n,C]
                          long long n, int k, long long nr, int C,
                          hipStream_t stream);
int launch_ensemble_vote(const EnsembleArgs* args,  // host pointer, passed on by value
                         float* avg,                // [n,C] or null
                         int* labels,               // [n]
                         float* conf,               // [n]
                         long long n, int C, hipStream_t stream);
int launch_proba_smooth(const float* proba,  // [n,C], 16-B aligned
                        float* state,        // [>=n,C], 16-B aligned, rows < n updated
                        int* held,           // [>=n], rows < n updated
                        const int* n_live,   // [1] or null
                        float a, float margin,
                        int* labels,         // [n]
                        float* conf,         // [n]
                        long long n, int C, hipStream_t stream);

// --- traffic_kernels.hip ---------------------------------------------------
// blocks of the partial kernel for n rows; sizes `partial`
int class_traffic_blocks(long long n);
// nonzero: C outside 2..8 or nb < 1
int launch_class_traffic(const float* X,       // [n,12]
                         const int* labels,    // [n]
                         const float* conf,    // [n] or null
                         const int* n_live,    // [1] or null
                         float min_conf,
                         double* partial,      // [nb,C+1,13]
                         double* totals,       // [C+1,13]
                         long long n, int C, int nb, hipStream_t stream);

// --- top_flows_kernels.hip -------------------------------------------------
// blocks of the partial kernel for n rows; sizes `partial`
int class_top_flows_blocks(long long n);
// nonzero: C outside 2..8, k outside 1..64, col_mask 0 or past bit 11, nb < 1
int launch_class_top_flows(const float* X,               // [n,12]
                           const int* labels,            // [n]
                           const float* conf,            // [n] or null
                           const int* n_live,            // [1] or null
                           float min_conf,
                           unsigned col_mask,            // bit c: column c is in the key
                           unsigned long long* partial,  // [nb,C+1,k]
                           int* rows,                    // [C+1,k]
                           float* keys,                  // [C+1,k]
                           long long n, int C, int k, int nb,
                           hipStream_t stream);

// --- svc_kernels.hip -------------------------------------------------------
// each nonzero for C outside 2..6; npair = C(C-1)/2
int launch_svc_predict(const float* X,                // [n,12]
                       const float* SV,               // [nsv,12]
                       const float* dual,             // [C-1,nsv]
                       const unsigned char* svclass,  // [nsv]
                       const float* intercept,        // [npair]
                       int* out,                      // [n]
                       long long n, int nsv, int C, float gamma,
                       hipStream_t stream);
int launch_svc_decision(const float* X,                // [n,12]
                        const float* SV,               // [nsv,12]
                        const float* dual,             // [C-1,nsv]
                        const unsigned char* svclass,  // [nsv]
                        const float* intercept,        // [npair]
                        double* out,                   // [n,npair]
                        long long n, int nsv, int C, float gamma,
                        hipStream_t stream);
int launch_svc_couple(const double* dec,    // [n,npair]
                      const double* probA,  // [npair]
                      const double* probB,  // [npair]
                      float* proba,         // [n,C]
                      int* idx,             // [n]
                      float* conf,          // [n]
                      long long n, int C, hipStream_t stream);

// --- knn_mfma.hip ----------------------------------------------------------
// k in 1..8, C <= 16, 1 <= S <= ceil(nr / 128)
void launch_knn_mfma(const float* Q,           // [nq,12]
                     const float* R,           // [nr,12]
                     const float* cmean,       // [12]
                     const unsigned char* ry,  // [nr] or null
                     float* part_d,            // [S,nq,k]
                     int* part_i,              // [S,nq,k]
                     float* out_d,             // [nq,k]
                     int* out_i,               // [nq,k]
                     int* out_lab,             // [nq] or null
                     long long nq, long long nr, int S, int k, int C,
                     long long idx_base, int approx, hipStream_t stream);

// --- fit_kernels.hip -------------------------------------------------------
void launch_gnb_fit_stats(const double* X,     // [n,12]
                          const long long* y,  // [n], values in [0,C)
                          double* count,       // [C], added to
                          double* sum,         // [C,12], added to
                          double* sumsq,       // [C,12], added to
                          long long n, int C, hipStream_t stream);
// nonzero: no kernel for C classes
int launch_logistic_grad(const double* X,     // [n,12]
                         const long long* y,  // [n]
                         const double* W,     // [C,12]
                         const double* b,     // [C]
                         double* grad,        // [C,13], added to
                         double* loss,        // [1], added to
                         long long n, int C, hipStream_t stream);
void launch_flow_features(const double* cur,    // [n,4] fp,fb,rp,rb
                          const double* prev,   // [n,4]
                          const double* times,  // [n,6] tfc,tfp,trc,trp,t0,_
                          float* out,           // [n,12]
                          long long n, hipStream_t stream);
// SMO working buffers: sel u64 [2] (WSS-1) or [3] (WSS-2) of key << 32 | row,
// rows f32 [24] = x_i, x_j; sol f64 [4] = yi*dai, yj*daj, status, gap
void launch_smo_select(const float* y,           // [n]
                       const double* alpha,      // [n]
                       const double* grad,       // [n]
                       double C, long long n,
                       unsigned long long* out,  // [2]
                       hipStream_t stream);
void launch_smo_solve(const float* X,           // [n,12], rows sel[0], sel[1] read
                      const float* y,           // [n]
                      double* alpha,            // [n]
                      const double* grad,       // [n]
                      unsigned long long* sel,  // [2]
                      float* rows,              // [24]
                      double* sol,              // [4]
                      double C, double tol, float gamma, hipStream_t stream);
void launch_smo_update_dev(const float* X,     // [n,12]
                           const float* y,     // [n]
                           double* grad,       // [n]
                           const float* rows,  // [24]
                           const double* sol,  // [4]
                           float gamma, long long n, hipStream_t stream);
void launch_smo_update(const float* X,     // [n,12]
                       const float* y,     // [n]
                       double* grad,       // [n]
                       const float* rows,  // [24]
                       double yidai, double yjdaj, float gamma, long long n,
                       hipStream_t stream);
void launch_smo_row(const float* X,                 // [n,12]
                    const unsigned long long* sel,  // [>=1]
                    const double* sol,              // [4]
                    float* krow,                    // [n]
                    float gamma, long long n, hipStream_t stream);
void launch_smo_select2(const float* y,           // [n]
                        const double* alpha,      // [n]
                        const double* grad,       // [n]
                        const float* krow,        // [n]
                        unsigned long long* sel,  // [3]
                        const double* sol,        // [4]
                        double C, long long n, hipStream_t stream);
void launch_smo_solve2(const float* X,           // [n,12], rows sel[0..2] read
                       const float* y,           // [n]
                       double* alpha,            // [n]
                       const double* grad,       // [n]
                       unsigned long long* sel,  // [3]
                       float* rows,              // [24]
                       double* sol,              // [4]
                       double C, double tol, float gamma, hipStream_t stream);
void launch_smo_update_dev2(const float* X,     // [n,12]
                            const float* y,     // [n]
                            double* grad,       // [n]
                            const float* rows,  // [24]
                            const double* sol,  // [4]
                            const float* krow,  // [n]
                            float gamma, long long n, hipStream_t stream);
void launch_rf_hist(const unsigned char* bins,  // [n,12]
                    const unsigned char* y,     // [n], values in [0,C)
                    const int* nid,             // [n], < 0 or a node of hist
                    const unsigned char* fsel,  // [nodes,12] or null
                    unsigned* hist,             // [nodes,12,256,C], added to
                    long long n, int C, hipStream_t stream);
// nonzero: no kernel for C classes
int launch_rf_split(const int* hist,            // [L,12,256,C]
                    const unsigned char* fsel,  // [L,12]
                    unsigned long long* best,   // [L], atomicMin
                    int* cnt,                   // [L,C]
                    int L, int C, hipStream_t stream);
void launch_rf_partition(const unsigned char* B,  // [n,12]
                         int* nid,                // [n], < 0 or an index of lmap
                         const int* lmap,         // [L]
                         const int* feat,         // [L], values in [0,12)
                         const int* binthr,       // [L]
                         long long n, hipStream_t stream);
void launch_rf_hist_compact(const unsigned char* bins,   // [n,12]
                            const unsigned char* y,      // [n], values in [0,C)
                            const int* nid,              // [n], < 0 or a node of hist
                            const unsigned char* frank,  // [L,12], slot < mf or 0xff
                            unsigned* hist,              // [L,mf,256,C], added to
                            long long n, int C, int mf, hipStream_t stream);
// nonzero: no kernel for C classes
int launch_rf_split_compact(const int* hist,            // [L,mf,256,C]
                            const unsigned char* fidx,  // [L,mf]
                            unsigned long long* best,   // [L], atomicMin
                            int* cnt,                   // [L,C]
                            int L, int C, int mf, hipStream_t stream);

}  // extern "C"
