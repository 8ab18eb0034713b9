// CDNA4 predict kernels for the estimators (the
// SVC kernels, N2, are in svc_kernels.hip and follow the same rules).
// Hand-written for gfx950: wave64 blocks, params staged in LDS, feature rows
// as float4 vector loads, grid-stride over rows.  All label outputs use
// first-maximum tie-breaking to match the sklearn semantics of the CPU
// oracles (ops/cpu.py).
//
// Register-pressure rule observed throughout: any per-lane array indexed by
// a RUNTIME value would be spilled to scratch by hipcc, so every such array
// (RF class accumulators, SVC OVO accumulators, KNN k-best lists) is sized
// by a template parameter and only indexed inside fully-unrolled loops; the
// per-row feature vector, whose index IS runtime (tree node feature ids),
// lives in LDS instead.

#include <cstdlib>

#include "common.h"
#include "launchers.h"

// ---------------------------------------------------------------------------
// Gaussian NB: fused joint-log-likelihood + argmax (reference N5).
//   score[c] = const[c] - 0.5 * sum_j (x_j - theta[c,j])^2 * inv_var[c,j]
// Params (C*F*2 + C floats) are broadcast via LDS.
// ---------------------------------------------------------------------------
__global__ void gnb_predict_kernel(const float* __restrict__ X,
                                   const float* __restrict__ theta,
                                   const float* __restrict__ inv_var,
                                   const float* __restrict__ cconst,
                                   int* __restrict__ out,
                                   long long n, int C) {
  constexpr int F = 12;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* s_theta = reinterpret_cast<float*>(smem);
  float* s_ivar = s_theta + C * F;
  float* s_const = s_ivar + C * F;
  for (int i = threadIdx.x; i < C * F; i += blockDim.x) {
    s_theta[i] = theta[i];
    s_ivar[i] = inv_var[i];
  }
  for (int i = threadIdx.x; i < C; i += blockDim.x) s_const[i] = cconst[i];
  __syncthreads();

  long long stride = (long long)gridDim.x * blockDim.x;
  for (long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x; row < n;
       row += stride) {
    Row12 x = load_row12(X, row);
    float best = -INFINITY;
    int bi = 0;
    for (int c = 0; c < C; ++c) {
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < F; ++j) {
        float d = x.v[j] - s_theta[c * F + j];
        s = fmaf(d * d, s_ivar[c * F + j], s);
      }
      s = s_const[c] - 0.5f * s;
      if (s > best) { best = s; bi = c; }
    }
    out[row] = bi;
  }
}

extern "C" void launch_gnb_predict(const float* X, const float* theta,
                                   const float* inv_var, const float* cconst,
                                   int* out, long long n, int C,
                                   hipStream_t stream) {
  const int block = 256;
  hipLaunchKernelGGL(gnb_predict_kernel, dim3(ts_grid(n, block)), dim3(block),
                     gnb_predict_lds_bytes(C), stream, X, theta, inv_var, cconst, out, n, C);
}

// ---------------------------------------------------------------------------
// Linear (logistic) argmax: out = argmax_c (W[c,:] . x + b[c])   (N1 serve)
// ---------------------------------------------------------------------------
__global__ void linear_argmax_kernel(const float* __restrict__ X,
                                     const float* __restrict__ W,
                                     const float* __restrict__ b,
                                     int* __restrict__ out,
                                     long long n, int C) {
  constexpr int F = 12;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* s_w = reinterpret_cast<float*>(smem);
  float* s_b = s_w + C * F;
  for (int i = threadIdx.x; i < C * F; i += blockDim.x) s_w[i] = W[i];
  for (int i = threadIdx.x; i < C; i += blockDim.x) s_b[i] = b[i];
  __syncthreads();

  long long stride = (long long)gridDim.x * blockDim.x;
  for (long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x; row < n;
       row += stride) {
    Row12 x = load_row12(X, row);
    float best = -INFINITY;
    int bi = 0;
    for (int c = 0; c < C; ++c) {
      float s = s_b[c];
#pragma unroll
      for (int j = 0; j < F; ++j) s = fmaf(x.v[j], s_w[c * F + j], s);
      if (s > best) { best = s; bi = c; }
    }
    out[row] = bi;
  }
}

extern "C" void launch_linear_argmax(const float* X, const float* W,
                                     const float* b, int* out, long long n,
                                     int C, hipStream_t stream) {
  const int block = 256;
  hipLaunchKernelGGL(linear_argmax_kernel, dim3(ts_grid(n, block)), dim3(block),
                     linear_argmax_lds_bytes(C), stream, X, W, b, out, n, C);
}

// ---------------------------------------------------------------------------
// KMeans assignment + partial update (N6): label = argmin_k ||x - c_k||^2,
// with per-block LDS partial (count, sum) per cluster flushed by f64 atomics
// (one atomic set per block, guide G12), plus inertia.
// ---------------------------------------------------------------------------
__global__ void kmeans_assign_kernel(const float* __restrict__ X,
                                     const float* __restrict__ centers,
                                     int* __restrict__ labels,
                                     double* __restrict__ counts,   // [K]
                                     double* __restrict__ sums,     // [K,F]
                                     double* __restrict__ inertia,  // [1]
                                     long long n, int K, int want_update) {
  constexpr int F = 12;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* s_sum = reinterpret_cast<double*>(smem);        // [K,F]
  double* s_cnt = s_sum + K * F;                          // [K]
  float* s_c = reinterpret_cast<float*>(s_cnt + K);       // [K,F]
  for (int i = threadIdx.x; i < K * F; i += blockDim.x) {
    s_c[i] = centers[i];
    if (want_update) s_sum[i] = 0.0;
  }
  if (want_update)
    for (int i = threadIdx.x; i < K; i += blockDim.x) s_cnt[i] = 0.0;
  __syncthreads();

  double local_inertia = 0.0;
  long long stride = (long long)gridDim.x * blockDim.x;
  for (long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x; row < n;
       row += stride) {
    Row12 x = load_row12(X, row);
    float best = INFINITY;
    int bi = 0;
    for (int k = 0; k < K; ++k) {
      float d = 0.f;
#pragma unroll
      for (int j = 0; j < F; ++j) {
        float t = x.v[j] - s_c[k * F + j];
        d = fmaf(t, t, d);
      }
      if (d < best) { best = d; bi = k; }
    }
    labels[row] = bi;
    local_inertia += (double)best;
    if (want_update) {
      // LDS atomics: contention limited to the block's 256 lanes
      atomicAdd(&s_cnt[bi], 1.0);
#pragma unroll
      for (int j = 0; j < F; ++j) atomicAdd(&s_sum[bi * F + j], (double)x.v[j]);
    }
  }
  // inertia: wave-reduce then one atomic per wave
  local_inertia = wave_sum(local_inertia);
  if ((threadIdx.x & (WAVE - 1)) == 0) atomicAdd(inertia, local_inertia);
  if (want_update) {
    __syncthreads();
    for (int i = threadIdx.x; i < K * F; i += blockDim.x)
      atomicAdd(&sums[i], s_sum[i]);
    for (int i = threadIdx.x; i < K; i += blockDim.x)
      atomicAdd(&counts[i], s_cnt[i]);
  }
}

extern "C" void launch_kmeans_assign(const float* X, const float* centers,
                                     int* labels, double* counts, double* sums,
                                     double* inertia, long long n, int K,
                                     int want_update, hipStream_t stream) {
  const int block = 256;
  hipLaunchKernelGGL(kmeans_assign_kernel, dim3(ts_grid(n, block)), dim3(block),
                     kmeans_assign_lds_bytes(K), stream, X, centers, labels, counts, sums, inertia, n,
                     K, want_update);
}

// ---------------------------------------------------------------------------
// Random forest traversal + vote (N4) — the flagship predict kernel.
// Packed node = uint2 { x: f32 threshold bits | leaf-prob row index,
//                       y: (right_child_global << 8) | feature (0xff = leaf) }
// Design (profiled on MI355X): the traversal is a dependent chain of node
// fetches, so occupancy is the lever.  Only the packed forest lives in LDS
// (shared by the whole block); the per-lane feature row stays in REGISTERS
// and the runtime feature index is resolved with an 11-op cndmask select
// tree (compile-time indices, ~8 cycles — far shorter than an LDS
// round-trip and no scratch spill).  512-thread blocks with nodes-only LDS
// give 3 blocks = 24 waves per CU.
// ---------------------------------------------------------------------------

// Traversal body shared by the four table-placement variants.  LDS_NODES /
// LDS_PROBS are compile-time so the node fetch lowers to ds_read_b64 (LDS)
// or global_load_dwordx2 — a runtime ternary over the two pointers would
// force generic/flat addressing (measured: LDS instr count collapses and
// VALU doubles on 64-bit flat address math).
//
// Leaf encoding: most leaves of a fully-grown forest are PURE (one-hot
// distribution).  A pure leaf carries its class in the feature byte
// (0xf0|class) and is counted with one shift+add into a packed u64 vote
// register (10 bits per class, forests up to 1023 trees) — no memory read
// at all.  Only mixed leaves (feature byte 0xff) touch the probability
// table.
template <int C, bool LDS_NODES, bool LDS_PROBS, bool LDS_FEAT>
__launch_bounds__(512, 1)
__global__ void rf_predict_kernel(const float* __restrict__ X,
                                  const uint2* __restrict__ nodes,
                                  const int* __restrict__ roots,  // [T]
                                  const float* __restrict__ leaf_proba,
                                  int* __restrict__ out,
                                  long long n, int n_nodes, int n_leaves,
                                  int T) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint2* s_nodes = reinterpret_cast<uint2*>(smem);
  float* s_probs = reinterpret_cast<float*>(s_nodes + (LDS_NODES ? n_nodes : 0));
  // LDS_FEAT: each thread's 12 features live in LDS at pitch 13 and the
  // per-node runtime feature pick is ONE ds_read_b32 instead of sel12's
  // ~10-op register select tree — trading idle LDS-pipe cycles for the VALU
  // issue slots this kernel is bound on (VALUBusy 99.2%).  Pitch 13
  // (gcd(13,32) = 1) puts the 32 lanes of a group on distinct banks only
  // while they read the same feature; lanes at different depths of a tree
  // do not, so the read does pay bank conflicts.  The feature-major rows of
  // the streaming kernel below avoid them; here, with the node table in
  // L2, they measured level (profiles/rf_predict_stream2.md) and the layout
  // stayed.
  float* s_feat = s_probs + (LDS_PROBS ? n_leaves * C : 0);

  if (LDS_NODES)
    for (int i = threadIdx.x; i < n_nodes; i += blockDim.x) s_nodes[i] = nodes[i];
  if (LDS_PROBS)
    for (int i = threadIdx.x; i < n_leaves * C; i += blockDim.x)
      s_probs[i] = leaf_proba[i];
  if (LDS_NODES || LDS_PROBS) __syncthreads();
  float* my_feat = s_feat + (int)threadIdx.x * 13;

  long long stride = (long long)gridDim.x * blockDim.x;
  for (long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x; row < n;
       row += stride) {
    Row12 x = load_row12(X, row);
    if (LDS_FEAT) {
#pragma unroll
      for (int j = 0; j < 12; ++j) my_feat[j] = x.v[j];
    }
    float acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.f;
    unsigned long long votes = 0ull;  // 10-bit packed per-class pure counts
    int decided = 0;
    for (int t = 0; t < T; ++t) {
      if (!decided) {
        int idx = roots[t];
        while (true) {
          uint2 node = LDS_NODES ? s_nodes[idx] : nodes[idx];
          unsigned feat = node.y & 0xffu;
          if (feat >= 0xf0u) {
            if (feat == 0xffu) {  // mixed leaf: read the distribution
              int pr = (int)node.x * C;
#pragma unroll
              for (int c = 0; c < C; ++c)
                acc[c] += LDS_PROBS ? s_probs[pr + c] : leaf_proba[pr + c];
            } else {  // pure leaf: class in the low nibble
              votes += 1ull << ((feat & 0xfu) * 10);
            }
            break;
          }
          float thr = __uint_as_float(node.x);
          float fv = LDS_FEAT ? my_feat[feat] : sel12(x, feat);
          idx = (fv <= thr) ? idx + 1 : (int)(node.y >> 8);
        }
      }
      // EXACT early majority exit: each remaining tree adds at most 1.0 to
      // any class score, so once leader - runner-up > trees left the argmax
      // is decided.  The kernel is VALU-bound and most rows of an accurate
      // forest are near-unanimous, so whole waves retire around tree T/2.
      if ((t & 7) == 7) {
        if (!decided) {
          float m1 = -INFINITY, m2 = -INFINITY;
#pragma unroll
          for (int c = 0; c < C; ++c) {
            float sc = acc[c] + vote_count(votes, c);
            if (sc > m1) { m2 = m1; m1 = sc; }
            else if (sc > m2) m2 = sc;
          }
          if (m1 - m2 > (float)(T - 1 - t)) decided = 1;
        }
        if (__all(decided)) break;  // work only stops wave-uniformly
      }
    }
    float best = -INFINITY;
    int bi = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      float sc = acc[c] + vote_count(votes, c);
      if (sc > best) { best = sc; bi = c; }
    }
    out[row] = bi;
  }
}

// Streaming variant (modes 4, 5 and 6; the large-batch default): a LANE, not
// a wave, is the unit that advances through trees and rows.  The row-per-lane
// kernel above reconverges after every tree and leaves together, so a wave
// pays the deepest path of its 64 lanes in every tree and the slowest row's
// exit: 765 node visits per row where the row itself needs 322
// (profiles/rf_predict_stream.md).  Here each lane carries
// (row, t, idx, acc, votes) and one loop iteration is one node visit for
// every lane, with no exec masking and no per-lane bookkeeping in it:
//
//  * It walks rf_pack's STREAM table (layout there).  A leaf's link is the
//    next tree's root, so a lane steps from leaf to root with no roots[]
//    load; a leaf "goes right" because it reads slot 12 of the lane's
//    13-slot LDS row, which holds NaN.
//  * The LDS rows are FEATURE-MAJOR: slot j of thread tid is
//    s_feat[j * blockDim.x + tid].  Every lane is at a node of its own and
//    asks for a feature of its own, and in this layout the bank is
//    tid mod 32 whatever j is, so the read (and the 12 stores of a refill)
//    never conflict.  One row per thread at pitch 13, the earlier layout,
//    is conflict-free only when all lanes read the same slot.
//  * The leaf byte carries the vote shift, so the pure-leaf count is one
//    shift and one add; mixed leaves (rare) read their row under a branch.
//  * The majority test belongs to whole trees (t & 7 == 7, once it can
//    succeed, and the last tree), so rf_pack flags those trees' leaves.  A
//    lane that meets a flagged leaf parks on the PARK node, which links to
//    itself, and remembers where to resume.  The wave serves its parked
//    lanes together, in one PASS, once `pass_min` of them wait (or nothing
//    else runs): majority test, label store for the rows that are decided,
//    and the idle lanes take the next rows of the wave's range in lane
//    order.  Per-row cost of the test and the refill is thus shared by many
//    lanes, which matters because the kernel is bound by instruction issue.
//
// COMPACT (modes 5 and 6 whenever the launcher's rule admits it): the host
// format is made for reading by tests and by the L2 walk; the LDS copy is
// made for the walk alone.  Every block stages the table once, a handful of
// nodes per thread, and a row visits about 322 nodes, so whatever can be
// decided per NODE is decided in the staging loop and stored:
//
//    word 1 = link << 16 | slot << 12 | byte        word 0, inner = threshold
//    word 0, leaf = next root << 16 | (row of the distribution + 1, or 0)
//
//  * link, next root, idx, resume and park are LDS BYTE ADDRESSES of nodes:
//    the node read takes idx as it stands, the left child is idx + 8, and
//    the link is the high half of word 1, which the select can take by
//    itself (SDWA WORD_1; when the compiler does not fold it, one shift).
//  * slot << 12 is the byte offset of a feature-major slot in a 1024-thread
//    block: the feature address is one `and` and one add of the lane's base.
//  * byte: an inner node has 60; a leaf 0x80 | mixed << 6 | shift.  Every
//    visit adds 1 << shift to the vote register, where bits 60..63 belong to
//    no class and may overflow, and t counts byte >= 0x80 by a carry-in: no
//    branch around the pair.  byte >= 0xc0 is a mixed leaf.
//  * A flagged leaf links to PARK, so the step is idx = next with no select,
//    and keeps its real link as the next root in word 0; only
//    resume = flagged ? (this leaf) : resume remains, and the pass reads the
//    root back from the leaf (16 bits at resume + 2).  "Flagged" is one
//    compare of word 1 as a whole: a leaf that links to PARK is the largest
//    link over the largest slot with a byte of 0x80 or more.  The terminal
//    entry n_nodes keeps itself as its next root; target >= its address
//    ends a row.
//  * The clamps live in the staging loop: a link past the table becomes
//    PARK, a feature byte above 12 becomes slot 12, a mixed leaf's row is
//    at most n_leaves - 1, and the two sentinels are written as they must be
//    whatever the table holds in their place.  The walk has no `min`.  So
//    for ANY table every idx is the address of one of the n_nodes + 2
//    entries, every slot one of the lane's 13 and every row one of
//    leaf_proba's: nothing outside them is read.  (A leaf without a flag
//    whose link was clamped to PARK counts as flagged and ends its row.)
//
// Loop control is one scalar counter (`pending`, at its declaration): a run
// of steps between two passes is a do-while with one compare and one branch.
// The steps of the run are what the counter holds beyond the slots that
// parked, and those are the slots the pass serves: a slot has a live
// `resume` only from a flagged leaf of this run, because every pass resets
// it, for the rows that go on as well as for those that end.
//
// Termination: in a table rf_pack accepted every link points forward, so a
// running lane reaches a flagged leaf within n_nodes steps and a pass
// follows; the wave leaves when its range is used up and every lane is
// idle.  Some lane runs in every step and a row's path is shorter than
// n_nodes + 2, so a wave needs fewer than rows x (n_nodes + 2) steps.  For
// any other table `pending` forces a pass after at most slots << kshift
// steps; every pass takes the steps of the run before it off `budget`,
// which starts at that product, and the wave gives up when it is spent.
// No table makes that count come out short: a pass serves at most the
// slots that added their 1 << kshift in the run (more can have added: a
// malformed PARK entry, a link clamped onto it), and the difference is
// taken saturating, at least 1.  So whatever the table holds a wave makes
// fewer than rows x (n_nodes + 2) + (slots << kshift) steps.
//
// Per row the arithmetic is the row-per-lane kernel's: trees in index
// order, mixed leaves added to acc in that order, the majority test after
// the same trees, first-maximum argmax — labels do not depend on which lane
// ran a row or when.
//
// R rows per lane (mode 6: R = 2, LDS node table only).  One block per CU
// is all the LDS admits and a block is at most 16 waves, so further
// independent chains have to come from inside the lane: a lane carries R
// SLOTS, each with the full per-row state above and a feature row of its own
// (slot s, feature j at s_feat[(s * 13 + j) * blockDim.x + tid]).  An
// iteration issues the R node reads, then the R feature reads, then does
// the R updates, so the two LDS latencies of a visit overlap across slots
// and the loop's scalar work (branch, ballots, counter) is shared by R
// visits.  A pass serves slot 0 and then slot 1, the cursor running on from
// one to the other; `pending`, `pass_min` and the exit condition count
// slots, R x 64 per wave.  In every iteration some slot advances, so the
// iteration bound is unchanged.
#define RF_LDS __attribute__((address_space(3)))

// LDS byte address of a pointer into the block's shared memory.
__device__ __forceinline__ unsigned rf_lds_addr(const void* p) {
  return (unsigned)(size_t)(RF_LDS const char*)p;
}

// Load from an LDS byte address held in a register: the address is the
// ds_read's operand as it stands, with no base to add.
template <typename T>
__device__ __forceinline__ T rf_lds_load(unsigned addr) {
  return *(RF_LDS const T*)(size_t)addr;
}
__device__ __forceinline__ uint2 rf_lds_load_node(unsigned addr) {  // one ds_read_b64
  typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
  const u32x2 v = rf_lds_load<u32x2>(addr);
  return make_uint2(v.x, v.y);
}

template <int C, bool LDS_NODES, int R, bool COMPACT>
__launch_bounds__(LDS_NODES ? 1024 : 256)
__global__ void rf_predict_stream_kernel(const float* __restrict__ X,
                                         const uint2* __restrict__ snodes,
                                         const float* __restrict__ leaf_proba,
                                         int* __restrict__ out, long long n,
                                         int rows_per_wave, int n_nodes,
                                         int n_leaves, int T, int pass_min) {
  static_assert(R == 1 || (R == 2 && LDS_NODES), "two rows per lane need the LDS table");
  static_assert(!COMPACT || LDS_NODES, "the compact form is made while staging into LDS");
  constexpr int BLOCK = LDS_NODES ? 1024 : 256;  // the launcher's block size
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint2* s_nodes = reinterpret_cast<uint2*>(smem);
  // slot j of this thread's row s: my_feat[(s * 13 + j) * BLOCK]
  float* my_feat = reinterpret_cast<float*>(s_nodes + (LDS_NODES ? n_nodes + 2 : 0)) +
                   (int)threadIdx.x;
#pragma unroll
  for (int s = 0; s < R; ++s)  // NaN: leaves compare false
    my_feat[(s * 13 + 12) * BLOCK] = __uint_as_float(0x7fc00000u);
  // What idx, resume and park hold: a node's index, or (COMPACT) its LDS byte
  // address.  node0 is node 0, `step` the way to the left child, `fin` the
  // terminal entry n_nodes and `park` the PARK entry.
  // COMPACT keeps addresses in 16 bits, and the launcher's rule
  // ((n_nodes + 2) * 8 <= 65536) counts from LDS address 0: this kernel has
  // no static __shared__ object, so its dynamic segment, and node 0, start
  // there.  Give it one and that rule has to shrink by its size.
  const unsigned node0 = COMPACT ? rf_lds_addr(s_nodes) : 0u;
  constexpr unsigned step = COMPACT ? 8u : 1u;
  const unsigned fin = node0 + (unsigned)n_nodes * step;
  const unsigned park = fin + step;
  // COMPACT: word 1 of a leaf that links to PARK, and of nothing else, is at
  // least this (PARK's own byte is below 0x80)
  const unsigned flag_min = park << 16 | 12u << 12 | 0x80u;
  if (LDS_NODES) {
    for (int i = threadIdx.x; i < n_nodes + 2; i += blockDim.x) {
      uint2 nd = snodes[i];
      if (COMPACT) {
        // Re-encode (COMPACT, above).  Every clamp of the walk is made
        // here, once per node, so that the walk itself needs none.
        const unsigned byte = nd.y & 0xffu;
        const unsigned to = node0 + min(nd.y >> 8, (unsigned)n_nodes + 1u) * 8u;
        const bool leaf = byte >= 0x80u, flagged = byte >= 0xc0u;
        unsigned low = 60u;  // inner node: slot 0..12 | shift 60
        if (leaf) {
          // the launcher starts this kernel only with 1 <= n_leaves < 65535,
          // so row1 is at most n_leaves and fits the low half
          const unsigned row1 = nd.x ? min(nd.x - 1u, (unsigned)(n_leaves - 1)) + 1u : 0u;
          nd.x = to << 16 | row1;
          low = 0x80u | (row1 ? 0x40u : 0u) | (byte & 63u);
        }
        nd.y = (flagged ? park : to) << 16 | min(byte, 12u) << 12 | low;
        // the two sentinels are made here, whatever the table holds there
        if (i == n_nodes) nd = make_uint2(fin << 16, park << 16 | 12u << 12 | 0x80u | 60u);
        if (i == n_nodes + 1) nd = make_uint2(0u, park << 16 | 12u << 12 | 60u);
      }
      s_nodes[i] = nd;
    }
    __syncthreads();
  }

  const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long begin =
      ((long long)blockIdx.x * (BLOCK >> 6) + wave_in_block) * rows_per_wave;
  const long long left = n - begin;
  // The range is the same for all lanes; readfirstlane says so to the
  // compiler, which otherwise does the 64-bit product above in vector
  // registers and with it everything that follows from `count`: cursor,
  // budget, waiting and trigger, and every branch of the loop on them.
  const int count = __builtin_amdgcn_readfirstlane(
      left < (long long)rows_per_wave ? (int)(left > 0 ? left : 0) : rows_per_wave);
  if (count <= 0) return;  // wave-uniform
  const float* __restrict__ Xw = X + begin * 12;
  int* __restrict__ outw = out + begin;
  const unsigned feat0 = rf_lds_addr(my_feat);  // COMPACT: this lane's slot 0, row 0

  // wave-uniform
  int cursor = 0;  // next unassigned row of the range
  // One counter ends a run of steps: every slot that parks at a flagged leaf
  // adds 1 << kshift to it and every step adds 1, and the pass is due at
  // `due` = (parked slots wanted) << kshift.  1 << kshift exceeds the
  // n_nodes + 2 steps within which every running slot of a table rf_pack
  // made has parked, so there the steps never bring a pass forward; with
  // any other table they force one, which is harmless (a pass serves
  // whoever waits) and is where `budget` is looked at.
  const int kshift = min(32 - __clz(n_nodes + 2), 23);
  unsigned pending = 0, due = 0;
  long long budget = (long long)count * (n_nodes + 2);
  // per slot; every slot starts idle: parked with nothing to resume
  unsigned idx[R], resume[R];
  int row[R], t[R];
  float acc[R][C];
  unsigned long long votes[R];  // 10-bit packed per-class pure counts
#pragma unroll
  for (int s = 0; s < R; ++s) {
    idx[s] = park;
    resume[s] = park;
    row[s] = 0;
    t[s] = 0;
    votes[s] = 0ull;
#pragma unroll
    for (int c = 0; c < C; ++c) acc[s][c] = 0.f;
  }

  while (true) {
    {  // PASS: serve the parked slots, slot by slot
      int nidle_all = 0, served = 0;
#pragma unroll
      for (int s = 0; s < R; ++s) {
        const bool waits = idx[s] == park && resume[s] != park;  // at a flagged leaf
        served += __popcll(__ballot(waits));
        if (waits) {
          float m1 = -INFINITY, m2 = -INFINITY;
          int bi = 0;
#pragma unroll
          for (int c = 0; c < C; ++c) {
            // same values as the row-per-lane kernel's if/else-if, as selects
            const float sc = acc[s][c] + vote_count(votes[s], c);
            const bool lead = sc > m1;
            m2 = lead ? m1 : (sc > m2 ? sc : m2);
            m1 = lead ? sc : m1;
            bi = lead ? c : bi;
          }
          // where the row goes on: the next tree's root, which the compact
          // form keeps in the leaf the slot parked on
          const unsigned target =
              COMPACT ? rf_lds_load<unsigned short>(resume[s] + 2u) : resume[s];
          // t trees are done, T - t are left; a link to n_nodes ends the row
          if (target >= fin || m1 - m2 > (float)(T - t[s])) {
            outw[row[s]] = bi;  // idx stays on PARK: idle
          } else {
            idx[s] = target;
          }
          resume[s] = park;  // live only from a flagged leaf to the pass after it
        }
        const unsigned long long idle = __ballot(idx[s] == park);
        int nidle = __popcll(idle);
        if (cursor < count) {
          // idle lanes take rows cursor, cursor+1, ... in lane order
          const int r = cursor + (int)__builtin_amdgcn_mbcnt_hi(
                                     (unsigned)(idle >> 32),
                                     __builtin_amdgcn_mbcnt_lo((unsigned)idle, 0u));
          if (idx[s] == park && r < count) {
            Row12 x = load_row12(Xw, r);
#pragma unroll
            for (int j = 0; j < 12; ++j) my_feat[(s * 13 + j) * BLOCK] = x.v[j];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[s][c] = 0.f;
            votes[s] = 0ull;
            row[s] = r;
            t[s] = 0;
            idx[s] = node0;
          }
          const int take = min(nidle, count - cursor);
          cursor += take;
          nidle -= take;
        }
        nidle_all += nidle;
      }
      if (nidle_all == R * WAVE) break;  // range used up and every slot idle
      // The steps of the run before this pass: `pending` less what the
      // slots served here added.  Only a slot that met a flagged leaf in
      // that run has a live resume (it is reset below, and the leaf added
      // 1 << kshift then), so served << kshift never exceeds what was
      // added; should it ever, the run still costs 1.
      const unsigned added = (unsigned)served << kshift;
      budget -= pending > added ? pending - added : 1u;
      if (budget < 0) break;  // not a table rf_pack made
      // slots still idle stay so; the next pass is due when pass_min slots
      // wait, or all that still run
      due = (unsigned)min(pass_min, R * WAVE - nidle_all) << kshift;
      pending = 0;
    }
    do {
      // one visit per slot: all node reads, then all feature reads, then the
      // updates, so the slots' LDS latencies overlap
      uint2 node[R];
      unsigned byte[R];
      float fv[R];
      int parked = 0;
#pragma unroll
      for (int s = 0; s < R; ++s)
        node[s] = COMPACT ? rf_lds_load_node(idx[s])
                          : LDS_NODES ? s_nodes[idx[s]] : snodes[idx[s]];
#pragma unroll
      for (int s = 0; s < R; ++s) {
        byte[s] = node[s].y & 0xffu;
        fv[s] = COMPACT ? rf_lds_load<float>((node[s].y & 0xf000u) + feat0 +
                                             (unsigned)(s * 13 * BLOCK * 4))
                        : my_feat[(s * 13 + (int)min(byte[s], 12u)) * BLOCK];
      }
      // COMPACT: a mixed leaf (byte 0xc0 and up) adds the distribution whose
      // row + 1, clamped while staging, is the low half of word 0
      auto add_mixed = [&](int s) {
        if (byte[s] >= 0xc0u) {
          const int pr = (int)((node[s].x & 0xffffu) - 1u) * C;
#pragma unroll
          for (int c = 0; c < C; ++c) acc[s][c] += leaf_proba[pr + c];
        }
      };
      if (COMPACT && R > 1) {
        // mixed leaves are rare: one scalar branch skips both slots' masked
        // regions when no lane is at one (measured: 7 % of mode 6's time).
        // With one slot the region's own skip is that branch already.
        bool mixed = false;
#pragma unroll
        for (int s = 0; s < R; ++s) mixed |= byte[s] >= 0xc0u;
        if (__any(mixed)) {
#pragma unroll
          for (int s = 0; s < R; ++s) add_mixed(s);
        }
      }
#pragma unroll
      for (int s = 0; s < R; ++s) {
        const bool left = fv[s] <= __uint_as_float(node[s].x);
        unsigned next = left ? idx[s] + step : node[s].y >> (COMPACT ? 16 : 8);
        if (!COMPACT) next = min(next, park);
        if (COMPACT) {
          // every node counts: an inner node's shift is 60, into the bits of
          // the vote register that belong to no class
          votes[s] += 1ull << (byte[s] & 63u);
          t[s] += byte[s] >= 0x80u;
          if (R == 1) add_mixed(s);
        } else if (byte[s] >= 0x80u) {  // leaf (some lane is at one nearly every step)
          votes[s] += 1ull << (byte[s] & 63u);
          ++t[s];
          if (node[s].x != 0u) {  // mixed leaf: row + 1 of its distribution
            const int pr = (int)min(node[s].x - 1u, (unsigned)(n_leaves - 1)) * C;
#pragma unroll
            for (int c = 0; c < C; ++c) acc[s][c] += leaf_proba[pr + c];
          }
        }
        // leaf of a tree the test follows
        const bool flagged = COMPACT ? node[s].y >= flag_min : byte[s] >= 0xc0u;
        parked += __popcll(__ballot(flagged));
        if (COMPACT) {  // a flagged leaf links to PARK: remember the leaf
          resume[s] = flagged ? idx[s] : resume[s];
          idx[s] = next;
        } else {
          resume[s] = flagged ? next : resume[s];
          idx[s] = flagged ? park : next;
        }
      }
      pending += ((unsigned)parked << kshift) + 1u;
    } while (pending < due);
  }
}

#undef RF_LDS

// Small-batch variant: ONE WAVE PER ROW, trees split across lanes.  At
// serve batch sizes the row-per-lane kernel runs a ~900-step serial
// dependent-load chain per row on a mostly idle chip; here each lane walks
// only ceil(T/64) trees and n waves fill the SIMDs.  The walk and the
// reduction are rf_wave_scores (common.h), shared with rf_scores_wave_kernel.
template <int C>
__launch_bounds__(256) __global__ void rf_predict_wave_kernel(
    const float* __restrict__ X, const uint2* __restrict__ nodes,
    const int* __restrict__ roots, const float* __restrict__ leaf_proba,
    int* __restrict__ out, long long n, int T) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long long row = (long long)blockIdx.x * (blockDim.x / WAVE) +
                        (threadIdx.x >> 6);
  if (row >= n) return;
  float sc[C];
  rf_wave_scores<C>(X, row, lane, nodes, roots, leaf_proba, T, sc);
  if (lane == 0) out[row] = first_max<C>(sc).idx;
}

// Below RF_STREAM_MIN_ROWS rows the default stays with the row-per-lane
// kernel: the streaming kernel runs one 1024-thread block per CU, each
// stages the node table, and a wave wants many rows to refill from.  With
// two rows per lane a wave wants twice as many, so mode 6 takes over from
// mode 5 at RF_STREAM2_MIN_ROWS.  Measured on the reference forest, ms per
// call for modes 2 / 5 / 6 (profiles/rf_predict_compact.md): 140k rows
// 0.165 / 0.099 / 0.164, 500k 0.216 / 0.167 / 0.170, 1M 0.413 / 0.276 /
// 0.292, 1.5M 0.600 / 0.376 / 0.382, 2M 0.793 / 0.481 / 0.469, 10M 3.78 /
// 2.10 / 1.83.  With the compact table mode 5 is ahead of mode 2 at every
// size measured, down to 140k rows, just above the wave-per-row cutover
// (131 072 rows and below); nothing was measured between the two, and the
// 140k value rests on that one point, 0.099 against 0.165 ms.
#define RF_STREAM_MIN_ROWS 140000
#define RF_STREAM2_MIN_ROWS 1500000
// Mode 6's parked slots (of 128 per wave) that start a pass: 24 and 32 are
// level, 16 and 48 behind (same profile).  Mode 5 (of 64): 16.
#define RF_STREAM_REFILL2 32

// The streaming kernel's LDS-table variants need more dynamic LDS than the
// default limit: raised once per instantiation (C, rows per lane).
template <int C, int R, bool COMPACT>
static void rf_stream_allow_lds() {
  static const hipError_t once = hipFuncSetAttribute(
      reinterpret_cast<const void*>(&rf_predict_stream_kernel<C, true, R, COMPACT>),
      hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  (void)once;
}

// Returns 0, or nonzero when no kernel exists for C classes (nothing is
// launched and the output stays unwritten: the caller must turn that into
// an error).
extern "C" int launch_rf_predict(const float* X, const unsigned* nodes,
                                 const unsigned* snodes, const int* roots,
                                 const float* leaf_proba,
                                 int* out, long long n, int n_nodes,
                                 int n_leaves, int T, int C,
                                 hipStream_t stream) {
  // TCSDN_RF_MODE (read per launch) picks the large-batch kernel:
  //   6  streaming kernel (lanes advance through trees and rows on their
  //      own), node table staged in LDS, 1024-thread blocks, TWO rows per
  //      lane; needs the table and two sets of feature rows in LDS, else it
  //      runs as mode 5
  //   5  the same with one row per lane; a table too big for LDS runs as
  //      mode 4
  //   4  streaming kernel, node table in L2, 256-thread blocks
  //   2  row-per-lane, features in LDS (pitch 13, one ds_read per node),
  //      node table in L2 — the default between the wave-per-row cutover
  //      and RF_STREAM_MIN_ROWS, and for forests too big for mode 5
  //   1  row-per-lane, features and nodes both in LDS (costs a block of
  //      occupancy next to a big forest)
  //   0  row-per-lane, features in registers (sel12 select tree), nodes in
  //      LDS when they fit
  // THE DEFAULT is mode 6 from RF_STREAM2_MIN_ROWS rows up and mode 5 from
  // RF_STREAM_MIN_ROWS up, each when its tables fit in LDS (mode 6 falls
  // back to 5, mode 5 to 2), and mode 2 below.
  // Set explicitly, 4, 5 and 6 apply at every n (how the tests reach the
  // streaming kernel with small inputs); 0..2 only above the cutover.
  // Measured on the 100-tree reference forest, 10M rows: modes 0/1/2 =
  // 2.09/2.12/2.60 Gflows/s (profiles/kernel_opt_r02.md), modes 4/5 against
  // mode 2 in profiles/rf_predict_stream.md, the feature-major rows and
  // mode 6 in profiles/rf_predict_stream2.md, the compact LDS table of
  // modes 5 and 6 in profiles/rf_predict_compact.md.
  const size_t snode_bytes = (size_t)(n_nodes + 2) * sizeof(uint2);
  const size_t feat_set = 1024 * 13 * sizeof(float);  // one row per thread of a block
  const bool snodes_fit = snode_bytes + feat_set <= 160 * 1024;
  const bool snodes_fit2 = snode_bytes + 2 * feat_set <= 160 * 1024;
  const char* mode_env = getenv("TCSDN_RF_MODE");
  int mode = mode_env ? atoi(mode_env)
             : n >= RF_STREAM2_MIN_ROWS && snodes_fit2 ? 6
             : n >= RF_STREAM_MIN_ROWS && snodes_fit ? 5 : 2;
  const bool force_stream = mode_env && (mode == 4 || mode == 5 || mode == 6);
  const uint2* nd = reinterpret_cast<const uint2*>(nodes);
  const uint2* snd = reinterpret_cast<const uint2*>(snodes);
  if (n <= 131072 && !force_stream) {  // wave-per-row fills the chip at serve batch sizes
    dim3 wgrid((unsigned)((n + 3) / 4));
    if (dispatch_int<2, 3, 4, 5, 6, 7, 8>(C, [&](auto c) {
          hipLaunchKernelGGL((rf_predict_wave_kernel<decltype(c)::value>), wgrid,
                             dim3(256), 0, stream, X, nd, roots, leaf_proba, out,
                             n, T);
        }))
      return 0;
    // 12 and 16 classes have no wave kernel: the row-per-lane kernel below
    // takes them at every n
  }
  if (mode >= 4 && mode <= 6 && n > 0 && n_nodes > 0 && n_leaves > 0 && T > 0) {
    // One row range per resident wave: the drain tail, the last rows of a
    // range running on a thinning wave, is then about one row in ~19 at
    // 10M rows.  Below one row per slot of a wave (64, or 128 with two rows
    // per lane) there is nothing to refill, so small batches get fewer
    // waves instead.
    // TCSDN_RF_STREAM_RANGE overrides the rows per wave, and
    // TCSDN_RF_STREAM_REFILL the count of parked slots that starts a pass.
    // Modes 5 and 6 stage the node table in LDS beside the feature rows
    // (one 1024-thread block per CU); a table too big for two sets of rows
    // runs as mode 5, one too big for that as mode 4.
    // The LDS-table kernels walk the COMPACT node form (comment above the
    // kernel) when its 16-bit fields hold the table: every node's LDS byte
    // address, so (n_nodes + 2) * 8 <= 65536, i.e. up to 8190 nodes, and a
    // mixed leaf's row + 1, so n_leaves + 1 < 65536.  A table that fits two
    // sets of rows has at most 7166 nodes, so two rows per lane exist in the
    // compact form only (more leaf rows than that run as mode 5); with one
    // row per lane a table of 8191 to 13 822 nodes walks the host format.
    const bool compact = snode_bytes <= 65536 && n_leaves + 1 < 65536;
    const bool two_rows = mode == 6 && snodes_fit2 && compact;
    const bool lds_nodes = mode != 4 && snodes_fit;
    const int slots = two_rows ? 2 * WAVE : WAVE;  // per wave
    const int sb = lds_nodes ? 1024 : 256;
    const long long resident = 256ll * (lds_nodes ? 16 : 32);
    long long range = (n + resident - 1) / resident;
    if (const char* e = getenv("TCSDN_RF_STREAM_RANGE")) range = atoll(e);
    if (range < slots) range = slots;
    if (range > (1ll << 30)) range = 1ll << 30;
    int refill = two_rows ? RF_STREAM_REFILL2 : 16;
    if (const char* e = getenv("TCSDN_RF_STREAM_REFILL")) refill = atoi(e);
    if (refill < 1) refill = 1;
    if (refill > slots) refill = slots;
    const long long waves = (n + range - 1) / range;
    dim3 sgrid((unsigned)((waves + sb / WAVE - 1) / (sb / WAVE)));
    size_t slds = (two_rows ? 2 * feat_set : (size_t)sb * 13 * sizeof(float)) +
                  (lds_nodes ? snode_bytes : 0);
    return !dispatch_int<2, 3, 4, 5, 6, 7, 8, 12, 16>(C, [&](auto c) {
      constexpr int CV = decltype(c)::value;
      auto* kernel = rf_predict_stream_kernel<CV, false, 1, false>;
      if (two_rows) {  // compact always: the table is at most 7166 nodes
        rf_stream_allow_lds<CV, 2, true>();
        kernel = rf_predict_stream_kernel<CV, true, 2, true>;
      } else if (lds_nodes && compact) {
        rf_stream_allow_lds<CV, 1, true>();
        kernel = rf_predict_stream_kernel<CV, true, 1, true>;
      } else if (lds_nodes) {
        rf_stream_allow_lds<CV, 1, false>();
        kernel = rf_predict_stream_kernel<CV, true, 1, false>;
      }
      hipLaunchKernelGGL(kernel, sgrid, dim3(sb), slds, stream, X, snd,
                         leaf_proba, out, n, (int)range, n_nodes, n_leaves, T,
                         refill);
    });
  }
  if (mode < 0 || mode > 2) mode = 2;
  const int block = 512;
  // Occupancy first: with nodes-only LDS a 43 KB forest admits 3 blocks
  // (24 waves) per CU.  Leaf probabilities go to LDS only when everything
  // still fits the 3-block budget; big forests fall back to the
  // (L2-resident) global tables.
  size_t node_bytes = (size_t)n_nodes * sizeof(uint2);
  size_t prob_bytes = (size_t)n_leaves * C * sizeof(float);
  size_t feat_bytes = (size_t)block * 13 * sizeof(float);
  size_t budget = 52 * 1024;  // 3 blocks/CU floor
  bool lds_feat = mode != 0;
  bool lds_nodes = mode != 2 && node_bytes + (lds_feat ? feat_bytes : 0) <=
                                    (mode == 1 ? (size_t)76 * 1024 : budget);
  bool lds_probs = lds_nodes && !lds_feat && (node_bytes + prob_bytes) <= budget;
  size_t lds = (lds_nodes ? node_bytes : 0) + (lds_probs ? prob_bytes : 0) +
               (lds_feat ? feat_bytes : 0);
  dim3 grid(ts_grid(n, block, 4096));
  return !dispatch_int<2, 3, 4, 5, 6, 7, 8, 12, 16>(C, [&](auto c) {
    constexpr int CV = decltype(c)::value;
    auto* kernel = lds_feat ? (lds_nodes ? rf_predict_kernel<CV, true, false, true>
                                         : rf_predict_kernel<CV, false, false, true>)
                   : lds_nodes && lds_probs ? rf_predict_kernel<CV, true, true, false>
                   : lds_nodes ? rf_predict_kernel<CV, true, false, false>
                               : rf_predict_kernel<CV, false, false, false>;
    hipLaunchKernelGGL(kernel, grid, dim3(block), lds, stream, X, nd, roots,
                       leaf_proba, out, n, n_nodes, n_leaves, T);
  });
}

// ---------------------------------------------------------------------------
// KNN brute-force top-k + fused vote (N3).  One lane per query; reference
// rows stream through LDS in tiles shared by the block; each lane keeps a
// sorted k-best (dist, idx) list in registers (K compile-time; ties keep the
// lower reference index, matching sklearn ordering).  idx_base offsets
// emitted indices for sharded reference sets (all-gather merge keys stay
// global).
// ---------------------------------------------------------------------------
#define KNN_TILE 256
#define KNN_MAXC 8

template <int K>
__global__ void knn_topk_kernel(const float* __restrict__ Q,
                                const float* __restrict__ R,
                                const unsigned char* __restrict__ ry,  // may be null
                                float* __restrict__ out_d,  // [nq,K]
                                int* __restrict__ out_i,    // [nq,K]
                                int* __restrict__ out_lab,  // [nq] or null
                                long long nq, long long nr, int C,
                                long long idx_base) {
  constexpr int F = 12;
  __shared__ __attribute__((aligned(16))) float s_r[KNN_TILE * F];
  __shared__ unsigned char s_y[KNN_TILE];

  long long stride = (long long)gridDim.x * blockDim.x;
  for (long long base = (long long)blockIdx.x * blockDim.x; base < nq;
       base += stride) {
    long long q = base + threadIdx.x;
    Row12 x;
    if (q < nq) x = load_row12(Q, q);
    float bd[K];
    int bi_[K];
    int bl[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { bd[k] = INFINITY; bi_[k] = -1; bl[k] = 0; }

    for (long long tile = 0; tile < nr; tile += KNN_TILE) {
      int cnt = (int)min((long long)KNN_TILE, nr - tile);
      __syncthreads();
      for (int i = threadIdx.x; i < cnt * F; i += blockDim.x)
        s_r[i] = R[tile * F + i];
      if (ry)
        for (int i = threadIdx.x; i < cnt; i += blockDim.x) s_y[i] = ry[tile + i];
      __syncthreads();
      if (q >= nq) continue;
      // branchless sorted insert: slot k takes bd[k-1] when the new element
      // lands above it, or the new element when it lands here; strict
      // compares keep earlier (lower) reference indices on ties.
      auto insert = [&](float d, int ins, int lab) {
#pragma unroll
        for (int k = K - 1; k > 0; --k) {
          bool above = bd[k - 1] > d;  // new element goes before slot k-1
          if (bd[k] > d) {
            bd[k] = above ? bd[k - 1] : d;
            bi_[k] = above ? bi_[k - 1] : ins;
            bl[k] = above ? bl[k - 1] : lab;
          }
        }
        if (bd[0] > d) { bd[0] = d; bi_[0] = ins; bl[0] = lab; }
      };
      // two candidates per iteration, two split accumulators each: four
      // independent FMA chains in flight hide VALU and LDS latency (a
      // single fmaf chain leaves the SIMD idle between dependent ops)
      auto dist2 = [&](const float* __restrict__ r) {
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          float t = x.v[j] - r[j];
          a = fmaf(t, t, a);
        }
#pragma unroll
        for (int j = 6; j < F; ++j) {
          float t = x.v[j] - r[j];
          b = fmaf(t, t, b);
        }
        return a + b;
      };
      int s = 0;
      for (; s + 2 <= cnt; s += 2) {
        float d0 = dist2(&s_r[s * F]);
        float d1 = dist2(&s_r[(s + 1) * F]);
        if (d0 < bd[K - 1]) insert(d0, (int)(tile + s), ry ? (int)s_y[s] : 0);
        if (d1 < bd[K - 1]) insert(d1, (int)(tile + s + 1), ry ? (int)s_y[s + 1] : 0);
      }
      if (s < cnt) {
        float d0 = dist2(&s_r[s * F]);
        if (d0 < bd[K - 1]) insert(d0, (int)(tile + s), ry ? (int)s_y[s] : 0);
      }
    }
    if (q >= nq) continue;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      out_d[q * K + k] = bd[k];
      out_i[q * K + k] = bi_[k] >= 0 ? (int)(bi_[k] + idx_base) : -1;
    }
    if (out_lab) {
      int best = 0, bc = 0;
      for (int c = 0; c < C; ++c) {
        int v = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) v += (bl[k] == c && bi_[k] >= 0) ? 1 : 0;
        if (v > best) { best = v; bc = c; }
      }
      out_lab[q] = bc;
    }
  }
}

// Returns 0, or nonzero when no kernel exists for this k (nothing is
// launched and the outputs stay unwritten: the caller must turn that into
// an error).
extern "C" int launch_knn_topk(const float* Q, const float* R,
                               const unsigned char* ry, float* out_d,
                               int* out_i, int* out_lab, long long nq,
                               long long nr, int k, int C, long long idx_base,
                               hipStream_t stream) {
  const int block = 256;
  dim3 grid(ts_grid(nq, block));
  return !dispatch_int<1, 2, 3, 4, 5, 6, 7, 8, 16, 32>(k, [&](auto kv) {
    hipLaunchKernelGGL((knn_topk_kernel<decltype(kv)::value>), grid,
                       dim3(block), 0, stream, Q, R, ry, out_d, out_i, out_lab,
                       nq, nr, C, idx_base);
  });
}
