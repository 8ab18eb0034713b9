// Top talkers: per predicted class, and for "unknown", the k live flows with
// the largest key, the key being an f32 sum of chosen feature columns.
//
//   class_top_flows_partial_kernel  one sorted list per group and block
//   class_top_flows_finish_kernel   one block per group merges the nb lists
//
// The group of a row is class_traffic's: its label, or C ("unknown") for a
// label outside 0..C-1 and for a confidence below min_conf (false for a NaN).
// The key is X[r, c] summed over the set bits c of `col_mask` in ascending c,
// plain f32 adds starting from -0.0f, which changes no first term.
//
// One total order, one integer compare.  The key's bits map to a u32 that is
// monotone in the float order, with every NaN at the top and -0 on +0, and a
// candidate is the word  mono(key) << 32 | ~row.  The larger word is the
// earlier flow: larger key first, lower row among equal keys.  No two rows
// have the same word, and no word is 0 (mono is at least 0x007fffff, that of
// -inf), so 0 marks an empty list cell.
//
// The result does not depend on the grid.  The k largest of a set of distinct
// words are the same whatever order the candidates arrive in, so the outputs
// are a pure function of the inputs: bit-identical across calls, grids and
// block caps by construction.  There is no atomic and nothing to make
// deterministic afterwards.
//
// A list is 64 words sorted downwards, cell i owned by lane i, of which the
// first k count (the cells past them hold runners-up or 0), in LDS as
// list[wave][group][64]: a lane reads and writes only its own cell of every
// list, so the LDS serves as a register file indexed by the (wave-uniform)
// group, which a register array indexed at run time would not be.  Each
// list's k-th word (0 until the list is full) is kept in kth[wave][group].
// A list takes candidates in two ways.
//   * One at a time: broadcast the candidate, ballot "my cell is larger",
//     count the ballot for the position, move the cells from there one lane
//     up.  Some 250 cycles of dependent latency each.
//   * 64 at once: a bitonic network over the lanes.  Two lists sorted
//     downwards merge in 7 exchanges (the second reversed, the cell-wise
//     maximum of the two is bitonic and holds the 64 largest of the 128; 6
//     exchanges sort it); 64 unsorted words sort in 21 first.  The cost does
//     not depend on the data.
//
// The partial kernel gives a wave 64 consecutive rows at a time.  Lane l loads
// the label, the confidence and the needed 16-byte quarters of row base + l,
// unconditionally (a row past the live ones re-reads the tile's last live row
// and joins no group), forms the row's group and word and compares the word
// with its group's k-th.  A ballot finds the lanes that beat it.  On rows in
// random order they are few after the first tiles (about k ln(n / k) per group
// and wave) and go in one at a time.  On rows sorted upwards within one class
// every row beats the list; from TOPF_SORT_AT candidates of one group in a tile
// the wave sorts them and merges, 28 exchanges for up to 64 rows, which bounds
// that case (measured in profiles/top_flows.md, with what it cost before).
// After its last tile the block's four waves merge their lists per group and
// write partial[block][group][k].
//
// The finish kernel runs one block of 8 waves per group.  A wave takes its
// share of the nb * k words of the group 64 at a time, four loads in flight
// ahead of their use, filters them by its list's k-th and takes the rest by
// the same two ways (with k = 64 a load is one block's list, sorted already);
// the 8 lists merge pairwise in three rounds and wave 0 writes the rows, and
// the keys recomputed from X by the same adds, so a key comes back with the
// bits the adds gave it.  Empty cells give -1 and 0.0.  Both kernels write
// every cell they own on every launch.
//
// n_live is read from memory (null: all n rows), so one captured launch over
// `capacity` rows follows the live count.
//
// Bytes requested per row: 4 of label, 4 of confidence if given, 16 for each
// quarter of the row that holds a chosen column (the default columns 4 and 10:
// 32).  The quarters of 64 consecutive rows lie in the same 128-byte lines as
// the rest of those rows, so memory still delivers all 48 bytes of a row.

#include "common.h"
#include "launchers.h"

#define TOPF_BLOCK 256
#define TOPF_WAVES (TOPF_BLOCK / WAVE)
#define TOPF_MAX_GROUPS 9  // 8 classes + unknown
#define TOPF_MAX_K 64
#define TOPF_FIN_WAVES 8
#define TOPF_FIN_BATCH 4
// candidates of one group in a tile from which they are sorted and merged:
// 28 exchanges against that many dependent inserts of about three exchanges
#define TOPF_SORT_AT 8

typedef unsigned long long u64;

// f32 bits -> u32 monotone in the float order; NaN on top, -0 on +0
DEV unsigned topf_mono(float key) {
  unsigned b = __float_as_uint(key);
  if ((b & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

DEV u64 topf_word(float key, int row) {
  return ((u64)topf_mono(key) << 32) | (u64)(~(unsigned)row);
}

// The chosen columns of a row, added in ascending column order.  q[i] is the
// row's i-th quarter, read only where mask has a bit in it.
DEV float topf_key(const float4 (&q)[3], unsigned mask) {
  float key = -0.0f;  // -0 + x == x for every x
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const unsigned m = mask >> (4 * i);
    key += (m & 1u) ? q[i].x : -0.0f;
    key += (m & 2u) ? q[i].y : -0.0f;
    key += (m & 4u) ? q[i].z : -0.0f;
    key += (m & 8u) ? q[i].w : -0.0f;
  }
  return key;
}

DEV void topf_load_row(const float* __restrict__ X, long long row, unsigned mask,
                       float4 (&q)[3]) {
  const float4* p = reinterpret_cast<const float4*>(X + row * 12);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    q[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if ((mask >> (4 * i)) & 0xfu) q[i] = p[i];  // wave-uniform
  }
}

DEV u64 topf_max(u64 a, u64 b) { return a > b ? a : b; }
DEV u64 topf_min(u64 a, u64 b) { return a < b ? a : b; }

// Sorts a bitonic sequence of one word per lane downwards.
DEV u64 topf_bitonic_merge(u64 v, int lane) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    const u64 o = __shfl_xor(v, s, WAVE);
    v = (lane & s) ? topf_min(v, o) : topf_max(v, o);
  }
  return v;
}

// Sorts any 64 words, one per lane, downwards: runs of 2, 4, .. 32 sorted in
// alternating directions, then the whole.
DEV u64 topf_sort(u64 v, int lane) {
#pragma unroll
  for (int size = 2; size <= WAVE; size <<= 1) {
    const bool down = (lane & size) == 0;  // size 64: every lane
#pragma unroll
    for (int s = size >> 1; s > 0; s >>= 1) {
      const u64 o = __shfl_xor(v, s, WAVE);
      const bool low = (lane & s) == 0;
      v = (low == down) ? topf_max(v, o) : topf_min(v, o);
    }
  }
  return v;
}

// The 64 largest of two lists sorted downwards, sorted downwards.
DEV u64 topf_merge64(u64 a, u64 b, int lane) {
  const u64 br = __shfl(b, WAVE - 1 - lane, WAVE);
  return topf_bitonic_merge(topf_max(a, br), lane);
}

// Merges the sorted words v (one per lane) into the list L.
DEV void topf_take64(u64* __restrict__ L, u64* __restrict__ kth, int lane, int k,
                     u64 v) {
  const u64 m = topf_merge64(L[lane], v, lane);
  L[lane] = m;
  if (lane == k - 1) *kth = m;
}

// Inserts the wave-uniform word cw into the list L and keeps *kth current.  A
// word that does not beat the k-th leaves the list as it is.
DEV void topf_insert(u64* __restrict__ L, u64* __restrict__ kth, int lane, int k,
                     u64 cw) {
  const u64 mine = L[lane];
  const int pos = __popcll(__ballot(lane < k && mine > cw));
  if (pos >= k) return;
  const u64 below = __shfl_up(mine, 1, WAVE);  // the cell one lane down
  const u64 v = lane < pos ? mine : (lane == pos ? cw : below);
  L[lane] = v;  // all 64 cells move, so the list stays sorted throughout
  if (lane == k - 1) *kth = v;
}

// Takes the words of the lanes in `pend` into the lists of their groups.
// `word` is each lane's own; `grp` its list; lists of the wave at `lists`.
// `sorted`: the words of `pend` descend with the lane already.
DEV void topf_drain(u64 pend, u64 word, int grp, u64* __restrict__ lists,
                    u64* __restrict__ kths, int lane, int k, bool sorted) {
  while (pend) {
    const int cg = __shfl(grp, __ffsll((long long)pend) - 1, WAVE);
    u64 same = __ballot(grp == cg) & pend;  // the group's lanes among them
    pend &= ~same;
    u64* L = lists + cg * TOPF_MAX_K;
    if (__popcll(same) >= TOPF_SORT_AT) {
      u64 v = ((same >> lane) & 1ull) ? word : 0ull;
      if (!sorted) v = topf_sort(v, lane);
      topf_take64(L, kths + cg, lane, k, v);
    } else {
      while (same) {
        const int src = __ffsll((long long)same) - 1;
        same &= same - 1;
        topf_insert(L, kths + cg, lane, k, __shfl(word, src, WAVE));
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
}

__launch_bounds__(TOPF_BLOCK) __global__ void class_top_flows_partial_kernel(
    const float* __restrict__ X, const int* __restrict__ labels,
    const float* __restrict__ conf, const int* __restrict__ n_live,
    float min_conf, unsigned col_mask, int C, int k, u64* __restrict__ partial,
    long long n) {
  __shared__ u64 list[TOPF_WAVES * TOPF_MAX_GROUPS * TOPF_MAX_K];
  __shared__ u64 kth[TOPF_WAVES * 16];
  long long live = n;
  if (n_live) {
    const long long v = *n_live;
    live = v < n ? v : n;
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  u64* lists = list + wave * (TOPF_MAX_GROUPS * TOPF_MAX_K);
  u64* kths = kth + wave * 16;
  for (int g = 0; g <= C; ++g) lists[g * TOPF_MAX_K + lane] = 0ull;
  if (lane < 16) kths[lane] = 0ull;
  __builtin_amdgcn_wave_barrier();

  const long long stride = (long long)gridDim.x * TOPF_BLOCK;
  for (long long base = ((long long)blockIdx.x * TOPF_WAVES + wave) * WAVE;
       base < live; base += stride) {
    const long long left = live - base;
    const int last = left < WAVE ? (int)left - 1 : WAVE - 1;
    const long long r = base + (lane < last ? lane : last);
    float4 q[3];
    topf_load_row(X, r, col_mask, q);
    const int lab = labels[r];
    const float cv = conf ? conf[r] : 0.f;
    const bool low = conf && cv < min_conf;  // false for a NaN
    int g = ((unsigned)lab < (unsigned)C && !low) ? lab : C;
    g = lane <= last ? g : -1;  // past the live rows: in no group
    const u64 word = topf_word(topf_key(q, col_mask), (int)r);
    const u64 bar = kths[g < 0 ? 0 : g];
    const u64 pend = __ballot(g >= 0 && word > bar);
    topf_drain(pend, word, g, lists, kths, lane, k, false);
  }
  __syncthreads();

  // wave w owns the groups w, w + 4, ...: it merges the other waves' lists of
  // such a group into its own, which no other wave reads
  for (int g = wave; g <= C; g += TOPF_WAVES) {
    u64* L = lists + g * TOPF_MAX_K;
    for (int o = 1; o < TOPF_WAVES; ++o) {
      const int v = (wave + o) % TOPF_WAVES;
      const u64* S = list + (v * TOPF_MAX_GROUPS + g) * TOPF_MAX_K;
      if (S[0] > kths[g]) topf_take64(L, kths + g, lane, k, S[lane]);
      __builtin_amdgcn_wave_barrier();
    }
    if (lane < k)
      partial[((long long)blockIdx.x * (C + 1) + g) * k + lane] = L[lane];
  }
}

__launch_bounds__(TOPF_FIN_WAVES * WAVE) __global__
void class_top_flows_finish_kernel(const u64* __restrict__ partial, int nb,
                                   const float* __restrict__ X,
                                   unsigned col_mask, int C, int k,
                                   int* __restrict__ rows,
                                   float* __restrict__ keys) {
  __shared__ u64 list[TOPF_FIN_WAVES * TOPF_MAX_K];
  __shared__ u64 kth[TOPF_FIN_WAVES];
  const int g = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  u64* L = list + wave * TOPF_MAX_K;
  L[lane] = 0ull;
  if (lane == 0) kth[wave] = 0ull;
  __builtin_amdgcn_wave_barrier();

  // candidate i of the group is word i % k of block i / k
  // (the launcher keeps nb * k inside an int); a word past the last re-reads
  // the last and counts as empty
  const int total = nb * k;
  const int step = TOPF_FIN_WAVES * WAVE;
  for (int base = wave * WAVE; base < total; base += step * TOPF_FIN_BATCH) {
    u64 w[TOPF_FIN_BATCH];
#pragma unroll
    for (int j = 0; j < TOPF_FIN_BATCH; ++j) {
      const int i = base + j * step + lane;
      const unsigned ii = i < total ? i : total - 1;
      const unsigned b = ii / (unsigned)k;
      const u64 v =
          partial[((long long)b * (C + 1) + g) * k + (ii - b * (unsigned)k)];
      w[j] = i < total ? v : 0ull;
    }
#pragma unroll
    for (int j = 0; j < TOPF_FIN_BATCH; ++j) {
      const u64 pend = __ballot(w[j] > kth[wave]);  // an empty word is 0
      // 64 words of 64-word lists are one block's list: what beats the k-th
      // is its head, and descends
      topf_drain(pend, w[j], 0, L, kth + wave, lane, k, k == TOPF_MAX_K);
    }
  }

  // the 8 lists pairwise: 4 merges, 2, 1
  for (int s = TOPF_FIN_WAVES / 2; s > 0; s >>= 1) {
    __syncthreads();
    if (wave < s) topf_take64(L, kth + wave, lane, k, list[(wave + s) * TOPF_MAX_K + lane]);
  }

  if (wave == 0 && lane < k) {
    const u64 word = L[lane];
    int row = -1;
    float key = 0.f;
    if (word != 0ull) {
      row = (int)~(unsigned)word;
      float4 q[3];
      topf_load_row(X, row, col_mask, q);
      key = topf_key(q, col_mask);
    }
    rows[g * k + lane] = row;
    keys[g * k + lane] = key;
  }
}

// Blocks of the partial kernel for n rows: class_traffic's grid, so
// TCSDN_PROBA_BLOCKS (read per call) caps it too.  The caller sizes `partial`
// with it and hands the same number to the launcher.
extern "C" int class_top_flows_blocks(long long n) {
  return ts_grid(n, TOPF_BLOCK, env_block_cap("TCSDN_PROBA_BLOCKS", 2048));
}

// `conf` and `n_live` may be null.  `partial` holds nb * (C + 1) * k words.
// Returns nonzero, and launches nothing, for C outside 2..8, k outside 1..64,
// a column mask that is empty or has a bit past column 11, or nb outside
// 1..2^20.  n <= 0 still launches: the outputs are written, as -1 and 0.0.
extern "C" int launch_class_top_flows(const float* X, const int* labels,
                                      const float* conf, const int* n_live,
                                      float min_conf, unsigned col_mask,
                                      unsigned long long* partial, int* rows,
                                      float* keys, long long n, int C, int k,
                                      int nb, hipStream_t stream) {
  if (C < 2 || C > 8 || k < 1 || k > TOPF_MAX_K || nb < 1 || nb > (1 << 20))
    return 1;
  if (col_mask == 0u || col_mask > 0xfffu) return 1;
  hipLaunchKernelGGL(class_top_flows_partial_kernel, dim3(nb), dim3(TOPF_BLOCK),
                     0, stream, X, labels, conf, n_live, min_conf, col_mask, C,
                     k, partial, n < 0 ? 0 : n);
  hipLaunchKernelGGL(class_top_flows_finish_kernel, dim3(C + 1),
                     dim3(TOPF_FIN_WAVES * WAVE), 0, stream, partial, nb, X,
                     col_mask, C, k, rows, keys);
  return 0;
}
