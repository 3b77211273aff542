// Device pieces of the prioritized-replay kernels, each written once: the descent step and the
// three-level global round of find_prefixsum_idx, the batch scalars, the leaf value and leaf update,
// the sorted-list and occurrence tests, the max_priority maximum, the counter increment, the subtree
// and top rebuilds and the last-workgroup protocol. Two translation units build their kernels from
// them: replay_kernels.hip, and learn_kernels.hip, whose k_adam_sample runs the sampler beside the
// critic's Adam step and whose k_wgrad_big_per runs the per-subtree priority update beside the
// critic's weight-gradient GEMM. Node layout and arithmetic of segment_tree.py /
// replay_buffer.py:139-218.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace cacto {

__device__ __forceinline__ double tree_min(double a, double b) { return b < a ? b : a; }  // Python min(a, b)

constexpr int PER_MAX_B = 8192;      // samples per call
constexpr int PER_MW_MIN = 512;      // batches from this size on take the multi-workgroup kernels
constexpr int PER_MW_TOP = 8192;     // k_per_sample_mw: staged top nodes (64 KiB of LDS)
constexpr int PER_FUSED_TOP = 4096;  // the sampler beside the Adam step (32 KiB)
constexpr int PER_RUN_SUB = 256;     // leaves per workgroup of per_update_run_body
constexpr int PER_RUN_EMPTY = 0x7f7f7f7f;  // runs[s] before any sample landed in subtree s (memset 0x7f)

// Select a[j] (j in [0, N)) from a register array without dynamic indexing (no scratch).
// A tournament of selects on j's bits (a chain of j == q selects gets folded back into an indexed
// load, which moves the array to scratch).
template <int N>
__device__ __forceinline__ double reg_pick(const double (&a)[N], int j) {
  static_assert((N & (N - 1)) == 0, "power of two");
  double w[N];
#pragma unroll
  for (int q = 0; q < N; ++q) w[q] = a[q];
#pragma unroll
  for (int h = N / 2, b = 0; h >= 1; h /= 2, ++b)
#pragma unroll
    for (int q = 0; q < h; ++q) w[q] = ((j >> b) & 1) ? w[2 * q + 1] : w[2 * q];
  return w[0];
}

// One step of find_prefixsum_idx (segment_tree.py:103-114): the reference's comparison and
// subtraction, in its order. `node` is a tree node or a position within a level.
template <class I>
__device__ __forceinline__ void per_step(double left, double& p, I& node) {
  if (left > p) {
    node = 2 * node;
  } else {
    p -= left;
    node = 2 * node + 1;
  }
}

// Up to three levels of the descent below node n in one memory latency: the seven candidate left
// children (n's, its children's, its grandchildren's) are loaded together, then per_round3 takes the
// steps. FULL: three levels exist below n (the caller knows); otherwise as many of them as lie
// above the leaves' end `cap`, and none (no load, no step) for a descent that is not `live`.
struct PerRound3 {
  double a, b0, b1, c[4];
};
template <bool FULL>
__device__ __forceinline__ PerRound3 per_round3_load(const double* __restrict__ tree, int64_t n, bool live,
                                                     int64_t cap) {
  const bool one = FULL || live, two = FULL || (live && 2 * n < cap), three = FULL || (live && 4 * n < cap);
  PerRound3 r;
  r.a = one ? tree[2 * n] : 0.0;
  r.b0 = two ? tree[4 * n] : 0.0;
  r.b1 = two ? tree[4 * n + 2] : 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) r.c[q] = three ? tree[8 * n + 2 * q] : 0.0;
  return r;
}
template <bool FULL>
__device__ __forceinline__ void per_round3(const PerRound3& r, bool live, int64_t cap, double& p, int64_t& node) {
  if (!FULL && !live) return;
  const int64_t n = node;
  int64_t m = n;
  per_step(r.a, p, m);
  if (FULL || 2 * n < cap) {
    per_step((m & 1) ? r.b1 : r.b0, p, m);
    if (FULL || 4 * n < cap) per_step(reg_pick(r.c, (int)(m - 4 * n)), p, m);
  }
  node = m;
}

// The last R levels of find_prefixsum_idx below node n (whose descendants R levels down are the
// leaves): the left child of every internal node and all 2^R leaves are loaded together, so the R
// comparisons and the sampled leaf's own value (P(i) of the IS weight) cost one memory latency.
// One internal level D (1-based) of per_tail: its left children are lv[2^(D-1) - 1 + q].
template <int D, int NLV>
__device__ __forceinline__ void tail_step(const double (&lv)[NLV], int& j, double& p) {
  double row[1 << (D - 1)];
#pragma unroll
  for (int q = 0; q < (1 << (D - 1)); ++q) row[q] = lv[(1 << (D - 1)) - 1 + q];
  per_step(reg_pick(row, j), p, j);
}

template <int R>
__device__ __forceinline__ void per_tail(const double* __restrict__ tree, int64_t n, double& p, int64_t& node,
                                         double& val) {
  static_assert(R >= 1 && R <= 5, "per_tail covers up to five levels");
  constexpr int NL = 1 << R;
  double lf[NL];
  double lv[R > 1 ? (1 << (R - 1)) - 1 : 1];
#pragma unroll
  for (int d = 1; d < R; ++d)
#pragma unroll
    for (int j = 0; j < (1 << (d - 1)); ++j) lv[(1 << (d - 1)) - 1 + j] = tree[(n << d) + 2 * j];
#pragma unroll
  for (int k = 0; k < NL; ++k) lf[k] = tree[(n << R) + k];
  int j = 0;  // position within the current level below n
  if constexpr (R > 1) tail_step<1>(lv, j, p);
  if constexpr (R > 2) tail_step<2>(lv, j, p);
  if constexpr (R > 3) tail_step<3>(lv, j, p);
  if constexpr (R > 4) tail_step<4>(lv, j, p);
  per_step(reg_pick(lf, 2 * j), p, j);
  node = (n << R) + j;
  val = reg_pick(lf, j);
}

// The batch scalars of one sample call, the segment aside: the root sum, the IS weights' scale (the
// row count) and their normaliser max_w. With shards (data parallel): every shard draws B stratified
// samples from its own tree, so sample i of shard g has probability p_i / (G * total_g) in the union
// of N = sum N_g rows; the IS weight (N * P(i))^-beta is normalised by its maximum over all shards.
// For one shard this is exactly the single-buffer formula.
__device__ __forceinline__ void per_batch_scalars(const double* __restrict__ sum_tree,
                                                  const double* __restrict__ min_tree, int64_t max_idx, double beta,
                                                  const double* __restrict__ shards, int n_shards, double& total,
                                                  double& scale, double& maxw) {
  total = sum_tree[1];
  if (shards) {
    double n_all = 0.0, ratio_min = __builtin_inf();
    for (int g = 0; g < n_shards; ++g) {
      n_all += shards[3 * g + 2];
      ratio_min = tree_min(ratio_min, shards[3 * g + 1] / shards[3 * g + 0]);
    }
    scale = n_all / n_shards;
    maxw = pow(ratio_min * scale, -beta);
  } else {
    const double p_min = min_tree[1] / total;
    scale = (double)max_idx;
    maxw = pow(p_min * scale, -beta);
  }
}

// A priority and its leaf: p = fresh^count |y - V| + eps evaluated as TF would (float32 tensors),
// leaf = p^alpha in f64 (replay_buffer.py:193-218).
__device__ __forceinline__ double per_leaf_value(double fresh, double count, float y, float V, double eps,
                                                 double alpha, float& p) {
  const float td = fabsf(__fsub_rn(y, V));
  const float fd = (float)pow(fresh, count);
  p = __fadd_rn(__fmul_rn(fd, td), (float)eps);
  return pow((double)p, alpha);
}

// Whether idx[0, n) is non-decreasing, for the whole workgroup of NT threads (one barrier). The
// stratified sampler's output is (monotone prefix-sum search), so duplicates are adjacent there.
template <int NT>
__device__ __forceinline__ bool per_list_sorted(const int32_t* idx, int n) {
  bool unsorted = false;
  for (int i = threadIdx.x; i + 1 < n; i += NT) unsorted |= idx[i + 1] < idx[i];
  return !__syncthreads_or(unsorted);
}

// Whether entry i is the first / last occurrence of its value in idx[lo, hi): the neighbour test
// for a sorted list, a scan otherwise.
__device__ __forceinline__ bool per_first_occ(const int32_t* idx, int lo, int i, bool sorted) {
  const int32_t id = idx[i];
  if (sorted) return i == lo || idx[i - 1] != id;
  for (int j = lo; j < i; ++j)
    if (idx[j] == id) return false;
  return true;
}
__device__ __forceinline__ bool per_last_occ(const int32_t* idx, int hi, int i, bool sorted) {
  const int32_t id = idx[i];
  if (sorted) return i + 1 == hi || idx[i + 1] != id;
  for (int j = i + 1; j < hi; ++j)
    if (idx[j] == id) return false;
  return true;
}

// What a priority update writes leaves from: given values (the ReLO rule, cacto_per_set_leaves) or
// y, V and the rule's constants.
struct PerLeafArgs {
  double* sum_tree;
  double* min_tree;
  int64_t cap;
  const double* vals;
  const float* y;
  const float* V;
  double fresh, eps, alpha;
};

// The leaf of entry i of a priority update (row id = idx[i], whose exp_counter value the rule sees
// is *count; not read with given values): formed, folded into my_max, and written to both trees
// when i is the row's last occurrence in idx[.., hi) (last-write-wins). Returns whether it wrote.
__device__ __forceinline__ bool per_leaf_update(const PerLeafArgs& a, const int32_t* idx, int hi, int i, bool sorted,
                                                const double* count, double count_add, double& my_max,
                                                double& leaf) {
  const int32_t id = idx[i];
  if (a.vals) {
    leaf = a.vals[i];
  } else {
    float p;
    leaf = per_leaf_value(a.fresh, *count + count_add, a.y[i], a.V[i], a.eps, a.alpha, p);
    my_max = fmax(my_max, (double)p);
  }
  const bool last = per_last_occ(idx, hi, i, sorted);
  if (last) {
    a.sum_tree[a.cap + id] = leaf;
    a.min_tree[a.cap + id] = leaf;
  }
  return last;
}

// max_priority = max(max_priority, max over the workgroup's m): wave reduction, then an atomic max
// on the bit pattern — the priorities are positive (p >= eps > 0), where the IEEE order and the
// integer order agree; NaN is skipped as fmax skips it.
__device__ __forceinline__ void per_publish_max(double m, double* max_priority) {
  if (!max_priority) return;
  for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off));
  if ((threadIdx.x & 63) == 0 && m > 0.0)  // false for -inf (no leaf) and NaN
    atomicMax(reinterpret_cast<unsigned long long*>(max_priority), (unsigned long long)__double_as_longlong(m));
}

// exp_counter[idx] += 1 as numpy's fancy-index increment does it (each distinct index once): one
// workgroup of NT threads, every read before any write.
template <int NT>
__device__ __forceinline__ void per_count_once(const int32_t* idx, int B, double* __restrict__ exp_counter) {
  double old[PER_MAX_B / NT];
  int k = 0;
  for (int i = threadIdx.x; i < B; i += NT) old[k++] = exp_counter[idx[i]];
  __syncthreads();
  k = 0;
  for (int i = threadIdx.x; i < B; i += NT) exp_counter[idx[i]] = old[k++] + 1.0;
}

// A level of `lo` nodes over NT threads: one pass when the level fits the workgroup (ONE_PASS, the
// 256-leaf form), a stride loop otherwise.
template <int NT, bool ONE_PASS, class F>
__device__ __forceinline__ void per_level_nodes(int lo, F&& node) {
  const int tid = threadIdx.x;
  if constexpr (ONE_PASS) {
    if (tid < lo) node(lo + tid);
  } else {
    for (int k = lo + tid; k < 2 * lo; k += NT) node(k);
  }
}

// The levels of a subtree of `sub` leaves staged in LDS (ts / tm: local node j of the 1-based heap,
// the leaves at [sub, 2 sub)) rebuilt bottom-up and every internal node written back; the subtree's
// leaves are the global nodes [leaf0, leaf0 + sub). The tree is consistent (each node =
// op(children)), so nodes over untouched leaves come out unchanged and the touched ones get
// op(final children) — the value the reference's leaf-by-leaf updates leave. root_at_agent_scope:
// the subtree's root is read by another workgroup (per_last_workgroup) and is stored at agent scope
// (coherent across the XCDs' L2s) instead of releasing the whole L2 with a fence — a fence's L2
// write-back here also flushed the concurrent chains' panel writes (29 us per launch).
template <int NT, bool ONE_PASS>
__device__ __forceinline__ void per_rebuild_subtree(double* ts, double* tm, int sub, int64_t leaf0,
                                                    bool root_at_agent_scope, double* __restrict__ sum_tree,
                                                    double* __restrict__ min_tree) {
  int lvl = 0;
  for (int lo = sub / 2; lo >= 1; lo /= 2) {
    ++lvl;
    per_level_nodes<NT, ONE_PASS>(lo, [&](int k) {
      ts[k] = ts[2 * k] + ts[2 * k + 1];
      tm[k] = tree_min(tm[2 * k], tm[2 * k + 1]);
      // local node k of level lvl is global node (leaf0 >> lvl) + (k - lo)
      const int64_t g = (leaf0 >> lvl) + (k - lo);
      if (k == 1 && root_at_agent_scope) {
        __hip_atomic_store(sum_tree + g, ts[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(min_tree + g, tm[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else {
        sum_tree[g] = ts[k];
        min_tree[g] = tm[k];
      }
    });
    __syncthreads();
  }
}

// The nodes above `nroot` roots, [1, nroot), rebuilt in LDS from the roots staged at
// ts / tm [nroot, 2 nroot) and written back (one workgroup).
template <int NT, bool ONE_PASS>
__device__ __forceinline__ void per_rebuild_top(double* ts, double* tm, int nroot, double* __restrict__ sum_tree,
                                                double* __restrict__ min_tree) {
  for (int lo = nroot / 2; lo >= 1; lo /= 2) {
    per_level_nodes<NT, ONE_PASS>(lo, [&](int k) {
      ts[k] = ts[2 * k] + ts[2 * k + 1];
      tm[k] = tree_min(tm[2 * k], tm[2 * k + 1]);
      sum_tree[k] = ts[k];
      min_tree[k] = tm[k];
    });
    __syncthreads();
  }
}

// The last-workgroup protocol of the one-launch priority updates ("Memory-ordering
// contract", site 1; written here only). Every workgroup calls it after storing its subtree's root
// at agent scope: thread 0 waits for its stores to complete (vmcnt 0), then counts the workgroup in
// the unused word sum_tree[0] by an agent-scope RMW — publication without a fence. The workgroup
// that counts last loads the nroot roots at agent scope, rebuilds the nodes above them
// (per_rebuild_top) and resets the word to 0 = +0.0; it alone returns true. flag: one LDS int.
template <int NT, bool ONE_PASS>
__device__ __forceinline__ bool per_last_workgroup(double* __restrict__ sum_tree, double* __restrict__ min_tree,
                                                   int nroot, int* flag, double* ts, double* tm) {
  const int tid = threadIdx.x;
  unsigned long long* done_word = reinterpret_cast<unsigned long long*>(sum_tree);
  if (tid == 0) {
    __builtin_amdgcn_s_waitcnt(0);
    *flag = __hip_atomic_fetch_add(done_word, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
            (unsigned long long)(nroot - 1);
  }
  __syncthreads();
  if (!*flag) return false;
  per_level_nodes<NT, ONE_PASS>(nroot, [&](int k) {
    ts[k] = __hip_atomic_load(sum_tree + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    tm[k] = __hip_atomic_load(min_tree + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  });
  __syncthreads();
  per_rebuild_top<NT, ONE_PASS>(ts, tm, nroot, sum_tree, min_tree);
  if (tid == 0) __hip_atomic_store(done_word, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // +0.0, node 0
  return true;
}

struct PerSampleArgs {
  const double* sum_tree;
  const double* min_tree;
  int64_t cap, max_idx;
  double beta;
  const double* uniforms;  // [B]
  int B;
  int32_t* idx_out;
  float* w_out;
  const double* shards;  // data-parallel shard statistics [n_shards][3] (nullptr: one buffer)
  int n_shards;
  // optional (the pipelined loop's fused priority update): runs[s] = min sample index and
  // runs[cap / PER_RUN_SUB + s] = sample count of subtree s, by relaxed atomics (the indices are
  // sorted, so each subtree's samples are one contiguous run)
  int32_t* runs;
};

// One sample per thread, 256 per workgroup (workgroup blk takes samples [256 blk, 256 blk + 256)).
// Each workgroup stages the top TOPN nodes of the sum tree in LDS with every thread's loads in flight
// at once while wave 0 gathers the batch scalars' terms (lane k the k-th term of prefix_reduce's
// sum(0, max_idx - 1)) in the same latency; the descent walks the staged levels in LDS, then rounds
// of three levels until at most five remain, then per_tail (one more memory latency for the
// remaining levels and the leaf value). For the 2^16-row buffer: two dependent global latencies per
// sample at TOPN = 8192 (four levels below the top) and at 4096 (five).
#ifdef CACTO_STAMPS
// diagnostic builds: s_memtime of thread 0 of each sampler workgroup at its phase boundaries (start,
// staged top + scalars, LDS descent done, tail done, end), [blk][8]; read by cacto_debug_per_stamps
__device__ unsigned long long g_per_stamps[64 * 8];
#define PER_STAMP(blk, k)                                                                        \
  do {                                                                                           \
    if (threadIdx.x == 0 && (blk) < 64) g_per_stamps[(blk) * 8 + (k)] = __builtin_amdgcn_s_memtime(); \
  } while (0)
#else
#define PER_STAMP(blk, k) \
  do {                    \
  } while (0)
#endif

template <int TOPN>
__device__ __forceinline__ void per_sample_body(int blk, const PerSampleArgs& a, double* top_s, double* scal_s) {
  PER_STAMP(blk, 0);
  const int64_t cap = a.cap, max_idx = a.max_idx;
  const double* __restrict__ sum_tree = a.sum_tree;
  const int B = a.B;
  const int64_t ntop = cap < TOPN ? cap : TOPN;
  const int tid = threadIdx.x;
  const int i = blk * 256 + tid;
  const double u = i < B ? a.uniforms[i] : 0.0;  // in flight with the loads below
  // the staging loads first (ntop / 2 double2 pairs over 256 threads), then, while they are in
  // flight: wave 0 walks prefix_reduce's path (lane k loads its k-th term) and wave 1 loads the roots
  // and forms the IS-weight normaliser (a pow) beside wave 0's sum
  constexpr int PAIRS = TOPN / 2 / 256;
  double2 st[PAIRS];
  {
    const double2* src = reinterpret_cast<const double2*>(sum_tree);
#pragma unroll
    for (int r = 0; r < PAIRS; ++r) {
      const int64_t q = tid + r * 256;
      st[r] = 2 * q < ntop ? src[q] : make_double2(0.0, 0.0);
    }
  }
  // lane k's term in closed form (cap = 2^L; [0, cap - 1] halves at every level, so the path to
  // `end` is end's bits from the top): the walk stops at depth d* = L - (trailing ones of end, at
  // most L) with the node itself as the last term; above it, a step right at depth k (bit L - 1 - k
  // of end set) adds that node's left child
  double term = 0.0;
  bool has_term = false;
  int dstar = -1;  // deepest term's depth (no term when end < 0)
  const int64_t end = max_idx - 2;
  if (end >= 0) {
    const int L = 63 - __builtin_clzll((unsigned long long)cap);
    const int ones = __builtin_ctzll(~(unsigned long long)end);
    dstar = L - (ones < L ? ones : L);
  }
  if (tid < 64) {
    const int k = tid;
    if (end >= 0) {
      const int L = 63 - __builtin_clzll((unsigned long long)cap);
      int64_t at = -1;
      if (k == dstar) at = ((int64_t)1 << k) | (end >> (L - k));
      else if (k < dstar && ((end >> (L - 1 - k)) & 1)) at = (((int64_t)1 << k) | (end >> (L - k))) * 2;
      has_term = at >= 0;
      PER_STAMP(blk, 5);
      if (has_term) term = sum_tree[at];
    }
  } else if (tid == 64) {
    per_batch_scalars(sum_tree, a.min_tree, max_idx, a.beta, a.shards, a.n_shards, scal_s[1], scal_s[3], scal_s[2]);
  }
#pragma unroll
  for (int r = 0; r < PAIRS; ++r) {
    const int64_t q = tid + r * 256;
    if (2 * q < ntop) reinterpret_cast<double2*>(top_s)[q] = st[r];
  }
  PER_STAMP(blk, 6);
  if (tid < 64) {
    // the right-nested sum, deepest term first, as prefix_reduce combines them
    const unsigned long long mask = __ballot(has_term);
    double r = 0.0;
    bool have = false;
    for (int k = dstar; k >= 0; --k)
      if ((mask >> k) & 1ull) {  // k is uniform: read the lane's term into scalar registers
        const long long tb = __double_as_longlong(term);
        const int lo = __builtin_amdgcn_readlane((int)(tb & 0xffffffffll), k);
        const int hi = __builtin_amdgcn_readlane((int)(tb >> 32), k);
        const double tk = __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
        r = have ? tk + r : tk;
        have = true;
      }
    if (tid == 0) scal_s[0] = r / B;  // segment
    PER_STAMP(blk, 7);
  }
  __syncthreads();
  PER_STAMP(blk, 1);
  if (i >= B) return;
  const double seg = scal_s[0];
  double p = u * seg + i * seg;
  int64_t nd = 1;
  while (4 * nd < ntop) {  // two staged levels per LDS latency: the left child and both left grandchildren
    const double a0 = top_s[2 * nd], b0 = top_s[4 * nd], b1 = top_s[4 * nd + 2];
    per_step(a0, p, nd);
    per_step((nd & 1) ? b1 : b0, p, nd);
  }
  if (2 * nd < ntop) per_step(top_s[2 * nd], p, nd);
  PER_STAMP(blk, 2);
  // levels below the staged top, three at a time, until at most five remain
  int rem = 0;
  for (int64_t s = nd; s < cap; s *= 2) ++rem;  // levels from nd down to the leaves
  while (rem > 5) {
    const PerRound3 r = per_round3_load<true>(sum_tree, nd, true, cap);
    per_round3<true>(r, true, cap, p, nd);
    rem -= 3;
  }
  int64_t leaf;
  double val;
  switch (rem) {
    case 5: per_tail<5>(sum_tree, nd, p, leaf, val); break;
    case 4: per_tail<4>(sum_tree, nd, p, leaf, val); break;
    case 3: per_tail<3>(sum_tree, nd, p, leaf, val); break;
    case 2: per_tail<2>(sum_tree, nd, p, leaf, val); break;
    case 1: per_tail<1>(sum_tree, nd, p, leaf, val); break;
    default: leaf = nd; val = sum_tree[nd]; break;  // capacity 1: the root is the leaf
  }
  PER_STAMP(blk, 3);
  const int32_t id = (int32_t)(leaf - cap);
  a.idx_out[i] = id;
  a.w_out[i] = (float)(pow(val / scal_s[1] * scal_s[3], -a.beta) / scal_s[2]);
  PER_STAMP(blk, 4);
  if (a.runs) {
    const int64_t nroot = cap / PER_RUN_SUB, s = id / PER_RUN_SUB;
    __hip_atomic_fetch_min(a.runs + s, i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(a.runs + nroot + s, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

struct PerRunArgs {
  double* sum_tree;
  double* min_tree;
  int64_t cap;
  const int32_t* idx;  // the sampler's (sorted) indices of this update
  const float* y;
  const float* V;
  double* exp_counter;
  int64_t rows;  // exp_counter's length (the replay size)
  double fresh, eps, alpha;
  double* max_priority;
  int32_t* runs;  // the sampler's per-subtree runs, reset here for the next sample
  // data parallel (cacto_update_n_per_dp): the ranks' (sum, min, rows) table [world][3], or nullptr.
  // The workgroup that rebuilds the top writes this shard's values (k_per_shard_stats') at
  // stats_off and zeros in the other ranks' words, so a sum all-reduce of the table is the
  // all-gather (x + 0.0 == x for the non-negative statistics)
  double* stats;
  int stats_off = 0, stats_words = 3;
};

struct PerRunLds {
  double ts[2 * PER_RUN_SUB], tm[2 * PER_RUN_SUB];  // local node j (1-based heap of the subtree)
  double cnt[PER_RUN_SUB];                          // exp_counter of the subtree's rows before this update
  int run[2];
  int last;
};

// update_priorities 'PER' for the samples in subtree blk (leaves [cap + 256 blk, cap + 256 blk + 256))
// of one stratified sample, with the sampler's deferred exp_counter += 1 — k_per_update_sub's
// arithmetic, for sorted indices whose run the sampler recorded, so nothing is searched:
//   1. one memory latency: the subtree's leaves of both trees, its rows' exp_counter values and the
//      run (runs[] reset for the next sample);
//   2. one more: the run's indices (and neighbours, for the duplicate tests), y and V; every
//      occurrence of a row reads the row's count from LDS (numpy's fancy-index increment reads the
//      old count once per distinct index), the first occurrence writes old + 1, the last one the leaf;
//   3. the subtree rebuilt in LDS and written back, its root at agent scope; the last of the nroot
//      workgroups to finish rebuilds the nodes above the roots (nroot <= PER_RUN_SUB).
// Values, last-write-wins and max_priority as k_per_update_sub (bit-identical trees and counters).
__device__ __forceinline__ void per_update_run_body(int blk, int nroot, const PerRunArgs& a, PerRunLds& L) {
  const int tid = threadIdx.x;
  constexpr int SUB = PER_RUN_SUB;
  const int64_t cap = a.cap;
  const int64_t id_lo = (int64_t)blk * SUB;
  const int64_t leaf0 = cap + id_lo;
  {
    const double sv = a.sum_tree[leaf0 + tid], mv = a.min_tree[leaf0 + tid];
    const double cv = id_lo + tid < a.rows ? a.exp_counter[id_lo + tid] : 0.0;
    if (tid == 0) {
      L.run[0] = a.runs[blk];
      L.run[1] = a.runs[nroot + blk];
      a.runs[blk] = PER_RUN_EMPTY;
      a.runs[nroot + blk] = 0;
    }
    L.ts[SUB + tid] = sv;
    L.tm[SUB + tid] = mv;
    L.cnt[tid] = cv;
  }
  __syncthreads();
  const int r0 = L.run[0], rn = L.run[1];
  if (rn > 0) {
    const PerLeafArgs la{a.sum_tree, a.min_tree, cap, nullptr, a.y, a.V, a.fresh, a.eps, a.alpha};
    double my_max = -__builtin_inf();
    for (int i = r0 + tid; i < r0 + rn; i += SUB) {
      const int32_t id = a.idx[i];
      const bool first = per_first_occ(a.idx, r0, i, true);
      const double old = L.cnt[id - id_lo];
      double leaf;
      if (per_leaf_update(la, a.idx, r0 + rn, i, true, &old, 1.0, my_max, leaf)) {
        L.ts[SUB + (id - id_lo)] = leaf;
        L.tm[SUB + (id - id_lo)] = leaf;
      }
      if (first) a.exp_counter[id] = old + 1.0;
    }
    per_publish_max(my_max, a.max_priority);
    __syncthreads();  // the leaves are in LDS
    per_rebuild_subtree<SUB, true>(L.ts, L.tm, SUB, leaf0, nroot > 1, a.sum_tree, a.min_tree);
  }
  if (nroot == 1) return;
  if (per_last_workgroup<SUB, true>(a.sum_tree, a.min_tree, nroot, &L.last, L.ts, L.tm) && tid == 0 && a.stats) {
    for (int k = 0; k < a.stats_words; ++k) a.stats[k] = 0.0;
    a.stats[a.stats_off + 0] = L.ts[1];
    a.stats[a.stats_off + 1] = L.tm[1];
    a.stats[a.stats_off + 2] = (double)a.rows;
  }
}

}  // namespace cacto
