// Prioritized replay on the GPU: float64 sum/min segment trees in the exact node layout and
// combination order of segment_tree.py (so sampled indices are bit-exact), stratified proportional
// sampling, IS weights, the duplicate-once exp_counter update and last-write-wins priority updates
// (replay_buffer.py:87-218).
#include "internal.h"
#include "per_device.h"

namespace cacto {

constexpr int PER_THREADS = 1024;


__global__ void k_per_init(double* sum_tree, double* min_tree, int64_t n2) {
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n2; k += (int64_t)gridDim.x * blockDim.x) {
    sum_tree[k] = 0.0;
    min_tree[k] = __builtin_inf();
  }
}

// Leaves [start, start+n) mod ring get `value`; then every ancestor is recomputed bottom-up.
// Recomputing an ancestor from final children yields the value the sequential Python updates
// leave behind (each node's last recomputation follows its subtree's last leaf write).
__global__ void k_per_fill_leaves(double* sum_tree, double* min_tree, int64_t cap, int64_t ring, int64_t start, int64_t n,
                                  double value, const double* __restrict__ max_priority, double alpha) {
  // replay_buffer.py:133-135: new leaves = max_priority ** alpha, read on the device (no host sync)
  if (max_priority) value = pow(max_priority[0], alpha);
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
    const int64_t leaf = cap + (start + k) % ring;
    sum_tree[leaf] = value;
    min_tree[leaf] = value;
  }
}

// One level of ancestors of the leaf range: nodes [lo, hi] at this level.
__global__ void k_per_level(double* sum_tree, double* min_tree, int64_t lo, int64_t hi) {
  for (int64_t k = lo + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k <= hi; k += (int64_t)gridDim.x * blockDim.x) {
    sum_tree[k] = sum_tree[2 * k] + sum_tree[2 * k + 1];
    min_tree[k] = tree_min(min_tree[2 * k], min_tree[2 * k + 1]);
  }
}

// Top of the sum tree staged in LDS by the one-workgroup kernels: nodes [1, TOP_NODES).
constexpr int TOP_NODES = 1024;

// _reduce_helper(0, end, 1, 0, cap-1) for the sum tree (end inclusive): right-nested sum of the
// maximal left-aligned nodes, exactly as the recursion combines them. The path depends on `end`
// only, so every term is loaded independently (one memory latency, not one per level).
__device__ __noinline__ double prefix_reduce(const double* tree, int64_t cap, int64_t end) {
  constexpr int MAXD = 32;  // capacity <= 2^31 (int32 indices)
  double t[MAXD];
  bool v[MAXD];
  int64_t node = 1, ns = 0, ne = cap - 1;
  bool done = false;
#pragma unroll
  for (int k = 0; k < MAXD; ++k) {
    v[k] = false;
    t[k] = 0.0;
    if (!done) {
      if (end == ne) {
        t[k] = tree[node];
        v[k] = true;
        done = true;
      } else {
        const int64_t mid = (ns + ne) / 2;
        if (end <= mid) {
          node = 2 * node;
          ne = mid;
        } else {
          t[k] = tree[2 * node];
          v[k] = true;
          node = 2 * node + 1;
          ns = mid + 1;
        }
      }
    }
  }
  double r = 0.0;
  bool have = false;
#pragma unroll
  for (int k = MAXD - 1; k >= 0; --k)
    if (v[k]) {
      r = have ? t[k] + r : t[k];
      have = true;
    }
  return r;
}

// The one-workgroup sampler (B < PER_MW_MIN): 1,024 threads, up to SPT = 8 samples per thread, PG = 4
// of them in lock-step, a 1,024-node top, and the exp_counter increment inside.
__global__ void __launch_bounds__(PER_THREADS) k_per_sample(const double* __restrict__ sum_tree,
                                                           const double* __restrict__ min_tree, int64_t cap,
                                                           int64_t max_idx, double beta,
                                                           const double* __restrict__ uniforms, int B,
                                                           int32_t* __restrict__ idx_out, float* __restrict__ w_out,
                                                           double* __restrict__ exp_counter,
                                                           const double* __restrict__ shards, int n_shards) {
  constexpr int SPT = PER_MAX_B / PER_THREADS, PG = 4;
  __shared__ double seg_s, total_s, maxw_s, scale_s;
  __shared__ int32_t idx_s[PER_MAX_B];
  __shared__ double top_s[TOP_NODES];
  const int64_t ntop = cap < TOP_NODES ? cap : TOP_NODES;
  // thread 0 forms the batch scalars from global memory while the others stage the top (the same
  // node values either way), so the two memory latencies overlap
  if (threadIdx.x > 0)  // threads 1.. stage the top
    for (int k = threadIdx.x - 1; k < ntop; k += blockDim.x - 1) top_s[k] = k ? sum_tree[k] : 0.0;
  if (threadIdx.x == 0) {
    seg_s = prefix_reduce(sum_tree, cap, max_idx - 2) / B;  // sum(0, max_idx - 1) / B
    per_batch_scalars(sum_tree, min_tree, max_idx, beta, shards, n_shards, total_s, scale_s, maxw_s);
  }
  __syncthreads();
  const double seg = seg_s, total = total_s, maxw = maxw_s, scale = scale_s;
  // find_prefixsum_idx for every sample: the top levels from LDS, the rest in rounds of up to three
  // levels (per_round3: one memory latency per round instead of per level). The (up to 8) descents of
  // a thread advance in lock-step, PG at a time, so their loads overlap too.
  int64_t node[SPT];
#pragma unroll
  for (int g = 0; g < SPT; g += PG) {
    if (threadIdx.x + g * blockDim.x >= (unsigned)B) {
#pragma unroll
      for (int j = g; j < g + PG; ++j) node[j] = cap;
      continue;
    }
    double p[PG];
    int64_t nd[PG];
#pragma unroll
    for (int jj = 0; jj < PG; ++jj) {
      const int i = threadIdx.x + (g + jj) * blockDim.x;
      p[jj] = i < B ? uniforms[i] * seg + i * seg : 0.0;
      nd[jj] = 1;
      if (i < B)
        while (2 * nd[jj] < ntop) per_step(top_s[2 * nd[jj]], p[jj], nd[jj]);
    }
    auto live = [&](int jj) { return threadIdx.x + (g + jj) * blockDim.x < (unsigned)B && nd[jj] < cap; };
    while (true) {
      bool any = false;
#pragma unroll
      for (int jj = 0; jj < PG; ++jj) any |= live(jj);
      if (!any) break;
      PerRound3 r[PG];
#pragma unroll
      for (int jj = 0; jj < PG; ++jj) r[jj] = per_round3_load<false>(sum_tree, nd[jj], live(jj), cap);
#pragma unroll
      for (int jj = 0; jj < PG; ++jj) per_round3<false>(r[jj], live(jj), cap, p[jj], nd[jj]);
    }
#pragma unroll
    for (int jj = 0; jj < PG; ++jj) node[g + jj] = nd[jj];
  }
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    const int i = threadIdx.x + j * blockDim.x;
    if (i < B) {
      const int32_t id = (int32_t)(node[j] - cap);
      idx_s[i] = id;
      idx_out[i] = id;
      const double pr = sum_tree[node[j]] / total;
      w_out[i] = (float)(pow(pr * scale, -beta) / maxw);
    }
  }
  __syncthreads();
  if (exp_counter) per_count_once<PER_THREADS>(idx_s, B, exp_counter);
}

// The multi-workgroup sampler (B >= PER_MW_MIN): per_sample_body (per_device.h)
// with an 8,192-node top, one sample per thread, 256 per workgroup. exp_counter follows in k_per_count.
__global__ void __launch_bounds__(256) k_per_sample_mw(PerSampleArgs a) {
  __shared__ double top_s[PER_MW_TOP];
  __shared__ double scal_s[4];
  per_sample_body<PER_MW_TOP>(blockIdx.x, a, top_s, scal_s);
}

// The pipelined PER loop's first sample (the later ones run inside k_adam_sample): the 4,096-node top
// of the fused form, with the per-subtree runs for per_update_run_body.
__global__ void __launch_bounds__(256) k_per_sample_runs(PerSampleArgs a) {
  __shared__ double top_s[PER_FUSED_TOP];
  __shared__ double scal_s[4];
  per_sample_body<PER_FUSED_TOP>(blockIdx.x, a, top_s, scal_s);
}

// The priority-update kernels' arguments (PerLeafArgs: the trees and what the leaves are formed from).
struct PerUpdateArgs {
  PerLeafArgs leaf;
  const int32_t* idx;
  int n;
  double* exp_counter;
  double* max_priority;
  const int32_t* skip;  // an int status that, when set, leaves everything unchanged (the ReLO rule's error flag)
};

// The leaf writes of the chain (capacity 2^21) over many workgroups, one leaf per thread (the two f64
// pows of a priority are the serial work): every workgroup checks the whole index list for order
// itself, so all take the same occurrence test. Same leaf values, same last-write-wins, same max as
// k_per_set (bit-identical).
__global__ void __launch_bounds__(256) k_per_leaves_mw(PerUpdateArgs a) {
  if (a.skip && *a.skip) return;
  const bool sorted = per_list_sorted<256>(a.idx, a.n);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double my_max = -__builtin_inf(), leaf;
  if (i < a.n) per_leaf_update(a.leaf, a.idx, a.n, i, sorted, a.exp_counter + a.idx[i], 0.0, my_max, leaf);
  per_publish_max(my_max, a.max_priority);
}

// exp_counter[idxes] += 1 after a multi-workgroup sample (numpy's fancy-index increment counts each
// distinct index once). With a sorted index list (the stratified sampler's output) each distinct
// index is incremented by the thread of its first occurrence alone, so no thread reads a counter
// another one writes; an unsorted list (checked by every workgroup) is counted by workgroup 0 with
// every read before any write. Same counters either way.
__global__ void __launch_bounds__(256) k_per_count(const int32_t* __restrict__ idx, int B,
                                                     double* __restrict__ exp_counter) {
  if (per_list_sorted<256>(idx, B)) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B && per_first_occ(idx, 0, i, true)) exp_counter[idx[i]] += 1.0;
    return;
  }
  if (blockIdx.x == 0) per_count_once<256>(idx, B, exp_counter);
}

// Ancestor refresh of the chain as whole subtrees in LDS: workgroup s loads the SUB leaves
// [cap + s SUB, cap + (s + 1) SUB) of both trees and rebuilds the subtree (per_rebuild_subtree).
// One memory latency per workgroup instead of one barrier-separated global round per level.
constexpr int PER_SUB = 1024;
__global__ void __launch_bounds__(256) k_per_subtrees(double* __restrict__ sum_tree, double* __restrict__ min_tree,
                                                     int64_t cap, int sub) {
  __shared__ double ts[2 * PER_SUB], tm[2 * PER_SUB];  // local node j (1-based heap of the subtree)
  const int64_t leaf0 = cap + (int64_t)blockIdx.x * sub;
  for (int k = threadIdx.x; k < sub; k += blockDim.x) {
    ts[sub + k] = sum_tree[leaf0 + k];
    tm[sub + k] = min_tree[leaf0 + k];
  }
  __syncthreads();
  per_rebuild_subtree<256, false>(ts, tm, sub, leaf0, false, sum_tree, min_tree);
}

// A whole priority update as one launch over the subtrees of `sub` leaves (large batches): workgroup s
// owns leaves [cap + s sub, cap + (s + 1) sub), so every sample whose index falls there — every write
// of those leaves, of their exp_counter entries and of the subtree's internal nodes — belongs to one
// workgroup, and no two workgroups write the same word. Per workgroup:
//   1. its samples: with a sorted index list (the stratified sampler's output) the contiguous run
//      [lower_bound(s sub), lower_bound((s + 1) sub)), two binary searches; otherwise a filter over
//      the whole list (every workgroup checks the order itself, so all take the same branch);
//   2. the leaves (per_leaf_update), duplicates last-write-wins, into the subtree staged in LDS and
//      into the trees; count = 1 also applies the sampler's exp_counter += 1 first (numpy's
//      fancy-index increment: once per distinct index; every occurrence reads the old count, the
//      first one then writes old + 1 after a barrier), so the pipelined update needs no separate
//      counting launch;
//   3. the subtree's levels rebuilt in LDS and written back, the root at agent scope;
//   4. the last workgroup to finish rebuilds the nodes above the subtree roots (per_last_workgroup).
// A set `skip` flag leaves the trees, counters and max_priority unchanged. Every value is formed as
// on the chain and in k_per_set, so the results are bit-identical to both.
constexpr int PER_FUSED_MAX_ROOTS = PER_SUB;  // the top fits the subtree's LDS arrays
__global__ void __launch_bounds__(256) k_per_update_sub(PerUpdateArgs a, int sub, int count) {
  // 64 KiB: both subtrees and the index list (binary searches and neighbour tests in LDS); the
  // unused heap slots ts[0] / tm[0] hold the run bounds and the last-workgroup flag
  __shared__ double ts[2 * PER_SUB], tm[2 * PER_SUB];  // local node j (1-based heap of the subtree)
  __shared__ int32_t id_s[PER_MAX_B];
  int* run_s = reinterpret_cast<int*>(&ts[0]);
  int* last_s = reinterpret_cast<int*>(&tm[0]);
  if (a.skip && *a.skip) return;  // uniform: every workgroup returns, the counter stays 0
  double* __restrict__ sum_tree = a.leaf.sum_tree;
  double* __restrict__ min_tree = a.leaf.min_tree;
  double* __restrict__ exp_counter = a.exp_counter;
  const int n = a.n;
  const int tid = threadIdx.x;
  const int64_t cap = a.leaf.cap, id_lo = (int64_t)blockIdx.x * sub, id_hi = id_lo + sub;
  const int64_t leaf0 = cap + id_lo;
  // the index list and both subtrees' leaves: every load in flight before the first LDS write (a
  // plain staging loop waited for each load in turn: 16 + 4 dependent memory latencies at B = 4096)
  {
    constexpr int NI = PER_MAX_B / 256, NL = PER_SUB / 256;
    int iv[NI];
    double sv[NL], mv[NL];
#pragma unroll
    for (int j = 0; j < NI; ++j) iv[j] = tid + 256 * j < n ? a.idx[tid + 256 * j] : 0;
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const int k = tid + 256 * j;
      sv[j] = k < sub ? sum_tree[leaf0 + k] : 0.0;
      mv[j] = k < sub ? min_tree[leaf0 + k] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < NI; ++j)
      if (tid + 256 * j < n) id_s[tid + 256 * j] = iv[j];
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const int k = tid + 256 * j;
      if (k < sub) {
        ts[sub + k] = sv[j];
        tm[sub + k] = mv[j];
      }
    }
  }
  __syncthreads();
  const bool sorted = per_list_sorted<256>(id_s, n);
  if (sorted && tid < 2) {  // lower_bound of id_lo (thread 0) and id_hi (thread 1)
    const int64_t key = tid ? id_hi : id_lo;
    int lo = 0, hi = n;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if ((int64_t)id_s[mid] < key) lo = mid + 1;
      else hi = mid;
    }
    run_s[tid] = lo;
  }
  __syncthreads();
  const int ra = sorted ? run_s[0] : 0, rb = sorted ? run_s[1] : n;
  auto mine = [&](int i) {
    if (sorted) return true;
    const int64_t id = id_s[i];
    return id >= id_lo && id < id_hi;
  };
  double my_max = -__builtin_inf();
  for (int i = ra + tid; i < rb; i += 256) {
    if (!mine(i)) continue;
    const int32_t id = id_s[i];
    double leaf;
    if (per_leaf_update(a.leaf, id_s, n, i, sorted, exp_counter + id, count ? 1.0 : 0.0, my_max, leaf)) {
      ts[sub + (id - id_lo)] = leaf;
      tm[sub + (id - id_lo)] = leaf;
    }
  }
  per_publish_max(my_max, a.max_priority);
  __syncthreads();  // every occurrence has read its old count; the leaves are in LDS
  if (count && exp_counter && !a.leaf.vals)
    for (int i = ra + tid; i < rb; i += 256)
      if (mine(i) && per_first_occ(id_s, 0, i, sorted)) exp_counter[id_s[i]] += 1.0;
  const int nroot = (int)(cap / sub);
  per_rebuild_subtree<256, false>(ts, tm, sub, leaf0, nroot > 1, sum_tree, min_tree);
  if (nroot > 1) per_last_workgroup<256, false>(sum_tree, min_tree, nroot, last_s, ts, tm);
}

// The nodes above the subtree roots, [1, cap / sub), from the roots (one workgroup, LDS).
__global__ void __launch_bounds__(PER_THREADS) k_per_top(double* __restrict__ sum_tree, double* __restrict__ min_tree,
                                                        int nroot) {
  extern __shared__ double sh[];  // 2 nroot sums, then 2 nroot mins
  double* ts = sh;
  double* tm = sh + 2 * nroot;
  for (int k = nroot + threadIdx.x; k < 2 * nroot; k += blockDim.x) {
    ts[k] = sum_tree[k];
    tm[k] = min_tree[k];
  }
  __syncthreads();
  per_rebuild_top<PER_THREADS, false>(ts, tm, nroot, sum_tree, min_tree);
}

// This shard's (sum, min, row count) for the data-parallel exchange of cacto_per_sample_global.
__global__ void k_per_shard_stats(const double* __restrict__ sum_tree, const double* __restrict__ min_tree,
                                  int64_t max_idx, double* __restrict__ stats) {
  if (threadIdx.x == 0) {
    stats[0] = sum_tree[1];
    stats[1] = min_tree[1];
    stats[2] = (double)max_idx;
  }
}

// The one-workgroup priority update (small batches, and trees of more than 2,048 subtrees): leaf
// writes with last-write-wins among duplicates, then ancestor refresh level by level.
__global__ void __launch_bounds__(PER_THREADS) k_per_set(PerUpdateArgs a) {
  __shared__ int32_t id_s[PER_MAX_B];
  if (a.skip && *a.skip) return;
  __shared__ double maxp_s[PER_THREADS / 64];
  __shared__ double top_sum[TOP_NODES], top_min[TOP_NODES];
  double* sum_tree = a.leaf.sum_tree;
  double* min_tree = a.leaf.min_tree;
  const int64_t cap = a.leaf.cap;
  const int n = a.n;
  double my_max = -__builtin_inf();
  for (int i = threadIdx.x; i < n; i += blockDim.x) id_s[i] = a.idx[i];
  __syncthreads();
  const bool sorted = per_list_sorted<PER_THREADS>(id_s, n);
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    double leaf;
    per_leaf_update(a.leaf, id_s, n, i, sorted, a.exp_counter + id_s[i], 0.0, my_max, leaf);
  }
  // one workgroup: max_priority takes a plain fmax (not per_publish_max's atomic on the bit pattern,
  // which orders a NaN or negative max_priority differently); wave reduction, then across the waves
  if (a.max_priority) {
    double m = my_max;
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63) == 0) maxp_s[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
      double mm = maxp_s[0];
      for (int w = 1; w < (int)(blockDim.x >> 6); ++w) mm = fmax(mm, maxp_s[w]);
      a.max_priority[0] = fmax(a.max_priority[0], mm);
    }
  }
  __syncthreads();
  // Ancestors below the LDS-staged top, one level per barrier. With sorted indices a node is
  // refreshed only by the first sample below it (the others would rewrite the same value). Each
  // thread loads the children of all its nodes before storing any parent, so the loads overlap.
  constexpr int PT = PER_MAX_B / PER_THREADS;
  int log2cap = 0;
  while (((int64_t)1 << log2cap) < cap) ++log2cap;
  const int ntop = (int)(cap < TOP_NODES / 2 ? cap : TOP_NODES / 2);  // rows [ntop, 2 ntop) fit the LDS arrays
  int log2top = 0;
  while ((1 << log2top) < ntop) ++log2top;
  for (int shift = 1; shift <= log2cap - log2top; ++shift) {
    int64_t nd[PT];
    double s0[PT], s1[PT], m0[PT], m1[PT];
#pragma unroll
    for (int j = 0; j < PT; ++j) {
      const int i = threadIdx.x + j * blockDim.x;
      nd[j] = 0;
      if (i < n) {
        const int64_t x = (cap + id_s[i]) >> shift;
        if (!(sorted && i > 0 && ((cap + id_s[i - 1]) >> shift) == x)) nd[j] = x;
      }
      if (nd[j]) {
        s0[j] = sum_tree[2 * nd[j]];
        s1[j] = sum_tree[2 * nd[j] + 1];
        m0[j] = min_tree[2 * nd[j]];
        m1[j] = min_tree[2 * nd[j] + 1];
      }
    }
#pragma unroll
    for (int j = 0; j < PT; ++j)
      if (nd[j]) {
        sum_tree[nd[j]] = s0[j] + s1[j];
        min_tree[nd[j]] = tree_min(m0[j], m1[j]);
      }
    __syncthreads();
  }
  // The top: its bottom row [ntop, 2 ntop) is current now; rebuild nodes [1, ntop). Nodes no sample
  // touched come out unchanged (the tree is consistent, the op is deterministic).
  for (int k = ntop + threadIdx.x; k < 2 * ntop; k += blockDim.x) {
    top_sum[k] = sum_tree[k];
    top_min[k] = min_tree[k];
  }
  __syncthreads();
  per_rebuild_top<PER_THREADS, false>(top_sum, top_min, ntop, sum_tree, min_tree);
}

}  // namespace cacto

using namespace cacto;

static bool pow2(int64_t c) { return c > 0 && (c & (c - 1)) == 0; }

extern "C" int cacto_per_init(double* sum_tree_d, double* min_tree_d, int64_t capacity, void* stream) {
  CACTO_REQUIRE(sum_tree_d && min_tree_d && pow2(capacity), "cacto_per_init: capacity must be a power of two");
  hipLaunchKernelGGL(k_per_init, dim3((unsigned)std::min<int64_t>((2 * capacity + 255) / 256, 4096)), dim3(256), 0,
                     as_stream(stream), sum_tree_d, min_tree_d, 2 * capacity);
  CACTO_CHECK_HIP(hipGetLastError());
  return CACTO_OK;
}

namespace {
int per_set_range(double* sum_tree_d, double* min_tree_d, int64_t capacity, int64_t ring_size, int64_t start,
                  int64_t n, double value, const double* max_priority_d, double alpha, hipStream_t st) {
  CACTO_REQUIRE(sum_tree_d && min_tree_d && pow2(capacity) && ring_size > 0 && ring_size <= capacity && n >= 0 &&
                    start >= 0 && start < ring_size,
                "cacto_per_set_range: bad arguments");
  if (n == 0) return CACTO_OK;
  n = std::min(n, ring_size);
  hipLaunchKernelGGL(k_per_fill_leaves, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, st,
                     sum_tree_d, min_tree_d, capacity, ring_size, start, n, value, max_priority_d, alpha);
  CACTO_CHECK_HIP(hipGetLastError());
  // affected leaf interval(s); refresh the covering node interval per level (superset is harmless)
  const int64_t a = start, b = start + n - 1;
  int64_t lo = capacity + (b < ring_size ? a : 0), hi = capacity + (b < ring_size ? b : ring_size - 1);
  while (lo > 1) {
    lo >>= 1;
    hi >>= 1;
    const int64_t cnt = hi - lo + 1;
    hipLaunchKernelGGL(k_per_level, dim3((unsigned)std::min<int64_t>((cnt + 255) / 256, 4096)), dim3(256), 0, st,
                       sum_tree_d, min_tree_d, lo, hi);
    CACTO_CHECK_HIP(hipGetLastError());
  }
  return CACTO_OK;
}
}  // namespace

// The route: which kernels a sample of B and a priority update of B take on a tree of `capacity`
// leaves. Batches of at least PER_MW_MIN samples take the multi-workgroup paths: the descents one
// sample per thread over 256-thread workgroups (+ k_per_count, or the count deferred into the
// priority update of the pipelined loops), and the priority update as one launch over the subtrees
// (k_per_update_sub), or — the one tree whose roots outgrow that kernel's LDS but fit k_per_top's,
// capacity 2^21 — as the chain k_per_leaves_mw, k_per_subtrees, k_per_top. Smaller batches, and
// larger trees still, keep the one-workgroup kernels. Every path forms the same values
// (bit-identical indices, weights, trees). Launches nothing; cacto_per_plan reports it.
PerRoute cacto::per_route(int64_t capacity, int B) {
  // k_per_top stages both trees' roots and their parents (4 nroot doubles) in dynamic LDS, which is
  // 64 KiB per workgroup without an opt-in attribute
  constexpr int64_t CHAIN_MAX_ROOTS = 2048;
  static_assert(4 * CHAIN_MAX_ROOTS * sizeof(double) <= 65536, "k_per_top: dynamic LDS above 64 KiB");
  const bool mw = B >= PER_MW_MIN;
  const int64_t sub = std::min<int64_t>(PER_SUB, capacity), roots = capacity / sub;
  PerRoute r;
  r.sampler = mw;
  r.sampler_top = mw ? PER_MW_TOP : TOP_NODES;
  r.sampler_wgs = mw ? (B + 255) / 256 : 1;
  r.count_deferred = mw;
  r.update = mw && roots <= PER_FUSED_MAX_ROOTS ? PER_UPDATE_SUB
             : !mw || roots > CHAIN_MAX_ROOTS   ? PER_UPDATE_SET
                                                : PER_UPDATE_CHAIN;
  r.update_sub = (int32_t)sub;
  r.update_roots = (int32_t)roots;
  // the overlapped form of the pipelined loops: 256-leaf subtrees whose roots fit one workgroup
  r.overlap_shape = mw && capacity >= 2 * PER_RUN_SUB && capacity <= (int64_t)PER_RUN_SUB * PER_RUN_SUB;
  return r;
}

namespace {
int launch_per_count(const int32_t* idx_d, int B, double* exp_counter_d, hipStream_t st) {
  hipLaunchKernelGGL(k_per_count, dim3((B + 255) / 256), dim3(256), 0, st, idx_d, B, exp_counter_d);
  CACTO_CHECK_HIP(hipGetLastError());
  return CACTO_OK;
}

// runs_d: k_per_sample_runs (the 4,096-node top, recording the per-subtree runs) in place of the
// route's sampler
int launch_per_sample(const double* sum_tree_d, const double* min_tree_d, int64_t capacity, int64_t max_idx,
                      double beta, const double* uniforms_d, int B, int32_t* idx_d, float* is_w_d,
                      double* exp_counter_d, const double* shards_d, int n_shards, hipStream_t st,
                      int32_t* runs_d = nullptr, bool runs_form = false) {
  const PerRoute r = per_route(capacity, B);
  if (!r.sampler && !runs_form) {
    hipLaunchKernelGGL(k_per_sample, dim3(1), dim3(PER_THREADS), 0, st, sum_tree_d, min_tree_d, capacity, max_idx,
                       beta, uniforms_d, B, idx_d, is_w_d, exp_counter_d, shards_d, n_shards);
    CACTO_CHECK_HIP(hipGetLastError());
    return CACTO_OK;
  }
  const PerSampleArgs sa{sum_tree_d, min_tree_d, capacity, max_idx, beta, uniforms_d, B, idx_d, is_w_d,
                         shards_d, n_shards, runs_d};
  if (runs_form) hipLaunchKernelGGL(k_per_sample_runs, dim3((B + 255) / 256), dim3(256), 0, st, sa);
  else hipLaunchKernelGGL(k_per_sample_mw, dim3(r.sampler_wgs), dim3(256), 0, st, sa);
  CACTO_CHECK_HIP(hipGetLastError());
  return exp_counter_d ? launch_per_count(idx_d, B, exp_counter_d, st) : CACTO_OK;
}

// count = 1: exp_counter += 1 (the sampler's count, deferred) applied inside the priority update
int launch_per_set(const PerUpdateArgs& a, hipStream_t st, int count = 0) {
  const int64_t capacity = a.leaf.cap;
  const PerRoute r = per_route(capacity, a.n);
  if (r.update == PER_UPDATE_SUB) {
    hipLaunchKernelGGL(k_per_update_sub, dim3(r.update_roots), dim3(256), 0, st, a, r.update_sub, count);
    CACTO_CHECK_HIP(hipGetLastError());
    return CACTO_OK;
  }
  if (count)
    if (int e = launch_per_count(a.idx, a.n, a.exp_counter, st)) return e;
  if (r.update == PER_UPDATE_SET) {
    hipLaunchKernelGGL(k_per_set, dim3(1), dim3(PER_THREADS), 0, st, a);
    CACTO_CHECK_HIP(hipGetLastError());
    return CACTO_OK;
  }
  hipLaunchKernelGGL(k_per_leaves_mw, dim3((a.n + 255) / 256), dim3(256), 0, st, a);
  CACTO_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_per_subtrees, dim3(r.update_roots), dim3(256), 0, st, a.leaf.sum_tree, a.leaf.min_tree,
                     capacity, r.update_sub);
  CACTO_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_per_top, dim3(1), dim3(PER_THREADS), (size_t)4 * r.update_roots * sizeof(double), st,
                     a.leaf.sum_tree, a.leaf.min_tree, r.update_roots);
  CACTO_CHECK_HIP(hipGetLastError());
  return CACTO_OK;
}
}  // namespace

#ifdef CACTO_STAMPS
extern "C" int cacto_debug_per_stamps(unsigned long long* out_h) {  // [64][8], this TU's samplers
  CACTO_CHECK_HIP(hipDeviceSynchronize());
  CACTO_CHECK_HIP(hipMemcpyFromSymbol(out_h, HIP_SYMBOL(cacto::g_per_stamps), sizeof(unsigned long long) * 64 * 8));
  return CACTO_OK;
}
#endif

extern "C" int cacto_per_plan(int64_t capacity, int B, struct cacto_per_plan* out) {
  CACTO_REQUIRE(out && pow2(capacity) && B >= 1 && B <= PER_MAX_B,
                "cacto_per_plan: need out, a power-of-two capacity and 1 <= B <= 8192");
  *out = per_route(capacity, B);
  return CACTO_OK;
}

// The pipelined loops' exp_counter += 1 of a deferred count alone (alpha == 0: no priority update
// follows), and their priority update with the deferred count applied first (the count's only
// reader is this update): one launch where the route is k_per_update_sub.
int cacto_per_count_launch(const int32_t* idx_d, int B, double* exp_counter_d, hipStream_t st) {
  return launch_per_count(idx_d, B, exp_counter_d, st);
}
int cacto_per_update_count(double* sum_tree_d, double* min_tree_d, int64_t capacity, const int32_t* idx_d,
                           const float* y_d, const float* V_d, double* exp_counter_d, double fresh_factor, double eps,
                           double alpha, double* max_priority_d, int B, hipStream_t st) {
  return launch_per_set(PerUpdateArgs{{sum_tree_d, min_tree_d, capacity, nullptr, y_d, V_d, fresh_factor, eps, alpha},
                                      idx_d, B, exp_counter_d, max_priority_d, nullptr},
                        st, 1);
}

extern "C" int cacto_per_set_range(double* sum_tree_d, double* min_tree_d, int64_t capacity, int64_t ring_size,
                                   int64_t start, int64_t n, double value, void* stream) {
  return per_set_range(sum_tree_d, min_tree_d, capacity, ring_size, start, n, value, nullptr, 0.0, as_stream(stream));
}

extern "C" int cacto_per_set_range_max(double* sum_tree_d, double* min_tree_d, int64_t capacity, int64_t ring_size,
                                       int64_t start, int64_t n, const double* max_priority_d, double alpha,
                                       void* stream) {
  CACTO_REQUIRE(max_priority_d, "cacto_per_set_range_max: null max_priority_d");
  return per_set_range(sum_tree_d, min_tree_d, capacity, ring_size, start, n, 0.0, max_priority_d, alpha,
                       as_stream(stream));
}

extern "C" int cacto_per_sample(const double* sum_tree_d, const double* min_tree_d, int64_t capacity, int64_t max_idx,
                                double beta, const double* uniforms_d, int B, int32_t* idx_d, float* is_w_d,
                                double* exp_counter_d, void* stream) {
  CACTO_REQUIRE(sum_tree_d && min_tree_d && uniforms_d && idx_d && is_w_d && pow2(capacity),
                "cacto_per_sample: bad arguments");
  CACTO_REQUIRE(B > 0 && B <= PER_MAX_B, "cacto_per_sample: 0 < B <= 8192");
  // max_idx <= 1 makes the reference's sum(0, max_idx - 1) recurse past the leaves (segment_tree.py:36-49)
  CACTO_REQUIRE(max_idx >= 2 && max_idx <= capacity, "cacto_per_sample: need 2 <= max_idx <= capacity");
  return launch_per_sample(sum_tree_d, min_tree_d, capacity, max_idx, beta, uniforms_d, B, idx_d, is_w_d, exp_counter_d,
                           nullptr, 0, as_stream(stream));
}

// The overlapped loops' first sample (learn_host.hip, per_first_sample; the later ones run inside
// k_adam_sample): k_per_sample_runs at any B, recording the per-subtree runs when runs_d is given.
extern "C" int cacto_per_sample_runs(const double* sum_tree_d, const double* min_tree_d, int64_t capacity,
                                     int64_t max_idx, double beta, const double* uniforms_d, int B, int32_t* idx_d,
                                     float* is_w_d, double* exp_counter_d, int32_t* runs_d,
                                     const double* shard_stats_d, int n_shards, void* stream) {
  CACTO_REQUIRE(sum_tree_d && min_tree_d && uniforms_d && idx_d && is_w_d && pow2(capacity) &&
                    (shard_stats_d ? n_shards > 0 : n_shards == 0),
                "cacto_per_sample_runs: bad arguments");
  CACTO_REQUIRE(B > 0 && B <= PER_MAX_B, "cacto_per_sample_runs: 0 < B <= 8192");
  CACTO_REQUIRE(max_idx >= 2 && max_idx <= capacity, "cacto_per_sample_runs: need 2 <= max_idx <= capacity");
  CACTO_REQUIRE(!runs_d || capacity >= 2 * PER_RUN_SUB, "cacto_per_sample_runs: runs_d needs capacity >= 512");
  return launch_per_sample(sum_tree_d, min_tree_d, capacity, max_idx, beta, uniforms_d, B, idx_d, is_w_d, exp_counter_d,
                           shard_stats_d, n_shards, as_stream(stream), runs_d, true);
}

extern "C" int cacto_per_shard_stats(const double* sum_tree_d, const double* min_tree_d, int64_t max_idx,
                                     double* stats_d, void* stream) {
  CACTO_REQUIRE(sum_tree_d && min_tree_d && stats_d && max_idx >= 0, "cacto_per_shard_stats: bad arguments");
  hipLaunchKernelGGL(k_per_shard_stats, dim3(1), dim3(64), 0, as_stream(stream), sum_tree_d, min_tree_d, max_idx,
                     stats_d);
  CACTO_CHECK_HIP(hipGetLastError());
  return CACTO_OK;
}

extern "C" int cacto_per_sample_global(const double* sum_tree_d, const double* min_tree_d, int64_t capacity,
                                       int64_t max_idx, double beta, const double* uniforms_d, int B,
                                       const double* shard_stats_d, int n_shards, int32_t* idx_d, float* is_w_d,
                                       double* exp_counter_d, void* stream) {
  CACTO_REQUIRE(sum_tree_d && min_tree_d && uniforms_d && idx_d && is_w_d && shard_stats_d && n_shards > 0 &&
                    pow2(capacity),
                "cacto_per_sample_global: bad arguments");
  CACTO_REQUIRE(B > 0 && B <= PER_MAX_B, "cacto_per_sample_global: 0 < B <= 8192");
  CACTO_REQUIRE(max_idx >= 2 && max_idx <= capacity, "cacto_per_sample_global: need 2 <= max_idx <= capacity");
  return launch_per_sample(sum_tree_d, min_tree_d, capacity, max_idx, beta, uniforms_d, B, idx_d, is_w_d, exp_counter_d,
                           shard_stats_d, n_shards, as_stream(stream));
}

extern "C" int cacto_per_update(double* sum_tree_d, double* min_tree_d, int64_t capacity, const int32_t* idx_d,
                                const float* y_d, const float* V_d, const double* exp_counter_d, double fresh_factor,
                                double eps, double alpha, double* max_priority_d, int B, void* stream) {
  CACTO_REQUIRE(sum_tree_d && min_tree_d && idx_d && y_d && V_d && exp_counter_d && max_priority_d && pow2(capacity),
                "cacto_per_update: bad arguments");
  CACTO_REQUIRE(B > 0 && B <= PER_MAX_B, "cacto_per_update: 0 < B <= 8192");
  return launch_per_set(PerUpdateArgs{{sum_tree_d, min_tree_d, capacity, nullptr, y_d, V_d, fresh_factor, eps, alpha},
                                      idx_d, B, const_cast<double*>(exp_counter_d), max_priority_d, nullptr},
                        as_stream(stream));
}

// update_priorities 'ReLO' (replay_buffer.py:193-196, :200-218; dead in the shipped reference,
// RB_type is never set): td_i = MSE(y, V)_i - MSE(y, V_tgt)_i with Keras MeanSquaredError
// (reduction NONE, so per sample: f32 (V - y)^2 over the size-1 last axis), clipped as numpy clips
// it, np.minimum(np.maximum(td, 0), max(td)); then p = fresh^count (f64) * td_norm (f32 -> f64, numpy
// promotion) + eps in f64 — unlike the 'PER' branch, whose TF tensor keeps p in f32. One workgroup
// (B <= PER_MAX_B): the per-sample leaves p^alpha go to leaves[], max_priority takes the batch max.
// The reference asserts p > 0 for every sample (replay_buffer.py:212). It fails when every td is
// negative (np.clip's upper bound max(td) < 0 then gives p = fresh^c max(td) + eps, possibly <= 0) or
// when any td is NaN (np.max propagates it, so every p is NaN): then *status = 1 and nothing is
// written — no leaf, no max_priority — and the leaf pass that follows skips on the flag, so the
// trees are unchanged. A set status (sticky until the host clears it) makes later calls no-ops too.
__global__ void __launch_bounds__(PER_THREADS) k_per_relo(const int32_t* __restrict__ idx, const float* __restrict__ y,
                                                         const float* __restrict__ V, const float* __restrict__ Vt,
                                                         const double* __restrict__ exp_counter, double fresh,
                                                         double eps, double alpha, int B, double* __restrict__ leaves,
                                                         double* __restrict__ max_priority, int32_t* status) {
  __shared__ float red_f[PER_THREADS / 64];
  __shared__ double red_d[PER_THREADS / 64];
  if (*status) return;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  auto td_of = [&](int i) {
    const float d1 = __fsub_rn(V[i], y[i]), d2 = __fsub_rn(Vt[i], y[i]);
    return __fsub_rn(__fmul_rn(d1, d1), __fmul_rn(d2, d2));
  };
  float mx = -__builtin_inff();
  bool nan_td = false;
  for (int i = tid; i < B; i += blockDim.x) {
    const float td = td_of(i);
    nan_td |= td != td;
    mx = fmaxf(mx, td);
  }
  for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
  if (lane == 0) red_f[wv] = mx;
  __syncthreads();
  mx = red_f[0];
  for (int k = 1; k < (int)(blockDim.x / 64); ++k) mx = fmaxf(mx, red_f[k]);
  double pm = -__builtin_inf();
  bool bad = nan_td;
  double leaf[PER_MAX_B / PER_THREADS];
  int k = 0;
  for (int i = tid; i < B; i += blockDim.x, ++k) {
    const float tn = fminf(fmaxf(td_of(i), 0.f), mx);
    const double p = pow(fresh, exp_counter[idx[i]]) * (double)tn + eps;
    bad |= !(p > 0.0);
    leaf[k] = pow(p, alpha);
    pm = fmax(pm, p);
  }
  if (__syncthreads_or(bad)) {
    if (tid == 0) *status = 1;
    return;
  }
  k = 0;
  for (int i = tid; i < B; i += blockDim.x, ++k) leaves[i] = leaf[k];
  for (int off = 32; off > 0; off >>= 1) pm = fmax(pm, __shfl_xor(pm, off));
  if (lane == 0) red_d[wv] = pm;
  __syncthreads();
  if (tid == 0) {
    double m = max_priority[0];
    for (int q = 0; q < (int)(blockDim.x / 64); ++q) m = fmax(m, red_d[q]);
    max_priority[0] = m;
  }
}

extern "C" int cacto_per_update_relo(double* sum_tree_d, double* min_tree_d, int64_t capacity, const int32_t* idx_d,
                                     const float* y_d, const float* V_d, const float* Vt_d,
                                     const double* exp_counter_d, double fresh_factor, double eps, double alpha,
                                     double* max_priority_d, double* leaves_ws_d, int32_t* status_d, int B,
                                     void* stream) {
  CACTO_REQUIRE(sum_tree_d && min_tree_d && idx_d && y_d && V_d && Vt_d && exp_counter_d && max_priority_d &&
                    leaves_ws_d && status_d && pow2(capacity),
                "cacto_per_update_relo: bad arguments");
  CACTO_REQUIRE(B > 0 && B <= PER_MAX_B, "cacto_per_update_relo: 0 < B <= 8192");
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(k_per_relo, dim3(1), dim3(PER_THREADS), 0, st, idx_d, y_d, V_d, Vt_d, exp_counter_d, fresh_factor,
                     eps, alpha, B, leaves_ws_d, max_priority_d, status_d);
  CACTO_CHECK_HIP(hipGetLastError());
  return launch_per_set(PerUpdateArgs{{sum_tree_d, min_tree_d, capacity, leaves_ws_d, nullptr, nullptr, 0.0, 0.0, 0.0},
                                      idx_d, B, nullptr, nullptr, status_d},
                        st);
}

extern "C" int cacto_per_set_leaves(double* sum_tree_d, double* min_tree_d, int64_t capacity, const int32_t* idx_d,
                                    const double* values_d, int n, void* stream) {
  CACTO_REQUIRE(sum_tree_d && min_tree_d && idx_d && values_d && pow2(capacity), "cacto_per_set_leaves: bad arguments");
  CACTO_REQUIRE(n > 0 && n <= PER_MAX_B, "cacto_per_set_leaves: 0 < n <= 8192");
  return launch_per_set(PerUpdateArgs{{sum_tree_d, min_tree_d, capacity, values_d, nullptr, nullptr, 0.0, 0.0, 0.0},
                                      idx_d, n, nullptr, nullptr, nullptr},
                        as_stream(stream));
}
