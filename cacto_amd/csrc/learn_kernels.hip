// Learner kernels: the per-sample chains of NN.compute_critic_grad (Sobolev, double backprop)
// and NN.compute_actor_grad (dynamics Jacobian path), the weight-gradient GEMM (K = samples,
// split-K partial slabs), and the fused slab-reduce + Keras Adam + packed refresh (+ soft update).
//
// Data flow per update (workspace, float32):
//   chain kernel (16 samples / workgroup) -> per-layer operand panels LT_l [in_pad][ld], RT_l
//   [out_pad][ld] (feature-major, sample rows contiguous) such that
//        dW_l = sum_rows LT_l[:, r] (x) RT_l[:, r],  db_l = sum_{rows >= bias_r0} RT_l[:, r]
//   critic rows: [0, Bp) = (Gbar_l, D_l) (Sobolev term), [Bp, 2Bp) = (h_l, zbar_l) (plain backprop)
//   actor rows : [0, Bp) = (h_l, zbar_l)
//   -> k_wgrad: one wave per (layer, 16x16 output tile | bias tile, row chunk) -> slab[chunk][P]
//   -> k_adam : sum chunks in fixed order (deterministic), Adam, packed copies, soft update.
// The host side (workspace, C ABI, update pipelines) is learn_host.hip; the two meet in learn.h.
// The chain device functions themselves are in chains.h, shared with elu_kernels.hip (the elu
// critic's chain kernels, which the launch_* functions here hand an elu-topology handle to).
#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "learn.h"
#include "net_common.h"

#ifdef CACTO_STAMPS
__device__ unsigned long long g_cstamps[32];
__device__ unsigned long long g_astamps[32];  // actor chain, tile 0 (also inside the paired kernel)
#define CSTAMP(k) PSTAMP(k)
#define CSTAMP_DECL
#define CSTAMP_FLUSH                                                                     \
  do {                                                                                   \
    if (blockIdx.x == 0 && threadIdx.x == 0)                                             \
      for (int k_ = 0; k_ < 32; ++k_) g_cstamps[k_] = cacto_stamp_s[k_];                 \
  } while (0)
#else
#define CSTAMP(k) \
  do {            \
  } while (0)
#define CSTAMP_DECL
#define CSTAMP_FLUSH \
  do {               \
  } while (0)
#endif

#include "chains.h"

namespace cacto {

// One-time probe per handle (cacto_update_n[_per]'s first two-stream call): can a kernel on the side
// stream and one on the caller's stream run at the same time? Role 0 (side) raises flag w[4] and
// polls for w[5]; role 1 (caller's stream) polls for w[4], then raises w[5]. Each records in w[6 +
// role] whether its poll succeeded (bounded: ~2^14 polls). When the device serializes kernels
// (AMD_SERIALIZE_KERNEL, HIP_LAUNCH_BLOCKING, counter collection) the first of the two to run cannot
// see the other's flag, so a device-side wait would spin until its bound: the pipeline then orders
// the streams with queue markers.
// ("Memory-ordering contract", site 4)
__global__ void k_pipe_probe(unsigned long long* w, int role) {
  if (threadIdx.x != 0) return;
  unsigned long long* mine = w + 4 + role;
  const unsigned long long* other = w + 5 - role;
  if (role == 0) __hip_atomic_store(mine, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  unsigned long long ok = 0;
  for (int k = 0; k < (1 << 14) && !ok; ++k) {
    ok = __hip_atomic_load(other, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!ok) __builtin_amdgcn_s_sleep(2);
  }
  if (role == 1) __hip_atomic_store(mine, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(w + 6 + role, ok ? 1ull : 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(CACTO_THREADS)
    k_critic_grad(const SysDevice* __restrict__ sdp, NetView C, NetView Tg, ChainScalars cs,
                  const double* __restrict__ storage, const int32_t* __restrict__ idx, const float* __restrict__ isw,
                  int B, GradBufs gb, float* __restrict__ y_out, float* __restrict__ V_out, float* __restrict__ Vt_out,
                  int32_t* __restrict__ step) {
  __shared__ CriticLds S;
  critic_chain(S, chain_tile_of(blockIdx.x, gridDim.x, cs.xcd_tiles), sdp, C, Tg, cs, storage, idx, isw, B, gb, y_out,
               V_out, Vt_out, step);
}

template <int NJ>
__global__ void __launch_bounds__(CACTO_THREADS) __attribute__((amdgpu_waves_per_eu(actor_grad_wpe<NJ>(), 8)))
    k_actor_grad(const SysDevice* __restrict__ sdp, NetView Ac, NetView C, ChainScalars cs,
                 const double* __restrict__ storage, const int32_t* __restrict__ idx, int B, GradBufs gb,
                 int32_t* __restrict__ step) {
  __shared__ ActorLds S;
  ChainScalars c = cs;
  if (cs.wait_p && cs.wait_at_start) {
    if (threadIdx.x == 0) pipe_wait(cs.wait_p, cs.wait_v, const_cast<unsigned long long*>(cs.wait_p) - 1);
    __syncthreads();
    c.wait_p = nullptr;
  }
  actor_chain<NJ>(S, chain_tile_of(blockIdx.x, gridDim.x, cs.xcd_tiles), sdp, Ac, C, c, storage, idx, B, gb, step);
}

// The critic chain of update t (workgroups [0, nct)) and the actor chain of update t - 1 (the
// rest) in one launch: neither reads what the other writes (the actor reads the critic C_t that
// both chains take; panels and counters are separate), so the single-stream small-batch pipeline
// issues the two as one grid. LDS is the larger of the two layouts, not their sum.
template <int NJ>
__global__ void __launch_bounds__(CACTO_THREADS)
    k_chain_pair(const SysDevice* __restrict__ sdp, NetView C, NetView Tg, NetView Ac, ChainScalars cs,
                 const double* __restrict__ storage, const int32_t* __restrict__ idx_c, const float* __restrict__ isw,
                 const int32_t* __restrict__ idx_a, int B, int nct, GradBufs gbc, GradBufs gba,
                 float* __restrict__ y_out, float* __restrict__ V_out, int32_t* __restrict__ step) {
  constexpr size_t bytes = sizeof(CriticLds) > sizeof(ActorLds) ? sizeof(CriticLds) : sizeof(ActorLds);
  __shared__ __attribute__((aligned(16))) unsigned char smem[bytes];
  if ((int)blockIdx.x < nct) {
    critic_chain(*reinterpret_cast<CriticLds*>(smem), blockIdx.x, sdp, C, Tg, cs, storage, idx_c, isw, B, gbc, y_out,
                 V_out, nullptr, step);
  } else {
    actor_chain<NJ>(*reinterpret_cast<ActorLds*>(smem), blockIdx.x - nct, sdp, Ac, C, cs, storage, idx_a, B, gba,
                    step);
  }
}

}  // namespace cacto

// the same chains on 4-sample tiles (small batches)
#include "chain_q4.h"

namespace cacto {

// ---------------------------------------------------------------- weight-gradient GEMM
// One workgroup per (row chunk, item). An item is a block of up to 4 x 4 output tiles of one layer
// (the 4 waves split the chunk's rows, each keeping 16 accumulator tiles, then reduce through LDS
// in a fixed order, so the result is deterministic), or up to 4 bias tiles (one per wave). A
// block loads each LT/RT panel slice once for 4 tiles instead of once per tile.
constexpr int WG_BLK = 4;

// One workgroup's block of NI x NO output tiles (of a layer) over the rows [lo, hi) of one chunk:
// the 4 waves split the rows, each keeping NI x NO accumulator tiles, then reduce through LDS in a
// fixed order ((p0 + p1) + p2) + p3 (deterministic), in rounds of 8 tiles. ni, no: the tiles that
// exist (<= NI, NO; the generic 4 x 4 instance runs edge blocks on clamped duplicate tiles).
template <int NI, int NO>
__device__ __forceinline__ void wg_block(const WgArgs& a, const WgLayer& Ly, int lo, int hi, int it0, int ot0, int ni,
                                         int no, float* __restrict__ out, float4* part) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
  const int span = ((hi - lo) / 16 + 3) / 4 * 16;  // rows per wave, multiple of 16
  const int r0 = lo + wave * span, r1 = min(hi, r0 + span);
  floatx4 acc[NI][NO];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int o = 0; o < NO; ++o) acc[i][o] = floatx4{0.f, 0.f, 0.f, 0.f};
  const float* ap = Ly.LT + (size_t)(16 * it0 + c) * a.ld + 4 * g;
  const float* bp = Ly.RT + (size_t)(16 * ot0 + c) * a.ld + 4 * g;
  // the panel slices of the next 16-row step are in flight while a step's MFMAs run (one step: a
  // deeper prefetch cost the GEMM its 4 waves per SIMD beside the chains); the steps are
  // summed in row order
  float4 An[NI], Bn[NO];
  auto fetch = [&](int r) {
    const int rr = min(r, r1 - 16);  // clamped (branch-free); a past-the-end fetch is unused
#pragma unroll
    for (int i = 0; i < NI; ++i) An[i] = *reinterpret_cast<const float4*>(ap + (size_t)16 * min(i, ni - 1) * a.ld + rr);
#pragma unroll
    for (int o = 0; o < NO; ++o) Bn[o] = *reinterpret_cast<const float4*>(bp + (size_t)16 * min(o, no - 1) * a.ld + rr);
  };
  auto step = [&](const float4 (&A)[NI], const float4 (&Bv)[NO]) {
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int o = 0; o < NO; ++o) acc[i][o] = mfma4(A[i].x, Bv[o].x, acc[i][o]);
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int o = 0; o < NO; ++o) acc[i][o] = mfma4(A[i].y, Bv[o].y, acc[i][o]);
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int o = 0; o < NO; ++o) acc[i][o] = mfma4(A[i].z, Bv[o].z, acc[i][o]);
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int o = 0; o < NO; ++o) acc[i][o] = mfma4(A[i].w, Bv[o].w, acc[i][o]);
  };
  if (r0 < r1) fetch(r0);
  for (int r = r0; r < r1; r += 16) {
    float4 A[NI], Bv[NO];
#pragma unroll
    for (int i = 0; i < NI; ++i) A[i] = An[i];
#pragma unroll
    for (int o = 0; o < NO; ++o) Bv[o] = Bn[o];
    fetch(r + 16);
    step(A, Bv);
  }
  constexpr int NT = NI * NO, HT = NT < 8 ? NT : 8;  // tiles, tiles per round
  constexpr int NR = (NT + HT - 1) / HT;
#pragma unroll
  for (int h = 0; h < NR; ++h) {
    if (h) __syncthreads();  // the previous round's partials are consumed
#pragma unroll
    for (int t = h * HT; t < h * HT + HT && t < NT; ++t) part[(wave * HT + (t - h * HT)) * 64 + lane] = f4(acc[t / NO][t % NO]);
    __syncthreads();
    // wave w finishes the round's tiles 2w, 2w + 1: ((p0 + p1) + p2) + p3
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int tl = wave * 2 + k, t = h * HT + tl, i = t / NO, o = t % NO;
      if (tl >= HT || t >= NT || i >= ni || o >= no) continue;
      float4 s4 = part[(0 * HT + tl) * 64 + lane];
#pragma unroll
      for (int w = 1; w < 4; ++w) {
        const float4 q = part[(w * HT + tl) * 64 + lane];
        s4.x += q.x;
        s4.y += q.y;
        s4.z += q.z;
        s4.w += q.w;
      }
      const float sv[4] = {s4.x, s4.y, s4.z, s4.w};
      const int oc = 16 * (ot0 + o) + c;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int ii = 16 * (it0 + i) + 4 * g + q;
        if (ii < Ly.in && oc < Ly.out) out[Ly.woff + ii * Ly.out + oc] = sv[q];
      }
    }
  }
}

// One split-K item, decoded (k_wgrad and k_wgrad_big share the items; each deals its workgroups to
// (chunk, item) its own way — the WgDeal): a block of ni x no (<= 4 x 4) output tiles of layer l from
// tile (it0, ot0), or, with ni == 0, the group of up to 4 bias tiles from tile ot0 (one per wave);
// over the rows [lo, hi) of the chunk, into the chunk's slab `out`.
struct WgDeal {
  int chunk, item;  // chunk < 0: a padding workgroup of the grid
};
struct WgItem {
  int l, it0, ot0, ni, no, lo, hi;
  float* out;
};
__device__ __forceinline__ WgItem wg_item(const WgArgs& a, float* __restrict__ slab, const WgDeal d) {
  WgItem w;
  int rem = d.item;
  w.l = 0;
  while (rem >= a.toff[w.l + 1]) ++w.l;
  const WgLayer& Ly = a.l[w.l];
  rem -= a.toff[w.l];
  w.lo = a.r_begin + d.chunk * a.CH;
  w.hi = min(a.r_end, w.lo + a.CH);
  w.out = slab + (size_t)d.chunk * a.P;
  const int nbi = (Ly.IT + WG_BLK - 1) / WG_BLK, nbo = (Ly.OT + WG_BLK - 1) / WG_BLK;
  if (rem < nbi * nbo) {
    w.it0 = (rem / nbo) * WG_BLK, w.ot0 = (rem % nbo) * WG_BLK;
    w.ni = min(WG_BLK, Ly.IT - w.it0), w.no = min(WG_BLK, Ly.OT - w.ot0);
  } else {
    w.it0 = w.ni = w.no = 0;
    w.ot0 = (rem - nbi * nbo) * WG_BLK;
  }
  return w;
}

// One wave's bias tile `ot` of a layer over the rows of [lo, hi) from bias_r0 on: 64-row groups (4
// loads in flight) then 16-row steps, summed in row order, then over the 4 row groups of the lanes.
__device__ __forceinline__ void wg_bias_tile(const WgArgs& a, const WgLayer& Ly, int ot, int lo, int hi,
                                             float* __restrict__ out) {
  const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
  if (ot >= Ly.OT) return;
  const float* bp = Ly.RT + (size_t)(16 * ot + c) * a.ld + 4 * g;
  float s = 0.f;
  int r = max(lo, a.bias_r0);
  for (; r + 64 <= hi; r += 64) {
    float4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = *reinterpret_cast<const float4*>(bp + r + 16 * k);
#pragma unroll
    for (int k = 0; k < 4; ++k) s += (v[k].x + v[k].y) + (v[k].z + v[k].w);
  }
  for (; r < hi; r += 16) {
    const float4 v = *reinterpret_cast<const float4*>(bp + r);
    s += (v.x + v.y) + (v.z + v.w);
  }
  s += __shfl_xor(s, 16);
  s += __shfl_xor(s, 32);
  if (g == 0 && 16 * ot + c < Ly.out) out[Ly.boff + 16 * ot + c] = s;
}

// k_wgrad's deal. xcd = 0: chunk-major (the small batches of cacto_critic_grad / cacto_actor_grad).
// xcd = 1 (from 8 chunks on): the items of one chunk run on blocks that share an XCD (blocks b and
// b + 8 are dealt to one; observed dealing, so it decides only which L2 serves a re-read): chunk
// (b / 8 / tpc) * 8 + b % 8, item (b / 8) % tpc. The 4 (resp. nbi) blocks that read one LT (RT) slice
// then read it from one L2 instead of up to four; the grid is padded to whole groups of 8 chunks.
__device__ __forceinline__ WgDeal wg_deal(const WgArgs& a, int blk, int xcd) {
  if (!xcd) return WgDeal{blk / a.tpc, blk % a.tpc};
  const int sl = blk >> 3, chunk = (sl / a.tpc) * 8 + (blk & 7);
  return WgDeal{chunk < a.nch ? chunk : -1, sl % a.tpc};
}

// sig_p (the pipeline's device-side ordering): this launch follows the actor chain of an iteration
// on its stream, so that chain has finished; block 0 publishes sig_v = (iterations done) for the
// critic stream's Adam, which must not overwrite a critic buffer the chain read (k_adam's wait_p).
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8))) k_wgrad(WgArgs a, float* __restrict__ slab, int xcd,
                                               unsigned long long* sig_p, unsigned long long sig_v) {
  // 32 KiB: the 16 tiles are reduced in two rounds of 8, so a GEMM workgroup fits on a CU beside
  // a chain workgroup — the pipelined update runs the two concurrently
  __shared__ float4 part[4 * (WG_BLK * WG_BLK / 2) * 64];
  if (sig_p && blockIdx.x == 0 && threadIdx.x == 0)  // write-after-read order only: relaxed
    __hip_atomic_store(sig_p, sig_v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const WgDeal d = wg_deal(a, blockIdx.x, xcd);
  if (d.chunk < 0) return;
  const WgItem w = wg_item(a, slab, d);
  const WgLayer& Ly = a.l[w.l];
  if (w.ni == 0) return wg_bias_tile(a, Ly, w.ot0 + (threadIdx.x >> 6), w.lo, w.hi, w.out);
  // the block shapes the networks have, compiled for their size (an edge block of the input or
  // output layer loads and multiplies only its own tiles); any other shape runs the 4 x 4 code
  // on clamped duplicate tiles (unused)
  if (w.ni == 1 && w.no == WG_BLK) wg_block<1, WG_BLK>(a, Ly, w.lo, w.hi, w.it0, w.ot0, w.ni, w.no, w.out, part);
  else if (w.ni == WG_BLK && w.no == 1) wg_block<WG_BLK, 1>(a, Ly, w.lo, w.hi, w.it0, w.ot0, w.ni, w.no, w.out, part);
  else wg_block<WG_BLK, WG_BLK>(a, Ly, w.lo, w.hi, w.it0, w.ot0, w.ni, w.no, w.out, part);
}

// ---------------------------------------------------------------- weight-gradient GEMM, large batches
// k_wgrad_big (rows > 1024: the B >= 1024 updates). The same items as k_wgrad (a block of up to 4 x 4
// output tiles of one layer over one row chunk, or up to 4 bias tiles, slab[chunk][P] out), but the
// 4 waves split the block's TILES instead of its rows: wave w owns A tile w (NI = 4; B tile w when
// NI = 1) and walks every 16-row step of the chunk, so each wave's accumulators cover the whole chunk
// and are written straight to the slab (no cross-wave LDS reduction). The workgroup stages each
// step's panel slices (NI + NO slices of 16 features x 16 rows, 2 float4 per thread) through a
// 2-buffer LDS ring, with the global loads issued WGB_AHEAD steps ahead into registers, so the
// latency of a step's loads hides behind WGB_AHEAD steps of MFMAs (k_wgrad: one step, and a wave
// covered only 2-4 steps of its chunk, so its time was mostly load latency: 18-21 us per launch at
// B = 4096 alone, 0.17 of the MFMA peak). Each tile's sum runs over the chunk's rows in row order
// (one MFMA accumulator chain; four k-phase chains for the 1-tile waves of edge blocks) — a
// different, fixed order than k_wgrad's four row spans, so the batch sizes that take this kernel
// form their own, schedule-independent, sums.
constexpr int WGB_FS = 20;                    // floats per staged feature row (16 rows + 4 pad: LDS banks)
constexpr int WGB_SLICE = 16 * WGB_FS;        // one 16 x 16 panel slice
constexpr int WGB_STAGE = 8 * WGB_SLICE;      // up to 4 A + 4 B slices
// The load lead in 16-row steps. A lead of 6 gave the same sums and measured no better (updates/s,
// two runs each): DI B = 4096 13.41 / 13.38 k at 6 against 13.33 / 13.37 k at 3, manipulator
// B = 8192 8.29 / 8.26 k against 8.36 / 8.34 k — inside the pipeline the GEMM is not waiting on its
// loads, so the lighter form stays.
constexpr int WGB_AHEAD = 3;

template <int NI, int NO>
__device__ __forceinline__ void wgb_block(const int ld, const WgLayer Ly, int lo, int hi, int it0, int ot0,
                                          float* __restrict__ out, float* stage) {
  static_assert((NI == 4 && (NO == 4 || NO == 1)) || (NI == 1 && NO == 4), "block shape");
  static_assert(WGB_AHEAD == 3, "the step loop below is unrolled by hand for 3 landing buffers");
  constexpr int NS = NI + NO;  // staged slices per step
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
  // the loader's part of a step: slice sl = tid >> 5 (if < NS), feature f = (tid >> 1) & 15, rows
  // [8 h, 8 h + 8) of the step, h = tid & 1
  const int sl = tid >> 5, f = (tid >> 1) & 15, h = tid & 1;
  const bool loader = sl < NS;
  const float* src = nullptr;
  if (loader) {
    const int slc = sl < NI ? sl : sl - NI;
    const float* base = sl < NI ? Ly.LT + (size_t)(16 * (it0 + slc)) * ld : Ly.RT + (size_t)(16 * (ot0 + slc)) * ld;
    src = base + (size_t)f * ld + 8 * h;
  }
  const int nsteps = (hi - lo) / 16;  // chunks are multiples of 16 rows
  // landing registers of the next WGB_AHEAD steps (named, not an array: an array passed by reference
  // went to scratch)
  float4 r0a, r0b, r1a, r1b, r2a, r2b;
  // clamped, branch-free loads (a past-the-end or non-loader load rereads a valid address; unused)
  const float* src_c = loader ? src : Ly.RT;
  auto load = [&](float4& ra, float4& rb, int s) {
    const float4* p = reinterpret_cast<const float4*>(src_c + lo + 16 * min(s, nsteps - 1));
    ra = p[0];
    rb = p[1];
  };
  load(r0a, r0b, 0);
  load(r1a, r1b, 1);
  load(r2a, r2b, 2);
  // this wave's tiles: NI = 4 -> (w, 0..NO-1); NI = 1 -> (0, w)
  constexpr int NT = NI == 4 ? NO : 1;
  // accumulator chains per tile: one when the wave has 4 tiles (their MFMAs interleave), one per
  // k-phase when it has one
  constexpr int NC = NT == 1 ? 4 : 1;
  floatx4 acc[NT][NC];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int k = 0; k < NC; ++k) acc[t][k] = floatx4{0.f, 0.f, 0.f, 0.f};
  const int ai = NI == 4 ? wave : 0;
  // one step from landing registers r: stage them, refill r with step s + WGB_AHEAD, MFMAs
  auto step = [&](float4& ra, float4& rb, int s) {
    float* st = stage + (s & 1) * WGB_STAGE;
    if (loader) {
      float4* q = reinterpret_cast<float4*>(st + sl * WGB_SLICE + f * WGB_FS + 8 * h);
      q[0] = ra;
      q[1] = rb;
    }
    load(ra, rb, s + WGB_AHEAD);
    __syncthreads();
    // operands: lane (g, c) = feature c, rows 4g .. 4g + 3 of the step (the k_wgrad layout)
    const float4 av = *reinterpret_cast<const float4*>(st + ai * WGB_SLICE + c * WGB_FS + 4 * g);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int bo = NI == 4 ? t : wave;
      const float4 bv = *reinterpret_cast<const float4*>(st + (NI + bo) * WGB_SLICE + c * WGB_FS + 4 * g);
      acc[t][0] = mfma4(av.x, bv.x, acc[t][0]);
      acc[t][1 % NC] = mfma4(av.y, bv.y, acc[t][1 % NC]);
      acc[t][2 % NC] = mfma4(av.z, bv.z, acc[t][2 % NC]);
      acc[t][3 % NC] = mfma4(av.w, bv.w, acc[t][3 % NC]);
    }
  };
  int s = 0;
  for (; s + WGB_AHEAD <= nsteps; s += WGB_AHEAD) {
    step(r0a, r0b, s);
    step(r1a, r1b, s + 1);
    step(r2a, r2b, s + 2);
  }
  if (s < nsteps) step(r0a, r0b, s);
  if (s + 1 < nsteps) step(r1a, r1b, s + 1);
  // tile sums (four k-phase chains: (c0 + c1) + (c2 + c3)), straight to the slab
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int i = NI == 4 ? wave : 0, o = NI == 4 ? t : wave;
    floatx4 sm = acc[t][0];
    if constexpr (NC == 4) sm = (acc[t][0] + acc[t][1 % NC]) + (acc[t][2 % NC] + acc[t][3 % NC]);
    const int oc = 16 * (ot0 + o) + c;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int ii = 16 * (it0 + i) + 4 * g + q;
      if (ii < Ly.in && oc < Ly.out) out[Ly.woff + ii * Ly.out + oc] = sm[q];
    }
  }
}

// k_wgrad_big's deal (it always has 9 chunks or more): block b runs on XCD b % 8 (observed dealing),
// which owns chunks x, x + 8, ...; its j-th block (j = b / 8) takes item perm[j / cpx] of its chunk
// j % cpx — every XCD starts with the full 4 x 4 blocks of all its chunks, one per CU, before the
// lighter items fill in (with the work dealt chunk-major, two heavy items could share a CU's matrix
// cores while others idled). The grid is padded to whole groups of 8 chunks.
__device__ __forceinline__ WgDeal wgb_deal(const WgArgs& a, int blk) {
  const int j = blk >> 3, cpx = (a.nch + 7) >> 3;
  const int pi = j / cpx, chunk = (j - pi * cpx) * 8 + (blk & 7);
  if (chunk >= a.nch || pi >= a.tpc) return WgDeal{-1, 0};
  return WgDeal{chunk, a.perm[pi]};
}

__device__ __forceinline__ void wgrad_big_body(const int blk, const WgArgs& a, float* __restrict__ slab,
                                               unsigned long long* sig_p, unsigned long long sig_v, float* stage) {
  if (sig_p && blk == 0 && threadIdx.x == 0)  // write-after-read order only: relaxed
    __hip_atomic_store(sig_p, sig_v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const WgDeal d = wgb_deal(a, blk);
  if (d.chunk < 0) return;
  const WgItem w = wg_item(a, slab, d);
  const WgLayer& Ly = a.l[w.l];
  if (w.ni == 0) return wg_bias_tile(a, Ly, w.ot0 + (threadIdx.x >> 6), w.lo, w.hi, w.out);
  const WgLayer lv{Ly.LT, Ly.RT, Ly.in, Ly.out, Ly.IT, Ly.OT, Ly.woff, Ly.boff};
  if (w.ni == 4 && w.no == 4) wgb_block<4, 4>(a.ld, lv, w.lo, w.hi, w.it0, w.ot0, w.out, stage);
  else if (w.ni == 1 && w.no == 4) wgb_block<1, 4>(a.ld, lv, w.lo, w.hi, w.it0, w.ot0, w.out, stage);
  else if (w.ni == 4 && w.no == 1) wgb_block<4, 1>(a.ld, lv, w.lo, w.hi, w.it0, w.ot0, w.out, stage);
  // (the route takes this kernel only when every block of the network has one of these shapes)
}

__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8))) k_wgrad_big(WgArgs a, float* __restrict__ slab,
                                                   unsigned long long* sig_p, unsigned long long sig_v) {
  __shared__ __attribute__((aligned(16))) float stage[2 * WGB_STAGE];  // 20 KiB
  wgrad_big_body(blockIdx.x, a, slab, sig_p, sig_v, stage);
}

// The pipelined PER loop's critic GEMM with the priority update of the same update in one grid:
// blocks [0, nwg) are k_wgrad_big's (the same XCD dealing: nwg is its grid), the next nroot run
// per_update_run_body over the subtrees. Both need only the critic chain before them, and the next
// sample needs both (the trees, and this stream's order). LDS: the GEMM's 20 KiB ring, the priority
// update's 10 KiB in the same bytes.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8)))
k_wgrad_big_per(WgArgs a, float* __restrict__ slab, int nwg, PerRunArgs pa, int nroot) {
  static_assert(sizeof(PerRunLds) <= 2 * WGB_STAGE * sizeof(float), "LDS union");
  __shared__ __attribute__((aligned(16))) float stage[2 * WGB_STAGE];  // 20 KiB
  if ((int)blockIdx.x < nwg) wgrad_big_body(blockIdx.x, a, slab, nullptr, 0, stage);
  else per_update_run_body(blockIdx.x - nwg, nroot, pa, *reinterpret_cast<PerRunLds*>(stage));
}

// ---------------------------------------------------------------- Adam (+ packed refresh, soft update)
// thru: the store written through to memory at agent scope (a relaxed atomic store), for a reader
// on another stream that orders itself by a device-side flag instead of a kernel boundary
__device__ __forceinline__ void store_f(float* p, float v, bool thru) {
  if (thru) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *p = v;
}

// The two packed copies of a weight W_l[i][o] whose layer and indices are known (no search, no
// division): the pk block (o tile, i tile) and the pkT block (i tile, o tile).
__device__ __forceinline__ void write_packed_w(float4* pk4, const NetTopo& t, int l, int i, int o, float val,
                                               bool thru = false) {
  float* pk = reinterpret_cast<float*>(pk4);
  store_f(pk + ((size_t)(t.pkoff[l] + (o >> 4) * t.KT[l] + (i >> 4)) * 64 + ((i & 15) >> 2) * 16 + (o & 15)) * 4 + (i & 3),
          val, thru);
  store_f(pk + ((size_t)(t.blocks + t.pkoff[l] + (i >> 4) * t.OT[l] + (o >> 4)) * 64 + ((o & 15) >> 2) * 16 + (i & 15)) * 4 +
              (o & 3),
          val, thru);
}

// ... of the Keras-flat parameter p: its layer searched for, nothing for a bias
__device__ __forceinline__ void write_packed(float4* pk4, const NetTopo& t, int p, float val, bool thru = false) {
  int l = t.L - 1;
  while (t.woff[l] > p) --l;
  if (p >= t.boff[l]) return;
  const int local = p - t.woff[l];
  const int i = local / t.out[l], o = local - (local / t.out[l]) * t.out[l];
  write_packed_w(pk4, t, l, i, o, val, thru);
}

struct AdamScalars {
  float alpha, c1, c2, eps, tau, omt;
};

__device__ __forceinline__ AdamScalars adam_scalars(const AdamArgs& a, const int32_t* step) {
  const int it = step[a.which];  // = Keras iterations + 1
  const int iters = it - 1;
  double lr = a.lr[4];
  for (int k = 0; k < 4; ++k)
    if ((double)iters <= a.bounds[k]) {
      lr = a.lr[k];
      break;
    }
  const float tf = (float)it;
  const float b1p = powf((float)a.beta1, tf), b2p = powf((float)a.beta2, tf);
  AdamScalars s;
  s.alpha = fdiv(fmul((float)lr, __fsqrt_rn(fsub(1.f, b2p))), fsub(1.f, b1p));
  s.c1 = (float)(1.0 - a.beta1);
  s.c2 = (float)(1.0 - a.beta2);
  s.eps = (float)a.eps;
  s.tau = (float)a.tau;
  s.omt = (float)(1.0 - a.tau);
  return s;
}

// The Adam step of one parameter (Keras), values only: gradient g; m, v and the weight th stepped in
// place; tg: the target's value in, its soft update against the new weight out (unused without one).
// The one place this arithmetic is written: every Adam kernel calls it, so the split, fused and
// data-parallel paths agree bit for bit.
__device__ __forceinline__ void adam_math(const AdamScalars& s, float g, float& mm, float& vv, float& th, float& tg) {
  mm = fadd(mm, fmul(fsub(g, mm), s.c1));
  vv = fadd(vv, fmul(fsub(fmul(g, g), vv), s.c2));
  th = fsub(th, fdiv(fmul(mm, s.alpha), fadd(__fsqrt_rn(vv), s.eps)));
  tg = fadd(fmul(th, s.tau), fmul(tg, s.omt));
}

// ... and of parameter p of the split path (k_adam, k_adam_sample) with its stores: m, v, the weight
// and its packed copies (thru: written through), the target and its packed copies with `soft`
__device__ __forceinline__ void adam_param(const AdamScalars& s, const NetTopo& t, int p, float g, float mm, float vv,
                                           float th, float tg, float* netbuf, float4* packed, float* __restrict__ m,
                                           float* __restrict__ v, bool soft, float* target, float4* target_packed,
                                           bool thru) {
  adam_math(s, g, mm, vv, th, tg);
  m[p] = mm;
  v[p] = vv;
  store_f(netbuf + p, th, thru);
  write_packed(packed, t, p, th, thru);
  if (soft) {
    target[p] = tg;
    write_packed(target_packed, t, p, tg);
  }
}

// The NCH chunk partials of parameter pc (of P) loaded at once (clamped to the nch that exist,
// branch-free), then summed in chunk order: g = q[0]; g += q[k] — the order of every chunk sum here.
template <int NCH>
struct ChunkPartials {
  float q[NCH];
  __device__ __forceinline__ void load(const float* __restrict__ slab, int nch, int P, int pc) {
#pragma unroll
    for (int k = 0; k < NCH; ++k) q[k] = slab[(size_t)min(k, nch - 1) * P + pc];
  }
  __device__ __forceinline__ float sum(int nch) const {
    float g = q[0];
#pragma unroll
    for (int k = 1; k < NCH; ++k)
      if (k < nch) g += q[k];
    return g;
  }
};

// NCH > 0: every chunk partial of a parameter is loaded at once (clamped, branch-free) together with
// m, v, the weight and the target value, so a thread waits for one memory latency instead of one per
// group of 8 chunks plus one per leftover chunk (B = 4096: 32 chunks, ~11 dependent rounds, 11 us);
// the partials are still summed in chunk order (bit-identical). NCH = 0: any chunk count.
//
// wait_p / wait_v: the pipeline's wait before overwriting a critic buffer an actor chain of the other
// stream read (k_wgrad's sig_p publishes those chains). sig_p / sig_v: after its stores (written
// through to memory, `thru`) the last workgroup to finish publishes sig_p[2] = sig_v (this Adam step
// done) for the actor chain's wait: every thread's stores have completed (waitcnt) before its
// workgroup counts itself; no fence, no L2 write-back.
// nblk: the Adam step's workgroups (the launch's, or the leading part of k_adam_sample's).
// ("Memory-ordering contract", site 2: why no release / acquire is needed here)
__device__ __forceinline__ void adam_publish_thru(unsigned long long* sig_p, unsigned long long sig_v, int nblk) {
  if (!sig_p) return;
  __shared__ int last;
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  if (threadIdx.x == 0)
    last = __hip_atomic_fetch_add(sig_p + 3, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
           (unsigned long long)(nblk - 1);
  __syncthreads();
  if (last && threadIdx.x == 0) {
    __hip_atomic_store(sig_p + 3, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(sig_p + 2, sig_v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <int NCH>
__device__ __forceinline__ void adam_nch_body(const int blk, const float* __restrict__ slab, int nch, const NetTopo& t,
                                              const float* src, float* netbuf, float4* packed, float* __restrict__ m,
                                              float* __restrict__ v, const int32_t* __restrict__ step, const AdamArgs& a,
                                              float* target, float4* target_packed, const unsigned long long* wait_p,
                                              unsigned long long wait_v, bool thru = false) {
  const int p0 = blk * 256 + threadIdx.x;
  const int pc = min(p0, t.params - 1);
  ChunkPartials<NCH> q;
  q.load(slab, nch, t.params, pc);
  const float mm = m[pc], vv = v[pc], th = src[pc], tg = a.soft ? target[pc] : 0.f;
  const AdamScalars s = adam_scalars(a, step);
  pipe_wait(wait_p, wait_v, const_cast<unsigned long long*>(wait_p) + 1);  // the loads above are in flight
  if (p0 < t.params)
    adam_param(s, t, p0, q.sum(nch), mm, vv, th, tg, netbuf, packed, m, v, a.soft, target, target_packed, thru);
}

// The pipelined PER loop's critic Adam step with the next update's sample in one grid: blocks
// [0, nadam) are k_adam<NCH>'s, the rest run per_sample_body (4,096-node top, recording the runs for
// the next priority update). The sample needs the trees this update's priority update left (the
// launch before on this stream); the next critic chain needs both.
template <int NCH>
__global__ void __launch_bounds__(256) k_adam_sample(const float* __restrict__ slab, int nch, NetTopo t, const float* src,
                                                     float* netbuf, float4* packed, float* __restrict__ m,
                                                     float* __restrict__ v, const int32_t* __restrict__ step, AdamArgs a,
                                                     float* target, float4* target_packed,
                                                     const unsigned long long* wait_p, unsigned long long wait_v,
                                                     int nadam, PerSampleArgs sa, unsigned long long* sig_p,
                                                     unsigned long long sig_v, int thru) {
  __shared__ double top_s[PER_FUSED_TOP];
  __shared__ double scal_s[4];
  if ((int)blockIdx.x < nadam) {
    adam_nch_body<NCH>(blockIdx.x, slab, nch, t, src, netbuf, packed, m, v, step, a, target, target_packed, wait_p,
                       wait_v, thru != 0);
    adam_publish_thru(sig_p, sig_v, nadam);  // (sig_p only with write-through stores)
  } else
    per_sample_body<PER_FUSED_TOP>(blockIdx.x - nadam, sa, top_s, scal_s);
}

template <int NCH>
__global__ void __launch_bounds__(256) k_adam(const float* __restrict__ slab, int nch, NetTopo t, const float* src,
                                              float* netbuf, float4* packed, float* __restrict__ m, float* __restrict__ v,
                                              const int32_t* __restrict__ step, AdamArgs a, float* target,
                                              float4* target_packed, const unsigned long long* wait_p,
                                              unsigned long long wait_v, unsigned long long* sig_p,
                                              unsigned long long sig_v, int thru) {
  if constexpr (NCH > 0) {
    adam_nch_body<NCH>(blockIdx.x, slab, nch, t, src, netbuf, packed, m, v, step, a, target, target_packed, wait_p,
                       wait_v, thru != 0);
    adam_publish_thru(sig_p, sig_v, gridDim.x);  // (sig_p only with write-through stores)
    return;
  }
  const AdamScalars s = adam_scalars(a, step);
  pipe_wait(wait_p, wait_v, const_cast<unsigned long long*>(wait_p) + 1);
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < t.params; p += gridDim.x * blockDim.x) {
    // chunk partials summed in chunk order; loads issued 8 at a time so they overlap
    float g = slab[p];
    int ch = 1;
    for (; ch + 8 <= nch; ch += 8) {
      float q[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) q[k] = slab[(size_t)(ch + k) * t.params + p];
#pragma unroll
      for (int k = 0; k < 8; ++k) g += q[k];
    }
    for (; ch < nch; ++ch) g += slab[(size_t)ch * t.params + p];
    adam_param(s, t, p, g, m[p], v[p], src[p], a.soft ? target[p] : 0.f, netbuf, packed, m, v, a.soft, target,
               target_packed, thru != 0);
  }
  adam_publish_thru(sig_p, sig_v, gridDim.x);
}

__global__ void __launch_bounds__(256) k_soft(NetTopo t, const float* __restrict__ src, float* target,
                                              float4* target_packed, double tau_d) {
  const float tau = (float)tau_d, omt = (float)(1.0 - tau_d);
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < t.params; p += gridDim.x * blockDim.x) {
    const float tg = fadd(fmul(src[p], tau), fmul(target[p], omt));
    target[p] = tg;
    write_packed(target_packed, t, p, tg);
  }
}

// The data-parallel path's chunk sum (the gradient each rank all-reduces): out[p] = the nch
// partials of parameter p summed in chunk order, as k_adam sums them. NCH > 0: one parameter per
// thread with every partial loaded at once (clamped, branch-free), so a thread waits for one memory
// latency instead of one per chunk (the looped form, NCH = 0, issued one load per add: 16-32
// dependent round trips, 7-8 us per launch at B = 4096).
template <int NCH>
__global__ void __launch_bounds__(256) k_reduce(const float* __restrict__ slab, int nch, int P, float* __restrict__ out) {
  if constexpr (NCH > 0) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    ChunkPartials<NCH> q;
    q.load(slab, nch, P, min(p, P - 1));
    if (p < P) out[p] = q.sum(nch);
    return;
  }
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) {
    float g = slab[p];
    for (int ch = 1; ch < nch; ++ch) g += slab[(size_t)ch * P + p];
    out[p] = g;
  }
}

// The <NCH> instance of k_adam / k_adam_sample / k_reduce that sums nch chunks: the smallest of 8, 16,
// 32, 64 that holds them (one parameter per thread, a grid of `full` workgroups), else 0 (the looped
// form on at most 1024 workgroups). go(integral_constant<NCH>, grid).
int nch_instance(int nch) { return nch <= 8 ? 8 : nch <= 16 ? 16 : nch <= 32 ? 32 : nch <= 64 ? 64 : 0; }
template <class Go>
static void nch_dispatch(int nch, int full, Go&& go) {
  switch (nch_instance(nch)) {
    case 8: return go(std::integral_constant<int, 8>{}, full);
    case 16: return go(std::integral_constant<int, 16>{}, full);
    case 32: return go(std::integral_constant<int, 32>{}, full);
    case 64: return go(std::integral_constant<int, 64>{}, full);
    default: return go(std::integral_constant<int, 0>{}, std::min(full, 1024));
  }
}

int launch_reduce(const float* slab, int nch, int P, float* out, hipStream_t st) {
  nch_dispatch(nch, (P + 255) / 256, [&](auto n, int grid) {
    hipLaunchKernelGGL(k_reduce<decltype(n)::value>, dim3(grid), dim3(256), 0, st, slab, nch, P, out);
  });
  CACTO_CHECK_HIP(hipGetLastError());
  return CACTO_OK;
}

// ---------------------------------------------------------------- fused weight gradient + Adam (small batches)
// For batches whose weight-gradient rows fit 64-row chunks (rows <= 1024), k_wgrad + k_adam run as
// one launch: one wave per 16 x 16 weight tile or 16-wide bias tile of a layer, over ALL rows,
// then the Adam step (+ packed refresh, + soft update) on the tile's parameters straight from the
// accumulators. No slab round trip and one launch instead of two. The sums are formed in exactly
// the order of k_wgrad (per chunk: the four 16-row wave spans, each a 4-MFMA chain from zero,
// reduced ((p0 + p1) + p2) + p3; bias: 64-row groups, then shuffles over g) followed by k_adam's
// chunk order, so results are bit-identical to the split path.

// One parameter's step with its stores; l >= 0: a weight W_l[i][o] (direct packed writes), l < 0: a
// bias (not packed)
__device__ __forceinline__ void adam_apply(const AdamNet& N, const AdamScalars& s, int p, float g, float mm, float vv,
                                           float th, float tg, int l, int i, int o) {
  adam_math(s, g, mm, vv, th, tg);
  N.m[p] = mm;
  N.v[p] = vv;
  N.nb[p] = th;
  if (l >= 0) write_packed_w(N.pk, N.t, l, i, o, th);
  if (N.target) {
    N.target[p] = tg;
    if (l >= 0) write_packed_w(N.tpk, N.t, l, i, o, tg);
  }
}

// One workgroup per item: the 64-row chunks are dealt to the 4 waves (chunk ch to wave ch % 4),
// each chunk's partial is formed exactly as before and parked in LDS (part[ch]), and wave 0 sums
// them in chunk order and runs the Adam step: the same sums in the same order (bit-identical),
// with a quarter of the chunk loads and MFMAs on each wave.
constexpr int WA_MAXCH = 16;  // fused path: <= 1024 rows of 64
constexpr int WA_CB = WA_MAXCH / 4;  // chunks per wave

// That scheme, for the weight tiles and the bias tiles alike: load(j, lo, hi) issues the loads of the
// wave's j-th chunk (all WA_CB in flight together), park(j, ch, lo, hi) forms chunk ch's partial and
// parks it in part[ch]; [lo, hi) are the chunk's rows. After the barrier wave 0 sums the parked
// partials (wa_chunk_sum).
template <class Load, class Park>
__device__ __forceinline__ void wa_chunks(const WgArgs& a, int wave, Load&& load, Park&& park) {
#pragma unroll
  for (int j = 0; j < WA_CB; ++j) {
    const int ch = min(wave + 4 * j, a.nch - 1);
    const int lo = a.r_begin + ch * a.CH, hi = min(a.r_end, lo + a.CH);
    if (wave + 4 * j < a.nch) load(j, lo, hi);
  }
#pragma unroll
  for (int j = 0; j < WA_CB; ++j) {
    const int ch = wave + 4 * j;
    if (ch < a.nch) {
      const int lo = a.r_begin + ch * a.CH, hi = min(a.r_end, lo + a.CH);
      park(j, ch, lo, hi);
    }
  }
  __syncthreads();
}
// the lane's NQ values of every chunk's parked partial, summed in chunk order
template <int NQ>
__device__ __forceinline__ void wa_chunk_sum(const float* part, int nch, int lane, float (&gs)[NQ]) {
#pragma unroll
  for (int q = 0; q < NQ; ++q) gs[q] = part[q * 64 + lane];
  for (int ch = 1; ch < nch; ++ch)
#pragma unroll
    for (int q = 0; q < NQ; ++q) gs[q] += part[ch * 256 + q * 64 + lane];
}

__device__ __forceinline__ void wgrad_adam_item(const AdamNet& N, int item, int l, const int32_t* __restrict__ step,
                                                int wave, int lane, float* tr, float* part) {
  const int g = lane >> 4, c = lane & 15;  // l: the item's layer, from the work list (no search)
  const int rem = item - N.ioff[l];
  const WgLayer& Ly = N.wg.l[l];
  const WgArgs& a = N.wg;
  CSTAMP(1);
  if (rem < Ly.IT * Ly.OT) {
    const int it = rem / Ly.OT, ot = rem - it * Ly.OT;
    const int oc = 16 * ot + c;
    // A full 16 x 16 tile runs Adam in the row layout: lane (g, c) owns W[16 it + c][16 ot + 4g + j],
    // 4 consecutive Keras-flat parameters (float4 loads / stores; the pkT block is this layout and
    // the pk block the MFMA's C layout, one LDS transpose away). Edge tiles: per element.
    const bool full = 16 * it + 16 <= Ly.in && 16 * ot + 16 <= Ly.out;
    const int pT = Ly.woff + (16 * it + c) * Ly.out + 16 * ot + 4 * g;
    // Adam operands of the lane's 4 parameters, in flight during the GEMM
    int p[4];
    float mm[4], vv[4], th[4], tg[4];
    bool ok[4];
    if (wave != 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) ok[q] = false, p[q] = 0, mm[q] = vv[q] = th[q] = tg[q] = 0.f;
    } else if (full) {
      const float4 m4 = *reinterpret_cast<const float4*>(N.m + pT), v4 = *reinterpret_cast<const float4*>(N.v + pT);
      const float4 t4 = *reinterpret_cast<const float4*>(N.src + pT);
      const float4 g4 = N.target ? *reinterpret_cast<const float4*>(N.target + pT) : make_float4(0.f, 0.f, 0.f, 0.f);
      mm[0] = m4.x, mm[1] = m4.y, mm[2] = m4.z, mm[3] = m4.w;
      vv[0] = v4.x, vv[1] = v4.y, vv[2] = v4.z, vv[3] = v4.w;
      th[0] = t4.x, th[1] = t4.y, th[2] = t4.z, th[3] = t4.w;
      tg[0] = g4.x, tg[1] = g4.y, tg[2] = g4.z, tg[3] = g4.w;
#pragma unroll
      for (int q = 0; q < 4; ++q) ok[q] = true, p[q] = pT + q;
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int ii = 16 * it + 4 * g + q;
        ok[q] = ii < Ly.in && oc < Ly.out;
        p[q] = ok[q] ? Ly.woff + ii * Ly.out + oc : 0;
        mm[q] = N.m[p[q]];
        vv[q] = N.v[p[q]];
        th[q] = N.src[p[q]];
        tg[q] = N.target ? N.target[p[q]] : 0.f;
      }
    }
    const float* ap = Ly.LT + (size_t)(16 * it + c) * a.ld + 4 * g;
    const float* bp = Ly.RT + (size_t)(16 * ot + c) * a.ld + 4 * g;
#ifdef CACTO_STAMPS
    {  // diagnostic: latency of a first touch of this tile's panel rows (chunk 0), then the real loop
      float4 t0 = *reinterpret_cast<const float4*>(ap + a.r_begin);
      float4 t1 = *reinterpret_cast<const float4*>(bp + a.r_begin);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (t0.x == 12345.f && t1.y == 54321.f) N.m[0] = 0.f;
    }
    CSTAMP(5);
#endif
    // this wave's chunks (ch = wave + 4 j), all their panel loads in flight together
    {
      float4 A[WA_CB][4], Bv[WA_CB][4];
      wa_chunks(
          a, wave,
          [&](int j, int lo, int hi) {
#pragma unroll
            for (int w = 0; w < 4; ++w) {
              const int r = min(lo + 16 * w, hi - 16);  // clamped (branch-free); unused past hi
              A[j][w] = *reinterpret_cast<const float4*>(ap + r);
              Bv[j][w] = *reinterpret_cast<const float4*>(bp + r);
            }
          },
          [&](int j, int ch, int lo, int hi) {
            floatx4 part4[4];
#pragma unroll
            for (int w = 0; w < 4; ++w) {
              floatx4 acc = {0.f, 0.f, 0.f, 0.f};
              if (lo + 16 * w < hi) {
                acc = mfma4(A[j][w].x, Bv[j][w].x, acc);
                acc = mfma4(A[j][w].y, Bv[j][w].y, acc);
                acc = mfma4(A[j][w].z, Bv[j][w].z, acc);
                acc = mfma4(A[j][w].w, Bv[j][w].w, acc);
              }
              part4[w] = acc;
            }
            floatx4 s4 = part4[0];
#pragma unroll
            for (int w = 1; w < 4; ++w) {
              s4[0] += part4[w][0];
              s4[1] += part4[w][1];
              s4[2] += part4[w][2];
              s4[3] += part4[w][3];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) part[ch * 256 + q * 64 + lane] = s4[q];
          });
    }
    if (wave != 0) return;
    float gs[4];
    wa_chunk_sum(part, a.nch, lane, gs);
    CSTAMP(2);
#ifdef CACTO_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // diagnostic: the GEMM's results landed
#endif
    CSTAMP(3);
    const AdamScalars s = adam_scalars(N.ad, step);  // after the loads are in flight
    if (full) {
      // gradient C layout -> row layout through the wave's LDS scratch (LDS operations of one wave
      // complete in order; the wave-scope fence keeps the compiler from reordering across lanes)
#pragma unroll
      for (int q = 0; q < 4; ++q) tr[(4 * g + q) * 16 + c] = gs[q];
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      const float4 gT = *reinterpret_cast<const float4*>(tr + c * 16 + 4 * g);
      const float gv[4] = {gT.x, gT.y, gT.z, gT.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) adam_math(s, gv[j], mm[j], vv[j], th[j], tg[j]);
      *reinterpret_cast<float4*>(N.m + pT) = make_float4(mm[0], mm[1], mm[2], mm[3]);
      *reinterpret_cast<float4*>(N.v + pT) = make_float4(vv[0], vv[1], vv[2], vv[3]);
      const float4 th4 = make_float4(th[0], th[1], th[2], th[3]);
      *reinterpret_cast<float4*>(N.nb + pT) = th4;
      const NetTopo& t = N.t;
      const size_t bT = (size_t)(t.blocks + t.pkoff[l] + it * t.OT[l] + ot) * 64 + lane;  // pkT block (it, ot)
      const size_t bF = (size_t)(t.pkoff[l] + ot * t.KT[l] + it) * 64 + lane;             // pk block (ot, it)
      N.pk[bT] = th4;
      auto to_c = [&](const float (&v)[4]) {  // row layout -> C layout (the pk block)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
        for (int j = 0; j < 4; ++j) tr[c * 16 + 4 * g + j] = v[j];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        float o[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = tr[(4 * g + q) * 16 + c];
        return make_float4(o[0], o[1], o[2], o[3]);
      };
      N.pk[bF] = to_c(th);
      if (N.target) {
        const float4 tg4 = make_float4(tg[0], tg[1], tg[2], tg[3]);
        *reinterpret_cast<float4*>(N.target + pT) = tg4;
        N.tpk[bT] = tg4;
        N.tpk[bF] = to_c(tg);
      }
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (ok[q]) adam_apply(N, s, p[q], gs[q], mm[q], vv[q], th[q], tg[q], l, 16 * it + 4 * g + q, oc);
    }
  } else {
    const int ot = rem - Ly.IT * Ly.OT;
    const int oc = 16 * ot + c;
    const bool ok = wave == 0 && g == 0 && oc < Ly.out;
    const int pp = ok ? Ly.boff + oc : 0;
    float mm = 0.f, vv = 0.f, th = 0.f, tg = 0.f;
    if (wave == 0) mm = N.m[pp], vv = N.v[pp], th = N.src[pp], tg = N.target ? N.target[pp] : 0.f;
    const float* bp = Ly.RT + (size_t)(16 * min(ot, Ly.OT - 1) + c) * a.ld + 4 * g;
    // per chunk: its (<= 4) 16-row steps from max(lo, bias_r0), summed in row order from 0 — the
    // sequence k_wgrad's 64-row groups and 16-row tail produce — then the shuffles over g; chunks
    // dealt to the waves as for the weight tiles, summed in chunk order by wave 0
    {
      float4 v4[WA_CB][4];
      wa_chunks(
          a, wave,
          [&](int j, int lo, int hi) {
            const int r0 = max(lo, a.bias_r0);
#pragma unroll
            for (int k = 0; k < 4; ++k) v4[j][k] = *reinterpret_cast<const float4*>(bp + max(0, min(r0 + 16 * k, hi - 16)));
          },
          [&](int j, int ch, int lo, int hi) {
            const int r0 = max(lo, a.bias_r0);
            float sb = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (r0 + 16 * k < hi) sb += (v4[j][k].x + v4[j][k].y) + (v4[j][k].z + v4[j][k].w);
            sb += __shfl_xor(sb, 16);
            sb += __shfl_xor(sb, 32);
            part[ch * 256 + lane] = sb;
          });
    }
    if (wave != 0) return;
    float gsum[1];
    wa_chunk_sum(part, a.nch, lane, gsum);
    const AdamScalars s = adam_scalars(N.ad, step);
    if (ok) adam_apply(N, s, pp, gsum[0], mm, vv, th, tg, -1, 0, 0);
  }
}

// One or two networks (the paired update runs the critic of update t and the actor of t - 1).
// Work list: workgroup b runs on XCD b % 8 (the dispatcher's round robin; used for locality only,
// nothing depends on it) and takes one item of that XCD's bin (its 4 waves split the item's row chunks). The bins group the tiles of a layer
// into blocks of in-tiles x out-tiles, so each XCD's L2 fetches a panel slice once for several
// tiles instead of every XCD fetching every slice from the memory-side cache.
__global__ void __launch_bounds__(256) k_wgrad_adam(AdamNet n0, AdamNet n1, const int32_t* __restrict__ items,
                                                    int stride, const int32_t* step) {
  CSTAMP(0);
  // the item is wave-uniform: readfirstlane lets the compiler keep the network descriptor in
  // scalar registers (s_load from the kernel arguments) instead of chasing it through VGPR pointers
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int code = __builtin_amdgcn_readfirstlane(items[(blockIdx.x & 7) * stride + (blockIdx.x >> 3)]);
  __shared__ float tr[256];                    // wave 0: one 16 x 16 transpose
  __shared__ float part[WA_MAXCH * 256];       // per-chunk partial sums
  if (code >= 0) {
    const int l = (code >> 16) & 0xf;
    if (((code >> 15) & 1) == 0) wgrad_adam_item(n0, code & 0x7fff, l, step, wave, lane, tr, part);
    else wgrad_adam_item(n1, code & 0x7fff, l, step, wave, lane, tr, part);
  }
  CSTAMP(4);
#ifdef CACTO_STAMPS
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int k_ = 0; k_ < 6; ++k_) g_cstamps[k_] = cacto_stamp_s[k_];
#endif
}

// ---------------------------------------------------------------- R independent learners (learn.h)
// k_chain_pair_q4's two chains for R replicas in one grid: workgroup -> (replica, tile) by
// ens_tile_of, the replica's descriptor from the device table (wave-uniform, read-only during the
// call: scalar loads). mode 0: every tile a critic tile (the loop's first step), 1: every tile an
// actor tile (its last), 2: critic tiles [0, nct) then actor tiles. Each tile runs q4_critic_chain /
// q4_actor_chain on exactly the arguments the one-learner kernels give it.
template <int NJ>
__global__ void __launch_bounds__(Q4_THREADS)
    k_chain_ens_q4(const SysDevice* __restrict__ sdp, const EnsReplica* __restrict__ tab, ChainScalars cs,
                   const int32_t* __restrict__ idx_c, const int32_t* __restrict__ idx_a, long long rstride, int B,
                   int nct, int mode, EnsDeal d) {
  constexpr size_t bytes = sizeof(Q4CriticLds) > sizeof(Q4ActorLds) ? sizeof(Q4CriticLds) : sizeof(Q4ActorLds);
  __shared__ __attribute__((aligned(16))) unsigned char smem[bytes];
  const EnsTile w = ens_tile_of(d, blockIdx.x);
  if (w.r >= d.R || w.j >= d.nt) return;
  const EnsReplica& E = tab[w.r];
  if (mode == 0 || (mode == 2 && w.j < nct)) {
    q4_critic_chain(*reinterpret_cast<Q4CriticLds*>(smem), w.j, sdp, E.C, E.Tg, cs, E.storage,
                    idx_c + (size_t)w.r * rstride, nullptr, B, E.gbc, E.y, E.V, nullptr, E.step);
  } else {
    q4_actor_chain<NJ>(*reinterpret_cast<Q4ActorLds*>(smem), mode == 2 ? w.j - nct : w.j, sdp, E.Ac, E.C, cs,
                       E.storage, idx_a + (size_t)w.r * rstride, B, E.gba, E.step);
  }
}

// k_wgrad_adam for R replicas: block b runs on XCD b % 8 and takes slot (b / 8) % stride of that
// XCD's bin for replica (b / 8) / stride — the one-learner work list, once per replica.
__global__ void __launch_bounds__(256) k_wgrad_adam_ens(const EnsReplica* __restrict__ tab,
                                                        const int32_t* __restrict__ items, int stride, int mode) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int sl = blockIdx.x >> 3, r = __builtin_amdgcn_readfirstlane(sl / stride);
  const int code = __builtin_amdgcn_readfirstlane(items[(blockIdx.x & 7) * stride + (sl - r * stride)]);
  __shared__ float tr[256];
  __shared__ float part[WA_MAXCH * 256];
  if (code < 0) return;
  const EnsReplica& E = tab[r];
  const int l = (code >> 16) & 0xf;
  // the work list's network bit: n1 of the paired launch is the actor; alone, n0 is the mode's network
  if (mode == 1 || ((code >> 15) & 1)) wgrad_adam_item(E.an, code & 0x7fff, l, E.step, wave, lane, tr, part);
  else wgrad_adam_item(E.cn, code & 0x7fff, l, E.step, wave, lane, tr, part);
}

}  // namespace cacto

#ifdef CACTO_STAMPS
extern "C" int cacto_debug_critic_stamps(unsigned long long* out_h) {
  CACTO_CHECK_HIP(hipDeviceSynchronize());
  CACTO_CHECK_HIP(hipMemcpyFromSymbol(out_h, HIP_SYMBOL(g_cstamps), sizeof(unsigned long long) * 32));
  return CACTO_OK;
}
extern "C" int cacto_debug_actor_stamps(unsigned long long* out_h) {
  CACTO_CHECK_HIP(hipDeviceSynchronize());
  CACTO_CHECK_HIP(hipMemcpyFromSymbol(out_h, HIP_SYMBOL(g_astamps), sizeof(unsigned long long) * 32));
  return CACTO_OK;
}
#endif

namespace cacto {

// k_wgrad_big serves a network when every 4 x 4 tile block of it is 4 x 4, 1 x 4 or 4 x 1 tiles (the
// configs' networks; not the elu critic's 16/32/256/256)
static bool wgb_shapes(const NetTopo& t) {
  for (int l = 0; l < t.L; ++l)
    for (int i0 = 0; i0 < t.KT[l]; i0 += WG_BLK)
      for (int o0 = 0; o0 < t.OT[l]; o0 += WG_BLK) {
        const int ni = std::min(WG_BLK, t.KT[l] - i0), no = std::min(WG_BLK, t.OT[l] - o0);
        if (!((ni == 4 && (no == 4 || no == 1)) || (ni == 1 && no == 4))) return false;
      }
  return true;
}

// The route (learn.h). The rules, each with its measurement in DESIGN §3 / §6:
//   chain tile   4-sample tiles (chain_q4.h) up to Bp = 512, so a reference-size batch (64 / 128)
//                spreads over 4x the workgroups; 16-sample tiles above, and always for the elu critic
//                (elu_kernels.hip has no 4-sample form)
//   paired       while the critic's 2 Bp rows fit 64-row chunks (2 Bp <= 1024): k_wgrad + k_adam as one
//                launch (k_wgrad_adam), the critic of update t and the actor of t - 1 as one grid
//   chunk        short chunks for small batches so the grid still fills the chip; from 4096 rows on
//                256: k_wgrad_big walks a whole chunk per wave, so longer chunks amortise its fill
//   k_wgrad_big  above 1024 rows, for the networks it has the block shapes of
//   xcd          chunks grouped by XCD from 8 chunks on
//   xcd_tiles    the 16-sample chain tiles dealt to the XCD that k_wgrad_big runs their 256-row chunk
//                on: whole groups of 128 tiles, both networks on 256-row chunks
//   pair_xcds    about 8 tiles of the paired q4 grid (2 Bp / 4) per XCD, at most all 8 XCDs
LearnRoute learn_route(const NetTopo& critic, const NetTopo& actor, bool sobolev, int B, int cus) {
  LearnRoute r{};
  r.Bp = (B + 15) / 16 * 16;
  r.elu = is_elu_topo(critic);
  r.tile = !r.elu && r.Bp <= 512 ? Q4_TILE : CACTO_TILE;
  r.paired = 2 * r.Bp <= 1024;
  auto net = [&](const NetTopo& t, int rows) {
    NetRoute n{};
    n.rows = rows;
    n.chunk = rows <= 1024 ? 64 : rows < 4096 ? 128 : 256;
    n.nch = ceil_div(rows, n.chunk);
    n.gemm = r.paired ? WG_FUSED : rows > 1024 && wgb_shapes(t) ? WG_BIG : WG_SPLIT;
    n.xcd = n.nch >= 8;
    n.adam_nch = nch_instance(n.nch);
    return n;
  };
  r.critic = net(critic, sobolev ? 2 * r.Bp : r.Bp);
  r.actor = net(actor, r.Bp);
  r.xcd_tiles = (r.Bp / CACTO_TILE) % 128 == 0 && r.critic.chunk == 256 && r.actor.chunk == 256;
  if (r.tile == Q4_TILE)
    for (r.pair_xcds = 1; r.pair_xcds < 8 && 2 * (r.Bp / Q4_TILE) > 8 * r.pair_xcds;) r.pair_xcds *= 2;
  r.per_overlap = r.critic.gemm == WG_BIG && r.critic.adam_nch != 0;
  r.devwait_actor = r.tile == CACTO_TILE && r.Bp / CACTO_TILE <= cus;
  return r;
}

int cu_count() {
  static const int cus = [] {
    int dev = 0, v = 0;
    return (hipGetDevice(&dev) == hipSuccess &&
            hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
               ? v
               : 256;
  }();
  return cus;
}
template <int NJ>
struct LaunchActorChain {
  static int run(const cacto_sys* sys, const LearnRoute& r, NetView Ac, NetView C, ChainScalars cs,
                 const double* storage, const int32_t* idx, int B, GradBufs gb, int32_t* step, hipStream_t st) {
    if (r.elu) return launch_actor_chain_elu(sys, Ac, C, cs, storage, idx, B, gb, step, st);
    if (r.tile == Q4_TILE)
      hipLaunchKernelGGL(k_actor_grad_q4<NJ>, dim3(r.Bp / Q4_TILE), dim3(Q4_THREADS), 0, st, sys->dev, Ac, C, cs,
                         storage, idx, B, gb, step);
    else
      hipLaunchKernelGGL(k_actor_grad<NJ>, dim3(r.Bp / 16), dim3(CACTO_THREADS), 0, st, sys->dev, Ac, C, cs, storage,
                         idx, B, gb, step);
    CACTO_CHECK_HIP(hipGetLastError());
    return CACTO_OK;
  }
};

// nct: critic tiles (= actor tiles) of the batch's chain tile size
template <int NJ>
struct LaunchChainPair {
  static int run(const cacto_sys* sys, const LearnRoute& r, NetView C, NetView Tg, NetView Ac, ChainScalars cs,
                 const double* storage, const int32_t* idx_c, const float* isw, const int32_t* idx_a, int B,
                 GradBufs gbc, GradBufs gba, float* y, float* V, int32_t* step, hipStream_t st) {
    const int Bp = r.Bp;
    if (r.tile == Q4_TILE) {
      const int nct = Bp / Q4_TILE;
      const int nx = r.pair_xcds;
      hipLaunchKernelGGL(k_chain_pair_q4<NJ>, dim3(8 * ceil_div(2 * nct, nx)), dim3(Q4_THREADS), 0, st, sys->dev, C,
                         Tg, Ac, cs, storage, idx_c, isw, idx_a, B, nct, gbc, gba, y, V, step, nx);
    } else {
      const int nct = Bp / CACTO_TILE;
      hipLaunchKernelGGL(k_chain_pair<NJ>, dim3(2 * nct), dim3(CACTO_THREADS), 0, st, sys->dev, C, Tg, Ac, cs,
                         storage, idx_c, isw, idx_a, B, nct, gbc, gba, y, V, step);
    }
    CACTO_CHECK_HIP(hipGetLastError());
    return CACTO_OK;
  }
};

// the GEMM's arguments for a network's n.rows gradient rows, which end at r_end
static WgArgs wg_args(const NetTopo& t, const GradBufs& gb, const NetRoute& n, int r_end, int bias_r0) {
  WgArgs a{};
  a.nl = t.L;
  a.ld = gb.ld;
  a.r_begin = r_end - n.rows;
  a.r_end = r_end;
  a.bias_r0 = bias_r0;
  a.CH = n.chunk;
  a.nch = n.nch;
  a.P = t.params;
  int tpc = 0;  // workgroups per chunk: 4x4 tile blocks + groups of 4 bias tiles, per layer
  for (int l = 0; l < t.L; ++l) {
    a.l[l] = WgLayer{gb.LT[l], gb.RT[l], t.in[l], t.out[l], t.KT[l], t.OT[l], t.woff[l], t.boff[l]};
    a.toff[l] = tpc;
    tpc += ceil_div(t.KT[l], WG_BLK) * ceil_div(t.OT[l], WG_BLK) + ceil_div(t.OT[l], WG_BLK);
  }
  a.toff[t.L] = tpc;
  a.tpc = tpc;
  // items by decreasing work: 4 x 4 tile blocks, then edge blocks, then bias groups (stable)
  std::vector<std::pair<int, int>> cost;
  for (int l = 0; l < t.L; ++l) {
    const int nbi = ceil_div(t.KT[l], WG_BLK), nbo = ceil_div(t.OT[l], WG_BLK);
    for (int k = 0; k < nbi * nbo; ++k) {
      const int ni = std::min(WG_BLK, t.KT[l] - (k / nbo) * WG_BLK), no = std::min(WG_BLK, t.OT[l] - (k % nbo) * WG_BLK);
      cost.push_back({-ni * no, a.toff[l] + k});
    }
    for (int k = 0; k < nbo; ++k) cost.push_back({0, a.toff[l] + nbi * nbo + k});
  }
  std::stable_sort(cost.begin(), cost.end(), [](const std::pair<int, int>& x, const std::pair<int, int>& y) {
    return x.first < y.first;
  });
  for (int k = 0; k < 64; ++k) a.perm[k] = k < tpc ? (unsigned char)cost[k].second : 0;
  return a;
}

// the split weight-gradient GEMM of one network into its n.nch slabs (the kernel of a fused batch's
// slab form is k_wgrad: its rows fit 64-row chunks)
static int launch_wgrad(const NetTopo& t, const GradBufs& gb, const NetRoute& n, int r_end, int bias_r0, float* slab,
                        hipStream_t st, unsigned long long* sig_p, unsigned long long sig_v,
                        const PerRunArgs* per_run) {
  const WgArgs a = wg_args(t, gb, n, r_end, bias_r0);
  // (k_wgrad_big's rows, more than 1024 in chunks of 128 or 256, make 9 chunks or more: always by XCD)
  const int grid = n.xcd ? 8 * ceil_div(a.nch, 8) * a.tpc : a.nch * a.tpc;
  if (per_run) {  // the PER loop's fused form (the caller checked route.per_overlap and the tree's shape)
    const int nroot = (int)(per_run->cap / PER_RUN_SUB);
    hipLaunchKernelGGL(k_wgrad_big_per, dim3(grid + nroot), dim3(256), 0, st, a, slab, grid, *per_run, nroot);
  } else if (n.gemm == WG_BIG) {
    hipLaunchKernelGGL(k_wgrad_big, dim3(grid), dim3(256), 0, st, a, slab, sig_p, sig_v);
  } else {
    hipLaunchKernelGGL(k_wgrad, dim3(grid), dim3(256), 0, st, a, slab, n.xcd, sig_p, sig_v);
  }
  CACTO_CHECK_HIP(hipGetLastError());
  return CACTO_OK;
}

// the critic's gradient rows end at 2 Bp: the plain half [Bp, 2 Bp) always, the Sobolev half [0, Bp)
// before it with w_S != 0; its biases sum over the plain half
int launch_critic_wgrad(const cacto_sys* sys, const Workspace& w, hipStream_t st, const PerRunArgs* per_run) {
  return launch_wgrad(sys->critic, w.crit, w.route.critic, 2 * w.Bp, w.Bp, w.slab, st, nullptr, 0, per_run);
}

int launch_actor_wgrad(const cacto_sys* sys, const Workspace& w, hipStream_t st, unsigned long long* sig_p,
                       unsigned long long sig_v) {
  return launch_wgrad(sys->actor, w.act, w.route.actor, w.Bp, 0, w.slab_a, st, sig_p, sig_v, nullptr);
}

ChainScalars chain_scalars(const cacto_update_cfg* cfg, const LearnRoute& r, int B) {
  ChainScalars cs;
  cs.w_S = (float)cfg->w_S;
  cs.MC = cfg->MC;
  cs.B_global = cfg->B_global > 0 ? cfg->B_global : B;
  cs.want_vt = cfg->want_target_V;
  cs.wait_p = nullptr;
  cs.wait_v = 0;
  cs.wait_at_start = 0;
  cs.xcd_tiles = r.xcd_tiles;
  return cs;
}

static AdamArgs adam_args(const cacto_update_cfg* cfg, int which, int soft) {
  AdamArgs a{};
  a.beta1 = cfg->beta1;
  a.beta2 = cfg->beta2;
  a.eps = cfg->epsilon;
  a.tau = cfg->tau;
  const double* lr = which == CACTO_NET_CRITIC ? cfg->critic_lr : cfg->actor_lr;
  for (int k = 0; k < 5; ++k) a.lr[k] = lr[k];
  for (int k = 0; k < 4; ++k) a.bounds[k] = cfg->lr_bounds[k];
  a.which = which == CACTO_NET_CRITIC ? 0 : 1;
  a.soft = soft;
  return a;
}

int launch_critic_chain(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg,
                        const double* storage, const int32_t* idx, const float* isw, int B, float* y, float* V,
                        float* Vt, const Workspace& w, hipStream_t st) {
  NetView C = cacto_make_view(sys, CACTO_NET_CRITIC, nets->critic_d);
  NetView Tg = cacto_make_view(sys, CACTO_NET_CRITIC, nets->target_d);
  const ChainScalars cs = chain_scalars(cfg, w.route, B);
  float* yb = y ? y : w.scal;
  float* Vb = V ? V : w.scal + w.Bp;
  float* Vtb = Vt ? Vt : w.scal + 2 * w.Bp;
  if (w.route.elu)
    return launch_critic_chain_elu(sys, C, Tg, cs, storage, idx, isw, B, w.crit, yb, Vb, Vtb, nets->step_d, st);
  if (w.route.tile == Q4_TILE)
    hipLaunchKernelGGL(k_critic_grad_q4, dim3(w.Bp / Q4_TILE), dim3(Q4_THREADS), 0, st, sys->dev, C, Tg, cs,
                       storage, idx, isw, B, w.crit, yb, Vb, Vtb, nets->step_d);
  else
    hipLaunchKernelGGL(k_critic_grad, dim3(w.Bp / 16), dim3(CACTO_THREADS), 0, st, sys->dev, C, Tg, cs, storage, idx,
                       isw, B, w.crit, yb, Vb, Vtb, nets->step_d);
  CACTO_CHECK_HIP(hipGetLastError());
  return CACTO_OK;
}

int launch_actor_chain(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg,
                       const double* storage, const int32_t* idx, int B, const Workspace& w, hipStream_t st,
                       const unsigned long long* wait_p, unsigned long long wait_v, int wait_at_start) {
  NetView Ac = cacto_make_view(sys, CACTO_NET_ACTOR, nets->actor_d);
  NetView C = cacto_make_view(sys, CACTO_NET_CRITIC, nets->critic_d);
  ChainScalars cs = chain_scalars(cfg, w.route, B);
  cs.wait_p = wait_p;
  cs.wait_v = wait_v;
  cs.wait_at_start = wait_at_start;
  return dispatch_nj<LaunchActorChain>(sys->host.p, sys, w.route, Ac, C, cs, storage, idx, B, w.act, nets->step_d, st);
}

// the critic chain of one update and the actor chain of the one before as one grid (small batches)
int launch_chain_pair(const cacto_sys* sys, const NetView& C, const NetView& Tg, const NetView& Ac,
                      const ChainScalars& cs, const double* storage, const int32_t* idx_c, const float* isw,
                      const int32_t* idx_a, int B, const Workspace& w, float* y, float* V, int32_t* step,
                      hipStream_t st) {
  if (w.route.elu)
    return launch_chain_pair_elu(sys, C, Tg, Ac, cs, storage, idx_c, isw, idx_a, B, w.crit, w.act, y, V, step, st);
  return dispatch_nj<LaunchChainPair>(sys->host.p, sys, w.route, C, Tg, Ac, cs, storage, idx_c, isw, idx_a, B, w.crit,
                                      w.act, y, V, step, st);
}

// src: the weights the step starts from (nullptr = in place; cacto_update_n steps the critic from one
// buffer into the other)
int launch_adam(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg, int which,
                const float* slab, int nch, int soft, hipStream_t st, const float* src,
                const unsigned long long* wait_p, unsigned long long wait_v, unsigned long long* sig_p,
                unsigned long long sig_v, const PerSampleArgs* sample, int thru) {
  const NetTopo& t = topo(sys, which);
  float* nb = which == CACTO_NET_CRITIC ? nets->critic_d : nets->actor_d;
  float* m = which == CACTO_NET_CRITIC ? nets->critic_m_d : nets->actor_m_d;
  float* v = which == CACTO_NET_CRITIC ? nets->critic_v_d : nets->actor_v_d;
  float4* pk = reinterpret_cast<float4*>(nb + flat_span(t));
  float4* tpk = reinterpret_cast<float4*>(nets->target_d + flat_span(t));
  const AdamArgs aa = adam_args(cfg, which, soft && which == CACTO_NET_CRITIC);
  const float* s0 = src ? src : nb;
  if (sample && ((sig_p && !thru) || nch > 64)) {  // the PER loop's fused form (route.per_overlap: nch <= 64)
    set_error("k_adam_sample: a publishing Adam writes through; at most 64 chunks");
    return CACTO_EINVAL;
  }
  // one parameter per thread with all chunk partials in flight (<NCH>), else the looped kernel
  nch_dispatch(nch, (t.params + 255) / 256, [&](auto n, int grid) {
    constexpr int NCH = decltype(n)::value;
    if constexpr (NCH > 0) {
      if (sample) {
        const int ns = (sample->B + 255) / 256;
        hipLaunchKernelGGL(k_adam_sample<NCH>, dim3(grid + ns), dim3(256), 0, st, slab, nch, t, s0, nb, pk, m, v,
                           nets->step_d, aa, nets->target_d, tpk, wait_p, wait_v, grid, *sample, sig_p, sig_v, thru);
        return;
      }
    }
    hipLaunchKernelGGL(k_adam<NCH>, dim3(grid), dim3(256), 0, st, slab, nch, t, s0, nb, pk, m, v, nets->step_d, aa,
                       nets->target_d, tpk, wait_p, wait_v, sig_p, sig_v, thru);
  });
  CACTO_CHECK_HIP(hipGetLastError());
  return CACTO_OK;
}

static AdamNet adam_net(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg, int which,
                        const GradBufs& gb, const NetRoute& nr, int r_end, int bias_r0, int soft, const float* src,
                        float* nb) {
  AdamNet n{};
  const NetTopo& t = topo(sys, which);
  n.wg = wg_args(t, gb, nr, r_end, bias_r0);
  n.t = t;
  n.nb = nb;
  n.src = src ? src : nb;
  n.pk = reinterpret_cast<float4*>(nb + flat_span(t));
  n.m = which == CACTO_NET_CRITIC ? nets->critic_m_d : nets->actor_m_d;
  n.v = which == CACTO_NET_CRITIC ? nets->critic_v_d : nets->actor_v_d;
  const bool sft = soft && which == CACTO_NET_CRITIC;
  n.target = sft ? nets->target_d : nullptr;
  n.tpk = sft ? reinterpret_cast<float4*>(nets->target_d + flat_span(t)) : nullptr;
  n.ad = adam_args(cfg, which, sft);
  int items = 0;
  for (int l = 0; l < t.L; ++l) {
    n.ioff[l] = items;
    items += t.KT[l] * t.OT[l] + t.OT[l];
  }
  n.ioff[t.L] = items;
  for (int l = t.L + 1; l <= MAX_LAYERS; ++l) n.ioff[l] = items;
  n.items = items;
  return n;
}

AdamNet critic_adam_net(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg, const Workspace& w,
                        int soft, const float* src, float* nb) {
  return adam_net(sys, nets, cfg, CACTO_NET_CRITIC, w.crit, w.route.critic, 2 * w.Bp, w.Bp, soft, src, nb);
}

AdamNet actor_adam_net(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg, const Workspace& w) {
  return adam_net(sys, nets, cfg, CACTO_NET_ACTOR, w.act, w.route.actor, w.Bp, 0, 0, nullptr, nets->actor_d);
}

// mode 0: critic alone (n0), 1: actor alone (n0), 2: critic (n0) and actor (n1)
int launch_wgrad_adam(const cacto_sys* sys, int mode, const AdamNet& n0, const AdamNet* n1, const int32_t* step,
                      hipStream_t st) {
  const int stride = sys->wa_stride[mode];
  // one item per workgroup (the 4 waves split its chunks); a paired batch's (learn_route) row sets
  // are within WA_MAXCH chunks of 64
  if (n0.wg.nch > WA_MAXCH || (n1 && n1->wg.nch > WA_MAXCH)) {
    set_error("k_wgrad_adam: more than WA_MAXCH row chunks");
    return CACTO_EINVAL;
  }
  hipLaunchKernelGGL(k_wgrad_adam, dim3(8 * stride), dim3(256), 0, st, n0, n1 ? *n1 : n0, sys->wa_items[mode],
                     stride, step);
  CACTO_CHECK_HIP(hipGetLastError());
  return CACTO_OK;
}

// One mode's work list of k_wgrad_adam (cacto_build_wgrad_adam_items, below): the 8 XCD bins padded
// to a common stride, which is returned; flat (optional): the [8][stride] item codes.
static int wa_bins(const NetTopo& critic, const NetTopo& actor, int mode, std::vector<int32_t>* flat) {
  std::vector<int32_t> bins[8];
  const NetTopo* nets[2] = {&critic, &actor};
  for (int n = 0; n < 2; ++n) {
    if ((mode == 0 && n == 1) || (mode == 1 && n == 0)) continue;
    const int tag = (mode == 2 && n == 1) ? 1 : 0;  // n1 in the paired launch
    const NetTopo& t = *nets[n];
    int base = 0;
    for (int l = 0; l < t.L; ++l) {
      const int IT = t.KT[l], OT = t.OT[l];
      // bi x bo = 8 with the blocks (IT/bi) x (OT/bo) closest to square; both within the grid
      int bi = 1;
      double best = 1e30;
      for (int c = 1; c <= 8; c *= 2) {
        if (c > IT || 8 / c > OT) continue;
        const double d = std::abs((double)IT / c - (double)OT / (8 / c));
        if (d < best) best = d, bi = c;
      }
      if (best == 1e30) bi = std::max(1, std::min(IT, 8));  // grid smaller than 8 blocks
      const int bo = std::max(1, 8 / bi);
      for (int it = 0; it < IT; ++it)
        for (int ot = 0; ot < OT; ++ot) {
          const int bin = ((it * bi) / IT) * bo + std::min(bo - 1, (ot * bo) / OT);
          bins[bin % 8].push_back((l << 16) | (tag << 15) | (base + it * OT + ot));
        }
      for (int ot = 0; ot < OT; ++ot) {
        const int bin = std::min(bo - 1, (ot * bo) / OT);
        bins[bin % 8].push_back((l << 16) | (tag << 15) | (base + IT * OT + ot));
      }
      base += IT * OT + OT;
    }
  }
  size_t S = 4;
  for (auto& b : bins) S = std::max(S, (b.size() + 3) / 4 * 4);
  if (flat) {
    flat->assign(8 * S, -1);
    for (int x = 0; x < 8; ++x)
      for (size_t k = 0; k < bins[x].size(); ++k) (*flat)[x * S + k] = bins[x][k];
  }
  return (int)S;
}
static int wa_stride_of(const NetTopo& critic, const NetTopo& actor, int mode) {
  return wa_bins(critic, actor, mode, nullptr);
}
// The ensemble's route (learn.h): the one-learner route of the batch, which must be the paired one
// on 4-sample tiles, and the replicas' deal over the XCDs. With R = 1 the paired steps' deal and
// grid are k_chain_pair_q4's (tile sl * nx + b % 8 on block b, 8 * ceil(2 nct / nx) workgroups) and
// the GEMM + Adam launches have k_wgrad_adam's grids. The lone first and last step differ from the
// one-learner kernels' plain grid of nct workgroups: they take the same XCD deal, 8 * ceil(nct / nx)
// workgroups (B = 64: 32 against 16), the surplus exiting at once.
EnsRoute ens_route(const NetTopo& critic, const NetTopo& actor, bool sobolev, int B, int R, int cus) {
  EnsRoute e{};
  e.R = R;
  if (B <= 0) {
    e.reason = ENS_BAD_B;
    return e;
  }
  e.one = learn_route(critic, actor, sobolev, B, cus);
  e.reason = R < 1 || R > ENS_MAX_R ? ENS_BAD_R
             : e.one.elu            ? ENS_ELU
             : !e.one.paired || e.one.tile != Q4_TILE ? ENS_NOT_PAIRED
                                                      : ENS_OK;
  if (e.reason != ENS_OK) return e;
  e.supported = 1;
  e.nct = e.one.Bp / Q4_TILE;
  const int nx = e.one.pair_xcds;
  e.pair = EnsDeal{R, nx, 8 / nx, ceil_div(2 * e.nct, nx), 2 * e.nct};
  e.lone = EnsDeal{R, nx, 8 / nx, ceil_div(e.nct, nx), e.nct};
  for (int m = 0; m < 3; ++m) e.wa_stride[m] = wa_stride_of(critic, actor, m);
  e.lds_bytes = (int)std::max(sizeof(Q4CriticLds), sizeof(Q4ActorLds));
  return e;
}

template <int NJ>
struct LaunchChainEns {
  static int run(const cacto_sys* sys, const EnsRoute& er, const EnsReplica* tab, const ChainScalars& cs,
                 const int32_t* idx_c, const int32_t* idx_a, long long rstride, int B, int mode, hipStream_t st) {
    const EnsDeal& d = mode == 2 ? er.pair : er.lone;
    hipLaunchKernelGGL(k_chain_ens_q4<NJ>, dim3(ens_chain_grid(d)), dim3(Q4_THREADS), 0, st, sys->dev, tab, cs, idx_c,
                       idx_a, rstride, B, er.nct, mode, d);
    CACTO_CHECK_HIP(hipGetLastError());
    return CACTO_OK;
  }
};

int launch_chain_ens(const cacto_sys* sys, const EnsRoute& er, const EnsReplica* tab, const ChainScalars& cs,
                     const int32_t* idx_c, const int32_t* idx_a, long long rstride, int B, int mode, hipStream_t st) {
  return dispatch_nj<LaunchChainEns>(sys->host.p, sys, er, tab, cs, idx_c, idx_a, rstride, B, mode, st);
}

int launch_wgrad_adam_ens(const cacto_sys* sys, const EnsRoute& er, const EnsReplica* tab, int mode, hipStream_t st) {
  const int stride = sys->wa_stride[mode];
  // as launch_wgrad_adam: one item per workgroup, its row chunks parked in part[WA_MAXCH]
  if ((mode != 1 && er.one.critic.nch > WA_MAXCH) || (mode != 0 && er.one.actor.nch > WA_MAXCH)) {
    set_error("k_wgrad_adam_ens: more than WA_MAXCH row chunks");
    return CACTO_EINVAL;
  }
  hipLaunchKernelGGL(k_wgrad_adam_ens, dim3(8 * stride * er.R), dim3(256), 0, st, tab, sys->wa_items[mode], stride,
                     mode);
  CACTO_CHECK_HIP(hipGetLastError());
  return CACTO_OK;
}

int launch_soft(const cacto_sys* sys, const cacto_nets* nets, float tau, hipStream_t st) {
  const NetTopo& t = sys->critic;
  hipLaunchKernelGGL(k_soft, dim3(std::min((t.params + 255) / 256, 1024)), dim3(256), 0, st, t, nets->critic_d,
                     nets->target_d, reinterpret_cast<float4*>(nets->target_d + flat_span(t)), (double)tau);
  CACTO_CHECK_HIP(hipGetLastError());
  return CACTO_OK;
}

int launch_pipe_probe(unsigned long long* w, int role, hipStream_t st) {
  hipLaunchKernelGGL(k_pipe_probe, dim3(1), dim3(64), 0, st, w, role);
  CACTO_CHECK_HIP(hipGetLastError());
  return CACTO_OK;
}

}  // namespace cacto

using namespace cacto;

// k_wgrad_adam's XCD bins (see the kernel). Per layer the IT x OT weight tiles are cut into bi x bo
// = 8 blocks (bi chosen so the blocks are as square as the tile grid allows), block k to bin k; a
// layer's bias tiles go to the bin of their out-tile block. Item numbering is AdamNet's (per layer:
// IT * OT weight tiles, row-major in (it, ot), then OT bias tiles).
// Code: bits 0-14 the item, bit 15 the network (n1 of the paired launch), bits 16-19 the layer
// (so the kernel does not search AdamNet::ioff with dependent scalar loads); -1 = no item.
int cacto_build_wgrad_adam_items(cacto_sys* sys) {
  for (int mode = 0; mode < 3; ++mode) {
    std::vector<int32_t> flat;
    sys->wa_stride[mode] = wa_bins(sys->critic, sys->actor, mode, &flat);
    CACTO_CHECK_HIP(hipMalloc(&sys->wa_items[mode], flat.size() * sizeof(int32_t)));
    CACTO_CHECK_HIP(hipMemcpy(sys->wa_items[mode], flat.data(), flat.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  return CACTO_OK;
}
