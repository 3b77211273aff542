// Host side of the learner: workspace planning, the C ABI of the update calls, the paired small-batch
// pipeline, the two-stream pipeline (side stream, concurrency probe, timeout latch) and its RCCL form.
// No kernel is named here: every launch goes through learn_kernels.hip's launch_* functions (learn.h).
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "learn.h"

using namespace cacto;

namespace {
inline size_t align64(size_t n) { return (n + 63) / 64 * 64; }
// One critic net buffer (flat weights + the two packed copies) of the three the two-stream pipelines
// rotate the critic over: its floats, and the stride of the two workspace copies (Workspace::cshadow).
inline size_t critic_buf_floats(const NetTopo& tc) { return (size_t)flat_span(tc) + (size_t)2 * tc.blocks * 256; }
inline size_t critic_buf_bytes(const NetTopo& tc) { return critic_buf_floats(tc) * sizeof(float); }
inline size_t critic_buf_stride(const NetTopo& tc) { return align64(critic_buf_floats(tc)); }

// The route and the workspace map of a call of batch B. The map does not depend on `sobolev`: the
// critic's slabs are sized for its 2 Bp rows either way.
Workspace plan(const cacto_sys* sys, bool sobolev, int B, char* base) {
  Workspace w{};
  w.route = learn_route(sys->critic, sys->actor, sobolev, B, cu_count());
  const int Bp = w.route.Bp;
  w.Bp = Bp;
  const NetTopo& tc = sys->critic;
  const NetTopo& ta = sys->actor;
  size_t off = 0;
  float* f = reinterpret_cast<float*>(base);
  // critic panels (ld = 2Bp)
  w.crit.ld = 2 * Bp;
  w.crit.Bp = Bp;
  size_t coff = 0;
  for (int l = 0; l < tc.L; ++l) {
    w.crit.LT[l] = f ? f + coff : nullptr;
    coff += (size_t)16 * tc.KT[l] * w.crit.ld;
    w.crit.RT[l] = f ? f + coff : nullptr;
    coff += (size_t)16 * tc.OT[l] * w.crit.ld;
  }
  w.act.ld = Bp;
  w.act.Bp = Bp;
  size_t aoff = align64(coff);  // the actor panels follow the critic's (no aliasing, see slab_a)
  for (int l = 0; l < ta.L; ++l) {
    w.act.LT[l] = f ? f + aoff : nullptr;
    aoff += (size_t)16 * ta.KT[l] * w.act.ld;
    w.act.RT[l] = f ? f + aoff : nullptr;
    aoff += (size_t)16 * ta.OT[l] * w.act.ld;
  }
  off = align64(aoff);
  const int nch_a = w.route.actor.nch;
  const int nch_c = sobolev ? w.route.critic.nch  // of the 2 Bp rows
                            : learn_route(sys->critic, sys->actor, true, B, cu_count()).critic.nch;
  w.slab = f ? f + off : nullptr;
  off += align64((size_t)nch_c * tc.params);
  w.slab_a = f ? f + off : nullptr;
  off += align64((size_t)nch_a * ta.params);
  w.cshadow = f ? f + off : nullptr;
  off += 2 * critic_buf_stride(tc);
  w.pidx = f ? reinterpret_cast<int32_t*>(f + off) : nullptr;
  off += align64((size_t)5 * Bp);
  w.pisw = f ? f + off : nullptr;
  off += align64((size_t)Bp);
  w.runs = f ? reinterpret_cast<int32_t*>(f + off) : nullptr;
  off += align64((size_t)2 * PER_RUN_SUB);
  w.scal = f ? f + off : nullptr;
  off += align64((size_t)3 * Bp);
  w.bytes = off * sizeof(float);
  return w;
}

int check_nets(const cacto_nets* n) {
  CACTO_REQUIRE(n && n->actor_d && n->actor_m_d && n->actor_v_d && n->critic_d && n->critic_m_d && n->critic_v_d &&
                    n->target_d && n->step_d,
                "cacto_nets: null member");
  return CACTO_OK;
}

// critic step after its chain: GEMM + Adam (+ soft update) from src into nb
int critic_step_tail(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg, const Workspace& w,
                     hipStream_t st, const float* src, float* nb, const unsigned long long* wait_p = nullptr,
                     unsigned long long wait_v = 0, unsigned long long* sig_p = nullptr, unsigned long long sig_v = 0,
                     const PerRunArgs* per_run = nullptr, const PerSampleArgs* sample = nullptr, int thru = 0) {
  const int soft = cfg->MC ? 0 : 1;
  if (w.route.critic.gemm == WG_FUSED)
    return launch_wgrad_adam(sys, 0, critic_adam_net(sys, nets, cfg, w, soft, src, nb), nullptr, nets->step_d, st);
  if (int e = launch_critic_wgrad(sys, w, st, per_run)) return e;
  cacto_nets dst = *nets;
  dst.critic_d = nb;
  return launch_adam(sys, &dst, cfg, CACTO_NET_CRITIC, w.slab, w.route.critic.nch, soft, st, src, wait_p, wait_v, sig_p,
                     sig_v, sample, thru);
}

int actor_step_tail(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg, const Workspace& w,
                    hipStream_t st, unsigned long long* sig_p = nullptr, unsigned long long sig_v = 0) {
  if (w.route.actor.gemm == WG_FUSED)
    return launch_wgrad_adam(sys, 1, actor_adam_net(sys, nets, cfg, w), nullptr, nets->step_d, st);
  if (int e = launch_actor_wgrad(sys, w, st, sig_p, sig_v)) return e;
  return launch_adam(sys, nets, cfg, CACTO_NET_ACTOR, w.slab_a, w.route.actor.nch, 0, st);
}

#define CHECK_WS(ws, nbytes, B)                                                                   \
  CACTO_REQUIRE((ws) != nullptr && (nbytes) >= plan(sys, true, (B), nullptr).bytes,               \
                "workspace too small: query cacto_workspace_bytes(sys, B)");                      \
  CACTO_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "workspace must be 256-byte aligned")

// Data-parallel form of the paired schedule (update_pipeline_pair): per step, the gradients of the
// critic step of update t and of the actor step of update t - 1 (either may be absent) go to one
// flat buffer [critic P | actor P], the caller all-reduces it once (RCCL), then both Adam steps.
// stage bit 0: the chain(s) and the critic's weight gradient; bit 1: the actor's weight gradient
// (which reads only the actor chain's panels in the workspace)
int pair_grads(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg, const double* storage_d,
               const int32_t* idx_c_d, const float* is_w_d, const int32_t* idx_a_d, int B, float* grad_d, float* y_d,
               float* V_d, void* workspace_d, size_t workspace_bytes, int stages, hipStream_t st) {
  CHECK_WS(workspace_d, workspace_bytes, B);
  const Workspace w = plan(sys, cfg->w_S != 0.0, B, static_cast<char*>(workspace_d));
  const int Pc = sys->critic.params, Pa = sys->actor.params;
  if (stages & 2) {
    if (!idx_a_d) return CACTO_OK;
    if (int e = launch_actor_wgrad(sys, w, st)) return e;
    return launch_reduce(w.slab_a, w.route.actor.nch, Pa, grad_d + Pc, st);
  }
  float* yb = y_d ? y_d : w.scal;
  float* Vb = V_d ? V_d : w.scal + w.Bp;
  if (idx_c_d && idx_a_d) {
    const NetView C = cacto_make_view(sys, CACTO_NET_CRITIC, nets->critic_d);
    const NetView Tg = cacto_make_view(sys, CACTO_NET_CRITIC, nets->target_d);
    const NetView Ac = cacto_make_view(sys, CACTO_NET_ACTOR, nets->actor_d);
    if (int e = launch_chain_pair(sys, C, Tg, Ac, chain_scalars(cfg, w.route, B), storage_d, idx_c_d, is_w_d, idx_a_d,
                                  B, w, yb, Vb, nets->step_d, st))
      return e;
  } else if (idx_c_d) {
    if (int e = launch_critic_chain(sys, nets, cfg, storage_d, idx_c_d, is_w_d, B, yb, Vb, nullptr, w, st)) return e;
  } else {
    if (int e = launch_actor_chain(sys, nets, cfg, storage_d, idx_a_d, B, w, st)) return e;
  }
  if (idx_c_d) {
    if (int e = launch_critic_wgrad(sys, w, st)) return e;
    if (int e = launch_reduce(w.slab, w.route.critic.nch, Pc, grad_d, st)) return e;
  }
  if (stages & 2) return pair_grads(sys, nets, cfg, storage_d, idx_c_d, is_w_d, idx_a_d, B, grad_d, y_d, V_d,
                                    workspace_d, workspace_bytes, 2, st);
  return CACTO_OK;
}
}  // namespace

extern "C" size_t cacto_workspace_bytes(const cacto_sys* sys, int B) {
  if (!sys || B <= 0) return 0;
  return plan(sys, true, B, nullptr).bytes;
}

// the route, reported
extern "C" int cacto_update_plan(const cacto_sys* sys, int sobolev, int B, cacto_upd_plan* out) {
  CACTO_REQUIRE(sys && out && B > 0, "cacto_update_plan: bad arguments");
  const int cus = cu_count();
  const LearnRoute r = learn_route(sys->critic, sys->actor, sobolev != 0, B, cus);
  const NetRoute &c = r.critic, &a = r.actor;
  *out = cacto_upd_plan{r.Bp,       r.tile,    r.elu,      r.paired,  c.rows,     c.chunk,     c.nch,
                        c.gemm,     c.xcd,     c.adam_nch, a.rows,    a.chunk,    a.nch,       a.gemm,
                        a.xcd,      a.adam_nch, r.xcd_tiles, r.pair_xcds, r.per_overlap, r.devwait_actor, cus};
  return CACTO_OK;
}

extern "C" int cacto_critic_grad(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg,
                                 const double* storage_d, const int32_t* idx_d, const float* is_w_d, int B,
                                 float* grad_d, float* y_d, float* V_d, float* Vt_d, void* workspace_d,
                                 size_t workspace_bytes, void* stream) {
  CACTO_REQUIRE(sys && cfg && storage_d && idx_d && grad_d && B > 0, "cacto_critic_grad: bad arguments");
  if (int e = check_nets(nets)) return e;
  CHECK_WS(workspace_d, workspace_bytes, B);
  const Workspace w = plan(sys, (float)cfg->w_S != 0.f, B, static_cast<char*>(workspace_d));
  hipStream_t st = as_stream(stream);
  if (int e = launch_critic_chain(sys, nets, cfg, storage_d, idx_d, is_w_d, B, y_d, V_d, Vt_d, w, st)) return e;
  if (int e = launch_critic_wgrad(sys, w, st)) return e;
  return launch_reduce(w.slab, w.route.critic.nch, sys->critic.params, grad_d, st);
}

extern "C" int cacto_actor_grad(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg,
                                const double* storage_d, const int32_t* idx_d, int B, float* grad_d, void* workspace_d,
                                size_t workspace_bytes, void* stream) {
  CACTO_REQUIRE(sys && cfg && storage_d && idx_d && grad_d && B > 0, "cacto_actor_grad: bad arguments");
  if (int e = check_nets(nets)) return e;
  CHECK_WS(workspace_d, workspace_bytes, B);
  const Workspace w = plan(sys, cfg->w_S != 0.0, B, static_cast<char*>(workspace_d));
  hipStream_t st = as_stream(stream);
  if (int e = launch_actor_chain(sys, nets, cfg, storage_d, idx_d, B, w, st)) return e;
  if (int e = launch_actor_wgrad(sys, w, st)) return e;
  return launch_reduce(w.slab_a, w.route.actor.nch, sys->actor.params, grad_d, st);
}

extern "C" int cacto_adam_step(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg, int which,
                               const float* grad_d, int soft_update, void* stream) {
  CACTO_REQUIRE(sys && cfg && grad_d && (which == CACTO_NET_ACTOR || which == CACTO_NET_CRITIC),
                "cacto_adam_step: bad arguments");
  if (int e = check_nets(nets)) return e;
  return launch_adam(sys, nets, cfg, which, grad_d, 1, soft_update, as_stream(stream));
}

extern "C" int cacto_soft_update(const cacto_sys* sys, const cacto_nets* nets, float tau, void* stream) {
  CACTO_REQUIRE(sys, "cacto_soft_update: bad arguments");
  if (int e = check_nets(nets)) return e;
  return launch_soft(sys, nets, tau, as_stream(stream));
}

extern "C" int cacto_update(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg,
                            const double* storage_d, const int32_t* idx_d, const float* is_w_d, int B, float* y_d,
                            float* V_d, float* Vt_d, void* workspace_d, size_t workspace_bytes, void* stream) {
  CACTO_REQUIRE(sys && cfg && storage_d && idx_d && B > 0, "cacto_update: bad arguments");
  if (int e = check_nets(nets)) return e;
  CHECK_WS(workspace_d, workspace_bytes, B);
  const Workspace w = plan(sys, cfg->w_S != 0.0, B, static_cast<char*>(workspace_d));
  hipStream_t st = as_stream(stream);
  if (int e = launch_critic_chain(sys, nets, cfg, storage_d, idx_d, is_w_d, B, y_d, V_d, Vt_d, w, st)) return e;
  if (int e = critic_step_tail(sys, nets, cfg, w, st, nullptr, nets->critic_d)) return e;
  if (int e = launch_actor_chain(sys, nets, cfg, storage_d, idx_d, B, w, st)) return e;
  return actor_step_tail(sys, nets, cfg, w, st);
}

extern "C" int cacto_update_pair_grads(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg,
                                       const double* storage_d, const int32_t* idx_c_d, const float* is_w_d,
                                       const int32_t* idx_a_d, int B, float* grad_d, float* y_d, float* V_d,
                                       void* workspace_d, size_t workspace_bytes, void* stream) {
  CACTO_REQUIRE(sys && cfg && storage_d && grad_d && B > 0 && (idx_c_d || idx_a_d),
                "cacto_update_pair_grads: bad arguments");
  if (int e = check_nets(nets)) return e;
  return pair_grads(sys, nets, cfg, storage_d, idx_c_d, is_w_d, idx_a_d, B, grad_d, y_d, V_d, workspace_d,
                    workspace_bytes, 1 | 2, as_stream(stream));
}

extern "C" int cacto_update_pair_grads_stage(const cacto_sys* sys, const cacto_nets* nets,
                                             const cacto_update_cfg* cfg, const double* storage_d,
                                             const int32_t* idx_c_d, const float* is_w_d, const int32_t* idx_a_d,
                                             int B, float* grad_d, float* y_d, float* V_d, void* workspace_d,
                                             size_t workspace_bytes, int stage, void* stream) {
  CACTO_REQUIRE(sys && cfg && storage_d && grad_d && B > 0 && (idx_c_d || idx_a_d) && (stage == 0 || stage == 1),
                "cacto_update_pair_grads_stage: bad arguments");
  if (int e = check_nets(nets)) return e;
  return pair_grads(sys, nets, cfg, storage_d, idx_c_d, is_w_d, idx_a_d, B, grad_d, y_d, V_d, workspace_d,
                    workspace_bytes, stage == 0 ? 1 : 2, as_stream(stream));
}

extern "C" int cacto_update_pair_apply(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg,
                                       const float* grad_d, int critic, int actor, int soft_update, void* stream) {
  CACTO_REQUIRE(sys && cfg && grad_d && (critic || actor), "cacto_update_pair_apply: bad arguments");
  if (int e = check_nets(nets)) return e;
  hipStream_t st = as_stream(stream);
  if (critic)
    if (int e = launch_adam(sys, nets, cfg, CACTO_NET_CRITIC, grad_d, 1, soft_update, st)) return e;
  if (actor)
    if (int e = launch_adam(sys, nets, cfg, CACTO_NET_ACTOR, grad_d + sys->critic.params, 1, 0, st)) return e;
  return CACTO_OK;
}

// K consecutive updates (learn_and_update's loop with its minibatches drawn up front, RL.py:120-143)
// as a two-stream pipeline. The critic step of update t+1 reads only the critic, the target and the
// rows — never the actor — so it runs while the actor step of update t is still going:
//   stream : critic chain(t) on C_t, wgrad, Adam(t): C_t -> C_{t+1} (+ soft target update)
//   side   : [wait Adam(t)], actor chain(t) against C_{t+1}, wgrad, Adam(actor), [event]
// The critic rotates over the caller's net buffer and two workspace copies (C_t in buffer t % 3),
// so Adam(t) overwrites the buffer actor chain(t-3) read (and, with PER, the sampler of update t
// the index buffer it read) — the only ordering the stream needs from the side stream: the event
// of side iteration t-3, recorded after that iteration's Adam, normally long signalled. (With two
// buffers the event had to follow the actor chain itself, and its record packet cost the side
// stream — the critical one — a queue gap between the chain and its GEMM.) Every kernel sees the
// same inputs as in K sequential cacto_update calls, so the results are bit-identical; the final
// critic is copied back if it ended in a workspace buffer, and the side stream joins the caller's
// stream before returning.
namespace {
// PER state of cacto_update_n_per (replay_buffer.py:139-218)
struct PerArgs {
  double *sum_tree, *min_tree;
  int64_t cap, max_idx;
  double beta, fresh, eps, alpha;
  const double* uniforms;  // [K][B]
  double *exp_counter, *max_priority;
};

// Whether the PER loop of this batch takes the overlapped form — the priority update and the next
// sample inside the critic GEMM's and Adam's launches (k_wgrad_big_per, k_adam_sample) instead of
// following them: the PER route's half (the count deferred, 256-leaf subtrees whose roots fit one
// workgroup), a priority update at all (alpha != 0), and the update route's half (the large-batch
// critic GEMM and an Adam step with all chunks in flight).
bool per_overlap_ok(const PerArgs* per, int B, const Workspace& w) {
  return per && per_route(per->cap, B).overlap_shape && per->alpha != 0.0 && w.route.per_overlap;
}

// The priority update of one PER step (RL.py:129-131). late_count: the sampler left its
// exp_counter += 1 to this call (large batches), which applies it first, in the same launch. With
// alpha == 0 the reference skips update_priorities (RL.py:130) — the count still happens.
int per_priority_update(const PerArgs* per, const int32_t* idx, const float* y, const float* V, int B, bool late_count,
                        hipStream_t st) {
  if (per->alpha == 0.0) return late_count ? cacto_per_count_launch(idx, B, per->exp_counter, st) : CACTO_OK;
  if (late_count)
    return cacto_per_update_count(per->sum_tree, per->min_tree, per->cap, idx, y, V, per->exp_counter, per->fresh,
                                  per->eps, per->alpha, per->max_priority, B, st);
  return cacto_per_update(per->sum_tree, per->min_tree, per->cap, idx, y, V, per->exp_counter, per->fresh, per->eps,
                          per->alpha, per->max_priority, B, st);
}

// Small batches (route.paired): one stream, K + 1 steps. Step t runs the critic chain of update t
// and the actor chain of update t - 1 as one grid (k_chain_pair), then both GEMM + Adam steps as
// one k_wgrad_adam launch:
//   critic(t) reads C_t, T_t (Adam of step t - 1 wrote them); actor(t-1) reads A_{t-1} and C_t —
//   exactly what RL.py:104-109 gives it (the critic after its own update t - 1);
//   Adam: C_t -> C_{t+1} (+ soft T), A_{t-1} -> A_t.
// Every kernel sees the inputs of the sequential loop, so results are bit-identical, with no
// cross-stream events and three launches per update (five with PER).
int update_pipeline_pair(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg,
                         const double* storage_d, const int32_t* idx_d, const PerArgs* per, int K, int B,
                         const Workspace& w, hipStream_t st) {
  float* const y = w.scal;
  float* const V = w.scal + w.Bp;
  const int soft = cfg->MC ? 0 : 1;
  const ChainScalars cs = chain_scalars(cfg, w.route, B);
  const NetView C = cacto_make_view(sys, CACTO_NET_CRITIC, nets->critic_d);
  const NetView Tg = cacto_make_view(sys, CACTO_NET_CRITIC, nets->target_d);
  const NetView Ac = cacto_make_view(sys, CACTO_NET_ACTOR, nets->actor_d);
  const AdamNet cn = critic_adam_net(sys, nets, cfg, w, soft, nullptr, nets->critic_d);
  const AdamNet an = actor_adam_net(sys, nets, cfg, w);
  const bool late_count = per && per_route(per->cap, B).count_deferred;  // the count moves to the priority update
  const int32_t* idx_prev = nullptr;
  for (int t = 0; t <= K; ++t) {
    const int32_t* idx = nullptr;
    const float* isw = nullptr;
    if (t < K) {
      idx = idx_d ? idx_d + (size_t)t * B : nullptr;
      if (per) {
        int32_t* pi = w.pidx + (size_t)(t & 1) * w.Bp;
        if (int e = cacto_per_sample(per->sum_tree, per->min_tree, per->cap, per->max_idx, per->beta,
                                     per->uniforms + (size_t)t * B, B, pi, w.pisw, late_count ? nullptr : per->exp_counter, st))
          return e;
        idx = pi;
        isw = w.pisw;
      }
    }
    if (t < K && t > 0) {
      if (int e = launch_chain_pair(sys, C, Tg, Ac, cs, storage_d, idx, isw, idx_prev, B, w, y, V, nets->step_d, st))
        return e;
      if (int e = launch_wgrad_adam(sys, 2, cn, &an, nets->step_d, st)) return e;
    } else if (t < K) {
      if (int e = launch_critic_chain(sys, nets, cfg, storage_d, idx, isw, B, y, V, nullptr, w, st)) return e;
      if (int e = launch_wgrad_adam(sys, 0, cn, nullptr, nets->step_d, st)) return e;
    } else {
      if (int e = launch_actor_chain(sys, nets, cfg, storage_d, idx_prev, B, w, st)) return e;
      if (int e = launch_wgrad_adam(sys, 1, an, nullptr, nets->step_d, st)) return e;
    }
    if (per && t < K)
      if (int e = per_priority_update(per, idx, y, V, B, late_count, st)) return e;
    idx_prev = idx;
  }
  return CACTO_OK;
}

// The side stream and its events, created once per handle and published only when all exist.
int ensure_side_stream(cacto_sys* ms) {
  if (ms->side) return CACTO_OK;
  hipStream_t side = nullptr;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  hipError_t e = hipStreamCreateWithFlags(&side, hipStreamNonBlocking);
  // device-scope events: every producer and consumer of these dependencies is a kernel on this device
  const unsigned evf = hipEventDisableTiming | hipEventDisableSystemFence;
  for (int k = 0; k < 4 && e == hipSuccess; ++k) e = hipEventCreateWithFlags(&ev[k], evf);
  unsigned long long* sig = nullptr;
  if (e == hipSuccess) e = hipMalloc(&sig, 8 * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMemset(sig, 0, 8 * sizeof(unsigned long long));
  if (e != hipSuccess) {
    if (sig) (void)hipFree(sig);
    for (hipEvent_t x : ev)
      if (x) (void)hipEventDestroy(x);
    if (side) (void)hipStreamDestroy(side);
    return hip_fail(e, "cacto_update_n: side stream / events / pipeline signal");
  }
  ms->pipe_sig = sig;
  ms->pipe_seq = 0;
  ms->ev_critic = ev[0];
  ms->ev_actor[0] = ev[1];
  ms->ev_actor[1] = ev[2];
  ms->ev_actor[2] = ev[3];
  ms->side = side;
  return CACTO_OK;
}

// How the two streams of this call are ordered: true = device-side waits (the default), false = queue
// markers (event record / wait). CACTO_PIPE_DEVWAIT=0 / 1 forces markers / device waits (read once;
// A/B and the timeout test). Otherwise markers when kernels are serialized by the environment
// (AMD_SERIALIZE_KERNEL, HIP_LAUNCH_BLOCKING) or when the handle's one-time concurrency probe failed
// (k_pipe_probe; e.g. counter collection). Always markers while `st` is being captured into a graph:
// the waits compare device counters with absolute targets baked into the launches, and a replayed
// graph would find its targets already reached.
int pipe_devwait(cacto_sys* ms, hipStream_t st, bool* out) {
  static const int env = [] {
    const char* e = std::getenv("CACTO_PIPE_DEVWAIT");
    if (e) return std::atoi(e) != 0 ? 1 : 0;
    const char* s1 = std::getenv("AMD_SERIALIZE_KERNEL");
    const char* s2 = std::getenv("HIP_LAUNCH_BLOCKING");
    if ((s1 && std::atoi(s1) != 0) || (s2 && std::atoi(s2) != 0)) return 0;
    return -1;  // probe
  }();
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  CACTO_CHECK_HIP(hipStreamIsCapturing(st, &cap));
  if (cap != hipStreamCaptureStatusNone) {
    *out = false;
    return CACTO_OK;
  }
  if (env >= 0) {
    *out = env == 1;
    return CACTO_OK;
  }
  if (ms->pipe_probe < 0) {
    // both probe kernels start after everything already queued on `st`; the side one first
    unsigned long long* w = ms->pipe_sig;
    CACTO_CHECK_HIP(hipMemsetAsync(w + 4, 0, 4 * sizeof(unsigned long long), st));
    CACTO_CHECK_HIP(hipEventRecord(ms->ev_critic, st));
    CACTO_CHECK_HIP(hipStreamWaitEvent(ms->side, ms->ev_critic, 0));
    if (int e = launch_pipe_probe(w, 0, ms->side)) return e;
    if (int e = launch_pipe_probe(w, 1, st)) return e;
    CACTO_CHECK_HIP(hipStreamSynchronize(ms->side));
    CACTO_CHECK_HIP(hipStreamSynchronize(st));
    unsigned long long ok[2] = {0, 0};
    CACTO_CHECK_HIP(hipMemcpy(ok, w + 6, sizeof(ok), hipMemcpyDeviceToHost));
    ms->pipe_probe = ok[0] && ok[1] ? 1 : 0;
  }
  *out = ms->pipe_probe == 1;
  return CACTO_OK;
}

// The frame of both two-stream pipelines (pipe_mu held, the side stream created): two shadow copies of
// the critic, the side stream forked off `st`, body(&cbuf), the side stream joined. cbuf: the buffer
// (0 caller's, 1-2 workspace) holding the newest critic; on every exit of the body, error or not, the
// side stream joins the caller's stream and the newest critic lands in the caller's buffer.
template <class Body>
int pipeline_frame(cacto_sys* ms, const cacto_nets* nets, const Workspace& w, hipStream_t st, bool devwait,
                   Body&& body) {
  const size_t nb_bytes = critic_buf_bytes(ms->critic), nb_stride = critic_buf_stride(ms->critic);
  CACTO_CHECK_HIP(hipMemcpyAsync(w.cshadow, nets->critic_d, nb_bytes, hipMemcpyDeviceToDevice, st));
  CACTO_CHECK_HIP(hipMemcpyAsync(w.cshadow + nb_stride, nets->critic_d, nb_bytes, hipMemcpyDeviceToDevice, st));
  CACTO_CHECK_HIP(hipEventRecord(ms->ev_critic, st));  // everything the caller queued before
  CACTO_CHECK_HIP(hipStreamWaitEvent(ms->side, ms->ev_critic, 0));
  int cbuf = 0;
  const int err = body(&cbuf);
  CACTO_CHECK_HIP(hipEventRecord(ms->ev_critic, ms->side));
  CACTO_CHECK_HIP(hipStreamWaitEvent(st, ms->ev_critic, 0));
  // the timeout latch's host copy, read by cacto_pipeline_check after a synchronisation of `st`
  if (devwait)
    CACTO_CHECK_HIP(hipMemcpyAsync(ms->latch_host, ms->pipe_sig + 1, sizeof(unsigned long long),
                                   hipMemcpyDeviceToHost, st));
  if (cbuf)
    CACTO_CHECK_HIP(hipMemcpyAsync(nets->critic_d, w.cshadow + (cbuf - 1) * nb_stride, nb_bytes,
                                   hipMemcpyDeviceToDevice, st));
  return err;
}

// Queue markers (no device-side waits): actor chain(t-3) read the critic buffer Adam(t) writes and
// (PER) the index buffer of update t, so the critic stream waits at the top of iteration t for side
// iteration t-3, recorded at its end. every2 (PER): the side stream records only at even iterations
// and the critic waits at even t for side iteration t-2 (which covers t-3 here and at t+1) — half the
// markers on each stream (car_park B = 4096: 9.04 k -> 9.36 k updates/s); every iteration without
// PER (manipulator B = 8192 lost 8 % to the tighter wait).
int marker_wait(cacto_sys* ms, hipStream_t st, bool every2, int t) {
  if (every2) {
    if (t >= 2 && (t & 1) == 0) CACTO_CHECK_HIP(hipStreamWaitEvent(st, ms->ev_actor[((t - 2) >> 1) & 1], 0));
  } else if (t >= 3) {
    CACTO_CHECK_HIP(hipStreamWaitEvent(st, ms->ev_actor[t % 3], 0));
  }
  return CACTO_OK;
}
int marker_record(cacto_sys* ms, bool every2, int t) {
  if (!every2) {
    CACTO_CHECK_HIP(hipEventRecord(ms->ev_actor[t % 3], ms->side));
  } else if ((t & 1) == 0) {
    CACTO_CHECK_HIP(hipEventRecord(ms->ev_actor[(t >> 1) & 1], ms->side));
  }
  return CACTO_OK;
}

// The overlapped PER form (per_overlap_ok): the first sample, recording its per-subtree runs; later
// ones run inside the Adam launch. shards: the ranks' statistics table (data parallel, filled by
// gather() between the memsets and the sample), else nullptr.
template <class Gather>
int per_first_sample(const PerArgs* per, int B, int32_t* pi, const Workspace& w, hipStream_t st, const double* shards,
                     int world, Gather&& gather) {
  const int nroot = (int)(per->cap / PER_RUN_SUB);
  CACTO_CHECK_HIP(hipMemsetAsync(w.runs, 0x7f, (size_t)nroot * sizeof(int32_t), st));
  CACTO_CHECK_HIP(hipMemsetAsync(w.runs + nroot, 0, (size_t)nroot * sizeof(int32_t), st));
  if (int e = gather()) return e;
  return cacto_per_sample_runs(per->sum_tree, per->min_tree, per->cap, per->max_idx, per->beta, per->uniforms, B, pi,
                               w.pisw, nullptr, w.runs, shards, shards ? world : 0, st);
}
// ... and what the critic GEMM's and Adam's launches of update t carry: the priority update of t (idx:
// its rows; stats: where a data-parallel rank leaves its shard's statistics) and the sample of t + 1
PerRunArgs per_run_args(const PerArgs* per, const int32_t* idx, const Workspace& w, double* stats = nullptr,
                        int stats_off = 0, int stats_words = 3) {
  return PerRunArgs{per->sum_tree, per->min_tree, per->cap, idx, w.scal, w.scal + w.Bp, per->exp_counter,
                    per->max_idx, per->fresh, per->eps, per->alpha, per->max_priority, w.runs, stats, stats_off,
                    stats_words};
}
PerSampleArgs per_sample_args(const PerArgs* per, int t, int B, int nring, const Workspace& w,
                              const double* shards = nullptr, int world = 0) {
  return PerSampleArgs{per->sum_tree, per->min_tree, per->cap, per->max_idx, per->beta,
                       per->uniforms + (size_t)(t + 1) * B, B, w.pidx + (size_t)((t + 1) % nring) * w.Bp,
                       w.pisw, shards, world, w.runs};
}

int update_pipeline_body(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg,
                         const double* storage_d, const int32_t* idx_d, const PerArgs* per, int K, int B,
                         const Workspace& w, hipStream_t st, int* cbuf, bool devwait) {
  cacto_sys* ms = const_cast<cacto_sys*>(sys);
  hipStream_t side = ms->side;
  float* const buf[3] = {nets->critic_d, w.cshadow, w.cshadow + critic_buf_stride(sys->critic)};
  float* const y = w.scal;
  float* const V = w.scal + w.Bp;
  const bool late_count = per && per_route(per->cap, B).count_deferred;  // the count moves to the priority update
  const bool every2 = per != nullptr;  // queue markers (devwait off): marker_wait
  // devwait: the critic stream's ordering against the side stream without queue markers — the
  // actor's GEMM (the launch after each actor chain) publishes the count of finished actor chains on
  // the device, and the critic's Adam(t) polls it (pipe_wait) before overwriting the buffer actor
  // chain(t-3) read; the PER index ring has four buffers, so the sampler of update t overwrites the
  // one actor chain(t-4) read, which Adam(t-1)'s wait covers. Measured r05 (1 MI355X, updates/s): DI
  // B = 4096 12.3 k -> 12.7 k, car_park PER B = 4096 9.88 k -> 9.98 k, manipulator B = 8192 unchanged.
  // ... and the side stream's wait on the critic's Adam too (devwait_actor): the critic's Adam writes
  // the weights through to memory at agent scope and publishes after its stores completed, the actor
  // chain polls relaxed just before its critic pass at s' (with PER at its start, before it gathers
  // the sampled rows) — where that cannot starve the critic stream of CUs: 16-sample actor tiles (the
  // q4 chains take no wait), at most one actor workgroup per CU (a CU holding one actor workgroup
  // still fits a critic chain, GEMM or Adam workgroup beside it, so the critic stream always
  // progresses). DI B = 4096 13.2-13.3 k -> 14.2-14.4 k updates/s (r05).
  const bool devwait_actor = devwait && w.route.devwait_actor;
  const int thru = devwait_actor ? 1 : 0;
  unsigned long long* const sig = ms->pipe_sig;
  // the overlapped PER form (per_overlap_ok): priority update t inside the critic GEMM's launch,
  // sample t + 1 inside its Adam's; the index ring has five buffers (sample t + 1 runs in the launch
  // after the Adam(t - 1) that waited for actor chain t - 4). Otherwise the sample and the priority
  // update run on the critic stream between its launches.
  const bool ovl = devwait && per_overlap_ok(per, B, w);
  const int nring = ovl ? 5 : devwait ? 4 : 3;
  const unsigned long long base = ms->pipe_seq;
  ms->pipe_seq = base + K;  // reserved up front: no later call's waits can be satisfied by this call's values
  // test hook (tests/test_gpu_per_pipeline.py): CACTO_PIPE_FAULT_INJECT=1 gives the first device-side
  // wait of the process an unreachable target, so it times out and latches (once per process)
  static std::atomic<int> inject{[] {
    const char* e = std::getenv("CACTO_PIPE_FAULT_INJECT");
    return e && e[0] == '1' ? 1 : 0;
  }()};
  for (int t = 0; t < K; ++t) {
    if (!devwait)
      if (int e = marker_wait(ms, st, every2, t)) return e;
    const int32_t* idx = idx_d + (size_t)t * B;
    const float* isw = nullptr;
    if (per) {
      int32_t* pi = w.pidx + (size_t)(t % nring) * w.Bp;
      if (ovl) {
        if (t == 0)
          if (int e = per_first_sample(per, B, pi, w, st, nullptr, 0, [] { return (int)CACTO_OK; })) return e;
      } else if (int e = cacto_per_sample(per->sum_tree, per->min_tree, per->cap, per->max_idx, per->beta,
                                          per->uniforms + (size_t)t * B, B, pi, w.pisw,
                                          late_count ? nullptr : per->exp_counter, st)) {
        return e;
      }
      idx = pi;
      isw = w.pisw;
    }
    cacto_nets cur = *nets, nxt = *nets;
    cur.critic_d = buf[t % 3];
    nxt.critic_d = buf[(t + 1) % 3];
    if (int e = launch_critic_chain(sys, &cur, cfg, storage_d, idx, isw, B, y, V, nullptr, w, st)) return e;
    const bool dw = devwait && t >= 3;
    const unsigned long long wait_c = dw && inject.exchange(0) ? ~0ull : base + t - 2;
    PerRunArgs pra{};
    PerSampleArgs psa{};
    if (ovl) {
      pra = per_run_args(per, idx, w);
      if (t + 1 < K) psa = per_sample_args(per, t, B, nring, w);
    }
    if (int e = critic_step_tail(sys, nets, cfg, w, st, cur.critic_d, nxt.critic_d, dw ? sig : nullptr, wait_c,
                                 devwait_actor ? sig : nullptr, base + t + 1, ovl ? &pra : nullptr,
                                 ovl && t + 1 < K ? &psa : nullptr, thru))
      return e;
    *cbuf = (t + 1) % 3;
    if (!devwait_actor) CACTO_CHECK_HIP(hipEventRecord(ms->ev_critic, st));
    if (per && !ovl)
      if (int e = per_priority_update(per, idx, y, V, B, late_count, st)) return e;
    if (!devwait_actor) CACTO_CHECK_HIP(hipStreamWaitEvent(side, ms->ev_critic, 0));
    if (int e = launch_actor_chain(sys, &nxt, cfg, storage_d, idx, B, w, side, devwait_actor ? sig + 2 : nullptr,
                                   base + t + 1, per ? 1 : 0))
      return e;
    if (int e = actor_step_tail(sys, nets, cfg, w, side, devwait ? sig : nullptr, base + t + 1)) return e;
    if (!devwait)
      if (int e = marker_record(ms, every2, t)) return e;
  }
  return CACTO_OK;
}

int update_pipeline(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg, const double* storage_d,
                    const int32_t* idx_d, const PerArgs* per, int K, int B, const Workspace& w, hipStream_t st) {
  cacto_sys* ms = const_cast<cacto_sys*>(sys);
  std::lock_guard<std::mutex> lock(ms->pipe_mu);
  if (int e = ensure_side_stream(ms)) return e;
  if (!ms->latch_host) {
    CACTO_CHECK_HIP(hipHostMalloc(reinterpret_cast<void**>(&ms->latch_host), sizeof(unsigned long long),
                                  hipHostMallocDefault));
    *ms->latch_host = 0;
  }
  // a device-side wait of an earlier call timed out and nobody has collected it with
  // cacto_pipeline_check (the Python layer does at the end of every learn_and_update and before
  // every checkpoint save): refuse to build on results whose order cannot be trusted
  CACTO_REQUIRE(!*reinterpret_cast<volatile unsigned long long*>(ms->latch_host),
                "cacto_update_n: a device-side pipeline wait of an earlier call timed out (kernels serialized?); its "
                "results are not trustworthy — collect it with cacto_pipeline_check, or run with CACTO_PIPE_DEVWAIT=0");
  bool devwait = false;
  if (int e = pipe_devwait(ms, st, &devwait)) return e;
  return pipeline_frame(ms, nets, w, st, devwait, [&](int* cbuf) {
    return update_pipeline_body(sys, nets, cfg, storage_d, idx_d, per, K, B, w, st, cbuf, devwait);
  });
}

// ---------------------------------------------------------------- data-parallel pipeline (RCCL)
// The data-parallel learn_and_update (main.py:219-225 runs the reference's loop on one process; here
// one process per GPU, the gradients all-reduced over xGMI). The K updates of a call run as the
// two-stream pipeline of cacto_update_n with each network's exchange inside its own stream:
//   stream : [PER: shard stats -> all-gather -> stratified sample over the union] critic chain(t) ->
//            weight-gradient GEMM -> slab reduce -> all-reduce (comm 0) -> Adam(t) (+ soft target
//            update) [-> PER priority update]
//   side   : [marker: Adam(t)] actor chain(t) against C_{t+1} -> GEMM -> reduce -> all-reduce (comm 1)
//            -> Adam
// Every rank issues the same collectives in the same order on each communicator, one communicator
// per stream, so neither stream's collectives can interleave with the other's. The streams are
// ordered with queue markers (no device-side polls beside collectives that wait for other ranks).
// The gradients are scaled by 1/B_global inside the chain kernels, so the exchange is a plain sum;
// every rank applies the same Adam to the same sum, so the replicas stay bit-identical. With one
// rank the all-reduce is the identity and the result equals cacto_update_n / the Python
// dp_pipeline bit for bit (tests/test_gpu_dp.py). The host issues ~14 HIP / RCCL calls per update
// (the Python loop of RL_AC issued ~10 ctypes calls and two torch.distributed collectives: ~160 us
// of host time per update, more than the GPU's).
// RCCL entry points of the copy already in the process (torch.distributed's, found by soname), else
// the ROCm library: no link-time dependency, one RCCL instance per process.
struct Rccl {
  decltype(&ncclGetUniqueId) get_id = nullptr;
  decltype(&ncclCommInitRank) init = nullptr;
  decltype(&ncclCommDestroy) destroy = nullptr;
  decltype(&ncclAllReduce) all_reduce = nullptr;
  decltype(&ncclAllGather) all_gather = nullptr;
  decltype(&ncclGetErrorString) err = nullptr;
  bool ok = false;
};
const Rccl& rccl() {
  static const Rccl r = [] {
    Rccl x;
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW);
    if (!h) return x;
    x.get_id = reinterpret_cast<decltype(x.get_id)>(dlsym(h, "ncclGetUniqueId"));
    x.init = reinterpret_cast<decltype(x.init)>(dlsym(h, "ncclCommInitRank"));
    x.destroy = reinterpret_cast<decltype(x.destroy)>(dlsym(h, "ncclCommDestroy"));
    x.all_reduce = reinterpret_cast<decltype(x.all_reduce)>(dlsym(h, "ncclAllReduce"));
    x.all_gather = reinterpret_cast<decltype(x.all_gather)>(dlsym(h, "ncclAllGather"));
    x.err = reinterpret_cast<decltype(x.err)>(dlsym(h, "ncclGetErrorString"));
    x.ok = x.get_id && x.init && x.destroy && x.all_reduce && x.all_gather && x.err;
    return x;
  }();
  return r;
}

int rccl_fail(ncclResult_t r, const char* what) {
  set_error(std::string(what) + ": " + (rccl().err ? rccl().err(r) : "RCCL error"));
  return CACTO_EHIP;
}
#define CACTO_CHECK_RCCL(call, what)            \
  do {                                          \
    const ncclResult_t r_ = (call);             \
    if (r_ != ncclSuccess) return rccl_fail(r_, what); \
  } while (0)

int update_pipeline_dp_body(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg,
                            const double* storage_d, const int32_t* idx_d, const PerArgs* per, int K, int B,
                            const Workspace& w, hipStream_t st, int* cbuf) {
  cacto_sys* ms = const_cast<cacto_sys*>(sys);
  const Rccl& R = rccl();
  ncclComm_t cc = static_cast<ncclComm_t>(ms->dp_comm[0]), ca = static_cast<ncclComm_t>(ms->dp_comm[1]);
  hipStream_t side = ms->side;
  const int Pc = sys->critic.params, Pa = sys->actor.params;
  float* const buf[3] = {nets->critic_d, w.cshadow, w.cshadow + critic_buf_stride(sys->critic)};
  float* const y = w.scal;
  float* const V = w.scal + w.Bp;
  const int soft = cfg->MC ? 0 : 1;
  const bool every2 = per != nullptr;  // queue markers: marker_wait
  // PER in the critic's GEMM and Adam launches (per_overlap_ok, as cacto_update_n_per): the priority
  // update of update t inside the GEMM's launch, then this shard's statistics and their all-gather,
  // and the sample of t + 1 (IS weights over the union) inside the Adam's launch; the index ring has
  // five buffers (sample t + 1 overwrites the one actor chain t - 4 read, which the marker before
  // update t - 1 or t covers). Otherwise the sample and the priority update run between the launches.
  const bool ovl = per_overlap_ok(per, B, w);
  const int nring = ovl ? 5 : 3;
  const int nroot = per ? (int)(per->cap / PER_RUN_SUB) : 0;
  double* const stats = ms->dp_stats;       // [3] this shard
  double* const shards = ms->dp_stats + 3;  // [world][3]
  auto gather_stats = [&]() -> int {
    if (int e = cacto_per_shard_stats(per->sum_tree, per->min_tree, per->max_idx, stats, st)) return e;
    CACTO_CHECK_RCCL(R.all_gather(stats, shards, 3, ncclFloat64, cc, st), "ncclAllGather(PER shards)");
    return CACTO_OK;
  };
  for (int t = 0; t < K; ++t) {
    if (int e = marker_wait(ms, st, every2, t)) return e;
    const int32_t* idx = idx_d + (size_t)t * B;
    const float* isw = nullptr;
    if (per) {
      // replay_buffer.py:139-188 over the union of the ranks' shards: this shard's (sum, min, rows),
      // all-gathered, then the stratified sample with IS weights against the union
      int32_t* pi = w.pidx + (size_t)(t % nring) * w.Bp;
      if (ovl) {
        if (t == 0)
          if (int e = per_first_sample(per, B, pi, w, st, shards, ms->dp_world, gather_stats)) return e;
      } else {
        if (int e = gather_stats()) return e;
        if (int e = cacto_per_sample_global(per->sum_tree, per->min_tree, per->cap, per->max_idx, per->beta,
                                            per->uniforms + (size_t)t * B, B, shards, ms->dp_world, pi, w.pisw,
                                            per->exp_counter, st))
          return e;
      }
      idx = pi;
      isw = w.pisw;
    }
    cacto_nets cur = *nets, nxt = *nets;
    cur.critic_d = buf[t % 3];
    nxt.critic_d = buf[(t + 1) % 3];
    if (int e = launch_critic_chain(sys, &cur, cfg, storage_d, idx, isw, B, y, V, nullptr, w, st)) return e;
    PerRunArgs pra{};
    PerSampleArgs psa{};
    if (ovl) {
      // the trees after priority update t: the statistics sample t + 1 weighs against, written by the
      // workgroup of the GEMM's launch that rebuilds the top of the trees (with one subtree, a launch)
      pra = per_run_args(per, idx, w, t + 1 < K && nroot > 1 ? shards : nullptr, 3 * ms->dp_rank, 3 * ms->dp_world);
      if (t + 1 < K) psa = per_sample_args(per, t, B, nring, w, shards, ms->dp_world);
    }
    if (int e = launch_critic_wgrad(sys, w, st, ovl ? &pra : nullptr)) return e;
    if (ovl && t + 1 < K) {
      if (nroot > 1)  // the table with this rank's words filled and the others zero: summed = gathered
        CACTO_CHECK_RCCL(R.all_reduce(shards, shards, (size_t)3 * ms->dp_world, ncclFloat64, ncclSum, cc, st),
                         "ncclAllReduce(PER shards)");
      else if (int e = gather_stats())
        return e;
    }
    if (int e = launch_reduce(w.slab, w.route.critic.nch, Pc, ms->dp_gc, st)) return e;
    CACTO_CHECK_RCCL(R.all_reduce(ms->dp_gc, ms->dp_gc, (size_t)Pc, ncclFloat32, ncclSum, cc, st),
                     "ncclAllReduce(critic gradient)");
    cacto_nets dst = *nets;
    dst.critic_d = nxt.critic_d;
    if (int e = launch_adam(sys, &dst, cfg, CACTO_NET_CRITIC, ms->dp_gc, 1, soft, st, cur.critic_d, nullptr, 0, nullptr,
                            0, ovl && t + 1 < K ? &psa : nullptr))
      return e;
    *cbuf = (t + 1) % 3;
    CACTO_CHECK_HIP(hipEventRecord(ms->ev_critic, st));
    if (per && !ovl)
      if (int e = per_priority_update(per, idx, y, V, B, false, st)) return e;
    CACTO_CHECK_HIP(hipStreamWaitEvent(side, ms->ev_critic, 0));
    if (int e = launch_actor_chain(sys, &nxt, cfg, storage_d, idx, B, w, side)) return e;
    if (int e = launch_actor_wgrad(sys, w, side)) return e;
    if (int e = launch_reduce(w.slab_a, w.route.actor.nch, Pa, ms->dp_ga, side)) return e;
    CACTO_CHECK_RCCL(R.all_reduce(ms->dp_ga, ms->dp_ga, (size_t)Pa, ncclFloat32, ncclSum, ca, side),
                     "ncclAllReduce(actor gradient)");
    if (int e = launch_adam(sys, nets, cfg, CACTO_NET_ACTOR, ms->dp_ga, 1, 0, side)) return e;
    if (int e = marker_record(ms, every2, t)) return e;
  }
  return CACTO_OK;
}

int update_pipeline_dp(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg,
                       const double* storage_d, const int32_t* idx_d, const PerArgs* per, int K, int B,
                       const Workspace& w, hipStream_t st) {
  cacto_sys* ms = const_cast<cacto_sys*>(sys);
  std::lock_guard<std::mutex> lock(ms->pipe_mu);
  CACTO_REQUIRE(ms->dp_comm[0] && ms->dp_comm[1],
                "cacto_update_n_dp: no RCCL communicators on this handle (cacto_dp_attach)");
  if (int e = ensure_side_stream(ms)) return e;
  return pipeline_frame(ms, nets, w, st, false, [&](int* cbuf) {
    return update_pipeline_dp_body(sys, nets, cfg, storage_d, idx_d, per, K, B, w, st, cbuf);
  });
}

// The four cacto_update_n* entry points (per: PER sampling, else the minibatches of idx_d).
int update_n(const char* name, bool dp, const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg,
             const double* storage_d, const int32_t* idx_d, const PerArgs* per, int K, int B, void* workspace_d,
             size_t workspace_bytes, void* stream) {
  const bool src = per ? per->sum_tree && per->min_tree && per->uniforms && per->exp_counter && per->max_priority
                       : idx_d != nullptr;
  CACTO_REQUIRE(sys && cfg && storage_d && src && B > 0 && K >= 0, std::string(name) + ": bad arguments");
  if (int e = check_nets(nets)) return e;
  CHECK_WS(workspace_d, workspace_bytes, B);
  if (K == 0) return CACTO_OK;
  const Workspace w = plan(sys, cfg->w_S != 0.0, B, static_cast<char*>(workspace_d));
  hipStream_t st = as_stream(stream);
  if (dp) return update_pipeline_dp(sys, nets, cfg, storage_d, idx_d, per, K, B, w, st);
  // small batches: the paired single-stream schedule with the sampling and priority update between
  // steps (car_park B = 64 with the q4 chains: 21.1 k vs 19.8 k updates/s two-stream); larger
  // batches keep the two-stream pipeline (the actor step beside the sampling / priority update)
  if (w.route.paired) return update_pipeline_pair(sys, nets, cfg, storage_d, idx_d, per, K, B, w, st);
  return update_pipeline(sys, nets, cfg, storage_d, idx_d, per, K, B, w, st);
}
}  // namespace

extern "C" int cacto_pipeline_status(const cacto_sys* sys, unsigned long long* out4_h) {
  CACTO_REQUIRE(sys && out4_h, "cacto_pipeline_status: bad arguments");
  for (int k = 0; k < 4; ++k) out4_h[k] = 0;
  if (!sys->pipe_sig) return CACTO_OK;
  CACTO_CHECK_HIP(hipDeviceSynchronize());
  CACTO_CHECK_HIP(hipMemcpy(out4_h, sys->pipe_sig, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  out4_h[3] = sys->pipe_probe < 0 ? 0 : (unsigned long long)sys->pipe_probe + 1;
  return CACTO_OK;
}

extern "C" int cacto_pipeline_check(cacto_sys* sys, void* stream) {
  CACTO_REQUIRE(sys, "cacto_pipeline_check: bad arguments");
  if (!sys->pipe_sig || !sys->latch_host) return CACTO_OK;
  std::lock_guard<std::mutex> lock(sys->pipe_mu);
  CACTO_CHECK_HIP(hipStreamSynchronize(as_stream(stream)));
  volatile unsigned long long* lh = reinterpret_cast<volatile unsigned long long*>(sys->latch_host);
  if (*lh == 0) return CACTO_OK;
  // collected: clear both copies, so the handle's next calls run again
  CACTO_CHECK_HIP(hipMemset(sys->pipe_sig + 1, 0, sizeof(unsigned long long)));
  *lh = 0;
  set_error("cacto_pipeline_check: a device-side wait of the two-stream update pipeline timed out since the last "
            "check (kernels serialized?); the updates of that call ran without their cross-stream order and their "
            "results are not trustworthy — rerun them with CACTO_PIPE_DEVWAIT=0");
  return CACTO_EINVAL;
}

void cacto_dp_release(cacto_sys* sys) {
  for (void*& c : sys->dp_comm) {
    if (c && rccl().ok) (void)rccl().destroy(static_cast<ncclComm_t>(c));
    c = nullptr;
  }
  if (sys->dp_gc) (void)hipFree(sys->dp_gc);
  if (sys->dp_ga) (void)hipFree(sys->dp_ga);
  if (sys->dp_stats) (void)hipFree(sys->dp_stats);
  sys->dp_gc = sys->dp_ga = nullptr;
  sys->dp_stats = nullptr;
  sys->dp_rank = sys->dp_world = 0;
}

extern "C" int cacto_dp_unique_ids(void* out_h, int n) {
  CACTO_REQUIRE(out_h && n >= 1 && n <= 16, "cacto_dp_unique_ids: bad arguments");
  const Rccl& R = rccl();
  CACTO_REQUIRE(R.ok, "cacto_dp_unique_ids: RCCL (librccl.so.1) not found");
  for (int k = 0; k < n; ++k) {
    ncclUniqueId id;
    CACTO_CHECK_RCCL(R.get_id(&id), "ncclGetUniqueId");
    std::memcpy(static_cast<char*>(out_h) + (size_t)k * sizeof(ncclUniqueId), &id, sizeof(ncclUniqueId));
  }
  return CACTO_OK;
}

extern "C" int cacto_dp_attach(cacto_sys* sys, const void* ids_h, int rank, int world) {
  CACTO_REQUIRE(sys && ids_h && world >= 1 && rank >= 0 && rank < world, "cacto_dp_attach: bad arguments");
  const Rccl& R = rccl();
  CACTO_REQUIRE(R.ok, "cacto_dp_attach: RCCL (librccl.so.1) not found");
  std::lock_guard<std::mutex> lock(sys->pipe_mu);
  // the side stream may still run collectives on the communicators about to go (as cacto_dp_detach)
  if (sys->side) CACTO_CHECK_HIP(hipStreamSynchronize(sys->side));
  cacto_dp_release(sys);
  // all or nothing: a failure below releases what was set, so the handle is never left half attached
  const int err = [&]() -> int {
    for (int k = 0; k < 2; ++k) {
      ncclUniqueId id;
      std::memcpy(&id, static_cast<const char*>(ids_h) + (size_t)k * sizeof(ncclUniqueId), sizeof(ncclUniqueId));
      ncclComm_t c = nullptr;
      CACTO_CHECK_RCCL(R.init(&c, world, id, rank), "ncclCommInitRank");
      sys->dp_comm[k] = c;
    }
    CACTO_CHECK_HIP(hipMalloc(&sys->dp_gc, sizeof(float) * sys->critic.params));
    CACTO_CHECK_HIP(hipMalloc(&sys->dp_ga, sizeof(float) * sys->actor.params));
    CACTO_CHECK_HIP(hipMalloc(&sys->dp_stats, sizeof(double) * 3 * (world + 1)));
    sys->dp_rank = rank;
    sys->dp_world = world;
    return CACTO_OK;
  }();
  if (err) cacto_dp_release(sys);
  return err;
}

extern "C" int cacto_dp_detach(cacto_sys* sys) {
  CACTO_REQUIRE(sys, "cacto_dp_detach: bad arguments");
  std::lock_guard<std::mutex> lock(sys->pipe_mu);
  if (sys->side) CACTO_CHECK_HIP(hipStreamSynchronize(sys->side));
  cacto_dp_release(sys);
  return CACTO_OK;
}

extern "C" int cacto_update_n(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg,
                              const double* storage_d, const int32_t* idx_d, int K, int B, void* workspace_d,
                              size_t workspace_bytes, void* stream) {
  return update_n("cacto_update_n", false, sys, nets, cfg, storage_d, idx_d, nullptr, K, B, workspace_d,
                  workspace_bytes, stream);
}

// ---------------------------------------------------------------- R independent learners
// update_pipeline_pair for R replicas (learn.h: EnsReplica, ens_route): the same K + 1 steps, each one
// chain launch and one GEMM + Adam launch over all replicas. The handle owns the device table of
// descriptors, written once at creation; a call passes only the indices, K and the step's offset.
struct cacto_ensemble {
  const cacto_sys* sys;
  EnsRoute route;
  ChainScalars cs;
  EnsReplica* tab_d = nullptr;
  int B = 0;
  float* y[ENS_MAX_R];
  float* V[ENS_MAX_R];
};

namespace {
int ens_refuse(const EnsRoute& er) {
  switch (er.reason) {
    case ENS_OK: return CACTO_OK;
    case ENS_BAD_R:
      set_error("ensemble: R must be in [1, " + std::to_string(ENS_MAX_R) + "] (CACTO_ENSEMBLE_MAX)");
      return CACTO_EINVAL;
    case ENS_BAD_B: set_error("ensemble: B must be positive"); return CACTO_EINVAL;
    case ENS_ELU:
      set_error("ensemble: the elu critic has no 4-sample chain kernels; train its seeds one by one");
      return CACTO_EUNSUPPORTED;
    default:
      set_error("ensemble: the batch is not paired (2 * Bp > 1024); only the paired small-batch route is built");
      return CACTO_EUNSUPPORTED;
  }
}
}  // namespace

extern "C" int cacto_ensemble_plan(int nb_state, int nb_action, int critic_type, int sobolev, int B, int R, int cus,
                                   cacto_ens_plan* out) {
  CACTO_REQUIRE(out && nb_state >= 2 && nb_state <= CACTO_MAX_STATE && nb_action >= 1 &&
                    nb_action <= CACTO_MAX_ACTION && critic_type >= 0 && critic_type <= 2,
                "cacto_ensemble_plan: bad arguments");
  const NetTopo tc = make_topo(CACTO_NET_CRITIC, nb_state, nb_action, critic_type);
  const NetTopo ta = make_topo(CACTO_NET_ACTOR, nb_state, nb_action);
  if (cus <= 0) cus = cu_count();
  const EnsRoute e = ens_route(tc, ta, sobolev != 0, B, R, cus);
  cacto_ens_plan p{};
  p.reason = e.reason;
  p.R = R;
  p.cus = cus;
  if (e.supported) {
    const int layers = ceil_div(R, e.pair.ng);
    p.supported = 1;
    p.Bp = e.one.Bp;
    p.pair_xcds = e.pair.nx;
    p.xcd_groups = e.pair.ng;
    p.layers = layers;
    p.xcds = e.pair.nx * std::min(R, e.pair.ng);
    p.chain_wgs = ens_chain_grid(e.pair);
    p.chain_wgs_lone = ens_chain_grid(e.lone);
    p.chain_threads = 512;
    p.chain_lds_bytes = e.lds_bytes;
    p.wgrad_wgs = 8 * e.wa_stride[2] * R;
    p.wgrad_wgs_critic = 8 * e.wa_stride[0] * R;
    p.wgrad_wgs_actor = 8 * e.wa_stride[1] * R;
    p.wgrad_threads = 256;
    p.wgrad_lds_bytes = (256 + 16 * 256) * (int)sizeof(float);
    p.launches_per_update = 2;
  }
  *out = p;
  return ens_refuse(e);
}

extern "C" int cacto_ensemble_create(const cacto_sys* sys, int R, const cacto_nets* nets_h,
                                     const double* const* storages_d, void* const* workspaces_d,
                                     size_t workspace_bytes, const cacto_update_cfg* cfg, int B, cacto_ensemble** out) {
  CACTO_REQUIRE(sys && nets_h && storages_d && workspaces_d && cfg && out, "cacto_ensemble_create: bad arguments");
  const EnsRoute er = ens_route(sys->critic, sys->actor, cfg->w_S != 0.0, B, R, cu_count());
  if (int e = ens_refuse(er)) return e;
  CACTO_REQUIRE(!sys->dp_comm[0] && !sys->dp_comm[1],
                "cacto_ensemble_create: the handle is data parallel (cacto_dp_attach); an ensemble runs on one rank");
  CACTO_REQUIRE(cfg->want_target_V == 0, "cacto_ensemble_create: want_target_V is not part of the paired loop");
  std::vector<EnsReplica> tab(R);
  cacto_ensemble* ens = new cacto_ensemble();
  ens->sys = sys;
  ens->route = er;
  ens->cs = chain_scalars(cfg, er.one, B);
  ens->B = B;
  const int soft = cfg->MC ? 0 : 1;
  for (int r = 0; r < R; ++r) {
    const cacto_nets* n = nets_h + r;
    int err = check_nets(n);
    if (!err && !storages_d[r]) set_error("cacto_ensemble_create: null storage"), err = CACTO_EINVAL;
    if (!err) err = [&]() -> int {
      CHECK_WS(workspaces_d[r], workspace_bytes, B);
      return CACTO_OK;
    }();
    if (err) {
      delete ens;
      return err;
    }
    const Workspace w = plan(sys, cfg->w_S != 0.0, B, static_cast<char*>(workspaces_d[r]));
    EnsReplica& E = tab[r];
    E.C = cacto_make_view(sys, CACTO_NET_CRITIC, n->critic_d);
    E.Tg = cacto_make_view(sys, CACTO_NET_CRITIC, n->target_d);
    E.Ac = cacto_make_view(sys, CACTO_NET_ACTOR, n->actor_d);
    E.gbc = w.crit;
    E.gba = w.act;
    E.y = ens->y[r] = w.scal;
    E.V = ens->V[r] = w.scal + w.Bp;
    E.step = n->step_d;
    E.cn = critic_adam_net(sys, n, cfg, w, soft, nullptr, n->critic_d);
    E.an = actor_adam_net(sys, n, cfg, w);
    E.storage = storages_d[r];
  }
  hipError_t he = hipMalloc(&ens->tab_d, sizeof(EnsReplica) * R);
  if (he == hipSuccess) he = hipMemcpy(ens->tab_d, tab.data(), sizeof(EnsReplica) * R, hipMemcpyHostToDevice);
  if (he != hipSuccess) {
    if (ens->tab_d) (void)hipFree(ens->tab_d);
    delete ens;
    return hip_fail(he, "cacto_ensemble_create: device table");
  }
  *out = ens;
  return CACTO_OK;
}

extern "C" int cacto_ensemble_destroy(cacto_ensemble* ens) {
  if (!ens) return CACTO_OK;
  if (ens->tab_d) (void)hipFree(ens->tab_d);
  delete ens;
  return CACTO_OK;
}

extern "C" int cacto_ensemble_update(cacto_ensemble* ens, const int32_t* idx_d, int K, void* stream) {
  CACTO_REQUIRE(ens && idx_d && K >= 0, "cacto_ensemble_update: bad arguments");
  hipStream_t st = as_stream(stream);
  const int B = ens->B;
  const long long rstride = (long long)K * B;
  for (int t = 0; t <= K && K > 0; ++t) {
    const int mode = t == 0 ? 0 : t < K ? 2 : 1;
    const int32_t* idx_c = idx_d + (size_t)std::min(t, K - 1) * B;  // (unused at t == K)
    const int32_t* idx_a = idx_d + (size_t)std::max(t - 1, 0) * B;  // (unused at t == 0)
    if (int e = launch_chain_ens(ens->sys, ens->route, ens->tab_d, ens->cs, idx_c, idx_a, rstride, B, mode, st))
      return e;
    if (int e = launch_wgrad_adam_ens(ens->sys, ens->route, ens->tab_d, mode, st)) return e;
  }
  return CACTO_OK;
}

extern "C" int cacto_ensemble_outputs(const cacto_ensemble* ens, int r, float** y_d, float** V_d) {
  CACTO_REQUIRE(ens && r >= 0 && r < ens->route.R && y_d && V_d, "cacto_ensemble_outputs: bad arguments");
  *y_d = ens->y[r];
  *V_d = ens->V[r];
  return CACTO_OK;
}

extern "C" size_t cacto_workspace_yv_offset(const cacto_sys* sys, int B) {
  if (!sys || B <= 0) return 0;
  const Workspace w = plan(sys, true, B, reinterpret_cast<char*>(256));
  return reinterpret_cast<char*>(w.scal) - reinterpret_cast<char*>(256);
}

extern "C" int cacto_update_n_dp(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg,
                                 const double* storage_d, const int32_t* idx_d, int K, int B, void* workspace_d,
                                 size_t workspace_bytes, void* stream) {
  return update_n("cacto_update_n_dp", true, sys, nets, cfg, storage_d, idx_d, nullptr, K, B, workspace_d,
                  workspace_bytes, stream);
}

// learn_and_update with PER (RL.py:122-137) for K updates: sample (stratified, IS weights) ->
// update -> priority update per step, the sampling and priority update on the critic's stream
// (the next sample depends on them), pipelined with the actor steps as in cacto_update_n.
extern "C" int cacto_update_n_per(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg,
                                  const double* storage_d, double* sum_tree_d, double* min_tree_d, int64_t capacity,
                                  int64_t max_idx, double beta, const double* uniforms_d, double* exp_counter_d,
                                  double fresh_factor, double eps, double alpha, double* max_priority_d, int K, int B,
                                  void* workspace_d, size_t workspace_bytes, void* stream) {
  const PerArgs per{sum_tree_d, min_tree_d, capacity, max_idx, beta, fresh_factor, eps, alpha, uniforms_d,
                    exp_counter_d, max_priority_d};
  return update_n("cacto_update_n_per", false, sys, nets, cfg, storage_d, nullptr, &per, K, B, workspace_d,
                  workspace_bytes, stream);
}

extern "C" int cacto_update_n_per_dp(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg,
                                     const double* storage_d, double* sum_tree_d, double* min_tree_d, int64_t capacity,
                                     int64_t max_idx, double beta, const double* uniforms_d, double* exp_counter_d,
                                     double fresh_factor, double eps, double alpha, double* max_priority_d, int K,
                                     int B, void* workspace_d, size_t workspace_bytes, void* stream) {
  const PerArgs per{sum_tree_d, min_tree_d, capacity, max_idx, beta, fresh_factor, eps, alpha, uniforms_d,
                    exp_counter_d, max_priority_d};
  return update_n("cacto_update_n_per_dp", true, sys, nets, cfg, storage_d, nullptr, &per, K, B, workspace_d,
                  workspace_bytes, stream);
}
