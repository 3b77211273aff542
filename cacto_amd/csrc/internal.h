// Host-side handle layout shared by the translation units of libcacto_hip.so.
#pragma once

#include <mutex>

#include "env.h"
#include "mlp.h"

struct cacto_sys {
  cacto::SysDevice host;  // host copy (validated)
  cacto::SysDevice* dev;  // device copy read by every kernel
  cacto::NetTopo actor, critic;
  void* ddp_ws = nullptr;  // cacto_ddp_backward's per-step derivative records (grow-only)
  size_t ddp_ws_bytes = 0;
  hipStream_t side = nullptr;  // cacto_update_n's actor-step stream and its events
  hipEvent_t ev_critic = nullptr, ev_actor[3] = {nullptr, nullptr, nullptr};
  std::mutex pipe_mu;  // one two-stream pipeline at a time per handle (they share side / events)
  // pinned host copy of pipe_sig[1] (the device waits' timeout latch), refreshed asynchronously at
  // the end of every pipelined call with device-side waits; read (and cleared) by
  // cacto_pipeline_check after a stream synchronisation, refused on at the start of the next call
  unsigned long long* latch_host = nullptr;
  // device-side ordering of the two-stream pipeline: pipe_sig[0] counts the actor iterations whose
  // chain has finished, [2] the critic Adam steps finished (both monotonic over the handle's life),
  // [1] latches a wait that timed out, [3] is k_adam's last-workgroup counter, [4..7] the one-time
  // concurrency probe's words; pipe_seq is the host's count of pipeline iterations issued before
  // this call; pipe_probe: -1 not run yet, 0 the streams' kernels did not run concurrently (queue
  // markers), 1 they did (device-side waits)
  unsigned long long* pipe_sig = nullptr;
  unsigned long long pipe_seq = 0;
  int pipe_probe = -1;
  // data-parallel updates over RCCL (cacto_dp_attach): one communicator per stream of the pipeline
  // (critic stream, side stream: each orders its own collectives), the all-reduced gradients (one
  // flat buffer per network) and the PER shard statistics ([3] this rank's, [world][3] all ranks')
  void* dp_comm[2] = {nullptr, nullptr};
  int dp_rank = 0, dp_world = 0;
  float *dp_gc = nullptr, *dp_ga = nullptr;
  double* dp_stats = nullptr;
  // k_wgrad_adam work lists, [8 XCD bins][wa_stride] item codes (layer << 16 | net << 15 | item, -1 = none), for
  // the critic alone, the actor alone and both (built at creation, cacto_build_wgrad_adam_items)
  int32_t* wa_items[3] = {nullptr, nullptr, nullptr};
  int wa_stride[3] = {0, 0, 0};
};

namespace cacto {
inline const NetTopo& topo(const cacto_sys* s, int net) { return net == CACTO_NET_ACTOR ? s->actor : s->critic; }
inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }
inline int64_t flat_span(const NetTopo& t) { return ((int64_t)t.params + 63) / 64 * 64; }
// elu_kernels.hip: V (and dV/ds when dVdS is non-null) of the elu critic
int launch_critic_forward_elu(const cacto_sys* sys, const NetView& N, const float* S, float* V, float* dVdS, int B,
                              hipStream_t st);
}  // namespace cacto

cacto::NetView cacto_make_view(const cacto_sys* sys, int net, const float* netbuf);
int cacto_const_dyn_init(cacto_sys* sys);  // SysDevice::cd_* of a prismatic-only chain (env_kernels.hip)
int cacto_build_wgrad_adam_items(cacto_sys* sys);  // learn_kernels.hip
// ddp_kernels.hip: the handle's grow-only device workspace (derivative records), at least `bytes`
int cacto_ddp_workspace(cacto_sys* sys, size_t bytes, double** out);
// ddp_kernels.hip: the derivative records (DdpRec, [t][k][e]) of steps 0 .. steps-1 of n_ep
// episodes at rec, ddp_rec_doubles(n_ep, steps) doubles (car_park, revolute chains); want_lx: l_x,
// l_xx too. The one launcher of k_ddp_prim / _lx / _tan / _derivs and reader of CACTO_DDP_SPLIT.
int cacto_ddp_launch_derivs(const cacto_sys* sys, const double* S, int64_t ldS, const double* U, int64_t ldU,
                            const int32_t* nsteps, int n_ep, double* rec, int64_t steps, bool want_lx, hipStream_t st);
void cacto_dp_release(cacto_sys* sys);  // learn_host.hip: the RCCL communicators and buffers
// replay_kernels.hip: the one PER route (which sampler and priority update a batch of B takes on a
// tree of `capacity` leaves, whether the pipelined loops defer the sampler's count into the priority
// update, whether the tree's shape allows the overlapped form); launches nothing. Reported by
// cacto_per_plan, whose struct it is.
namespace cacto {
using PerRoute = struct ::cacto_per_plan;
enum { PER_UPDATE_SET = 0, PER_UPDATE_SUB = 1, PER_UPDATE_CHAIN = 2 };
PerRoute per_route(int64_t capacity, int B);
}  // namespace cacto
// ... and the two launches of a deferred count no public entry covers: the count alone, and the
// priority update with the count applied first
int cacto_per_count_launch(const int32_t* idx_d, int B, double* exp_counter_d, hipStream_t st);
int cacto_per_update_count(double* sum_tree_d, double* min_tree_d, int64_t capacity, const int32_t* idx_d,
                           const float* y_d, const float* V_d, double* exp_counter_d, double fresh_factor, double eps,
                           double alpha, double* max_priority_d, int B, hipStream_t st);
