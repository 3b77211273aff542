// Where learn_kernels.hip (the kernels, the launch_* functions that name one, the route that picks
// one) and learn_host.hip (workspace, C ABI, update pipelines) meet: plain structs and declarations.
#pragma once

#include "internal.h"
#include "per_device.h"

namespace cacto {

struct GradBufs {
  float* LT[MAX_LAYERS];
  float* RT[MAX_LAYERS];
  int ld;  // row stride of the panels
  int Bp;  // batch rounded up to 16
};

struct ChainScalars {
  float w_S;
  int MC;
  int B_global;
  int want_vt;
  // the two-stream pipeline's device-side ordering (DESIGN §3 "memory-ordering contract"): the actor
  // chain waits, before its critic pass at s', until *wait_p >= wait_v (the critic's Adam of the same
  // update has run) — a relaxed poll, no fence: the Adam wrote the critic through to memory at agent
  // scope and published after its stores completed, and no L2 holds a line of the buffer from before
  // (kernel starts invalidate; nothing reads it in between)
  const unsigned long long* wait_p;
  unsigned long long wait_v;
  // 1 (the PER loops): that wait at the chain's start, before it gathers the sampled rows (the
  // sample of the update precedes the critic's Adam on the other stream)
  int wait_at_start;
  // 1: the 16-sample tiles dealt so that the tiles of one 256-row GEMM chunk run on the XCD that
  // k_wgrad_big runs that chunk on (chain_tile_of)
  int xcd_tiles;
};

struct WgLayer {
  const float* LT;
  const float* RT;
  int in, out, IT, OT, woff, boff;
};
struct WgArgs {
  WgLayer l[MAX_LAYERS];
  int nl, ld, r_begin, r_end, bias_r0, CH, nch, P, tpc;
  int toff[MAX_LAYERS + 1];
  unsigned char perm[64];  // k_wgrad_big: the items of a chunk by decreasing work (full 4 x 4 blocks first)
};

struct AdamArgs {
  double beta1, beta2, eps, tau;
  double lr[5];
  double bounds[4];
  int which;  // 0 critic counter, 1 actor counter
  int soft;
};
struct AdamNet {  // one network of the fused weight-gradient + Adam launch (k_wgrad_adam)
  WgArgs wg;  // panels, rows, 64-row chunking (as k_wgrad)
  NetTopo t;
  const float* src;  // weights the step starts from (== nb for an in-place step)
  float* nb;
  float4* pk;
  float* m;
  float* v;
  float* target;  // soft update (critic) or nullptr
  float4* tpk;
  AdamArgs ad;
  int items;                    // weight tiles + bias tiles, all layers
  int ioff[MAX_LAYERS + 1];     // first item of layer l: KT*OT weight tiles then OT bias tiles
};

// Which kernels a batch takes: the one place it is decided (learn_route), a function of the two
// networks, whether the critic's Sobolev half is on, the batch and the device's CU count — no
// environment, no launches. Every update path of one batch reads the same route, so every path
// runs the same kernels on the same sums (bit-identical results). cacto_update_plan reports it.
enum { WG_FUSED = 0, WG_SPLIT = 1, WG_BIG = 2 };
struct NetRoute {  // one network's weight-gradient GEMM and Adam step
  int rows;      // gradient rows: critic 2 Bp with the Sobolev half, else Bp; actor Bp
  int chunk;     // rows per split-K chunk (one slab each): 64 up to 1024 rows, 128 below 4096, else 256
  int nch;       // chunks
  int gemm;      // the update's: WG_FUSED (k_wgrad_adam, with its Adam), WG_SPLIT (k_wgrad), WG_BIG
                 // (k_wgrad_big). cacto_critic_grad / cacto_actor_grad and the data-parallel paths keep
                 // the slabs at every batch: k_wgrad where the update fuses
  int xcd;       // the split GEMM's workgroups dealt by XCD (from 8 chunks on)
  int adam_nch;  // the k_adam / k_reduce instance that sums the chunks (nch_instance)
};
struct LearnRoute {
  int Bp;             // batch rounded up to 16
  int tile;           // samples per chain workgroup: Q4_TILE or CACTO_TILE
  int elu;            // the elu critic's chain kernels (elu_kernels.hip)
  int paired;         // cacto_update_n[_per]: the paired single-stream pipeline with fused GEMM + Adam
                      // launches; else two streams and split launches
  NetRoute critic, actor;
  int xcd_tiles;      // ChainScalars::xcd_tiles
  int pair_xcds;      // XCDs the paired q4 chain grid runs on (0: not a q4 batch)
  int per_overlap;    // the batch's half of per_overlap_ok: k_wgrad_big and a k_adam<NCH> that holds
                      // every chunk, for the critic
  int devwait_actor;  // the batch's half of the actor chain's device-side wait: 16-sample tiles, at
                      // most one actor workgroup per CU
};
LearnRoute learn_route(const NetTopo& critic, const NetTopo& actor, bool sobolev, int B, int cus);
int nch_instance(int nch);
int cu_count();

struct Workspace {
  LearnRoute route;  // of the call's batch (plan)
  GradBufs crit, act;
  float* slab;    // critic weight-gradient slabs
  float* slab_a;  // actor's (a separate region: cacto_update_n overlaps the two steps)
  float* cshadow; // two more critic net buffers (cacto_update_n rotates the critic over three)
  int32_t* pidx;  // cacto_update_n_per: sampled indices, a ring of five buffers of Bp
  float* pisw;    // and the IS weights of the current update
  int32_t* runs;  // the overlapped PER loop's per-subtree sample runs (2 x PER_RUN_SUB ints)
  float* scal;  // y, V, Vt scratch (3 * Bp)
  size_t bytes;
  int Bp;
};

// The launches (learn_kernels.hip); each reads w.route.
int launch_reduce(const float* slab, int nch, int P, float* out, hipStream_t st);
// the weight-gradient GEMM of a network into its slabs (route.critic.nch / route.actor.nch of them)
int launch_critic_wgrad(const cacto_sys* sys, const Workspace& w, hipStream_t st, const PerRunArgs* per_run = nullptr);
int launch_actor_wgrad(const cacto_sys* sys, const Workspace& w, hipStream_t st, unsigned long long* sig_p = nullptr,
                       unsigned long long sig_v = 0);
int launch_critic_chain(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg,
                        const double* storage, const int32_t* idx, const float* isw, int B, float* y, float* V,
                        float* Vt, const Workspace& w, hipStream_t st);
int launch_actor_chain(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg,
                       const double* storage, const int32_t* idx, int B, const Workspace& w, hipStream_t st,
                       const unsigned long long* wait_p = nullptr, unsigned long long wait_v = 0,
                       int wait_at_start = 0);
ChainScalars chain_scalars(const cacto_update_cfg* cfg, const LearnRoute& r, int B);
int launch_chain_pair(const cacto_sys* sys, const NetView& C, const NetView& Tg, const NetView& Ac,
                      const ChainScalars& cs, const double* storage, const int32_t* idx_c, const float* isw,
                      const int32_t* idx_a, int B, const Workspace& w, float* y, float* V, int32_t* step,
                      hipStream_t st);
int launch_adam(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg, int which,
                const float* slab, int nch, int soft, hipStream_t st, const float* src = nullptr,
                const unsigned long long* wait_p = nullptr, unsigned long long wait_v = 0,
                unsigned long long* sig_p = nullptr, unsigned long long sig_v = 0,
                const PerSampleArgs* sample = nullptr, int thru = 0);
AdamNet critic_adam_net(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg, const Workspace& w,
                        int soft, const float* src, float* nb);
AdamNet actor_adam_net(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg, const Workspace& w);
int launch_wgrad_adam(const cacto_sys* sys, int mode, const AdamNet& n0, const AdamNet* n1, const int32_t* step,
                      hipStream_t st);
int launch_soft(const cacto_sys* sys, const cacto_nets* nets, float tau, hipStream_t st);
int launch_pipe_probe(unsigned long long* w, int role, hipStream_t st);

// ---------------------------------------------------------------- R independent learners (ensemble)
// The paired update loop (update_pipeline_pair) for R replicas of one system as one chain launch and
// one GEMM + Adam launch per step: k_chain_ens_q4 / k_wgrad_adam_ens run the device bodies of
// k_chain_pair_q4 / k_wgrad_adam with a replica index taken from the block index. What a replica's
// workgroups read lives in a device table written once, when the ensemble handle is created.
struct EnsReplica {
  NetView C, Tg, Ac;
  GradBufs gbc, gba;
  float* y;
  float* V;
  int32_t* step;
  AdamNet cn, an;  // critic (with its soft target update unless MC), actor
  const double* storage;
};

// How the R replicas' chain tiles are dealt to workgroups: the one place it is decided (ens_route).
// Block b runs on XCD b % 8 (observed dealing: it decides only which L2 serves a tile, never a
// result). The 8 XCDs form ng = 8 / nx groups of nx (the one-learner route's pair_xcds); replica r
// runs on group r % ng, so the replicas spread over the XCDs instead of all landing on XCDs
// [0, nx), and the replicas of one group are stacked in layers of `per` = ceil(nt / nx) slices.
struct EnsDeal {
  int R, nx, ng, per, nt;  // nt: tiles per replica in this launch (2 nct paired, nct alone)
};
struct EnsTile {
  int r, j;  // replica, tile; r >= R or j >= nt: a padding workgroup
};
__host__ __device__ inline EnsTile ens_tile_of(const EnsDeal& d, int b) {
  const int x = b & 7, sl = b >> 3;
  const int g = x / d.nx, lay = sl / d.per;
  return EnsTile{lay * d.ng + g, (sl - lay * d.per) * d.nx + (x - g * d.nx)};
}
inline int ens_chain_grid(const EnsDeal& d) { return 8 * d.per * ((d.R + d.ng - 1) / d.ng); }

enum { ENS_OK = 0, ENS_BAD_R = 1, ENS_NOT_PAIRED = 2, ENS_ELU = 3, ENS_BAD_B = 4 };
constexpr int ENS_MAX_R = CACTO_ENSEMBLE_MAX;
struct EnsRoute {
  int supported, reason;  // ENS_*
  LearnRoute one;         // the one-learner route of the batch
  int R, nct;             // replicas, 4-sample tiles per chain
  EnsDeal pair, lone;     // the paired steps' deal, the lone first / last step's
  int wa_stride[3];       // k_wgrad_adam's work-list stride per mode (critic, actor, both)
  int lds_bytes;          // chain launch
};
EnsRoute ens_route(const NetTopo& critic, const NetTopo& actor, bool sobolev, int B, int R, int cus);
// mode 0: critic chains alone, 1: actor chains alone, 2: both. idx_c / idx_a: replica 0's minibatch of
// the step; replica r's is rstride int32 further on.
int launch_chain_ens(const cacto_sys* sys, const EnsRoute& er, const EnsReplica* tab, const ChainScalars& cs,
                     const int32_t* idx_c, const int32_t* idx_a, long long rstride, int B, int mode, hipStream_t st);
int launch_wgrad_adam_ens(const cacto_sys* sys, const EnsRoute& er, const EnsReplica* tab, int mode, hipStream_t st);

// elu_kernels.hip: the chain kernels of a handle whose critic is the elu network (is_elu_topo);
// launch_critic_chain / launch_actor_chain / launch_chain_pair hand over to them
int launch_critic_chain_elu(const cacto_sys* sys, const NetView& C, const NetView& Tg, const ChainScalars& cs,
                            const double* storage, const int32_t* idx, const float* isw, int B, const GradBufs& gb,
                            float* y, float* V, float* Vt, int32_t* step, hipStream_t st);
int launch_actor_chain_elu(const cacto_sys* sys, const NetView& Ac, const NetView& C, const ChainScalars& cs,
                           const double* storage, const int32_t* idx, int B, const GradBufs& gb, int32_t* step,
                           hipStream_t st);
int launch_chain_pair_elu(const cacto_sys* sys, const NetView& C, const NetView& Tg, const NetView& Ac,
                          const ChainScalars& cs, const double* storage, const int32_t* idx_c, const float* isw,
                          const int32_t* idx_a, int B, const GradBufs& gbc, const GradBufs& gba, float* y, float* V,
                          int32_t* step, hipStream_t st);

}  // namespace cacto
