/*
 * cacto_hip.h — C-ABI of libcacto_hip.so, the MI355X (gfx950) hot path of CACTO.
 *
 * Drop-in boundary for the data-parallel hot path of nadimkanazi/cacto (reference paths below are
 * relative to its repository root). Each entry point replaces a Python/TF/Pinocchio call site:
 *
 *   cacto_env_step_batch   Env.simulate_batch + derivative_batch + reward_batch (+ dr/da tape)
 *                          environment.py:134-144, :277-286 (and per-system overrides); as called
 *                          from NN.compute_actor_grad NeuralNetwork.py:188, :199-204
 *   cacto_env_step         Env.step + get_end_effector_position (float64 rollout semantics)
 *                          environment.py:70-78, :146-156; plot_utils.py:262-264
 *   cacto_env_jacobians    Env.augmented_derivative environment.py:111-132 (as called by TO.py:181)
 *   cacto_env_bound_control_cost  Env.bound_control_cost environment.py:158-163
 *   cacto_rollout          RL_AC.create_TO_init loop RL.py:223-231 / PLOT.rollout plot_utils.py:245-279
 *   cacto_rollout_rewards  Env.step reward / get_end_effector_position over recorded trajectories
 *   cacto_ddp_backward     TO.backward_pass TO.py:119-202 (dV/dx Sobolev labels);
 *                          cacto_ddp_backward_box: the same pass under the solve's hard control limits
 *                          (cacto_to_box), the labels of the bounded problem (no reference counterpart)
 *   cacto_to_solve         TO.TO_System_Solve TO.py:37-100: the trajectory optimisation itself, as a
 *                          batched iLQR on the same cost and dynamics (the reference: CasADi + IPOPT,
 *                          one NLP per episode); cacto_to_backward_gains / cacto_to_forward are its
 *                          two building blocks
 *   cacto_mlp_pack         (layout transform for the kernels; no reference counterpart)
 *   cacto_sys_set_critic_type  RL_AC.setup_model's critic_type choice RL.py:65-76 ('sine' /
 *                          'sine-elu', NeuralNetwork.py:80-108)
 *   cacto_actor_forward    NN.eval(actor, s)  NeuralNetwork.py:130-138 (+ utils.py:17-24)
 *   cacto_critic_forward   NN.eval(critic, s)
 *   cacto_critic_input_grad tape.gradient(V, s)  NeuralNetwork.py:162-165, :190-195
 *   cacto_critic_grad      NN.compute_critic_grad  NeuralNetwork.py:150-178
 *   cacto_actor_grad       NN.compute_actor_grad   NeuralNetwork.py:180-233
 *   cacto_adam_step        optimizer.apply_gradients RL.py:105, :109 (Keras-2.11 Adam, RL.py:79-88)
 *   cacto_soft_update      RL_AC.update_target RL.py:113-118
 *   cacto_update           RL_AC.update + update_target (one learn_and_update iteration, RL.py:122-137)
 *   cacto_update_n[_per]   the learn_and_update loop RL.py:120-143 for K updates (with PER:
 *                          sample -> update -> priority update), pipelined on two streams
 *   cacto_ensemble_*       the same loop (RL.py:120-143) for R independent learners of one system —
 *                          the ten-seed sets of generate_tests_set_script.py — in one call
 *   cacto_buffer_gather    ReplayBuffer.sample row gather replay_buffer.py:47-61
 *   cacto_buffer_add       ReplayBuffer.add ring write replay_buffer.py:25-36
 *   cacto_rl_solve_add     RL_AC.RL_Solve n-step targets RL.py:145-189 fused with the
 *                          buffer.add of its output (main.py:240)
 *   cacto_validate         the critic and the actor against an iteration's fresh TO trajectories
 *                          (value, Sobolev-gradient and action errors; no reference counterpart)
 *   cacto_per_*            PrioritizedReplayBuffer + segment trees replay_buffer.py:87-218,
 *                          segment_tree.py:4-145 (cacto_per_plan: which kernels a batch takes; no
 *                          reference counterpart)
 *
 * Conventions
 *   - Every pointer argument named *_d is DEVICE memory (e.g. torch tensor .data_ptr()), contiguous
 *     row-major. Host pointers are named *_h. The library never frees caller memory.
 *   - Every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream)
 *     and enqueues no host synchronisation, so sequences can be captured into a hipGraph.
 *     cacto_update_n[_per] also use a side stream owned by the handle, joined back into `stream`
 *     before they return; cacto_ddp_backward (car_park, revolute chains) grows a device workspace
 *     owned by the handle (a hipMalloc, so warm it up before capturing), and so does
 *     cacto_to_backward_gains. cacto_to_solve with cfg.poll_every > 0 on the revolute chains
 *     (either path) and on car_park with cfg.path = CACTO_TO_PATH_DEFAULT synchronises the stream
 *     every poll_every iterations (it reads a device counter of finished episodes to stop early);
 *     with poll_every == 0, or where cacto_to_solve_plan says on_device, it never synchronises.
 *   - Return 0 on success, <0 on error; cacto_last_error() returns a thread-local message.
 *     No C++ exception crosses the ABI.
 *   - Handles (cacto_sys) are created/destroyed by the caller; concurrent calls on one handle are
 *     undefined (as in the reference's single-threaded loop).
 */
#ifndef CACTO_HIP_H
#define CACTO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CACTO_ABI_VERSION 1

/* error codes */
#define CACTO_OK 0
#define CACTO_EINVAL -1
#define CACTO_EHIP -2
#define CACTO_ENOMEM -3
#define CACTO_EUNSUPPORTED -4

/* dynamics kinds */
#define CACTO_DYN_SINGLE_INTEGRATOR 0 /* environment.py:235-243 */
#define CACTO_DYN_CHAIN 1             /* Pinocchio chain: robot_utils.py:348-432 */
#define CACTO_DYN_CAR 2               /* environment.py:437-448 */
#define CACTO_DYN_CAR_PARK 3          /* environment.py:584-595 */

/* reward kinds */
#define CACTO_REW_PLANAR 0      /* SI / DI / Car: environment.py:252-275, :329-351, :457-480 */
#define CACTO_REW_MANIPULATOR 1 /* planar + w2*|v|^2 when w2 != 0: environment.py:695-723 */
#define CACTO_REW_UR5 2         /* 3-D ellipsoids: environment.py:780-805 */
#define CACTO_REW_CAR_PARK 3    /* smooth-box obstacles: environment.py:604-641 */

#define CACTO_MAX_STATE 16
#define CACTO_MAX_ACTION 8
#define CACTO_MAX_JOINTS 6
#define CACTO_JOINT_COLS 27 /* parent, type, axis[3], R[9], p[3], mass, com[3], I[6] */

/* System description: the numeric content of a conf_*.py module the hot path reads. */
typedef struct {
  int32_t dyn_kind;
  int32_t reward_kind;
  int32_t nb_state;  /* ns = nx + 1 (time last) */
  int32_t nb_action; /* na */
  int32_t nq, nv;    /* chain only */
  int32_t normalize; /* NORMALIZE_INPUTS */
  int32_t n_joints;  /* chain only */
  int32_t ee_parent; /* chain only: joint index of the 'EE' frame's parent */
  int32_t n_check;   /* car_park only */
  int32_t n_weights; /* length of cost_weights_* (7, car_park 8) */
  int32_t const_dyn; /* filled by cacto_sys_create: 1 if every joint is prismatic, so M and nle
                      * do not depend on the state (DI) — input value ignored */
  double dt;
  double state_norm[CACTO_MAX_STATE];
  double u_max[CACTO_MAX_ACTION];
  double w_b;
  double scale, offset;  /* cost_funct_param[1], [0] */
  double alpha, alpha2;  /* soft_max_param */
  double obs[18];        /* obs_param */
  double target[3];      /* TARGET_STATE */
  double w_running[8];   /* cost_weights_running */
  double w_terminal[8];  /* cost_weights_terminal */
  double L_delta, tau_delta, k_db; /* car / car_park */
  double check_points[20];         /* car_park check_points_BF (x, y) pairs */
  double ee_R[9], ee_p[3];         /* chain: EE frame placement in its parent joint frame */
  double gravity[3];               /* chain: model.gravity linear part */
} cacto_sys_params;

typedef struct cacto_sys cacto_sys;

const char* cacto_last_error(void);
int cacto_abi_version(void);

/* joint_table_h: n_joints x CACTO_JOINT_COLS float64 (host), see cacto_amd/robots.py */
int cacto_sys_create(const cacto_sys_params* params_h, const double* joint_table_h, cacto_sys** out);
int cacto_sys_destroy(cacto_sys* sys);
/* The critic network of this handle (RL.py:65-76 critic_type): 0 = 'sine' (4 SIREN layers 64, 64,
 * 128, 128 wide, the default, every shipped config), 1 = 'sine-elu' (NeuralNetwork.py:80-93: sine,
 * elu, sine, elu layers of the same widths; the CACTO_CRITIC_ELU build only), 2 = 'elu'
 * (NeuralNetwork.py:65-78: Dense 16, 32, 256, 256 with elu, then Dense 1; 16 ns + 75,057 parameters,
 * kernels of its own in every build). Set before creating or updating critic networks of this
 * handle: 2 (and leaving 2) changes the critic's topology, so cacto_mlp_param_count,
 * cacto_mlp_netbuf_floats and cacto_workspace_bytes answer for the new network from then on, and no
 * critic net buffer, workspace or captured graph of the old one may be used after it (the call
 * synchronises the device and rebuilds the handle's fused weight-gradient + Adam work lists). The
 * 'relu' critic is not built (CACTO_EINVAL). */
int cacto_sys_set_critic_type(cacto_sys* sys, int critic_type);

/* ---------------------------------------------------------------- environment ------------ */

/* compute_actor_grad's environment calls for a batch (float32 tensors in/out, float64 math):
 *   S_next = simulate_batch(S, A); Fu = derivative_batch(S, A);
 *   R = reward_batch(W, S, A); dR_dA = d R / d A  (TF tape over u_cost)
 * W: W_d [B, n_weights] float64 if given, else term*cost_weights_terminal +
 * (1-term)*cost_weights_running from term_d [B] (NeuralNetwork.py:197-201), else running weights.
 * Any output pointer may be NULL. Shapes: S [B,ns], A [B,na], S_next [B,ns], Fu [B,ns,na], R [B],
 * dR_dA [B,na]. */
int cacto_env_step_batch(const cacto_sys* sys, const float* S_d, const float* A_d, const double* term_d,
                         const double* W_d, float* S_next_d, float* Fu_d, float* R_d, float* dR_dA_d, int B,
                         void* stream);

/* get_end_effector_position for B float64 states: EE_d [B,3] (environment.py:146-156). */
int cacto_env_ee(const cacto_sys* sys, const double* S_d, double* EE_d, int B, void* stream);

/* Env.step(W, s, a) in float64 plus the EE position of the next state, for B independent rows.
 * W_d may be NULL (running weights). EE_d [B,3], any output may be NULL. */
int cacto_env_step(const cacto_sys* sys, const double* S_d, const double* A_d, const double* W_d,
                   double* S_next_d, double* R_d, double* EE_d, int B, void* stream);

/* Env.augmented_derivative(s, a) (environment.py:111-132; SI :221-233, Car :420-435, CarPark
 * :567-582) for B float64 rows S_d [B,ns], A_d [B,na]: Fx_d [B,nx,nx] = I + dt*[[0,I],[ddq_dq,ddq_dv]]
 * (closed forms for SI / car / car_park / the prismatic DI pair; hyper-dual RNEA for revolute chains,
 * computeABADerivatives) and Fu_d [B,nx,na] = dt*[0; M^-1] (not normalised), nx = ns-1. Called by the
 * host TO backward pass (TO.py:181); cacto_ddp_backward evaluates the same device code inline. */
int cacto_env_jacobians(const cacto_sys* sys, const double* S_d, const double* A_d, int B, double* Fx_d,
                        double* Fu_d, void* stream);

/* Env.bound_control_cost(a) (environment.py:158-163) for B float64 action rows A_d [B,na]:
 * out_d[b] = sum_i a_i^2 + w_b*(a_i/u_max_i)^10, accumulated in action order. */
int cacto_env_bound_control_cost(const cacto_sys* sys, const double* A_d, double* out_d, int B, void* stream);

/* ---------------------------------------------------------------- networks --------------- */

/* Flat parameter layout = Keras trainable_variables order, kernels [in,out] row-major:
 *   actor : W1[ns,256] b1 W2[256,256] b2 W3[256,na] b3            (NeuralNetwork.py:51-63)
 *   critic: W1[ns,64] b1 W2[64,64] b2 W3[64,128] b3 W4[128,128] b4 W5[128,1] b5  (:95-108)
 * A "net buffer" is one float32 device buffer [flat params | pad to 64 | packed MFMA fragments]
 * of cacto_mlp_netbuf_floats() floats. cacto_mlp_pack() refreshes the packed part from the flat
 * part (the Adam kernels keep both in sync during training). */
#define CACTO_NET_ACTOR 0
#define CACTO_NET_CRITIC 1
int64_t cacto_mlp_param_count(const cacto_sys* sys, int net);
int64_t cacto_mlp_netbuf_floats(const cacto_sys* sys, int net);
int cacto_mlp_pack(const cacto_sys* sys, int net, float* netbuf_d, void* stream);

/* NN.eval: normalisation inside, float32. A [B,na], V [B], dVdS [B,ns] (w.r.t. the raw state). */
int cacto_actor_forward(const cacto_sys* sys, const float* actor_netbuf_d, const float* S_d, float* A_d,
                        int B, void* stream);
int cacto_critic_forward(const cacto_sys* sys, const float* critic_netbuf_d, const float* S_d, float* V_d,
                         int B, void* stream);
int cacto_critic_input_grad(const cacto_sys* sys, const float* critic_netbuf_d, const float* S_d,
                            float* V_d, float* dVdS_d, int B, void* stream);

/* ---------------------------------------------------------------- learner ---------------- */

/* Network state for an update: flat params + Adam moments (+ packed copies maintained by Adam). */
typedef struct {
  float* actor_d;  float* actor_m_d;  float* actor_v_d;   /* net buffer + flat Adam moments */
  float* critic_d; float* critic_m_d; float* critic_v_d;
  float* target_d;                                        /* target critic net buffer */
  int32_t* step_d; /* device counters = Keras optimizer iterations: [0] critic, [1] actor.
                    * cacto_critic_grad / cacto_actor_grad increment their counter; the following
                    * cacto_adam_step uses it as `iterations + 1`. */
} cacto_nets;

typedef struct {
  double w_S;         /* Sobolev weight (main.py --w-S) */
  double tau;         /* UPDATE_RATE */
  double beta1, beta2, epsilon; /* Keras Adam defaults 0.9, 0.999, 1e-7 (python floats) */
  double critic_lr[5]; /* PiecewiseConstantDecay values (all equal when LR_SCHEDULE = 0) */
  double actor_lr[5];
  double lr_bounds[4]; /* boundaries (in iterations) */
  int32_t MC;         /* conf.MC */
  int32_t B_global;   /* batch size the loss means are taken over (= B on one GPU) */
  int32_t want_target_V; /* also compute V_tgt(s) (NeuralNetwork.py:178) */
  int32_t pad;
} cacto_update_cfg;

/* Replay rows are float64 [s | R | s_next | dVdx | d | term] (3ns+3 columns, replay_buffer.py:20). */

/* Bytes of workspace cacto_critic_grad / cacto_actor_grad / cacto_update need for batch B. */
size_t cacto_workspace_bytes(const cacto_sys* sys, int B);

/* Which kernels the update calls run for a batch of B (the role cacto_rollout_plan plays for the
 * rollout), decided by the same function every update path reads: a function of the handle's two
 * networks, of whether the critic's Sobolev half is on (w_S != 0), of B and of the CU count — never of
 * the process environment. Bp = B rounded up to 16. A network's gradient rows: critic 2 Bp with the
 * Sobolev half, else Bp; actor Bp.
 *   chain tile  4 samples per chain workgroup up to Bp = 512, 16 above and always for the elu critic
 *   paired      2 Bp <= 1024: cacto_update_n[_per] runs one stream with the critic chain of update t
 *               and the actor chain of t - 1 as one grid, and every update call runs a network's
 *               weight-gradient GEMM and Adam step as one launch (gemm 0); else two streams, split
 *   chunk       64 rows up to 1024 rows, 128 below 4096, 256 from there on
 *   gemm        2 above 1024 rows when every 4 x 4 tile block of the network is 4 x 4, 1 x 4 or
 *               4 x 1 tiles (not the elu critic), else 1; 0 when paired (cacto_critic_grad,
 *               cacto_actor_grad and the data-parallel calls keep the slabs: kernel 1 there)
 *   xcd         the split GEMM's workgroups dealt by XCD: from 8 chunks on
 *   adam_nch    the smallest of 8, 16, 32, 64 that holds the chunk count, else 0 (looped) */
typedef struct {
  int32_t Bp;
  int32_t chain_tile;      /* samples per chain workgroup: 4 or 16 */
  int32_t elu;             /* 1: the elu critic's chain kernels */
  int32_t paired;
  int32_t critic_rows;
  int32_t critic_chunk;
  int32_t critic_nch;      /* chunks = slabs */
  int32_t critic_gemm;     /* 0 k_wgrad_adam (fused with Adam), 1 k_wgrad, 2 k_wgrad_big */
  int32_t critic_xcd;
  int32_t critic_adam_nch; /* the k_adam<NCH> / k_reduce<NCH> instance */
  int32_t actor_rows;
  int32_t actor_chunk;
  int32_t actor_nch;
  int32_t actor_gemm;
  int32_t actor_xcd;
  int32_t actor_adam_nch;
  int32_t xcd_tiles;       /* 1: the 16-sample chain tiles dealt to the XCD that runs their 256-row GEMM
                            * chunk (Bp / 16 a multiple of 128, both networks on 256-row chunks) */
  int32_t pair_xcds;       /* XCDs the paired 4-sample chain grid runs on; 0 above Bp = 512 and for elu */
  int32_t per_overlap;     /* 1: cacto_update_n_per may run the priority update and the next sample
                            * inside the critic's GEMM and Adam launches (critic_gemm 2, adam_nch != 0);
                            * they do when per_overlap && cacto_per_plan's overlap_shape && alpha != 0 and
                            * the pipeline orders its streams on the device */
  int32_t devwait_actor;   /* 1: the two-stream pipeline may order the actor chain after the critic's
                            * Adam with a device-side wait (16-sample tiles, Bp / 16 <= cus) */
  int32_t cus;             /* the compute-unit count the decision used */
} cacto_upd_plan;

/* sobolev: w_S != 0. CACTO_EINVAL for a null argument or B <= 0; no device work, nothing enqueued. */
int cacto_update_plan(const cacto_sys* sys, int sobolev, int B, cacto_upd_plan* out);

/* Critic gradient (flat, Keras order, summed over the B local rows with 1/B_global scaling).
 * rows: storage_d indexed by idx_d[B] (int32); is_w_d = IS weights [B] or NULL (= 1).
 * Outputs: grad_d [PC]; y_d [B] (reward_to_go), V_d [B], Vt_d [B] (if cfg->want_target_V). */
int cacto_critic_grad(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg,
                      const double* storage_d, const int32_t* idx_d, const float* is_w_d, int B,
                      float* grad_d, float* y_d, float* V_d, float* Vt_d,
                      void* workspace_d, size_t workspace_bytes, void* stream);

/* Actor gradient against the CURRENT critic (call after the critic step, RL.py:104-109). */
int cacto_actor_grad(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg,
                     const double* storage_d, const int32_t* idx_d, int B, float* grad_d,
                     void* workspace_d, size_t workspace_bytes, void* stream);

/* Keras-2.11 Adam on a flat tensor + packed copy refresh; `which` = CACTO_NET_*.
 * The iteration counter nets->step_d[which] is read and incremented on the device.
 * For the critic this also performs the soft target update when soft_update != 0. */
int cacto_adam_step(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg, int which,
                    const float* grad_d, int soft_update, void* stream);

/* target <- tau*critic + (1-tau)*target (and its packed copy) */
int cacto_soft_update(const cacto_sys* sys, const cacto_nets* nets, float tau, void* stream);

/* One full RL_AC.update + update_target (single device): critic grad -> Adam(critic) + soft
 * update -> actor grad (new critic) -> Adam(actor). */
int cacto_update(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg,
                 const double* storage_d, const int32_t* idx_d, const float* is_w_d, int B,
                 float* y_d, float* V_d, float* Vt_d, void* workspace_d, size_t workspace_bytes,
                 void* stream);

/* Diagnostic: the two-stream pipeline's device-side ordering words: out4_h[0] actor chains finished,
 * [1] 1 if a device-side wait timed out since the last cacto_pipeline_check (the waits are bounded
 * so that an ordering fault cannot hang the GPU), [2] critic Adam steps finished, [3] the handle's
 * concurrency probe: 0 not run, 1 the two streams' kernels did not run concurrently (queue markers
 * order them), 2 they did (device-side waits). Synchronizes the device. All zero before the first
 * pipelined call. */
int cacto_pipeline_status(const cacto_sys* sys, unsigned long long* out4_h);
/* Collects the two-stream pipeline's timeout latch: synchronizes `stream` (the stream the pipelined
 * calls were issued on), and if a device-side wait of any cacto_update_n[_per] call since the last
 * check timed out — its updates then ran without their cross-stream order — clears the latch and
 * returns CACTO_EINVAL (the message says so); otherwise CACTO_OK. A set latch also makes the next
 * pipelined call refuse to run until it is collected. The Python layer calls it at the end of every
 * learn_and_update and before every checkpoint save (RL.py:139-143), so no result of a timed-out
 * call leaves unflagged. Ordering: device-side waits are the default; queue markers are used while
 * the stream is being captured into a graph, when the environment serializes kernels
 * (AMD_SERIALIZE_KERNEL, HIP_LAUNCH_BLOCKING) and when a one-time probe per handle finds that the
 * two streams' kernels do not run concurrently (e.g. under counter collection);
 * CACTO_PIPE_DEVWAIT=0 / 1 forces markers / device waits. */
int cacto_pipeline_check(cacto_sys* sys, void* stream);
/* K consecutive updates on minibatch indices idx_d [K][B] (learn_and_update's loop with its
 * minibatches drawn up front, RL.py:120-143; no IS weights). Bit-identical to K cacto_update calls.
 * The critic step of update t+1 overlaps the actor step of update t (the critic step never reads
 * the actor): for batches of at most 512 the two chains run as one grid on `stream` (three launches
 * per update); larger batches use a second stream owned by the system handle, joined back into
 * `stream` before the call returns (also on error). Calls on one handle are serialised internally
 * (a mutex), so two host threads may call it, but their updates are not interleaved. */
int cacto_update_n(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg,
                   const double* storage_d, const int32_t* idx_d, int K, int B, void* workspace_d,
                   size_t workspace_bytes, void* stream);

/* The same pipeline for learn_and_update with PER (RL.py:122-137): per update, the stratified
 * sample (uniforms_d [K][B], as cacto_per_sample) -> update with IS weights -> priority update
 * (as cacto_per_update); bit-identical to the K-step sequential loop. */
int cacto_update_n_per(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg,
                       const double* storage_d, double* sum_tree_d, double* min_tree_d, int64_t capacity,
                       int64_t max_idx, double beta, const double* uniforms_d, double* exp_counter_d,
                       double fresh_factor, double eps, double alpha, double* max_priority_d, int K, int B,
                       void* workspace_d, size_t workspace_bytes, void* stream);

/* ---- R independent learners of one system (the ten-seed sets: generate_tests_set_script.py writes
 * ten `main.py --seed=...` runs per system, n_runs = 10; each runs the loop of RL.py:120-143) ----
 * cacto_update_n's paired small-batch loop for R replicas — each with its own networks, Adam state,
 * counters and replay storage, all of one system handle — as ONE chain launch and ONE weight-gradient
 * + Adam launch per step, whatever R is (K + 1 steps per call, 2 launches each). Replica r's networks,
 * moments, counters, y and V equal those of cacto_update_n run alone on replica r's inputs, bit for
 * bit: every tile runs the same device code on the same inputs, and only the dealing of tiles to
 * workgroups (cacto_ens_plan) differs. Only the paired route on 4-sample tiles is built: a sine (or,
 * in the sine-elu build, sine-elu) critic, 2 * Bp <= 1024, uniform replay, one rank. */
#define CACTO_ENSEMBLE_MAX 64 /* replicas per ensemble handle */
typedef struct cacto_ensemble cacto_ensemble;

/* reason codes of cacto_ens_plan.reason */
#define CACTO_ENS_OK 0
#define CACTO_ENS_BAD_R 1      /* R < 1 or R > CACTO_ENSEMBLE_MAX            (CACTO_EINVAL) */
#define CACTO_ENS_NOT_PAIRED 2 /* 2 * Bp > 1024: the batch is not paired     (CACTO_EUNSUPPORTED) */
#define CACTO_ENS_ELU 3        /* the elu critic (critic_type 2)             (CACTO_EUNSUPPORTED) */
#define CACTO_ENS_BAD_B 4      /* B <= 0                                     (CACTO_EINVAL) */

/* What cacto_ensemble_update launches. The 8 XCDs form xcd_groups = 8 / pair_xcds groups (pair_xcds:
 * the one-learner route's); replica r runs on group r % xcd_groups, stacked in `layers`. With R = 1
 * the workgroup counts are the one-learner route's. */
typedef struct {
  int32_t supported;
  int32_t reason;          /* CACTO_ENS_* */
  int32_t R;
  int32_t Bp;
  int32_t pair_xcds;       /* XCDs one replica's chain tiles run on */
  int32_t xcd_groups;
  int32_t layers;          /* ceil(R / xcd_groups) */
  int32_t xcds;            /* XCDs the chain launch uses */
  int32_t chain_wgs;       /* workgroups of a paired step's chain launch (steps 1 .. K - 1) */
  int32_t chain_wgs_lone;  /* ... of the first (critic alone) and last (actor alone) step's */
  int32_t chain_threads;
  int32_t chain_lds_bytes;
  int32_t wgrad_wgs;       /* workgroups of a paired step's GEMM + Adam launch */
  int32_t wgrad_wgs_critic; /* ... of the first step's */
  int32_t wgrad_wgs_actor;  /* ... of the last step's */
  int32_t wgrad_threads;
  int32_t wgrad_lds_bytes;
  int32_t launches_per_update; /* 2 (K + 1 steps of 2 launches per call of K updates) */
  int32_t cus;
} cacto_ens_plan;

/* The plan for a system of nb_state / nb_action with critic_type (0 sine, 1 sine-elu, 2 elu), sobolev
 * (w_S != 0), batch B, R replicas and `cus` compute units (<= 0: this device's, 256 without one). Needs
 * no handle and no GPU. Always fills *out; returns CACTO_OK when supported, else the code beside the
 * reason above with a message in cacto_last_error. */
int cacto_ensemble_plan(int nb_state, int nb_action, int critic_type, int sobolev, int B, int R, int cus,
                        cacto_ens_plan* out);

/* Creates the handle that owns the device table of the R replicas' descriptors (written once, here).
 * nets_h [R], storages_d [R] (each replica's replay rows), workspaces_d [R] (each workspace_bytes >=
 * cacto_workspace_bytes(sys, B), 256-byte aligned, distinct) are host arrays; what they point to, and
 * `sys`, must outlive the handle and stay where they are. cfg is copied (want_target_V must be 0).
 * Refused with CACTO_EINVAL: null arguments, R out of range, a workspace that is too small, a handle
 * with data-parallel communicators attached (cacto_dp_attach); with CACTO_EUNSUPPORTED: a batch that
 * is not paired, the elu critic. Allocates and copies (synchronous); not for use inside a capture. */
int cacto_ensemble_create(const cacto_sys* sys, int R, const cacto_nets* nets_h, const double* const* storages_d,
                          void* const* workspaces_d, size_t workspace_bytes, const cacto_update_cfg* cfg, int B,
                          cacto_ensemble** out);
/* Frees the table. The caller orders it after the handle's last update (e.g. a stream synchronise). */
int cacto_ensemble_destroy(cacto_ensemble* ens);
/* K consecutive updates of every replica. idx_d: int32 [R][K][B], replica-major — replica r's
 * minibatch of update t at idx_d + (r * K + t) * B — indexing that replica's storage. Asynchronous on
 * `stream`: kernel launches only, no host synchronisation, no allocation, nothing read from the
 * environment, so a call can be captured into a hipGraph. K == 0 is a no-op. */
int cacto_ensemble_update(cacto_ensemble* ens, const int32_t* idx_d, int K, void* stream);
/* Diagnostics (no reference counterpart; the training loop needs neither): where the paired loops
 * leave the reward-to-go y and the critic value V of their last critic step, so that a test can
 * compare them between the ensemble and the one-learner call.
 * The device addresses of replica r's y [Bp] and V [Bp] (inside its workspace). */
int cacto_ensemble_outputs(const cacto_ensemble* ens, int r, float** y_d, float** V_d);
/* Diagnostics: byte offset, in a workspace of cacto_workspace_bytes(sys, B), of the y [Bp] that
 * cacto_update_n's paired route leaves of its last critic step; V [Bp] follows it. 0 for bad
 * arguments. */
size_t cacto_workspace_yv_offset(const cacto_sys* sys, int B);

/* Data-parallel K-update loop (RL.py:101-118 per update, replaces the two blocking all-reduces of
 * learn_and_update's DP form with one per update). The host runs K + 1 steps; step t computes the
 * gradient of the critic step of update t (idx_c_d != NULL, with is_w_d / y_d / V_d as in
 * cacto_update) and of the actor step of update t - 1 (idx_a_d != NULL) into
 * grad_d [critic params | actor params] (each scaled by 1/cfg->B_global, so the exchange is a plain
 * sum), the caller all-reduces the present part(s) of grad_d once, then cacto_update_pair_apply runs
 * the Adam steps (critic with the soft target update when soft_update). The actor gradient of
 * update t - 1 is taken against the critic after its update t - 1, as in the sequential loop. */
int cacto_update_pair_grads(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg,
                            const double* storage_d, const int32_t* idx_c_d, const float* is_w_d,
                            const int32_t* idx_a_d, int B, float* grad_d, float* y_d, float* V_d,
                            void* workspace_d, size_t workspace_bytes, void* stream);
/* cacto_update_pair_grads in two stream-ordered stages, so the critic part's all-reduce can be
 * issued while the actor part is still being formed: stage 0 runs the chain(s) and writes the
 * critic gradient (when idx_c_d), stage 1 the actor's weight gradient into grad_d + P_critic (when
 * idx_a_d; a no-op otherwise). Stage 1 reads the panels stage 0 left in the workspace, so the two
 * calls take the same arguments, stage 0 first, on the same stream. Stage 0 + stage 1 = one
 * cacto_update_pair_grads call, bit for bit. */
int cacto_update_pair_grads_stage(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg,
                                  const double* storage_d, const int32_t* idx_c_d, const float* is_w_d,
                                  const int32_t* idx_a_d, int B, float* grad_d, float* y_d, float* V_d,
                                  void* workspace_d, size_t workspace_bytes, int stage, void* stream);
int cacto_update_pair_apply(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg,
                            const float* grad_d, int critic, int actor, int soft_update, void* stream);

/* Data-parallel learn_and_update over RCCL (main.py:219-225's parallelism as one process per GPU,
 * SURVEY §8e). cacto_dp_unique_ids writes n RCCL unique ids (128 bytes each) on one rank; every
 * rank then calls cacto_dp_attach with the same 2 ids (collective: it returns once all `world`
 * ranks have joined), which gives the handle one communicator per stream of the update pipeline.
 * The RCCL library is the one already loaded in the process (torch.distributed's), else
 * librccl.so.1. cacto_dp_detach releases them (cacto_sys_destroy does too). */
int cacto_dp_unique_ids(void* out_h, int n);
int cacto_dp_attach(cacto_sys* sys, const void* ids_h, int rank, int world);
int cacto_dp_detach(cacto_sys* sys);
/* K data-parallel updates (RL.py:101-118 each) on this rank's minibatch indices idx_d [K][B] (B =
 * the local batch; cfg->B_global = B * world, the gradients are scaled by 1 / B_global so the
 * exchange is a plain sum): the two-stream pipeline of cacto_update_n with each network's gradient
 * all-reduced on its own stream's communicator between its GEMM and its Adam step. Every rank
 * applies the same Adam to the same sum, so the replicas stay identical; with one rank the result
 * equals cacto_update_n bit for bit. */
int cacto_update_n_dp(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg,
                      const double* storage_d, const int32_t* idx_d, int K, int B, void* workspace_d,
                      size_t workspace_bytes, void* stream);
/* The same with PER (RL.py:122-137 on every rank's replay shard): per update this shard's (sum,
 * min, rows) exchanged over the critic stream's communicator (its row of a [world][3] table, the
 * other rows zero, sum all-reduced — the all-gather of the statistics), the stratified sample with IS
 * weights against the union (cacto_per_sample_global), the update, then this shard's priority
 * update. Arguments as cacto_update_n_per. */
int cacto_update_n_per_dp(const cacto_sys* sys, const cacto_nets* nets, const cacto_update_cfg* cfg,
                          const double* storage_d, double* sum_tree_d, double* min_tree_d, int64_t capacity,
                          int64_t max_idx, double beta, const double* uniforms_d, double* exp_counter_d,
                          double fresh_factor, double eps, double alpha, double* max_priority_d, int K, int B,
                          void* workspace_d, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- rollouts --------------- */

/* B episodes from S0_d [B,ns] (float64), each for nsteps_d[b] <= T steps:
 *   a_t = actor(s_t) (float32; zeros when use_actor == 0, i.e. ep == 0 in RL.py:224-225),
 *   s_{t+1}, r_t = Env.step(W, s_t, a_t), ee_{t+1} = EE(s_{t+1}).
 * Outputs (any may be NULL): S_traj [B,T+1,ns] f64, A_traj [B,T,na] f32, R_traj [B,T] f64,
 * EE_traj [B,T+1,3] f64. Steps past nsteps_d[b] are not written. W_d: weights [n_weights] or NULL
 * (running). status_d [B] int32 (optional): 0 ok, 1 NaN state encountered (RL.py:229-231).
 * R_traj / EE_traj are evaluated from the recorded trajectory after the sequential pass
 * (cacto_rollout_rewards), so they need S_traj (and A_traj when use_actor).
 * order_d [B] int32 (optional): a permutation of the episodes, longest first (e.g. a stable
 * argsort of -nsteps). Its ranks are dealt to the workgroups in snake order and each workgroup's
 * episode slots take them longest first as earlier episodes end, so every slot runs about the same
 * number of steps. Results do not depend on the order or on the schedule. */
int cacto_rollout(const cacto_sys* sys, const float* actor_netbuf_d, const double* S0_d,
                  const int32_t* nsteps_d, int T, int use_actor, const double* W_d,
                  double* S_traj_d, float* A_traj_d, double* R_traj_d, double* EE_traj_d,
                  int32_t* status_d, const int32_t* order_d, int B, void* stream);

/* cacto_rollout with an explicit schedule: `groups` 4-episode groups per workgroup (1, 2 or 4;
 * 0 = automatic: about two episodes per slot) or, for systems whose step needs no workgroup-wide
 * dynamics (SI, car, car_park and the prismatic DI), an 8-slot workgroup kind: -1 = two
 * independent 4-slot teams (k_rollout_tt), -3 = one slot per wave with layer 2 split over K, the
 * layer-2 weights in registers (k_rollout_ks; automatic for those systems up to two episodes per
 * slot); and `workgroups` (0 = one per CU, capped by B).
 * Same outputs as cacto_rollout for any schedule (tests use it to force slot refills and to
 * compare the kernels). */
int cacto_rollout_sched(const cacto_sys* sys, const float* actor_netbuf_d, const double* S0_d,
                        const int32_t* nsteps_d, int T, int use_actor, const double* W_d,
                        double* S_traj_d, float* A_traj_d, double* R_traj_d, double* EE_traj_d,
                        int32_t* status_d, const int32_t* order_d, int B, int groups, int workgroups,
                        void* stream);

/* Env.step's reward r_t = reward(W, s_t, a_t) (t < nsteps[b]) and EE_t = EE(s_t) (t <= nsteps[b])
 * of recorded trajectories (environment.py:70-78, :146-156): S_traj [B,T+1,ns] f64, A_traj
 * [B,T,na] f32 (ignored, a = 0, when use_actor == 0), outputs R_traj [B,T] / EE_traj [B,T+1,3] f64
 * (either may be NULL). NaN states (a dropped episode) are skipped. Fully parallel over (b, t);
 * cacto_rollout calls it when R_traj or EE_traj is requested. */
int cacto_rollout_rewards(const cacto_sys* sys, const double* S_traj_d, const float* A_traj_d,
                          const int32_t* nsteps_d, int T, int use_actor, const double* W_d,
                          double* R_traj_d, double* EE_traj_d, int B, void* stream);

/* Sobolev labels without CasADi: the DDP backward pass of TO.backward_pass
 * (TO.py:119-202) along n_ep recorded trajectories. Episode e has Te = nsteps_d[e] steps:
 *   S_traj_d [n_ep, ldS, ns] f64 (s_0..s_Te; the time column is ignored), U_traj_d [n_ep, ldU, na]
 *   f64 (u_0..u_{Te-1}), output dVdx_d [n_ep, ldS, ns] f64: V_x(s_t) for t = 0..Te, time column 0 —
 *   the layout cacto_rl_solve_add reads. mu: the Qbar_uu regulariser (1e-9 in the reference).
 *   nsteps_d[e] < 0 skips episode e (a rollout dropped for a NaN state, RL.py:229-231 /
 *   main.py:236): nothing is read or written for it.
 * The reward's derivatives are those of the TO cost (= -reward, environment_TO.py): closed forms
 * for the planar family (SI, DI, car), hyper-dual forward-mode derivatives through the forward
 * kinematics (manipulator, UR5) and the body check points (car_park). Dynamics Jacobians as
 * augmented_derivative (environment.py:111-132, :221-233, :420-435, :567-582); for revolute chains
 * ddq_dq, ddq_dv (computeABADerivatives) come from hyper-dual RNEA. Every system is supported; a
 * (dynamics, reward) combination outside the six systems returns CACTO_EUNSUPPORTED. */
int cacto_ddp_backward(const cacto_sys* sys, const double* S_traj_d, int64_t ldS, const double* U_traj_d,
                       int64_t ldU, const int32_t* nsteps_d, int n_ep, double mu, double* dVdx_d, void* stream);

/* ---------------------------------------------------------------- trajectory optimisation - */

/* TO_System_Solve (TO.py:37-100) as a batched iLQR: single shooting on the reference's problem
 * (cost = -reward with the control bounds as the penalty w_b (u/u_max)^10, environment_TO.py; the
 * environment's dynamics; fixed initial state), Gauss-Newton DDP with first-order dynamics and
 * exact cost Hessians, a backtracking line search and Levenberg-Marquardt regularisation. All
 * float64. Layouts as cacto_ddp_backward: S [n_ep, ldS, ns] with the time column, U [n_ep, ldU, na],
 * nsteps_d[e] = Te (Te + 1 states, Te controls; needs Te < ldS and Te <= ldU); Te < 0 skips episode
 * e: nothing of it is read or written. nx = ns - 1. The cost of UR5 is -reward plus the bound
 * penalty scale w6 w_b sum (u/u_max)^10 that environment_TO.py:731-758 has and UR5.reward leaves
 * to reward_batch; for the other systems it is -Env.reward. */

enum cacto_to_status {
  CACTO_TO_CONVERGED = 0, /* max_t |Q_u,t|_inf <= gtol */
  CACTO_TO_MAXITER = 1,   /* max_iter backward passes without convergence */
  CACTO_TO_FAILED = 2     /* the regulariser passed mu_max (or the warm start's cost is not finite) */
};

typedef struct {
  int32_t max_iter; /* backward passes per episode */
  int32_t max_ls;   /* step sizes alpha = 2^-j, j = 0..max_ls (<= 63) */
  double gtol;      /* convergence: max_t |Q_u,t|_inf <= gtol */
  double armijo;    /* accept when J - J(alpha) >= armijo * -(alpha dJ1 + alpha^2 dJ2) and J(alpha) <= J */
  double mu_min, mu_up, mu_down, mu_max; /* mu <- max(mu mu_up, mu_min) on failure (> mu_max: FAILED);
                                          * mu <- mu / mu_down on acceptance, 0 once below mu_min. Starts at 0. */
  int32_t poll_every; /* > 0: the host reads the finished-episode counter every so many iterations */
  int32_t path;       /* enum cacto_to_path; any other value: CACTO_EINVAL */
} cacto_to_cfg;

/* Which kernels cacto_to_solve runs; the algorithm, cost, dynamics and line-search rule are the
 * same, and for car_park, the manipulator and UR5 so is every output, bit for bit. */
enum cacto_to_path {
  CACTO_TO_PATH_DEFAULT = 0, /* single integrator, car, double integrator: one persistent kernel, one thread
                              * per episode. car_park, manipulator, UR5: a loop issued by the host */
  CACTO_TO_PATH_WAVE = 1     /* single integrator, car, double integrator, car_park: one persistent kernel,
                              * one workgroup per episode (small batches, per-episode calls); no host round
                              * trip, poll_every is not used. Manipulator, UR5: as 0 */
};

/* Per-call options of the trajectory optimiser, beside cacto_to_cfg (whose 64 bytes are fixed): the
 * `_opts` entries below take the arguments of the entry they are named after plus a pointer to
 * this struct, NULL meaning the defaults; the entries without the suffix are those calls with NULL.
 * hessian: the node Hessian l_xx the backward pass uses.
 *   CACTO_TO_HESS_EXACT  the exact Hessian of the cost (the default).
 *   CACTO_TO_HESS_PSD    its projection onto the positive semidefinite cone, P(H) = V max(L, 0) V^T
 *                        with H = V L V^T (a cyclic Jacobi iteration in float64), at every running
 *                        and terminal node, in the cost convention. With l_uu > 0 this keeps
 *                        Q_uu = l_uu + B^T V_xx B positive definite without mu where the cost is
 *                        concave (near the obstacles). l_x, l_u, l_uu, the dynamics, the line search,
 *                        the mu schedule, gtol and the statuses are untouched, so the stationary
 *                        points are the same. cacto_ddp_backward (the Sobolev labels) always uses the
 *                        exact Hessian.
 * An unknown hessian or a non-zero reserved word: CACTO_EINVAL (workspace query: 0), reported before
 * the other arguments are looked at, no device work. */
enum cacto_to_hessian { CACTO_TO_HESS_EXACT = 0, CACTO_TO_HESS_PSD = 1 };

typedef struct {
  int32_t hessian;     /* enum cacto_to_hessian */
  int32_t reserved[3]; /* must be 0 */
} cacto_to_opts;

/* Hard control limits, beside cacto_to_cfg and cacto_to_opts (both fixed): the `_box` entries below
 * take the arguments of the entry they extend plus a pointer to this struct last. NULL, or mode
 * CACTO_TO_BOUNDS_NONE (lo, hi are then not read): the call is the entry it extends — the same
 * kernels, the same numbers, the controls held only by the penalty inside the cost.
 *   CACTO_TO_BOUNDS_BOX  control-limited DDP (Tassa, Mansard, Todorov, ICRA 2014) on lo <= u <= hi:
 *     backward  Qbar_uu = Q_uu + mu I is factored first as without bounds (the same verdict, the same
 *               mu schedule); then k = argmin 1/2 x^T Qbar_uu x + Q_u^T x over lo - ubar <= x <= hi - ubar
 *               (a projected-Newton iteration in float64; one that does not finish counts as a Qbar_uu
 *               that is not positive definite; the two offsets are moved outward by one unit in the
 *               last place where ubar + offset would stop short of the bound in float64, so that the
 *               clamped full step of a clamped control is the bound itself), K = -Qbar_ff^-1 Q_ux,f on the rows of the controls the
 *               solution leaves free and exactly 0 on the clamped rows; V_x, V_xx, dJ[0], dJ[1] by the
 *               formulas above. dJ[2], the quantity gtol stops on, becomes the projected gradient: the
 *               maximum of |Q_u,j| over the nodes and the j that are not held at a bound (ubar_j == lo_j
 *               with Q_u,j > 0, or ubar_j == hi_j with Q_u,j < 0).
 *     forward   u = min(max(ubar + alpha k + K dx, lo), hi) in every roll-out, the line search's
 *               candidates and cacto_to_forward_box's open-loop roll-out included. The warm start is
 *               clamped the same way before it is rolled out, and J[0] is the clamped warm start's cost.
 *     Every control the solver returns lies in [lo, hi] exactly. The two solvers of a system agree
 *     bit for bit. The Sobolev labels take the bounds through cacto_ddp_backward_box (below);
 *     cacto_ddp_backward itself stays the reference's unconstrained dV/dx (TO.py:119-202) along any
 *     trajectory, a bounded one included.
 * An unknown mode, a non-zero reserved word, or with CACTO_TO_BOUNDS_BOX a NaN or lo[j] >= hi[j] for
 * some j < nb_action: CACTO_EINVAL "bad bounds" (workspace query: 0), no device work, reported right
 * after the options and before the other arguments; with a null system, where nb_action is not known
 * yet, entry 0 is the one checked. */
enum cacto_to_bounds { CACTO_TO_BOUNDS_NONE = 0, CACTO_TO_BOUNDS_BOX = 1 };

typedef struct {
  int32_t mode;     /* enum cacto_to_bounds */
  int32_t reserved; /* must be 0 */
  double lo[CACTO_MAX_ACTION], hi[CACTO_MAX_ACTION]; /* first nb_action entries; -inf / +inf: that side open */
} cacto_to_box;     /* 136 bytes */

/* cacto_ddp_backward under bounds: the Sobolev labels of the problem a bounded solve solved. Per
 * node, from Q_x, Q_u, Q_xx, Q_xu, Qbar_uu = Q_uu + mu I formed exactly as in cacto_ddp_backward (the
 * reward's derivatives), control j is held when it sits on or outside a limit and the gradient points
 * out of the box: u_j <= lo_j with Q_u,j < 0, or u_j >= hi_j with Q_u,j > 0 (the first-order rule of
 * the solver's stopping test in the reward's sign; no box QP, so no positive definite Qbar_uu is
 * asked for). With f the controls not held,
 *   V_x = Q_x - Q_xu[:, f] Qbar_uu[f, f]^-1 Q_u[f],  V_xx = Q_xx - Q_xu[:, f] Qbar_uu[f, f]^-1 Q_xu[:, f]^T
 * (f empty: V_x = Q_x, V_xx = Q_xx). At a stationary point of the bounded problem Q_u[f] = 0, and V_x
 * is the adjoint of the constrained problem: the gradient of its optimal cost. Along a trajectory on
 * which no control is held the output equals cacto_ddp_backward's bit for bit. Everything else (the
 * terminal row, the time column, nsteps_d[e] < 0, rows past Te, the exact cost Hessian whatever
 * Hessian the solve used, the workspace) is cacto_ddp_backward's. NULL or mode CACTO_TO_BOUNDS_NONE:
 * that call itself. Bad bounds: CACTO_EINVAL "bad bounds" before the other arguments are looked at,
 * no device work. */
int cacto_ddp_backward_box(const cacto_sys* sys, const double* S_traj_d, int64_t ldS, const double* U_traj_d,
                           int64_t ldU, const int32_t* nsteps_d, int n_ep, double mu, double* dVdx_d, void* stream,
                           const cacto_to_box* box);

/* One regularised backward pass along given trajectories (cost convention, l_xu = 0):
 *   Qbar_uu = Q_uu + mu I, k = -Qbar_uu^-1 Q_u, K = -Qbar_uu^-1 Q_ux,
 *   V_x = Q_x + K^T Q_uu k + K^T Q_u + Q_ux^T k, V_xx = Q_xx + K^T Q_uu K + K^T Q_ux + Q_ux^T K
 *   (symmetrised); terminal node: terminal weights at S[Te].
 * k_d [n_ep, ldU, na], K_d [n_ep, ldU, na, nx]; dJ_d [n_ep, 3] = (sum k^T Q_u, 1/2 sum k^T Q_uu k,
 * max_t |Q_u,t|_inf) with the unregularised Q_uu; pd_d [n_ep] int32 = -1 when Qbar_uu was positive
 * definite at every step, else the step at which its Cholesky met a pivot <= 0 or a non-finite one
 * (the pass stops there: gains below that step and dJ are undefined). */
int cacto_to_backward_gains(const cacto_sys* sys, const double* S_d, int64_t ldS, const double* U_d, int64_t ldU,
                            const int32_t* nsteps_d, int n_ep, double mu, double* k_d, double* K_d, double* dJ_d,
                            int32_t* pd_d, void* stream);
int cacto_to_backward_gains_opts(const cacto_sys* sys, const double* S_d, int64_t ldS, const double* U_d, int64_t ldU,
                                 const int32_t* nsteps_d, int n_ep, double mu, double* k_d, double* K_d, double* dJ_d,
                                 int32_t* pd_d, void* stream, const cacto_to_opts* opts);
/* ... under bounds (cacto_to_box): U_d is the nominal control the box is taken around; dJ_d[2] is
 * the projected gradient. */
int cacto_to_backward_gains_box(const cacto_sys* sys, const double* S_d, int64_t ldS, const double* U_d, int64_t ldU,
                                const int32_t* nsteps_d, int n_ep, double mu, double* k_d, double* K_d, double* dJ_d,
                                int32_t* pd_d, void* stream, const cacto_to_opts* opts, const cacto_to_box* box);

/* One closed-loop roll-out: u_t = ubar_t + alpha k_t + K_t (x_t - xbar_t), x_{t+1} = Env.simulate
 * (float64). S_new_d [n_ep, ldS, ns] (time column t0 + dt t), U_new_d [n_ep, ldU, na], cost_new_d
 * [n_ep, ldS]: running cost at nodes 0..Te-1, terminal cost at node Te (TO_step_cost, TO.py:84-89).
 * S_new_d / U_new_d may be S_d / U_d (in place). k_d, K_d NULL: the open-loop roll-out of U_d. */
int cacto_to_forward(const cacto_sys* sys, const double* S_d, int64_t ldS, const double* U_d, int64_t ldU,
                     const double* k_d, const double* K_d, const int32_t* nsteps_d, int n_ep, double alpha,
                     double* S_new_d, double* U_new_d, double* cost_new_d, void* stream);
/* ... with every control clamped to the bounds before it is applied (cacto_to_box). */
int cacto_to_forward_box(const cacto_sys* sys, const double* S_d, int64_t ldS, const double* U_d, int64_t ldU,
                         const double* k_d, const double* K_d, const int32_t* nsteps_d, int n_ep, double alpha,
                         double* S_new_d, double* U_new_d, double* cost_new_d, void* stream, const cacto_to_box* box);

/* Workspace of cacto_to_solve: for cfg.path = CACTO_TO_PATH_DEFAULT, and for the path of a given
 * config (CACTO_TO_PATH_WAVE adds the per-node derivative records of the closed-form family; for
 * car_park it keeps gains and records per episode and no solver state).
 * 0 on bad arguments or an unknown path. */
size_t cacto_to_workspace_bytes(const cacto_sys* sys, int n_ep, int64_t ldS);
size_t cacto_to_workspace_bytes_cfg(const cacto_sys* sys, int n_ep, int64_t ldS, const cacto_to_cfg* cfg_h);
/* ... for a config (cfg_h NULL: CACTO_TO_PATH_DEFAULT) and options. The projection of
 * CACTO_TO_HESS_PSD works in place, so the size does not depend on the Hessian mode. */
size_t cacto_to_workspace_bytes_opts(const cacto_sys* sys, int n_ep, int64_t ldS, const cacto_to_cfg* cfg_h,
                                     const cacto_to_opts* opts);
/* ... and bounds: the box QP needs no memory, so the size does not depend on them (0 on bad bounds). */
size_t cacto_to_workspace_bytes_box(const cacto_sys* sys, int n_ep, int64_t ldS, const cacto_to_cfg* cfg_h,
                                    const cacto_to_opts* opts, const cacto_to_box* box);

/* The solver. S0_d [n_ep, ns] initial states (with time), U_init_d [n_ep, ldU, na] warm start.
 * Outputs: S_d [n_ep, ldS, ns], U_d [n_ep, ldU, na], step_cost_d [n_ep, ldS], status_d [n_ep] int32
 * (cacto_to_status), iters_d [n_ep] int32 (backward passes used), J_d [n_ep, 2] = (cost of the warm
 * start's roll-out, final cost; J[1] <= J[0]). Rows past Te are untouched. Te == 0: S[0] = s0, its
 * terminal cost, CONVERGED, 0 iterations. Requires w_terminal[6] == 0 (CACTO_EUNSUPPORTED otherwise;
 * true of every shipped conf). ws_d: cacto_to_workspace_bytes_cfg(sys, n_ep, ldS, cfg_h) bytes
 * (path 0: cacto_to_workspace_bytes). ldU <= ldS.
 * Single integrator, car, double integrator: one persistent kernel, no host round trip (poll_every
 * is not used): one thread per episode, or with cfg.path = CACTO_TO_PATH_WAVE one 64-lane workgroup
 * per episode (derivatives over the nodes, every step size of the line search at once).
 * car_park, manipulator, UR5, path 0: max_iter iterations of derivative kernels + a
 * one-wave-per-episode backward pass + a line-search kernel, issued by the host; poll_every > 0
 * stops issuing once every episode has finished (see Conventions). car_park with cfg.path =
 * CACTO_TO_PATH_WAVE: one persistent kernel, one workgroup of 256 threads per episode running the
 * same device functions (derivatives over the nodes, the backward pass over all its waves, every
 * step size at once) — the same outputs bit for bit, no host round trip, nothing synchronised,
 * poll_every not used. The manipulator and UR5 run the host-issued loop under either path. */
int cacto_to_solve(const cacto_sys* sys, const double* S0_d, const double* U_init_d, int64_t ldU,
                   const int32_t* nsteps_d, int n_ep, int64_t ldS, const cacto_to_cfg* cfg_h, double* S_d,
                   double* U_d, double* step_cost_d, int32_t* status_d, int32_t* iters_d, double* J_d, void* ws_d,
                   size_t ws_bytes, void* stream);
/* ... with options. CACTO_TO_HESS_PSD: the persistent kernels are instantiated once more with the
 * projection in their derivative phase (the two solvers of a system still agree bit for bit); the
 * host-issued loop runs one more kernel per iteration, over the l_xx blocks of the records. */
int cacto_to_solve_opts(const cacto_sys* sys, const double* S0_d, const double* U_init_d, int64_t ldU,
                        const int32_t* nsteps_d, int n_ep, int64_t ldS, const cacto_to_cfg* cfg_h, double* S_d,
                        double* U_d, double* step_cost_d, int32_t* status_d, int32_t* iters_d, double* J_d, void* ws_d,
                        size_t ws_bytes, void* stream, const cacto_to_opts* opts);
/* ... under bounds (cacto_to_box): every solving kernel is instantiated once more per bounds mode,
 * so the unbounded kernels carry no trace of the box QP; the launches and the workspace are the same. */
int cacto_to_solve_box(const cacto_sys* sys, const double* S0_d, const double* U_init_d, int64_t ldU,
                       const int32_t* nsteps_d, int n_ep, int64_t ldS, const cacto_to_cfg* cfg_h, double* S_d,
                       double* U_d, double* step_cost_d, int32_t* status_d, int32_t* iters_d, double* J_d, void* ws_d,
                       size_t ws_bytes, void* stream, const cacto_to_opts* opts, const cacto_to_box* box);

/* What cacto_to_solve runs for a system and a config (the role cacto_rollout_plan plays for the
 * rollout: TO.py:37-100 has one host-side IPOPT call per episode and nothing to plan), so a
 * caller can tell before capturing a call into a hipGraph whether it is one kernel. */
typedef struct {
  int32_t on_device;         /* 1: the whole iteration loop runs in one kernel, no host round trip and
                              * no synchronisation (poll_every is not used) */
  int32_t block_threads;     /* threads per workgroup of the solving kernel (on_device == 0: of the
                              * one-wave-per-episode backward pass of the host-issued loop) */
  int32_t lds_bytes;         /* that kernel's static LDS */
  int32_t launches_per_iter; /* kernel launches the host issues per iteration; 0 when on_device */
} cacto_to_plan;

/* CACTO_EINVAL for a null argument or an unknown cfg_h->path; no device work, nothing enqueued. */
int cacto_to_solve_plan(const cacto_sys* sys, const cacto_to_cfg* cfg_h, cacto_to_plan* out);
/* ... with options: CACTO_TO_HESS_PSD adds one launch to launches_per_iter of a host-issued loop. */
int cacto_to_solve_plan_opts(const cacto_sys* sys, const cacto_to_cfg* cfg_h, cacto_to_plan* out,
                             const cacto_to_opts* opts);
/* ... and bounds, which change nothing of the plan. */
int cacto_to_solve_plan_box(const cacto_sys* sys, const cacto_to_cfg* cfg_h, cacto_to_plan* out,
                            const cacto_to_opts* opts, const cacto_to_box* box);

/* Multi-start solves (no reference counterpart): every episode is solved from n_starts candidate warm
 * starts in ONE cacto_to_solve over n_starts * n_ep episodes, and the best acceptable candidate is
 * kept. cacto_to_starts builds that batch, cacto_to_select reduces its solution to the n_ep-shaped
 * outputs cacto_to_solve writes. Both enqueue one kernel on the given stream, synchronise nothing and
 * read nothing back. The layout of every `_all` array is candidate-major: candidate c of episode e is
 * row c * n_ep + e, so rows [0, n_ep) are the caller's own batch. */
#define CACTO_TO_STARTS_MAX 16

/* S0_all_d [n_starts n_ep, ns] and nsteps_all_d [n_starts n_ep] are S0_d and nsteps_d tiled.
 * U_all_d [n_starts n_ep, ldU, na], for every t < ldU and k < na (whatever nsteps_d says):
 *   candidate 0             U_init_d[e, t, k], the same bits;
 *   candidate 1             0.0 when zero_start != 0 (a caller whose warm start is zero already passes
 *                           zero_start = 0, and candidate 1 is then a perturbation like the rest);
 *   every other candidate   U_init_d[e, t, k] + s_k * xi, s_k = sigma * half_range_h[k] (a host array of
 *                           na doubles, each finite and >= 0), two roundings: the product xi s_k, then
 *                           the sum (the library is built with -ffp-contract=off).
 * xi is uniform in [-1, 1) and constant over blocks of `hold` steps, block = t / hold (a perturbation
 * that is smooth in t moves the trajectory; white noise averages out). It comes from a counter-based
 * generator in 64-bit integer arithmetic, every operation modulo 2^64:
 *   mix(z):  z += 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *            z = (z ^ (z >> 27)) * 0x94D049BB133111EB; return z ^ (z >> 31)          (splitmix64)
 *   packed = e * 2^31 + block * 2^7 + c * 2^3 + k      (e < 2^31, block < 2^24, c < 16, k < 8)
 *   h      = mix(mix(seed) ^ packed)
 *   xi     = (double)(h >> 11) * 2^-52 - 1.0           (53 bits: exact)
 * so an element depends on (seed, e, c, block, k) alone: not on n_ep, n_starts or the launch. No host
 * random number is drawn.
 * CACTO_EINVAL, nothing enqueued: a null pointer; n_starts outside [1, CACTO_TO_STARTS_MAX]; hold < 1;
 * sigma negative or not finite; n_ep <= 0; ldU outside [1, 2^24); a bad half_range_h entry. */
int cacto_to_starts(const cacto_sys* sys, const double* S0_d, const double* U_init_d, int64_t ldU,
                    const int32_t* nsteps_d, int n_ep, int n_starts, double sigma, int hold,
                    const double* half_range_h, int zero_start, uint64_t seed, double* S0_all_d, double* U_all_d,
                    int32_t* nsteps_all_d, void* stream);

/* The `_all` inputs are cacto_to_solve's outputs over the n_starts * n_ep rows cacto_to_starts laid
 * out (S [.., ldS, ns], U [.., ldU, na], step_cost [.., ldS], status, iters, J [.., 2]); nsteps_d [n_ep]
 * are the caller's lengths. Per episode e with Te = nsteps_d[e]:
 *   acceptable  candidate c is acceptable when its status is CACTO_TO_CONVERGED, or CACTO_TO_MAXITER
 *               with accept_maxiter != 0, AND its final cost J_all[c n_ep + e, 1] is finite;
 *   winner      the acceptable candidate with the lowest final cost, the lowest index among equal
 *               costs; candidate 0 when none is acceptable (the episode then fares as it does with
 *               one start);
 *   outputs     S_d[e, 0..Te], U_d[e, 0..Te-1], step_cost_d[e, 0..Te], status_d[e], iters_d[e] are the
 *               winner's; J_d[e, 0] = J_all[e, 0], the cost of candidate 0's warm start (the caller's
 *               own warm start, whoever wins), J_d[e, 1] the winner's final cost. Rows past Te keep
 *               what the outputs held;
 *   extras      start_d[e] = the winner's index, n_ok_d[e] = the number of acceptable candidates,
 *               J_starts_d[e, c] = J_all[c n_ep + e, 1], status_starts_d[e, c] = status_all[c n_ep + e]
 *               ([n_ep, n_starts] each).
 * Te < 0 (a skipped episode; also a Te that does not fit ldS / ldU): none of the six outputs is
 * written, start_d[e] = -1, n_ok_d[e] = 0, and J_starts_d / status_starts_d hold what the `_all`
 * arrays held. These are cacto_to_solve's own masking rules, so with n_starts = 1 the outputs are a
 * copy of the inputs' live parts. The outputs must not overlap the inputs.
 * CACTO_EINVAL, nothing enqueued: a null pointer; n_starts outside [1, CACTO_TO_STARTS_MAX];
 * n_ep <= 0; ldS <= 0; ldU <= 0. */
int cacto_to_select(const cacto_sys* sys, const double* S_all_d, const double* U_all_d,
                    const double* step_cost_all_d, const int32_t* status_all_d, const int32_t* iters_all_d,
                    const double* J_all_d, const int32_t* nsteps_d, int n_ep, int n_starts, int64_t ldS, int64_t ldU,
                    int accept_maxiter, double* S_d, double* U_d, double* step_cost_d, int32_t* status_d,
                    int32_t* iters_d, double* J_d, int32_t* start_d, int32_t* n_ok_d, double* J_starts_d,
                    int32_t* status_starts_d, void* stream);

/* What cacto_rollout_sched runs for B episodes under a schedule (groups, workgroups), decided by the
 * same function that launches it. "eight" = the systems whose step needs no workgroup-wide dynamics
 * (SI, car, car_park, the prismatic DI), "planar" = a planar 3-joint chain (the manipulator), CUs =
 * the device's compute units, per = B / (8 CUs):
 *   groups -3: eight or planar -> kind 2;  -1: eight -> kind 1;  any other system: CACTO_EINVAL
 *   groups 1, 2, 4: kind 0 with that many slot groups
 *   groups 0: planar -> kind 2; eight with B <= 16 CUs -> kind 2; else the prismatic chain with
 *             per == 2 -> kind 1; else kind 0 with per >= 4 ? 4 : per >= 2 ? 2 : 1 slot groups
 *   workgroups 0 -> one per CU; always clamped to [1, ceil(B / (4 groups))] */
typedef struct {
  int32_t kind;          /* 0 single team (k_rollout), 1 two teams (k_rollout_tt), 2 one slot per wave
                          * (k_rollout_ks) */
  int32_t groups;        /* groups of 4 episode slots per workgroup (kinds 1 and 2: 2) */
  int32_t workgroups;    /* the grid */
  int32_t block_threads; /* threads per workgroup */
  int32_t lds_bytes;     /* the kernel's static LDS */
  int32_t cus;           /* the compute-unit count the decision used */
} cacto_ro_plan;

/* CACTO_EINVAL for a null argument, B < 0 or a schedule the system does not accept; no device work,
 * nothing enqueued. */
int cacto_rollout_plan(const cacto_sys* sys, int B, int groups, int workgroups, cacto_ro_plan* out);

/* ---------------------------------------------------------------- replay ------------------ */

/* rows_d [n, 3ns+3] f64 written at ring position next_idx (wraps modulo capacity). */
int cacto_buffer_add(const cacto_sys* sys, double* storage_d, int64_t capacity, int64_t next_idx,
                     const double* rows_d, int64_t n, void* stream);

/* RL_Solve (RL.py:145-189) for n_ep episodes, rows written straight into the ring as
 * buffer.add(state_arr, partial_reward_to_go_arr, state_next_rollout_arr, dVdx, done_arr, term_arr)
 * does after it (main.py:240). Episode e has Te = row_off_d[e+1] - row_off_d[e] - 1 steps
 * (NSTEPS_SH), 0 <= Te <= max_T, and its Te+1 rows go to ring slots
 * (next_idx + row_off_d[e] + i) % capacity; total_rows = row_off_d[n_ep] <= capacity.
 *   S_traj_d [n_ep, ldS, ns] f64: s_0..s_Te (ldS >= max_T+1; the cacto_rollout layout with T = max_T)
 *   R_d [n_ep, ldR] f64: rwrd_arr r_0..r_Te, or r_0..r_{Te-1} when R_term_d [n_ep] (f64) gives r_Te
 *     (env_RL: RL.py:160-165); pass -TO_step_cost for env_RL = 0 (RL.py:167)
 *   dVdx_d [n_ep, ldS, ns] f64 or NULL (zeros)
 *   nsteps_td = conf.nsteps_TD_N, mc = conf.MC
 *   total_d [n_ep, ldS] f64 or NULL: total_reward_to_go_arr.
 * Partial/total reward-to-go are Python's left-to-right sums rounded to float32, bit-exact. */
int cacto_rl_solve_add(const cacto_sys* sys, const double* S_traj_d, int64_t ldS, const double* R_d,
                       int64_t ldR, const double* R_term_d, const double* dVdx_d, const int64_t* row_off_d,
                       int n_ep, int max_T, int64_t total_rows, int nsteps_td, int mc, double* storage_d,
                       int64_t capacity, int64_t next_idx, double* total_d, void* stream);

/* The sample-collection stage (compute_sample, main.py:174-195, for every initial state of an
 * iteration, and the buffer.add of main.py:240). These three take the caller's stream, enqueue one
 * kernel each and synchronise nothing; a bad argument is reported before anything is enqueued.
 *
 * cacto_env_rl_episodes — RL_Solve with env_RL = 1 (RL.py:157-165) for n_ep episodes, one thread per
 * episode. With Te = nsteps_d[e]: S[e,0] = S0_d[e], EE[e,0] = EE(s_0); for t < Te
 * S[e,t+1], R[e,t] = Env.step(cost_weights_running, S[e,t], U_d[e,t]) and EE[e,t+1] = EE(S[e,t+1]);
 * R[e,Te] = reward(cost_weights_terminal, S[e,Te]) with no action. The device functions are those of
 * cacto_env_step, so the numbers equal Te calls of it plus cacto_env_ee bit for bit.
 *   S0_d [n_ep, ns], U_d [n_ep, ldU, na], nsteps_d [n_ep]; S_d [n_ep, ldS, ns], R_d [n_ep, ldS],
 *   EE_d [n_ep, ldS, 3] (all f64; any output may be NULL). Needs Te < ldS and Te <= ldU.
 * Te < 0 skips the episode (nothing read or written); rows past Te are untouched; Te == 0 writes
 * row 0 only. */
int cacto_env_rl_episodes(const cacto_sys* sys, const double* S0_d, const double* U_d, int64_t ldU,
                          const int32_t* nsteps_d, int n_ep, int64_t ldS, double* S_d, double* R_d, double* EE_d,
                          void* stream);

/* The filter of main.py:181-187 and :236 with the row offsets cacto_rl_solve_add reads.
 * kept_d[e] = nsteps_d[e] when nsteps_d[e] > 0 (RL.py:206-207), the roll-out status is 0
 * (RL.py:229-231; rollout_status_d NULL: every roll-out counts as clean) and the TO status is
 * CACTO_TO_CONVERGED, or CACTO_TO_MAXITER with accept_maxiter (to_status_d NULL: every solve counts as
 * a success); otherwise -1. row_off_d [n_ep + 1]: the exclusive prefix sum, in episode order, of
 * kept + 1 over kept episodes and 0 over dropped ones (a dropped episode has an empty row range).
 * counts_d [8] = rows, kept, episodes with nsteps <= 0, NaN roll-outs (of those with nsteps > 0),
 * CONVERGED, MAXITER, FAILED (of those that reached the solver: nsteps > 0 and a clean roll-out), 0.
 * One workgroup, any n_ep >= 1. */
int cacto_collect_plan(const int32_t* nsteps_d, const int32_t* rollout_status_d, const int32_t* to_status_d,
                       int accept_maxiter, int n_ep, int32_t* kept_d, int64_t* row_off_d, int64_t* counts_d,
                       void* stream);

/* ep_return = sum(rwrd_arr) (main.py:190 / RL.py:188): ret_d[e] = 0.0 + x_0 + ... + x_Te added left to
 * right, Te = kept_d[e] (needs Te < ldR), x_t = R_d[e, t], or -R_d[e, t] with negate (pass
 * TO_step_cost for env_RL = 0: RL.py:167 negates each element first). ret_d[e] = 0 for kept_d[e] < 0.
 * One thread per episode. */
int cacto_episode_returns(const double* R_d, int64_t ldR, const int32_t* kept_d, int n_ep, int negate,
                          double* ret_d, void* stream);

/* The validation stage: the critic and the actor against the trajectories of an iteration's freshly
 * drawn initial states, before learn_and_update has seen them (no reference counterpart). Columns of
 * per_ep_d / totals_d: */
#define CACTO_VAL_ROWS 0     /* Te + 1 */
#define CACTO_VAL_SUM_G 1    /* sum_t G_t */
#define CACTO_VAL_SUM_G2 2   /* sum_t G_t^2 */
#define CACTO_VAL_SUM_V 3    /* sum_t V_t */
#define CACTO_VAL_SSE_V 4    /* sum_t (V_t - G_t)^2 */
#define CACTO_VAL_SSE_G 5    /* sum_t sum_{j < ns-1} (g_tj - l_tj)^2 */
#define CACTO_VAL_SUM_L2 6   /* sum_t sum_{j < ns-1} l_tj^2 */
#define CACTO_VAL_SSE_CLOG 7 /* sum_t sum_{j < ns-1} (clog(g_tj) - clog(l_tj))^2 */
#define CACTO_VAL_SSE_U 8    /* + j, j < nb_action: sum_{t < Te} (a_tj - u_tj)^2; the rest 0 */
#define CACTO_VAL_COLS 16    /* CACTO_VAL_SSE_U + CACTO_MAX_ACTION */
/* With Te = kept_d[e] (Te < 0: nothing of episode e is read, its per_ep row is all zero) and
 * kept_d, row_off_d, total_rows exactly what cacto_collect_plan produced:
 *   1. the live rows S_traj_d[e, t], t = 0..Te, are cast to float32 as NN.eval casts them and written
 *      at row row_off_d[e] + t of a compact [total_rows, ns] matrix in the workspace;
 *   2. G_t, the reward-to-go, in float64 by the backward recursion G_Te = r_Te, G_t = r_t + G_{t+1},
 *      r_t = R_d[e, t], or -R_d[e, t] with negate (pass TO_step_cost with negate = 1 for env_RL = 0, as
 *      for cacto_episode_returns). This is a NEW quantity: it is not RL_Solve's total_reward_to_go,
 *      which is a left-to-right sum rounded to float32 (cacto_rl_solve_add's total_d);
 *   3. V_t and g_t = dV/ds(s_t) by cacto_critic_input_grad's launcher and a_t by cacto_actor_forward's
 *      on the compact matrix (in chunks of 2^24 rows): bit for bit what those entries give on the same
 *      float32 rows;
 *   4. per_ep_d [n_ep, CACTO_VAL_COLS]: the sums named above in float64, l = dVdx_d[e, t] (the Sobolev
 *      labels, [n_ep, ldS, ns]), clog = custom_logarithm (NeuralNetwork.py:140-148) in float64, the
 *      components j < ns - 1 as compute_critic_grad takes them (NeuralNetwork.py:168), u = U_traj_d[e, t]
 *      ([n_ep, ldU, na]). One wave per episode: lane i adds the terms of t = i, i + 64, ... within
 *      1024-step chunks taken last chunk first, and the lanes' partial sums are combined pairwise
 *      (lane distance 32, 16, .., 1), so a row depends on its episode alone;
 *   5. totals_d [CACTO_VAL_COLS] = 0.0 + per_ep[0] + per_ep[1] + ... left to right in episode order.
 * Two runs on the same inputs give the same bits, and so do the same episodes inside a larger batch
 * whose other episodes are dropped.
 * dVdx_d, critic_netbuf_d and actor_netbuf_d may each be NULL: that part is skipped and its columns
 * are 0 (SSE_G and SSE_CLOG need the labels and the critic, SUM_L2 the labels alone). Needs Te < ldS,
 * Te <= ldU, Te < ldR and row_off_d[e] + Te + 1 <= total_rows; an episode that violates this is not
 * read and its per_ep row (and so the totals) is NaN. workspace_d: cacto_validate_workspace_bytes(sys,
 * total_rows) bytes (0 for a null handle or total_rows < 0). Stream-ordered, no synchronisation; five
 * launches per 2^24 rows, whatever n_ep; total_rows == 0 only zeroes the two outputs. CACTO_EINVAL,
 * before anything is enqueued: a null required argument, n_ep < 1, total_rows < 0, a leading dimension
 * < 1, a workspace that is too small. This stage is bound by launch and memory latency (a few tens of
 * thousands of rows), not by throughput. */
size_t cacto_validate_workspace_bytes(const cacto_sys* sys, int64_t total_rows);
int cacto_validate(const cacto_sys* sys, const float* critic_netbuf_d, const float* actor_netbuf_d,
                   const double* S_traj_d, int64_t ldS, const double* U_traj_d, int64_t ldU, const double* R_d,
                   int64_t ldR, int negate, const double* dVdx_d, const int32_t* kept_d, const int64_t* row_off_d,
                   int n_ep, int64_t total_rows, double* per_ep_d, double* totals_d, void* workspace_d,
                   size_t workspace_bytes, void* stream);

/* replay_buffer.py:47-61: S, R, S_next, dVdx, d as float32, term float64; any may be NULL. */
int cacto_buffer_gather(const cacto_sys* sys, const double* storage_d, const int32_t* idx_d, int B,
                        float* S_d, float* R_d, float* S_next_d, float* dVdx_d, float* d_d, double* term_d,
                        void* stream);

/* Prioritized replay. Trees are float64 arrays of 2*capacity (capacity a power of two), node 1 =
 * root, leaves at [capacity, 2*capacity) — the layout of segment_tree.py:33. */
int cacto_per_init(double* sum_tree_d, double* min_tree_d, int64_t capacity, void* stream);
/* Set leaves [start, start+n) (mod ring_size) to `value` and refresh ancestors (replay_buffer.py:133-135). */
int cacto_per_set_range(double* sum_tree_d, double* min_tree_d, int64_t capacity, int64_t ring_size,
                        int64_t start, int64_t n, double value, void* stream);
/* The same with the value max_priority_d[0] ** alpha read on the device (what ReplayBuffer.add sets new
 * leaves to, replay_buffer.py:133-135), so adding episodes needs no host read of max_priority. The
 * device pow may differ from the host libm pow the reference uses by an ulp; the Python layer
 * computes the power on the host and calls cacto_per_set_range. */
int cacto_per_set_range_max(double* sum_tree_d, double* min_tree_d, int64_t capacity, int64_t ring_size,
                            int64_t start, int64_t n, const double* max_priority_d, double alpha, void* stream);
/* Stratified proportional sampling (replay_buffer.py:139-188). uniforms_d [B] = random.random()
 * draws. Outputs idx_d [B] int32, is_w_d [B] float32 (IS weights), and exp_counter_d (float64
 * [ring]) incremented once per distinct index. */
int cacto_per_sample(const double* sum_tree_d, const double* min_tree_d, int64_t capacity, int64_t max_idx,
                     double beta, const double* uniforms_d, int B, int32_t* idx_d, float* is_w_d,
                     double* exp_counter_d, void* stream);
/* Which PER kernels a sample of B and a priority update of B run on a tree of `capacity` leaves (the
 * role cacto_update_plan plays for the update calls): a function of capacity and B alone, decided by
 * the one function every PER entry and the pipelined loops read. With sub = min(1024, capacity) and
 * roots = capacity / sub:
 *   sampler         0 for B < 512: one workgroup, a 1,024-node top staged in LDS, the exp_counter
 *                   increment inside; 1 from there on: ceil(B / 256) workgroups, an 8,192-node top,
 *                   the increment as its own launch
 *   count_deferred  1 (B >= 512): cacto_update_n[_per] leave the sampler's increment to the priority
 *                   update, its only reader
 *   update          1 for B >= 512 && roots <= 1024: one launch over the subtrees; 0 for B < 512 or
 *                   roots > 2048: one workgroup; else 2 (capacity 2^21): leaves, subtrees, top as
 *                   three launches
 *   overlap_shape   1 for B >= 512 && 512 <= capacity <= 65536: see cacto_upd_plan.per_overlap */
struct cacto_per_plan {
  int32_t sampler;
  int32_t sampler_top;     /* nodes of the sum tree the sampler stages in LDS */
  int32_t sampler_wgs;
  int32_t count_deferred;
  int32_t update;
  int32_t update_sub;      /* leaves per subtree */
  int32_t update_roots;
  int32_t overlap_shape;
};
/* CACTO_EINVAL for a null out, a capacity that is no power of two or B outside [1, 8192]; no device
 * work, nothing enqueued. (The struct has no typedef: in C a typedef could not share the entry's name.) */
int cacto_per_plan(int64_t capacity, int B, struct cacto_per_plan* out);
/* cacto_per_sample[_global] by the sampler of the overlapped loop at any B: one sample per thread over
 * ceil(B / 256) workgroups with a 4,096-node top. shard_stats_d / n_shards: as cacto_per_sample_global,
 * or NULL / 0. runs_d (2 * capacity / 256 int32, or NULL; needs capacity >= 512): on entry
 * PER_RUN_EMPTY = 0x7f7f7f7f in the first half and 0 in the second; on return runs_d[s] is the first
 * sample index and runs_d[capacity / 256 + s] the sample count of the 256-leaf subtree s, untouched
 * subtrees keeping the fill. Indices, weights and counters equal cacto_per_sample's bit for bit. */
int cacto_per_sample_runs(const double* sum_tree_d, const double* min_tree_d, int64_t capacity, int64_t max_idx,
                          double beta, const double* uniforms_d, int B, int32_t* idx_d, float* is_w_d,
                          double* exp_counter_d, int32_t* runs_d, const double* shard_stats_d, int n_shards,
                          void* stream);
/* Data-parallel PER: stats_d [3] = (total sum, min leaf, max_idx) of this shard,
 * for an all-gather into shard_stats_d [n_shards, 3]. cacto_per_sample_global then samples B
 * stratified indices from the local tree exactly as cacto_per_sample, with IS weights taken
 * against the union of the shards: w = (N p_i / (G T_g))^-beta / (N min_h(m_h/T_h) / G)^-beta,
 * N = sum of the shards' max_idx, T_g / m_g this shard's sum / min. With one shard the weights
 * equal cacto_per_sample's bit for bit. */
int cacto_per_shard_stats(const double* sum_tree_d, const double* min_tree_d, int64_t max_idx, double* stats_d,
                          void* stream);
int cacto_per_sample_global(const double* sum_tree_d, const double* min_tree_d, int64_t capacity, int64_t max_idx,
                            double beta, const double* uniforms_d, int B, const double* shard_stats_d,
                            int n_shards, int32_t* idx_d, float* is_w_d, double* exp_counter_d, void* stream);
/* update_priorities 'PER' (replay_buffer.py:190-218): p = fresh^count*|y-V| + eps; leaves p^alpha,
 * duplicates last-write-wins; max_priority_d[0] = max(max_priority, p). */
int cacto_per_update(double* sum_tree_d, double* min_tree_d, int64_t capacity, const int32_t* idx_d,
                     const float* y_d, const float* V_d, const double* exp_counter_d, double fresh_factor,
                     double eps, double alpha, double* max_priority_d, int B, void* stream);
/* update_priorities 'ReLO' (replay_buffer.py:193-196): td = (V - y)^2 - (V_tgt - y)^2 in f32 (Keras
 * MeanSquaredError, reduction NONE), clipped as np.clip(td, 0, max(td)); p = fresh^count * td + eps
 * in f64; leaves p^alpha (duplicates last-write-wins), max_priority_d[0] = max(max_priority, p).
 * leaves_ws_d: B doubles of caller workspace. Replaces PrioritizedReplayBuffer.update_priorities
 * with RB_type == 'ReLO'. The reference asserts p > 0 for every sample (replay_buffer.py:212): when
 * some p <= 0 (every td negative) or is NaN (any td NaN), *status_d is set to 1 and the trees,
 * counters and max_priority are left unchanged; a set status makes later calls no-ops until the
 * caller clears it (the host raises the reference's AssertionError). status_d: one device int32. */
int cacto_per_update_relo(double* sum_tree_d, double* min_tree_d, int64_t capacity, const int32_t* idx_d,
                          const float* y_d, const float* V_d, const float* Vt_d, const double* exp_counter_d,
                          double fresh_factor, double eps, double alpha, double* max_priority_d, double* leaves_ws_d,
                          int32_t* status_d, int B, void* stream);
/* Set arbitrary leaves (already raised to alpha) and refresh ancestors; duplicates last-write-wins. */
int cacto_per_set_leaves(double* sum_tree_d, double* min_tree_d, int64_t capacity, const int32_t* idx_d,
                         const double* values_d, int n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CACTO_HIP_H */
