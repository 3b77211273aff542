// The kernels of the sample-collection stage (main.py:174-243 for every initial state of an
// iteration at once): the env_RL re-simulation of whole episodes, the filter of failed episodes
// with the ring offsets of the kept ones, the episode returns, and the optional validation stage
// (the learner's critic and actor against the kept trajectories before they are trained on).
#include "internal.h"

namespace cacto {

// RL.py:157-165 for a batch: one thread per episode, sequential in t, calling the device functions
// k_env_step calls (env_simulate / env_reward / env_ee, float64), so every number equals what Te
// cacto_env_step launches and cacto_env_ee give. An episode whose Te does not fit ldS / ldU violates
// the documented precondition and writes nothing.
template <int NJ>
__global__ void __launch_bounds__(64) k_env_rl_episodes(const SysDevice* __restrict__ sdp,
                                                        const double* __restrict__ S0, const double* __restrict__ U,
                                                        int64_t ldU, const int32_t* __restrict__ nsteps, int n_ep,
                                                        int64_t ldS, double* __restrict__ S, double* __restrict__ R,
                                                        double* __restrict__ EE) {
  constexpr int ns = Dims<NJ>::NS, na = Dims<NJ>::NA;
  const SysDevice& sd = *sdp;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_ep) return;
  const int Te = nsteps[e];
  if (Te < 0 || Te >= ldS || Te > ldU) return;
  double s[ns], a[na], out[ns], w[8], wt[8];
#pragma unroll
  for (int i = 0; i < ns; ++i) s[i] = S0[(size_t)e * ns + i];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    w[k] = k >= sd.p.n_weights ? 0.0 : sd.p.w_running[k];
    wt[k] = k >= sd.p.n_weights ? 0.0 : sd.p.w_terminal[k];
  }
  double* Se = S ? S + (size_t)e * ldS * ns : nullptr;
  double* Re = R ? R + (size_t)e * ldS : nullptr;
  double* Ee = EE ? EE + (size_t)e * ldS * 3 : nullptr;
  const double* Ue = U + (size_t)e * ldU * na;
  if (Se)
#pragma unroll
    for (int i = 0; i < ns; ++i) Se[i] = s[i];
  if (Ee) {
    const V3 p = env_ee<NJ>(sd, s);
    Ee[0] = p.x;
    Ee[1] = p.y;
    Ee[2] = p.z;
  }
  for (int t = 0; t < Te; ++t) {
#pragma unroll
    for (int i = 0; i < na; ++i) a[i] = Ue[(size_t)t * na + i];
    env_simulate<NJ>(sd, s, a, false, out);
    if (Re) Re[t] = env_reward<NJ>(sd, w, s, a, false);
    if (Ee) {
      const V3 p = env_ee<NJ>(sd, out);
      Ee[(size_t)(t + 1) * 3 + 0] = p.x;
      Ee[(size_t)(t + 1) * 3 + 1] = p.y;
      Ee[(size_t)(t + 1) * 3 + 2] = p.z;
    }
#pragma unroll
    for (int i = 0; i < ns; ++i) s[i] = out[i];
    if (Se)
#pragma unroll
      for (int i = 0; i < ns; ++i) Se[(size_t)(t + 1) * ns + i] = s[i];
  }
  if (Re) {
    // reward(cost_weights_terminal, s_T) with action None: u_cost of a zero action
#pragma unroll
    for (int i = 0; i < na; ++i) a[i] = 0.0;
    Re[Te] = env_reward<NJ>(sd, wt, s, a, false);
  }
}

constexpr int PLAN_THREADS = 256;  // one workgroup; also the scan's chunk (one episode per thread)

// main.py:181-187, :236: which episodes survive, and where their rows go. One workgroup walks the
// episodes in chunks of PLAN_THREADS: an inclusive scan of the row counts inside each wave
// (__shfl_up), the wave totals combined through LDS, the chunk's total carried into the next chunk.
__global__ void __launch_bounds__(PLAN_THREADS) k_collect_plan(const int32_t* __restrict__ nsteps,
                                                               const int32_t* __restrict__ rollout_status,
                                                               const int32_t* __restrict__ to_status,
                                                               int accept_maxiter, int n_ep,
                                                               int32_t* __restrict__ kept,
                                                               int64_t* __restrict__ row_off,
                                                               int64_t* __restrict__ counts) {
  constexpr int NW = PLAN_THREADS / 64;
  __shared__ long long wave_total[NW];
  __shared__ unsigned long long tally[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < 8) tally[tid] = 0ull;
  unsigned int mine[6] = {0u, 0u, 0u, 0u, 0u, 0u};  // kept, nsteps <= 0, NaN, CONVERGED, MAXITER, FAILED
  long long carry = 0;
  for (int base = 0; base < n_ep; base += PLAN_THREADS) {
    const int e = base + tid;
    long long c = 0;
    if (e < n_ep) {
      const int n = nsteps[e];
      bool keep = false;
      if (n <= 0) {
        ++mine[1];
      } else if (rollout_status && rollout_status[e] != 0) {
        ++mine[2];
      } else if (!to_status) {
        keep = true;
      } else {
        const int st = to_status[e];
        if (st == CACTO_TO_CONVERGED) ++mine[3];
        else if (st == CACTO_TO_MAXITER) ++mine[4];
        else if (st == CACTO_TO_FAILED) ++mine[5];
        keep = st == CACTO_TO_CONVERGED || (accept_maxiter && st == CACTO_TO_MAXITER);
      }
      if (keep) {
        ++mine[0];
        c = (long long)n + 1;
      }
      kept[e] = keep ? n : -1;
    }
    long long incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    __syncthreads();  // the previous chunk's readers of wave_total are done
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    long long before = carry, chunk = 0;
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      if (k < wave) before += wave_total[k];
      chunk += wave_total[k];
    }
    if (e < n_ep) row_off[e] = before + incl - c;
    carry += chunk;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 6; ++k)
    if (mine[k]) atomicAdd(&tally[k], (unsigned long long)mine[k]);
  __syncthreads();
  if (tid == 0) {
    row_off[n_ep] = carry;
    counts[0] = carry;
    for (int k = 0; k < 6; ++k) counts[1 + k] = (int64_t)tally[k];
    counts[7] = 0;
  }
}

// main.py:190 `ep_return = sum(rwrd)`: Python's sum starts at integer 0 and adds left to right, so
// acc = 0.0 and the same additions give the same bits (as k_rl_solve_add's sums). One thread per
// episode. An episode longer than ldR violates the documented precondition and gets NaN.
__global__ void __launch_bounds__(64) k_episode_returns(const double* __restrict__ R, int64_t ldR,
                                                        const int32_t* __restrict__ kept, int n_ep, int negate,
                                                        double* __restrict__ ret) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_ep) return;
  const int Te = kept[e];
  double acc = 0.0;
  if (Te >= ldR) {
    acc = __longlong_as_double(0x7ff8000000000000ll);
  } else {
    const double* Re = R + (size_t)e * ldR;
    for (int t = 0; t <= Te; ++t) acc += negate ? -Re[t] : Re[t];
  }
  ret[e] = acc;
}

// ---- the validation stage (cacto_validate): the networks against fresh TO trajectories ----

constexpr int VAL_CHUNK = 1024;  // rewards staged in LDS per pass of the reward-to-go recursion

// An episode's live rows fit its own arrays and the compact matrix. One that does not violates the
// documented precondition: nothing of it is read or written and its per_ep row is NaN.
__device__ __forceinline__ bool val_fits(int Te, int64_t off, int64_t ldS, int64_t ldU, int64_t ldR,
                                         int64_t total_rows) {
  return Te < ldS && Te <= ldU && Te < ldR && off >= 0 && off + Te + 1 <= total_rows;
}

// The live rows (e, t), t = 0..Te, as float32 (NN.eval's cast: round to nearest) at row_off[e] + t
// of the compact [total_rows, ns] matrix. One wave per episode; an episode's rows are contiguous in
// both arrays, so the copy is one coalesced run of (Te + 1) * ns elements.
__global__ void __launch_bounds__(64) k_val_gather(const double* __restrict__ S, int64_t ldS, int64_t ldU,
                                                   int64_t ldR, const int32_t* __restrict__ kept,
                                                   const int64_t* __restrict__ row_off, int64_t total_rows, int ns,
                                                   float* __restrict__ Sf) {
  const int e = blockIdx.x;
  const int Te = kept[e];
  if (Te < 0) return;
  const int64_t off = row_off[e];
  if (!val_fits(Te, off, ldS, ldU, ldR, total_rows)) return;
  const double* src = S + (size_t)e * ldS * ns;
  float* dst = Sf + (size_t)off * ns;
  const int64_t n = ((int64_t)Te + 1) * ns;
  for (int64_t i = threadIdx.x; i < n; i += 64) dst[i] = (float)src[i];
}

// custom_logarithm (NeuralNetwork.py:140-148) in float64.
__device__ __forceinline__ double clog64(double x) {
  return x > 0.0 ? log(fmax(x, 1e-7) + 1.0) : -log(fmax(-x, 1e-7) + 1.0);
}

// The per-episode sums, one wave per episode. The rewards go through LDS in chunks of VAL_CHUNK
// steps, last chunk first: lane 0 turns a chunk into G_t = r_t + G_{t+1} in place (the sequential
// recursion, carried from the chunk above), then lane i adds the terms of t = base + i, base + i +
// 64, ... to its own partial sums. The partials are combined by a butterfly (__shfl_xor 32, 16, ..,
// 1). Which lane adds what, and in which order, depends on t and Te alone, so an episode's row does
// not depend on where the episode stands in the batch.
__global__ void __launch_bounds__(64) k_val_reduce(const double* __restrict__ R, int64_t ldR, int negate,
                                                   const double* __restrict__ U, int64_t ldU,
                                                   const double* __restrict__ dVdx, int64_t ldS,
                                                   const int32_t* __restrict__ kept,
                                                   const int64_t* __restrict__ row_off, int64_t total_rows, int ns,
                                                   int na, const float* __restrict__ V, const float* __restrict__ g,
                                                   const float* __restrict__ A, double* __restrict__ per_ep) {
  __shared__ double G[VAL_CHUNK];
  const int e = blockIdx.x, lane = threadIdx.x;
  double* out = per_ep + (size_t)e * CACTO_VAL_COLS;
  const int Te = kept[e];
  const int64_t off = Te < 0 ? 0 : row_off[e];
  if (Te < 0 || !val_fits(Te, off, ldS, ldU, ldR, total_rows)) {
    if (lane < CACTO_VAL_COLS) out[lane] = Te < 0 ? 0.0 : __longlong_as_double(0x7ff8000000000000ll);
    return;
  }
  double acc[CACTO_VAL_COLS];
#pragma unroll
  for (int c = 0; c < CACTO_VAL_COLS; ++c) acc[c] = 0.0;
  const double* Re = R + (size_t)e * ldR;
  const double* Ue = U + (size_t)e * ldU * na;
  const double* Le = dVdx ? dVdx + (size_t)e * ldS * ns : nullptr;
  double carry = 0.0;
  for (int base = Te / VAL_CHUNK * VAL_CHUNK; base >= 0; base -= VAL_CHUNK) {
    const int n = min(VAL_CHUNK, Te + 1 - base);
    __syncthreads();  // the chunk above has been consumed
    for (int i = lane; i < n; i += 64) G[i] = negate ? -Re[base + i] : Re[base + i];
    __syncthreads();
    if (lane == 0) {
      double Gn = carry;
      if (base + n == Te + 1) {  // G_Te = r_Te
        Gn = G[n - 1];
        for (int i = n - 2; i >= 0; --i) G[i] = Gn = G[i] + Gn;
      } else {
        for (int i = n - 1; i >= 0; --i) G[i] = Gn = G[i] + Gn;
      }
    }
    __syncthreads();
    carry = G[0];
    for (int i = lane; i < n; i += 64) {
      const int t = base + i;
      const int64_t row = off + t;
      const double Gt = G[i];
      acc[CACTO_VAL_SUM_G] += Gt;
      acc[CACTO_VAL_SUM_G2] += Gt * Gt;
      if (V) {
        const double v = (double)V[row];
        acc[CACTO_VAL_SUM_V] += v;
        acc[CACTO_VAL_SSE_V] += (v - Gt) * (v - Gt);
      }
      if (Le) {
        for (int j = 0; j < ns - 1; ++j) {
          const double l = Le[(size_t)t * ns + j];
          acc[CACTO_VAL_SUM_L2] += l * l;
          if (g) {
            const double gj = (double)g[(size_t)row * ns + j];
            const double dc = clog64(gj) - clog64(l);
            acc[CACTO_VAL_SSE_G] += (gj - l) * (gj - l);
            acc[CACTO_VAL_SSE_CLOG] += dc * dc;
          }
        }
      }
      if (A && t < Te) {
#pragma unroll
        for (int j = 0; j < CACTO_MAX_ACTION; ++j) {
          if (j < na) {
            const double d = (double)A[(size_t)row * na + j] - Ue[(size_t)t * na + j];
            acc[CACTO_VAL_SSE_U + j] += d * d;
          }
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < CACTO_VAL_COLS; ++c) {
    double v = acc[c];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    acc[c] = v;
  }
  acc[CACTO_VAL_ROWS] = (double)Te + 1.0;
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < CACTO_VAL_COLS; ++c) out[c] = acc[c];
  }
}

// totals[c] = 0.0 + per_ep[0][c] + per_ep[1][c] + ..., left to right in episode order: a dropped
// episode adds an exact zero, so the same episodes inside a larger batch give the same bits. One
// workgroup, one thread per column.
__global__ void __launch_bounds__(64) k_val_totals(const double* __restrict__ per_ep, int n_ep,
                                                   double* __restrict__ totals) {
  const int c = threadIdx.x;
  if (c >= CACTO_VAL_COLS) return;
  double acc = 0.0;
#pragma unroll 8
  for (int e = 0; e < n_ep; ++e) acc += per_ep[(size_t)e * CACTO_VAL_COLS + c];
  totals[c] = acc;
}

}  // namespace cacto

using namespace cacto;

namespace {
// cacto_validate's workspace: the compact float32 states, then V, dV/ds and the actions of every
// row, each part starting on a 256-byte boundary.
struct ValWorkspace {
  size_t S, V, g, A, bytes;
};
ValWorkspace val_workspace(const cacto_sys* sys, int64_t total_rows) {
  const size_t n = (size_t)total_rows, ns = (size_t)sys->host.p.nb_state, na = (size_t)sys->host.p.nb_action;
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  ValWorkspace w;
  w.S = 0;
  w.V = w.S + up(n * ns * sizeof(float));
  w.g = w.V + up(n * sizeof(float));
  w.A = w.g + up(n * ns * sizeof(float));
  w.bytes = w.A + up(n * na * sizeof(float));
  return w;
}
constexpr int64_t VAL_NET_ROWS = int64_t(1) << 24;  // rows per network launch (their batch is an int)

template <int NJ>
struct LaunchEnvRlEpisodes {
  static int run(const cacto_sys* sys, const double* S0, const double* U, int64_t ldU, const int32_t* nsteps,
                 int n_ep, int64_t ldS, double* S, double* R, double* EE, hipStream_t st) {
    hipLaunchKernelGGL(k_env_rl_episodes<NJ>, dim3(ceil_div(n_ep, 64)), dim3(64), 0, st, sys->dev, S0, U, ldU, nsteps,
                       n_ep, ldS, S, R, EE);
    CACTO_CHECK_HIP(hipGetLastError());
    return CACTO_OK;
  }
};
}  // namespace

extern "C" int cacto_env_rl_episodes(const cacto_sys* sys, const double* S0_d, const double* U_d, int64_t ldU,
                                     const int32_t* nsteps_d, int n_ep, int64_t ldS, double* S_d, double* R_d,
                                     double* EE_d, void* stream) {
  CACTO_REQUIRE(sys && S0_d && U_d && nsteps_d && n_ep > 0 && ldU > 0 && ldS > 0,
                "cacto_env_rl_episodes: bad arguments");
  return dispatch_nj<LaunchEnvRlEpisodes>(sys->host.p, sys, S0_d, U_d, ldU, nsteps_d, n_ep, ldS, S_d, R_d, EE_d,
                                          as_stream(stream));
}

extern "C" int cacto_collect_plan(const int32_t* nsteps_d, const int32_t* rollout_status_d,
                                  const int32_t* to_status_d, int accept_maxiter, int n_ep, int32_t* kept_d,
                                  int64_t* row_off_d, int64_t* counts_d, void* stream) {
  CACTO_REQUIRE(nsteps_d && kept_d && row_off_d && counts_d && n_ep > 0, "cacto_collect_plan: bad arguments");
  hipLaunchKernelGGL(k_collect_plan, dim3(1), dim3(PLAN_THREADS), 0, as_stream(stream), nsteps_d, rollout_status_d,
                     to_status_d, accept_maxiter, n_ep, kept_d, row_off_d, counts_d);
  CACTO_CHECK_HIP(hipGetLastError());
  return CACTO_OK;
}

extern "C" int cacto_episode_returns(const double* R_d, int64_t ldR, const int32_t* kept_d, int n_ep, int negate,
                                     double* ret_d, void* stream) {
  CACTO_REQUIRE(R_d && kept_d && ret_d && n_ep > 0 && ldR > 0, "cacto_episode_returns: bad arguments");
  hipLaunchKernelGGL(k_episode_returns, dim3(ceil_div(n_ep, 64)), dim3(64), 0, as_stream(stream), R_d, ldR, kept_d,
                     n_ep, negate, ret_d);
  CACTO_CHECK_HIP(hipGetLastError());
  return CACTO_OK;
}

extern "C" size_t cacto_validate_workspace_bytes(const cacto_sys* sys, int64_t total_rows) {
  if (!sys || total_rows < 0) return 0;
  return val_workspace(sys, total_rows).bytes;
}

extern "C" int cacto_validate(const cacto_sys* sys, const float* critic_netbuf_d, const float* actor_netbuf_d,
                              const double* S_traj_d, int64_t ldS, const double* U_traj_d, int64_t ldU,
                              const double* R_d, int64_t ldR, int negate, const double* dVdx_d,
                              const int32_t* kept_d, const int64_t* row_off_d, int n_ep, int64_t total_rows,
                              double* per_ep_d, double* totals_d, void* workspace_d, size_t workspace_bytes,
                              void* stream) {
  CACTO_REQUIRE(sys && S_traj_d && U_traj_d && R_d && kept_d && row_off_d && per_ep_d && totals_d && n_ep >= 1 &&
                    total_rows >= 0 && ldS > 0 && ldU > 0 && ldR > 0,
                "cacto_validate: bad arguments");
  const ValWorkspace w = val_workspace(sys, total_rows);
  CACTO_REQUIRE(total_rows == 0 || (workspace_d && workspace_bytes >= w.bytes), "cacto_validate: workspace too small");
  hipStream_t st = as_stream(stream);
  if (total_rows == 0) {
    CACTO_CHECK_HIP(hipMemsetAsync(per_ep_d, 0, (size_t)n_ep * CACTO_VAL_COLS * sizeof(double), st));
    CACTO_CHECK_HIP(hipMemsetAsync(totals_d, 0, CACTO_VAL_COLS * sizeof(double), st));
    return CACTO_OK;
  }
  const int ns = sys->host.p.nb_state, na = sys->host.p.nb_action;
  char* base = static_cast<char*>(workspace_d);
  float* Sf = reinterpret_cast<float*>(base + w.S);
  float* V = critic_netbuf_d ? reinterpret_cast<float*>(base + w.V) : nullptr;
  float* g = critic_netbuf_d ? reinterpret_cast<float*>(base + w.g) : nullptr;
  float* A = actor_netbuf_d ? reinterpret_cast<float*>(base + w.A) : nullptr;
  hipLaunchKernelGGL(k_val_gather, dim3(n_ep), dim3(64), 0, st, S_traj_d, ldS, ldU, ldR, kept_d, row_off_d,
                     total_rows, ns, Sf);
  CACTO_CHECK_HIP(hipGetLastError());
  // the public entries' own launchers, so V, dV/ds and the actions are theirs bit for bit
  for (int64_t r0 = 0; r0 < total_rows; r0 += VAL_NET_ROWS) {
    const int B = (int)(total_rows - r0 < VAL_NET_ROWS ? total_rows - r0 : VAL_NET_ROWS);
    if (critic_netbuf_d) {
      const int rc = cacto_critic_input_grad(sys, critic_netbuf_d, Sf + (size_t)r0 * ns, V + r0, g + (size_t)r0 * ns,
                                             B, stream);
      if (rc != CACTO_OK) return rc;
    }
    if (actor_netbuf_d) {
      const int rc = cacto_actor_forward(sys, actor_netbuf_d, Sf + (size_t)r0 * ns, A + (size_t)r0 * na, B, stream);
      if (rc != CACTO_OK) return rc;
    }
  }
  hipLaunchKernelGGL(k_val_reduce, dim3(n_ep), dim3(64), 0, st, R_d, ldR, negate, U_traj_d, ldU, dVdx_d, ldS, kept_d,
                     row_off_d, total_rows, ns, na, V, g, A, per_ep_d);
  CACTO_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_val_totals, dim3(1), dim3(64), 0, st, per_ep_d, n_ep, totals_d);
  CACTO_CHECK_HIP(hipGetLastError());
  return CACTO_OK;
}
