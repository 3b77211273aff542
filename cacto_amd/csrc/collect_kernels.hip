// The kernels of the sample-collection stage (main.py:174-243 for every initial state of an
// iteration at once): the env_RL re-simulation of whole episodes, the filter of failed episodes
// with the ring offsets of the kept ones, and the episode returns.
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

}  // namespace cacto

using namespace cacto;

namespace {
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
