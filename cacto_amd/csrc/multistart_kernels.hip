// Multi-start trajectory optimisation: the two kernels around one cacto_to_solve over N candidate
// warm starts per episode. k_to_starts builds the candidate batch (candidate 0 the caller's warm
// start, the others perturbations of it drawn from a counter-based integer generator), k_to_select
// picks each episode's best acceptable candidate and gathers its rows into the outputs
// cacto_to_solve would have written. Both are asynchronous and read nothing back, so a multi-start
// solve whose plan says on_device stays capturable. The rules are stated in include/cacto_hip.h.
#include <cmath>

#include "internal.h"

namespace cacto {

// splitmix64's output function of the state z (Steele, Lea, Flood 2014): the increment, then the
// finaliser. Integer arithmetic modulo 2^64 only.
__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// xi(seed, e, c, block, k) in [-1, 1): the header's packing and formula. (h >> 11) has 53 bits, so
// the conversion, the scaling by 2^-52 and the subtraction are all exact.
__device__ __forceinline__ double start_xi(uint64_t seed_mix, int e, int c, int64_t block, int k) {
  const uint64_t packed = ((uint64_t)(uint32_t)e << 31) | ((uint64_t)block << 7) | ((uint64_t)c << 3) | (uint64_t)k;
  const uint64_t h = splitmix64(seed_mix ^ packed);
  return (double)(h >> 11) * 0x1p-52 - 1.0;
}

struct StartScale {
  double v[CACTO_MAX_ACTION];  // sigma * half_range[k], rounded once on the host
};

constexpr int STARTS_THREADS = 256;

// One thread per element of U_all [N E, ldU, na] (k fastest, then t: consecutive lanes write
// consecutive doubles and read consecutive doubles of U_init); the first N E ns threads also tile
// S0 and the first N E the lengths. No LDS, no atomics.
__global__ void __launch_bounds__(STARTS_THREADS) k_to_starts(const double* __restrict__ S0,
                                                              const double* __restrict__ U_init, int64_t ldU,
                                                              const int32_t* __restrict__ nsteps, int n_ep, int N,
                                                              int ns, int na, int hold, StartScale scale,
                                                              int zero_start, uint64_t seed_mix,
                                                              double* __restrict__ S0_all,
                                                              double* __restrict__ U_all,
                                                              int32_t* __restrict__ nsteps_all) {
  const int64_t i = (int64_t)blockIdx.x * STARTS_THREADS + threadIdx.x;
  const int64_t rows = (int64_t)N * n_ep;
  const int64_t per_ep = ldU * na;
  if (i < rows * per_ep) {
    const int64_t row = i / per_ep, in_ep = i - row * per_ep;
    const int c = (int)(row / n_ep), e = (int)(row - (int64_t)c * n_ep);
    const int64_t t = in_ep / na;
    const int k = (int)(in_ep - t * na);
    const double u = U_init[(int64_t)e * per_ep + in_ep];
    double v;
    if (c == 0) {
      v = u;
    } else if (c == 1 && zero_start) {
      v = 0.0;
    } else {
      v = u + scale.v[k] * start_xi(seed_mix, e, c, t / hold, k);
    }
    U_all[i] = v;
  }
  if (i < rows * ns) {
    const int64_t row = i / ns;
    const int e = (int)(row % n_ep);
    S0_all[i] = S0[(int64_t)e * ns + (i - row * ns)];
  }
  if (i < rows) nsteps_all[i] = nsteps[i % n_ep];
}

constexpr int SELECT_THREADS = 256;

__device__ __forceinline__ void copy_run(double* __restrict__ dst, const double* __restrict__ src, int64_t n) {
  for (int64_t i = threadIdx.x; i < n; i += SELECT_THREADS) dst[i] = src[i];
}

// One workgroup per episode. Every thread reads the same <= CACTO_TO_STARTS_MAX (status, J) pairs
// (uniform addresses: scalar loads) and so computes the same winner: no LDS, no barrier, every
// branch below is wave-uniform. Then the winner's live rows, each a contiguous run, are copied with
// consecutive lanes on consecutive doubles. An episode whose Te does not fit ldS / ldU violates the
// documented precondition: nothing of it is written but start = -1, n_ok = 0.
__global__ void __launch_bounds__(SELECT_THREADS) k_to_select(
    const double* __restrict__ S_all, const double* __restrict__ U_all, const double* __restrict__ cost_all,
    const int32_t* __restrict__ status_all, const int32_t* __restrict__ iters_all, const double* __restrict__ J_all,
    const int32_t* __restrict__ nsteps, int n_ep, int N, int64_t ldS, int64_t ldU, int ns, int na, int accept_maxiter,
    double* __restrict__ S, double* __restrict__ U, double* __restrict__ cost, int32_t* __restrict__ status,
    int32_t* __restrict__ iters, double* __restrict__ J, int32_t* __restrict__ start, int32_t* __restrict__ n_ok,
    double* __restrict__ J_starts, int32_t* __restrict__ status_starts) {
  const int e = blockIdx.x;
  const int Te = nsteps[e];
  int win = 0, ok = 0;
  double best = 0.0;
  for (int c = 0; c < N; ++c) {
    const int64_t row = (int64_t)c * n_ep + e;
    const int st = status_all[row];
    const double Jc = J_all[row * 2 + 1];
    if (threadIdx.x == 0) {
      J_starts[(int64_t)e * N + c] = Jc;
      status_starts[(int64_t)e * N + c] = st;
    }
    const bool acc = (st == CACTO_TO_CONVERGED || (accept_maxiter && st == CACTO_TO_MAXITER)) && isfinite(Jc);
    if (acc && (ok == 0 || Jc < best)) {
      best = Jc;
      win = c;
    }
    ok += acc ? 1 : 0;
  }
  const bool live = Te >= 0 && Te < ldS && Te <= ldU;
  if (threadIdx.x == 0) {
    start[e] = live ? win : -1;
    n_ok[e] = live ? ok : 0;
  }
  if (!live) return;
  const int64_t w = (int64_t)win * n_ep + e;
  copy_run(S + (int64_t)e * ldS * ns, S_all + w * ldS * ns, ((int64_t)Te + 1) * ns);
  copy_run(U + (int64_t)e * ldU * na, U_all + w * ldU * na, (int64_t)Te * na);
  copy_run(cost + (int64_t)e * ldS, cost_all + w * ldS, (int64_t)Te + 1);
  if (threadIdx.x == 0) {
    status[e] = status_all[w];
    iters[e] = iters_all[w];
    J[(int64_t)e * 2 + 0] = J_all[(int64_t)e * 2 + 0];  // candidate 0 is row e
    J[(int64_t)e * 2 + 1] = J_all[w * 2 + 1];
  }
}

}  // namespace cacto

using namespace cacto;

extern "C" int cacto_to_starts(const cacto_sys* sys, const double* S0_d, const double* U_init_d, int64_t ldU,
                               const int32_t* nsteps_d, int n_ep, int n_starts, double sigma, int hold,
                               const double* half_range_h, int zero_start, uint64_t seed, double* S0_all_d,
                               double* U_all_d, int32_t* nsteps_all_d, void* stream) {
  CACTO_REQUIRE(sys && S0_d && U_init_d && nsteps_d && half_range_h && S0_all_d && U_all_d && nsteps_all_d,
                "cacto_to_starts: null argument");
  CACTO_REQUIRE(n_starts >= 1 && n_starts <= CACTO_TO_STARTS_MAX,
                "cacto_to_starts: n_starts outside [1, CACTO_TO_STARTS_MAX]");
  CACTO_REQUIRE(hold >= 1, "cacto_to_starts: hold < 1");
  CACTO_REQUIRE(std::isfinite(sigma) && sigma >= 0.0, "cacto_to_starts: sigma negative or not finite");
  CACTO_REQUIRE(n_ep > 0 && ldU > 0 && ldU < (int64_t(1) << 24), "cacto_to_starts: bad arguments");
  const int ns = sys->host.p.nb_state, na = sys->host.p.nb_action;
  StartScale scale;
  for (int k = 0; k < CACTO_MAX_ACTION; ++k) scale.v[k] = 0.0;
  for (int k = 0; k < na; ++k) {
    CACTO_REQUIRE(std::isfinite(half_range_h[k]) && half_range_h[k] >= 0.0,
                  "cacto_to_starts: half_range negative or not finite");
    scale.v[k] = sigma * half_range_h[k];
  }
  const int64_t rows = (int64_t)n_starts * n_ep;
  const int64_t work = rows * (ldU * na > ns ? ldU * na : ns);
  const int64_t blocks = (work + STARTS_THREADS - 1) / STARTS_THREADS;
  CACTO_REQUIRE(blocks <= 0x7fffffffll, "cacto_to_starts: batch too large");
  // the seed goes through the generator once, so seeds that differ in one bit give unrelated keys
  uint64_t z = seed + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  const uint64_t seed_mix = z ^ (z >> 31);
  hipLaunchKernelGGL(k_to_starts, dim3((unsigned)blocks), dim3(STARTS_THREADS), 0, as_stream(stream), S0_d, U_init_d,
                     ldU, nsteps_d, n_ep, n_starts, ns, na, hold, scale, zero_start ? 1 : 0, seed_mix, S0_all_d,
                     U_all_d, nsteps_all_d);
  CACTO_CHECK_HIP(hipGetLastError());
  return CACTO_OK;
}

extern "C" int cacto_to_select(const cacto_sys* sys, const double* S_all_d, const double* U_all_d,
                               const double* step_cost_all_d, const int32_t* status_all_d,
                               const int32_t* iters_all_d, const double* J_all_d, const int32_t* nsteps_d, int n_ep,
                               int n_starts, int64_t ldS, int64_t ldU, int accept_maxiter, double* S_d, double* U_d,
                               double* step_cost_d, int32_t* status_d, int32_t* iters_d, double* J_d,
                               int32_t* start_d, int32_t* n_ok_d, double* J_starts_d, int32_t* status_starts_d,
                               void* stream) {
  CACTO_REQUIRE(sys && S_all_d && U_all_d && step_cost_all_d && status_all_d && iters_all_d && J_all_d && nsteps_d &&
                    S_d && U_d && step_cost_d && status_d && iters_d && J_d && start_d && n_ok_d && J_starts_d &&
                    status_starts_d,
                "cacto_to_select: null argument");
  CACTO_REQUIRE(n_starts >= 1 && n_starts <= CACTO_TO_STARTS_MAX,
                "cacto_to_select: n_starts outside [1, CACTO_TO_STARTS_MAX]");
  CACTO_REQUIRE(n_ep > 0 && ldS > 0 && ldU > 0, "cacto_to_select: bad arguments");
  const int ns = sys->host.p.nb_state, na = sys->host.p.nb_action;
  hipLaunchKernelGGL(k_to_select, dim3(n_ep), dim3(SELECT_THREADS), 0, as_stream(stream), S_all_d, U_all_d,
                     step_cost_all_d, status_all_d, iters_all_d, J_all_d, nsteps_d, n_ep, n_starts, ldS, ldU, ns, na,
                     accept_maxiter ? 1 : 0, S_d, U_d, step_cost_d, status_d, iters_d, J_d, start_d, n_ok_d,
                     J_starts_d, status_starts_d);
  CACTO_CHECK_HIP(hipGetLastError());
  return CACTO_OK;
}
