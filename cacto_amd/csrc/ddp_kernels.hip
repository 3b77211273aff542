#include <cstdlib>
// Sobolev labels without CasADi: the DDP backward pass of TO.backward_pass
// (TO.py:119-202) along recorded trajectories, on the GPU.
//
// Per episode (one thread; the recursion is sequential in t, episodes are independent):
//   V_x, V_xx      = d/dx, d2/dx2 of the terminal reward at x_T            (TO.py:166-168)
//   for i = T-1 .. 0:
//     A, B         = augmented_derivative(x_i, u_i)                        (environment.py:111-132,
//                                                                            SI :221-233, Car :420-435)
//     l_x, l_xx, l_u, l_uu of the running reward (l_xu = 0: the cost separates in x and u)
//     Q_x = l_x + A^T V_x   Q_u = l_u + B^T V_x   Q_xx = l_xx + A^T V_xx A
//     Q_uu = l_uu + B^T V_xx B   Q_xu = A^T V_xx B   (TO.py:182-186)
//     V_x = Q_x - Q_xu Qbar^-1 Q_u,  V_xx = Q_xx - Q_xu Qbar^-1 Q_xu^T, Qbar = Q_uu + mu I (:188-194)
// The reference differentiates the TO cost (environment_TO.py, = -reward) symbolically with CasADi;
// here the planar-family derivatives are closed forms of the same expression (ellipses and the
// peak term as softplus of their arguments: d softplus(z)/dz = sigmoid(z)). Qbar is inverted by
// Gauss-Jordan with partial pivoting (np.linalg.pinv in the reference equals the inverse for the
// nonsingular, mu-regularised Qbar): float64 results within 1e-9 relative of the oracle at the short
// horizons of tests/test_gpu_ddp.py (<= 24 steps). At full episode length the oracle's own formula is
// not accurate in float64: it never symmetrises V_xx, and the antisymmetric rounding residue of
// A^T V_xx A grows geometrically (a factor ~2.5 per step on a solved double-integrator episode; no
// correct digit ~60 steps from the end). Both recursions below therefore end each node with
//     V_xx = (V_xx + V_xx^T) / 2
// (after the masked products, so bounds and no bounds share it) and are checked at full length against
// the recursion at 80 digits (tests/ddp_mp_ref.py, tests/test_gpu_ddp_long.py).
//
// Every system: the single integrator (NJ = 0), car (NJ = -1) and prismatic Pinocchio chains (the
// double integrator: M and nle constant, so ddq_dq = ddq_dv = 0 and Fu = dt [0; M^-1]) use closed
// forms; car_park (NJ = -2) closed-form Jacobians (environment.py:567-582) with its smooth-box cost
// differentiated by hyper-dual numbers (ad.h); revolute chains (manipulator NJ = 3, UR5 NJ = 6) take
// ddq_dq, ddq_dv from hyper-dual RNEA (computeABADerivatives) and l_x, l_xx through hyper-dual
// forward kinematics.
// cacto_ddp_launch_derivs (internal.h) is the library's one launcher of the derivative kernels (label
// pass, cacto_env_jacobians, to_kernels.hip). Each pass keeps its wave recursion written out in its
// own file: a shared front half was slower.
#include "ddp_device.h"

namespace cacto {

// Env.augmented_derivative (environment.py:111-132; SI :221-233, Car :420-435, CarPark :567-582) for
// B independent (state, action) rows: the discrete-time Jacobians Fx [nx, nx], Fu [nx, na] that the
// DDP pass consumes (the same device code), for host-side callers such as TO.backward_pass
// (TO.py:181). Closed-form systems: one thread per row. Revolute chains go through the split DDP
// pass's derivative kernel (k_ddp_derivs: each row as a one-step episode, records extracted by
// k_jac_extract), so their hyper-dual RNEA runs in exactly one kernel.
template <int NJ>
__global__ void __launch_bounds__(64) k_env_jacobians(const SysDevice* __restrict__ sdp, const double* __restrict__ S,
                                                      const double* __restrict__ U, int B, double* __restrict__ Fx,
                                                      double* __restrict__ Fu) {
  constexpr int N = DdpDims<NJ>::N, M = DdpDims<NJ>::M, ns = Dims<NJ>::NS, na = Dims<NJ>::NA;
  if constexpr (NJ <= 2) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const SysDevice& sd = *sdp;
    double x[N], A[N * N], Bm[N * M];
#pragma unroll
    for (int k = 0; k < N; ++k) x[k] = S[(size_t)b * ns + k];
    if constexpr (NJ > 0) {
      double Mm[M * M], Minv[M * M];
      chain_mass<NJ>(sd, x, Mm);
      small_inverse<M>(Mm, Minv);
      ddp_jacobians<NJ>(sd, x, Minv, A, Bm);
    } else {
      ddp_jacobians<NJ>(sd, x, nullptr, A, Bm);
    }
#pragma unroll
    for (int k = 0; k < N * N; ++k) Fx[(size_t)b * N * N + k] = A[k];
#pragma unroll
    for (int k = 0; k < N * M; ++k) Fu[(size_t)b * N * M + k] = Bm[k];
  }
}

// Rows -> one-step episodes for the derivative kernels: S2 [B, 2, ns] (the state twice), nsteps = 1.
template <int NJ>
__global__ void k_jac_prep(const double* __restrict__ S, int B, double* __restrict__ S2, int32_t* __restrict__ n1) {
  constexpr int ns = Dims<NJ>::NS;
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= B * 2 * ns) return;
  const int b = k / (2 * ns), c = k % ns;
  S2[k] = S[(size_t)b * ns + c];
  if (k < B) n1[k] = 1;
}

// Step-0 A, B records ([t][k][e] layout of DdpRec) -> Fx [B, N, N], Fu [B, N, M].
template <int NJ>
__global__ void k_jac_extract(const double* __restrict__ ws, int B, double* __restrict__ Fx, double* __restrict__ Fu) {
  using RC = DdpRec<NJ>;
  constexpr int N = RC::N, M = RC::M;
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= B * (N * N + N * M)) return;
  const int b = k % B, r = k / B;
  const double v = ws[(size_t)(RC::A + r) * B + b];
  if (r < N * N)
    Fx[(size_t)b * N * N + r] = v;
  else
    Fu[(size_t)b * N * M + (r - N * N)] = v;
}

// The fused pass for the closed-form systems (SI, car, DI): one thread per episode computes each
// step's A, B, l_x, l_xx inline and runs the Riccati recursion (sequential in t). BX: the bounds of
// the call (ToNoBox / ToBoxDev, ddp_device.h); under bounds each node's Q_u, Q_xu and Qbar_uu are masked
// (ddp_label_mask) before the same inverse and products.
template <int NJ, class BX>
__global__ void __launch_bounds__(64) k_ddp_backward(const SysDevice* __restrict__ sdp, const double* __restrict__ S,
                                                      int64_t ldS, const double* __restrict__ U, int64_t ldU,
                                                      const int32_t* __restrict__ nsteps, int n_ep, double mu,
                                                      double* __restrict__ dVdx, BX bx) {
  constexpr int N = DdpDims<NJ>::N, M = DdpDims<NJ>::M, ns = Dims<NJ>::NS, na = Dims<NJ>::NA;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_ep) return;
  const SysDevice& sd = *sdp;
  const cacto_sys_params& p = sd.p;
  const int Te = nsteps[e];
  if (Te < 0) return;  // a dropped episode (main.py:236): no labels
  const double* Se = S + (size_t)e * ldS * ns;
  const double* Ue = U + (size_t)e * ldU * na;
  double* Oe = dVdx + (size_t)e * ldS * ns;
  double Minv[NJ > 0 ? M * M : 1];
  if constexpr (NJ > 0) {
    // prismatic chain (the launcher sends only constant-M chains here): M^-1 once per episode
    double Mm[M * M], q[NJ];
#pragma unroll
    for (int i = 0; i < NJ; ++i) q[i] = Se[i];
    chain_mass<NJ>(sd, q, Mm);
    small_inverse<M>(Mm, Minv);
  }
  double w_run[7], w_term[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    w_run[k] = p.w_running[k];
    w_term[k] = p.w_terminal[k];
  }
  double Vx[N], Vxx[N * N], x[N];
#pragma unroll
  for (int k = 0; k < N; ++k) x[k] = Se[(size_t)Te * ns + k];
  ddp_lx<NJ>(sd, w_term, x, Vx, Vxx);
#pragma unroll
  for (int k = 0; k < N; ++k) Oe[(size_t)Te * ns + k] = Vx[k];
  Oe[(size_t)Te * ns + N] = 0.0;
  for (int i = Te - 1; i >= 0; --i) {
    double u[M], A[N * N], B[N * M], lx[N], lxx[N * N];
#pragma unroll
    for (int k = 0; k < N; ++k) x[k] = Se[(size_t)i * ns + k];
#pragma unroll
    for (int k = 0; k < M; ++k) u[k] = Ue[(size_t)i * na + k];
    ddp_jacobians<NJ>(sd, x, Minv, A, B);
    ddp_lx<NJ>(sd, w_run, x, lx, lxx);
    // Q_x = l_x + A^T V_x, Q_u = l_u + B^T V_x
    double Qx[N], Qu[M], Qxx[N * N], Quu[M * M], Qxu[N * M], VA[N * N], VB[N * M];
#pragma unroll
    for (int r = 0; r < N; ++r) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < N; ++k)
        if (a_nz<NJ>(k, r)) s += A[k * N + r] * Vx[k];
      Qx[r] = lx[r] + s;
    }
#pragma unroll
    for (int j = 0; j < M; ++j) {
      double lu, luu;
      ddp_lu(p, w_run[6], u[j], j, &lu, &luu);
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < N; ++k)
        if (b_nz<NJ>(k, j)) s += B[k * M + j] * Vx[k];
      Qu[j] = lu + s;
    }
    // V_xx A, V_xx B
#pragma unroll
    for (int r = 0; r < N; ++r) {
#pragma unroll
      for (int c = 0; c < N; ++c) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k)
          if (a_nz<NJ>(k, c)) s += Vxx[r * N + k] * A[k * N + c];
        VA[r * N + c] = s;
      }
#pragma unroll
      for (int c = 0; c < M; ++c) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k)
          if (b_nz<NJ>(k, c)) s += Vxx[r * N + k] * B[k * M + c];
        VB[r * M + c] = s;
      }
    }
#pragma unroll
    for (int r = 0; r < N; ++r) {
#pragma unroll
      for (int c = 0; c < N; ++c) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k)
          if (a_nz<NJ>(k, r)) s += A[k * N + r] * VA[k * N + c];
        Qxx[r * N + c] = lxx[r * N + c] + s;
      }
#pragma unroll
      for (int c = 0; c < M; ++c) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k)
          if (a_nz<NJ>(k, r)) s += A[k * N + r] * VB[k * M + c];
        Qxu[r * M + c] = s;  // + l_xu = 0
      }
    }
#pragma unroll
    for (int r = 0; r < M; ++r)
#pragma unroll
      for (int c = 0; c < M; ++c) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k)
          if (b_nz<NJ>(k, r)) s += B[k * M + r] * VB[k * M + c];
        double lu, luu = 0.0;
        if (r == c) ddp_lu(p, w_run[6], u[r], r, &lu, &luu);
        Quu[r * M + c] = luu + s + (r == c ? mu : 0.0);
      }
    if constexpr (BX::on) ddp_label_mask<N, M>(bx, u, Qu, Quu, Qxu);
    double Qi[M * M];
    small_inverse<M>(Quu, Qi);
    // K = Qbar^-1 Q_xu^T [M x N], k = Qbar^-1 Q_u [M]
    double Kk[M];
#pragma unroll
    for (int r = 0; r < M; ++r) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < M; ++k) s += Qi[r * M + k] * Qu[k];
      Kk[r] = s;
    }
#pragma unroll
    for (int r = 0; r < N; ++r) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < M; ++k) s += Qxu[r * M + k] * Kk[k];
      Vx[r] = Qx[r] - s;
    }
#pragma unroll
    for (int r = 0; r < N; ++r) {
      double QK[M];  // row r of Q_xu Qbar^-1
#pragma unroll
      for (int c = 0; c < M; ++c) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < M; ++k) s += Qxu[r * M + k] * Qi[k * M + c];
        QK[c] = s;
      }
#pragma unroll
      for (int c = 0; c < N; ++c) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < M; ++k) s += QK[k] * Qxu[c * M + k];
        Vxx[r * N + c] = Qxx[r * N + c] - s;
      }
    }
    // V_xx = (V_xx + V_xx^T) / 2: see the header
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
      for (int c = r + 1; c < N; ++c) Vxx[r * N + c] = Vxx[c * N + r] = 0.5 * (Vxx[r * N + c] + Vxx[c * N + r]);
#pragma unroll
    for (int k = 0; k < N; ++k) Oe[(size_t)i * ns + k] = Vx[k];
    Oe[(size_t)i * ns + N] = 0.0;
  }
}

// The Riccati recursion of the split pass with one wavefront per episode: the lanes share each
// step's matrix products (outputs spread over lanes, operands in LDS), so the N = 12 recursion of
// UR5 is ~N^3 / 64 dependent FMAs per product instead of N^3 on one thread. Same products, same
// summation order as k_ddp_backward; Qbar_uu^-1 (M x M) on lane 0, which under bounds (BX) also
// decides which controls are held and masks Qbar_uu, Q_u and the columns of Q_xu (ddp_label_mask): no
// other lane touches those between the barriers around its stage, and the barrier after it makes the
// zeroed columns visible to the V_x / Q_xu Qbar^-1 stage.
template <int NJ, class BX>
__global__ void __launch_bounds__(64) k_ddp_riccati_wave(const SysDevice* __restrict__ sdp,
                                                         const double* __restrict__ U, int64_t ldU,
                                                         const int32_t* __restrict__ nsteps, int n_ep, double mu,
                                                         const double* __restrict__ ws, int64_t ldS,
                                                         double* __restrict__ dVdx, BX bx) {
  using RC = DdpRec<NJ>;
  constexpr int N = RC::N, M = RC::M, ns = Dims<NJ>::NS, na = Dims<NJ>::NA;
  __shared__ double sA[N * N], sB[N * M], sLx[N], sLxx[N * N], sVx[N], sVxx[N * N], sU[M];
  __shared__ double sVA[N * N], sVB[N * M], sQx[N], sQu[M], sQxx[N * N], sQxu[N * M], sQuu[M * M], sQi[M * M];
  __shared__ double sK[M], sQK[N * M];
  const int e = blockIdx.x, lane = threadIdx.x;
  const cacto_sys_params& p = sdp->p;
  const double w6 = p.w_running[6];
  const int Te = nsteps[e];
  if (Te < 0) return;  // a dropped episode (main.py:236): no labels (uniform over the workgroup)
  double* Oe = dVdx + (size_t)e * ldS * ns;
  const double* Ue = U + (size_t)e * ldU * na;
  {
    const double* rec = ws + (size_t)Te * RC::R * n_ep + e;
    for (int k = lane; k < N; k += 64) sVx[k] = rec[(size_t)(RC::LX + k) * n_ep];
    for (int k = lane; k < N * N; k += 64) sVxx[k] = rec[(size_t)(RC::LXX + k) * n_ep];
  }
  __syncthreads();
  for (int k = lane; k <= N; k += 64) Oe[(size_t)Te * ns + k] = k < N ? sVx[k] : 0.0;
  for (int i = Te - 1; i >= 0; --i) {
    const double* rec = ws + (size_t)i * RC::R * n_ep + e;
    for (int k = lane; k < N * N; k += 64) {
      sA[k] = rec[(size_t)(RC::A + k) * n_ep];
      sLxx[k] = rec[(size_t)(RC::LXX + k) * n_ep];
    }
    for (int k = lane; k < N * M; k += 64) sB[k] = rec[(size_t)(RC::B + k) * n_ep];
    for (int k = lane; k < N; k += 64) sLx[k] = rec[(size_t)(RC::LX + k) * n_ep];
    for (int k = lane; k < M; k += 64) sU[k] = Ue[(size_t)i * na + k];
    __syncthreads();
    // V_xx A, V_xx B, Q_x = l_x + A^T V_x, Q_u = l_u + B^T V_x
    for (int o = lane; o < N * N + N * M + N + M; o += 64) {
      double s = 0.0;
      if (o < N * N) {
        const int r = o / N, c = o - r * N;
#pragma unroll
        for (int k = 0; k < N; ++k) s += sVxx[r * N + k] * sA[k * N + c];
        sVA[o] = s;
      } else if (o < N * N + N * M) {
        const int q = o - N * N, r = q / M, c = q - r * M;
#pragma unroll
        for (int k = 0; k < N; ++k) s += sVxx[r * N + k] * sB[k * M + c];
        sVB[q] = s;
      } else if (o < N * N + N * M + N) {
        const int r = o - N * N - N * M;
#pragma unroll
        for (int k = 0; k < N; ++k) s += sA[k * N + r] * sVx[k];
        sQx[r] = sLx[r] + s;
      } else {
        const int j = o - N * N - N * M - N;
        double lu, luu;
        ddp_lu(p, w6, sU[j], j, &lu, &luu);
#pragma unroll
        for (int k = 0; k < N; ++k) s += sB[k * M + j] * sVx[k];
        sQu[j] = lu + s;
      }
    }
    __syncthreads();
    // Q_xx = l_xx + A^T V_xx A, Q_xu = A^T V_xx B, Qbar_uu = l_uu + B^T V_xx B + mu I
    for (int o = lane; o < N * N + N * M + M * M; o += 64) {
      double s = 0.0;
      if (o < N * N) {
        const int r = o / N, c = o - r * N;
#pragma unroll
        for (int k = 0; k < N; ++k) s += sA[k * N + r] * sVA[k * N + c];
        sQxx[o] = sLxx[o] + s;
      } else if (o < N * N + N * M) {
        const int q = o - N * N, r = q / M, c = q - r * M;
#pragma unroll
        for (int k = 0; k < N; ++k) s += sA[k * N + r] * sVB[k * M + c];
        sQxu[q] = s;
      } else {
        const int q = o - N * N - N * M, r = q / M, c = q - r * M;
#pragma unroll
        for (int k = 0; k < N; ++k) s += sB[k * M + r] * sVB[k * M + c];
        double lu, luu = 0.0;
        if (r == c) ddp_lu(p, w6, sU[r], r, &lu, &luu);
        sQuu[q] = luu + s + (r == c ? mu : 0.0);
      }
    }
    __syncthreads();
    if (lane == 0) {
      double a[M * M], inv[M * M];
#pragma unroll
      for (int k = 0; k < M * M; ++k) a[k] = sQuu[k];
      if constexpr (BX::on) ddp_label_mask<N, M>(bx, sU, sQu, a, sQxu);
      small_inverse<M>(a, inv);
#pragma unroll
      for (int r = 0; r < M; ++r) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < M; ++k) s += inv[r * M + k] * sQu[k];
        sK[r] = s;
      }
#pragma unroll
      for (int k = 0; k < M * M; ++k) sQi[k] = inv[k];
    }
    __syncthreads();
    // V_x = Q_x - Q_xu (Qbar^-1 Q_u); row r of Q_xu Qbar^-1
    for (int o = lane; o < N + N * M; o += 64) {
      double s = 0.0;
      if (o < N) {
#pragma unroll
        for (int k = 0; k < M; ++k) s += sQxu[o * M + k] * sK[k];
        sVx[o] = sQx[o] - s;
      } else {
        const int q = o - N, r = q / M, c = q - r * M;
#pragma unroll
        for (int k = 0; k < M; ++k) s += sQxu[r * M + k] * sQi[k * M + c];
        sQK[q] = s;
      }
    }
    __syncthreads();
    // Q_xx - (Q_xu Qbar^-1) Q_xu^T into sVA (last read two barriers ago), then V_xx = its symmetric part:
    // element (c, r) comes from another lane, hence the barrier between the two
    for (int o = lane; o < N * N; o += 64) {
      const int r = o / N, c = o - r * N;
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < M; ++k) s += sQK[r * M + k] * sQxu[c * M + k];
      sVA[o] = sQxx[o] - s;
    }
    __syncthreads();
    for (int o = lane; o < N * N; o += 64) {
      const int r = o / N, c = o - r * N;
      sVxx[o] = 0.5 * (sVA[o] + sVA[c * N + r]);
    }
    for (int k = lane; k <= N; k += 64) Oe[(size_t)i * ns + k] = k < N ? sVx[k] : 0.0;
    __syncthreads();
  }
}

}  // namespace cacto

using namespace cacto;

// Grow-only device workspace of the split pass, owned by the system handle (freed by
// cacto_sys_destroy). Growing frees the old block (hipFree synchronises the device).
int cacto_ddp_workspace(cacto_sys* sys, size_t bytes, double** out) {
  if (bytes > sys->ddp_ws_bytes) {
    if (sys->ddp_ws) CACTO_CHECK_HIP(hipFree(sys->ddp_ws));
    sys->ddp_ws = nullptr;
    sys->ddp_ws_bytes = 0;
    CACTO_CHECK_HIP(hipMalloc(&sys->ddp_ws, bytes));
    sys->ddp_ws_bytes = bytes;
  }
  *out = static_cast<double*>(sys->ddp_ws);
  return CACTO_OK;
}

namespace {
// The derivative kernels over (episode, step < steps): k_ddp_derivs for car_park; for the revolute
// chains the primal / cost-derivative / per-direction tangent kernels, the primal block behind the
// records, or with CACTO_DDP_SPLIT=0 k_ddp_derivs too (the same records bit for bit).
template <int NJ>
struct LaunchDerivs {
  static int run(const cacto_sys* sys, const double* S, int64_t ldS, const double* U, int64_t ldU, const int32_t* n,
                 int n_ep, double* rec, int64_t steps, bool want_lx, hipStream_t st) {
    if constexpr (NJ > 2 || NJ == -2) {
      const dim3 g(ceil_div(n_ep, 64), (unsigned)steps);
      if constexpr (NJ > 2) {
        static const char* split_env = std::getenv("CACTO_DDP_SPLIT");
        if (!(split_env && split_env[0] == '0')) {
          double* pw = rec + (size_t)steps * DdpRec<NJ>::R * n_ep;
          hipLaunchKernelGGL(k_ddp_prim<NJ>, g, dim3(64), 0, st, sys->dev, S, ldS, U, ldU, n, n_ep, rec, pw);
          CACTO_CHECK_HIP(hipGetLastError());
          if (want_lx) {
            hipLaunchKernelGGL(k_ddp_lx<NJ>, g, dim3(64), 0, st, sys->dev, S, ldS, n, n_ep, rec);
            CACTO_CHECK_HIP(hipGetLastError());
          }
          hipLaunchKernelGGL(k_ddp_tan<NJ>, dim3(g.x, g.y, 2 * NJ), dim3(64), 0, st, sys->dev, S, ldS, n, n_ep, rec, pw);
          CACTO_CHECK_HIP(hipGetLastError());
          return CACTO_OK;
        }
      }
      hipLaunchKernelGGL(k_ddp_derivs<NJ>, g, dim3(64), 0, st, sys->dev, S, ldS, U, ldU, n, n_ep, rec);
      CACTO_CHECK_HIP(hipGetLastError());
      return CACTO_OK;
    } else {  // not reached: every caller is a car_park or revolute-chain instantiation
      set_error("cacto_ddp_launch_derivs: the closed-form systems have no derivative records");
      return CACTO_EUNSUPPORTED;
    }
  }
};

template <int NJ>
struct LaunchDdp {
  static int run(const cacto_sys* sys, const double* S, int64_t ldS, const double* U, int64_t ldU, const int32_t* n,
                 int n_ep, double mu, const cacto_to_box* box, double* out, hipStream_t st) {
    if constexpr (!DdpDims<NJ>::ok) {
      set_error("cacto_ddp_backward: supported for the single integrator, car and prismatic chains (double integrator)");
      return CACTO_EUNSUPPORTED;
    } else {
      if (!ddp_supported<NJ>(sys, "cacto_ddp_backward")) return CACTO_EUNSUPPORTED;
      // one instantiation of a recursion per bounds mode (the derivative kernels know no bounds)
      if constexpr (NJ > 2 || NJ == -2) {
        // split pass: per-step derivatives over (episode, step), then the recursion
        double* ws = nullptr;
        const int rc = cacto_ddp_workspace(const_cast<cacto_sys*>(sys), ddp_rec_doubles<NJ>(n_ep, ldS) * sizeof(double), &ws);
        if (rc != CACTO_OK) return rc;
        const int rc2 = LaunchDerivs<NJ>::run(sys, S, ldS, U, ldU, n, n_ep, ws, ldS, true, st);
        if (rc2 != CACTO_OK) return rc2;
        to_with_box(box, [&](auto bx) {
          hipLaunchKernelGGL((k_ddp_riccati_wave<NJ, decltype(bx)>), dim3(n_ep), dim3(64), 0, st, sys->dev, U, ldU, n,
                             n_ep, mu, ws, ldS, out, bx);
          return CACTO_OK;
        });
      } else {
        to_with_box(box, [&](auto bx) {
          hipLaunchKernelGGL((k_ddp_backward<NJ, decltype(bx)>), dim3(ceil_div(n_ep, 64)), dim3(64), 0, st, sys->dev, S,
                             ldS, U, ldU, n, n_ep, mu, out, bx);
          return CACTO_OK;
        });
      }
      CACTO_CHECK_HIP(hipGetLastError());
    }
    return CACTO_OK;
  }
};
template <int NJ>
struct LaunchJac {
  static int run(const cacto_sys* sys, const double* S, const double* U, int B, double* Fx, double* Fu,
                 hipStream_t st) {
    if constexpr (!DdpDims<NJ>::ok) {
      set_error("cacto_env_jacobians: unsupported dynamics");
      return CACTO_EUNSUPPORTED;
    } else {
      if (NJ == 2 && !sys->host.p.const_dyn) {
        set_error("cacto_env_jacobians: 2-joint chains are instantiated for the prismatic pair (double integrator)");
        return CACTO_EUNSUPPORTED;
      }
      if constexpr (NJ > 2) {
        using RC = DdpRec<NJ>;
        constexpr int ns = Dims<NJ>::NS;
        // step 0 of B one-step episodes: only A, B are read, so no l_x, l_xx
        const size_t rec = ddp_rec_doubles<NJ>(B, 1), s2 = (size_t)2 * B * ns;
        double* ws = nullptr;
        const int rc = cacto_ddp_workspace(const_cast<cacto_sys*>(sys), (rec + s2 + B) * sizeof(double), &ws);
        if (rc != CACTO_OK) return rc;
        double* S2 = ws + rec;
        int32_t* n1 = reinterpret_cast<int32_t*>(S2 + s2);
        hipLaunchKernelGGL(k_jac_prep<NJ>, dim3(ceil_div(B * 2 * ns, 256)), dim3(256), 0, st, S, B, S2, n1);
        CACTO_CHECK_HIP(hipGetLastError());
        const int rc2 = LaunchDerivs<NJ>::run(sys, S2, 2, U, 1, n1, B, ws, 1, false, st);
        if (rc2 != CACTO_OK) return rc2;
        constexpr int per = RC::N * RC::N + RC::N * RC::M;
        hipLaunchKernelGGL(k_jac_extract<NJ>, dim3(ceil_div(B * per, 256)), dim3(256), 0, st, ws, B, Fx, Fu);
      } else {
        hipLaunchKernelGGL(k_env_jacobians<NJ>, dim3(ceil_div(B, 64)), dim3(64), 0, st, sys->dev, S, U, B, Fx, Fu);
      }
      CACTO_CHECK_HIP(hipGetLastError());
      return CACTO_OK;
    }
  }
};
}  // namespace

int cacto_ddp_launch_derivs(const cacto_sys* sys, const double* S, int64_t ldS, const double* U, int64_t ldU,
                            const int32_t* nsteps, int n_ep, double* rec, int64_t steps, bool want_lx, hipStream_t st) {
  return dispatch_nj<LaunchDerivs>(sys->host.p, sys, S, ldS, U, ldU, nsteps, n_ep, rec, steps, want_lx, st);
}

extern "C" int cacto_ddp_backward_box(const cacto_sys* sys, const double* S_traj_d, int64_t ldS, const double* U_traj_d,
                                      int64_t ldU, const int32_t* nsteps_d, int n_ep, double mu, double* dVdx_d,
                                      void* stream, const cacto_to_box* box) {
  CACTO_TO_REQUIRE_BOX(box, sys, "cacto_ddp_backward");
  CACTO_REQUIRE(sys && S_traj_d && U_traj_d && nsteps_d && dVdx_d && n_ep >= 0 && ldS >= 1 && ldU >= 0,
                "cacto_ddp_backward: bad arguments");
  if (n_ep == 0) return CACTO_OK;
  return dispatch_nj<LaunchDdp>(sys->host.p, sys, S_traj_d, ldS, U_traj_d, ldU, nsteps_d, n_ep, mu, box, dVdx_d,
                                as_stream(stream));
}

extern "C" int cacto_ddp_backward(const cacto_sys* sys, const double* S_traj_d, int64_t ldS, const double* U_traj_d,
                                  int64_t ldU, const int32_t* nsteps_d, int n_ep, double mu, double* dVdx_d,
                                  void* stream) {
  return cacto_ddp_backward_box(sys, S_traj_d, ldS, U_traj_d, ldU, nsteps_d, n_ep, mu, dVdx_d, stream, nullptr);
}

extern "C" int cacto_env_jacobians(const cacto_sys* sys, const double* S_d, const double* A_d, int B, double* Fx_d,
                                   double* Fu_d, void* stream) {
  CACTO_REQUIRE(sys && S_d && A_d && Fx_d && Fu_d && B >= 0, "cacto_env_jacobians: bad arguments");
  if (B == 0) return CACTO_OK;
  return dispatch_nj<LaunchJac>(sys->host.p, sys, S_d, A_d, B, Fx_d, Fu_d, as_stream(stream));
}
