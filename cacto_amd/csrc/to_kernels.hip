// TO_System_Solve (TO.py:37-100) on the GPU: a batched iLQR on the reference's problem.
//
// The reference states one NLP per episode (CasADi + IPOPT, multiple shooting): minimise
// sum_t cost(x_t, u_t; w_running) + cost(x_T; w_terminal) subject to x_{t+1} = simulate(x_t, u_t) and
// the given x_0, with the control bounds as the penalty w_b (u/u_max)^10 inside the cost
// (environment_TO.py:201-206). Apart from the dynamics it is unconstrained, so single shooting
// with Gauss-Newton DDP works on exactly that problem:
//   backward   Q_x = l_x + A^T V_x, Q_u = l_u + B^T V_x, Q_xx = l_xx + A^T V_xx A,
//              Q_ux = B^T V_xx A, Q_uu = l_uu + B^T V_xx B (cost convention, l_xu = 0),
//              Qbar_uu = Q_uu + mu I by Cholesky (a pivot <= 0: not positive definite, raise mu),
//              k = -Qbar_uu^-1 Q_u, K = -Qbar_uu^-1 Q_ux,
//              V_x = Q_x + K^T Q_uu k + K^T Q_u + Q_ux^T k,
//              V_xx = Q_xx + K^T Q_uu K + K^T Q_ux + Q_ux^T K, symmetrised;
//   forward    u_t = ubar_t + alpha k_t + K_t (x_t - xbar_t), x_{t+1} = env_simulate (float64), the
//              largest alpha = 2^-j, j = 0..max_ls, with J - J(alpha) >= armijo * -(alpha dJ1 +
//              alpha^2 dJ2) and J(alpha) <= J;
//   mu         x mu_up (at least mu_min) after a failed factorisation or line search, / mu_down
//              after an accepted step (0 once below mu_min).
// The derivatives are those of cacto_ddp_backward (ddp_device.h; they are the reward's, so the
// signs flip on the way in; car_park's and the chains' records come from cacto_ddp_launch_derivs of
// ddp_kernels.hip, this file instantiates no derivative kernel). Everything is float64 VALU and
// LDS; there is no matrix-core work here.
// With cacto_to_opts.hessian = CACTO_TO_HESS_PSD every node's l_xx is first replaced by its projection
// onto the positive semidefinite cone (psd_project.h): a bool template parameter of the solving
// kernels, and for the records of the label pass's derivative kernels one more kernel
// (k_to_psd_records); nothing else of the algorithm changes.
// With a cacto_to_box of mode CACTO_TO_BOUNDS_BOX the problem gains hard limits lo <= u <= hi and the
// method becomes control-limited DDP (Tassa, Mansard, Todorov, ICRA 2014): after the same Cholesky
// verdict on Qbar_uu, k is the solution of the node's box QP (box_qp.h) over lo - ubar <= x <= hi - ubar,
// K = -Qbar_ff^-1 Q_ux,f on the rows the QP leaves free and exactly 0 on the clamped ones, dJ[2] skips
// the components held at a bound, and every roll-out (the warm start's too) clamps its controls. The
// bounds are a class template parameter of every kernel (ToNoBox / ToBoxDev): without them each kernel
// is what it was. cacto_ddp_backward, the label pass, knows no bounds: along a bounded trajectory the
// Sobolev labels are the reference's unconstrained dV/dx (TO.py:119-202).
//
//
// The file, in order:
//   the pieces of a pass  to_riccati_step / to_gains_episode (the same algebra on one thread / spread
//                         over a workgroup), to_node_record + to_backward_thread (a closed-form
//                         episode's records and its recursion), to_forward_thread (a roll-out);
//   the loop              ToIter, one episode's status / pass count / mu / J / J0, and its transitions
//                         to_enter, to_iter_begin, to_verdict, to_decide, to_iter_store: the entry
//                         checks, the stopping rule and the mu schedule are there and nowhere else;
//                         the warm start and the line search's candidate beside them;
//   the route and the map to_route<NJ>(path) names the solver of a (system, path); ToWs<NJ> carves
//                         the workspace for it and hands the kernels their pointers and views;
//   the four solvers      each runs that loop and differs in who computes a pass and where the state
//                         lives between passes:
//     k_to_solve_thread   single integrator, car, double integrator, path 0: one thread per episode,
//                         episodes handed out longest first (k_to_order); sequential backtracking;
//     k_to_solve_wave     the same systems, path 1: one 64-lane workgroup per episode, records over
//                         the lanes, the recursion on lane 0, every step size at once;
//     host-issued         car_park, manipulator, UR5, path 0 (the chains also path 1): k_to_init,
//                         then per pass the label pass's derivative kernels, k_to_gains_wave and
//                         k_to_linesearch, the state in global memory (ToState) between launches;
//     k_to_solve_split    car_park, path 1: those kernels' bodies run by one 256-thread workgroup
//                         per episode.
//   The library is built with -ffp-contract=off and the solvers share these functions, so the two
//   solvers of a system give the same numbers bit for bit.
#include "ddp_device.h"
#include "box_qp.h"
#include "psd_project.h"

namespace cacto {

// element (t, i) of a per-episode array at p[t * st + i * si]: the caller's [e][t][i] layout
// (st = width, si = 1) or the workspace's [t][i][e] (st = width * n_ep, si = n_ep)
struct View {
  double* p;
  size_t st, si;
  __device__ __forceinline__ double& at(int t, int i) const { return p[(size_t)t * st + (size_t)i * si]; }
};
struct Traj {
  View S, U;
};
struct Gains {
  View k, K;  // K: element (i, j) of step t at index i * N + j
};

// The control bounds of a call (ToNoBox / ToBoxDev, ddp_device.h) are a template parameter of every
// kernel below and its last argument.

// The gains of a node under bounds, on one thread: k = argmin 1/2 x^T Qbar x + Q_u^T x over
// lo - ubar <= x <= hi - ubar (the offsets by box_offset_lo / box_offset_hi, so that a clamped control's
// full step reaches its bound exactly; Qbar = Q_uu + mu I, whose own Cholesky verdict the caller has
// taken already); Lf the factor of its free block (box_chol_free). false: the QP gave no solution, which the
// caller treats as a Qbar that is not positive definite.
template <int M>
__device__ __forceinline__ bool to_box_gain(const ToBoxDev& bx, const double* Quu, double mu, const double* Qu, const double* ub,
                                            double* k, unsigned* free_mask, double* Lf) {
  double Hb[M * M], bl[M], bh[M];
#pragma unroll
  for (int j = 0; j < M; ++j) {
#pragma unroll
    for (int c = 0; c < M; ++c) Hb[j * M + c] = Quu[j * M + c] + (j == c ? mu : 0.0);
    bl[j] = box_offset_lo(ub[j], bx.lo[j]);
    bh[j] = box_offset_hi(ub[j], bx.hi[j]);
  }
  return to_box_qp<M>(Hb, Qu, bl, bh, k, free_mask, Lf);
}

// The TO cost of one node: -Env.reward; UR5.reward leaves the bound penalty to reward_batch
// (environment.py:780-805) while its TO cost has it (environment_TO.py:731-758), so it is added here.
template <int NJ>
__device__ inline double to_cost(const SysDevice& sd, const double* w, const double* s, const double* u) {
  double c = -env_reward<NJ>(sd, w, s, u, false);
  if constexpr (NJ > 2) {
    if (u && sd.p.reward_kind == CACTO_REW_UR5) {
      double b = 0.0;
#pragma unroll
      for (int i = 0; i < NJ; ++i) b += sd.p.w_b * pow(u[i] / sd.p.u_max[i], 10.0);
      c += sd.p.scale * (w[6] * b);
    }
  }
  return c;
}

// Cholesky of the M x M matrix a (lower triangle, in place, L L^T): false at a pivot <= 0 or a
// non-finite one.
template <int M>
__device__ inline bool to_chol(double* a) {
#pragma unroll
  for (int j = 0; j < M; ++j) {
    double d = a[j * M + j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= a[j * M + k] * a[j * M + k];
    if (!(d > 0.0) || !isfinite(d)) return false;
    const double l = sqrt(d);
    a[j * M + j] = l;
#pragma unroll
    for (int i = j + 1; i < M; ++i) {
      double s = a[i * M + j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= a[i * M + k] * a[j * M + k];
      a[i * M + j] = s / l;
    }
  }
  return true;
}
// x <- (L L^T)^-1 x, x with stride sx
template <int M>
__device__ inline void to_chol_solve(const double* L, double* x, int sx) {
#pragma unroll
  for (int i = 0; i < M; ++i) {
    double s = x[i * sx];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= L[i * M + k] * x[k * sx];
    x[i * sx] = s / L[i * M + i];
  }
#pragma unroll
  for (int i = M - 1; i >= 0; --i) {
    double s = x[i * sx];
#pragma unroll
    for (int k = i + 1; k < M; ++k) s -= L[k * M + i] * x[k * sx];
    x[i * sx] = s / L[i * M + i];
  }
}

// One step of the backward recursion on one thread (cost convention). In: A, B, l_x, l_xx, l_u,
// diagonal l_uu, V_x / V_xx of step t+1. Out: k [M], K [M*N], V_x / V_xx of step t, dJ
// accumulated. false: Qbar_uu is not positive definite (nothing is updated). Under bounds (ub: the
// node's nominal control) Qbar_uu is factored for that verdict all the same; then k is the box QP's
// solution, K = -Qbar_ff^-1 Q_ux,f on its free rows and exactly 0 on the clamped ones, and dJ[2]
// leaves out the components held at a bound; V_x, V_xx, dJ[0], dJ[1] are the same formulas.
template <int N, int M, class BX>
__device__ inline bool to_riccati_step(const double* A, const double* B, const double* lx, const double* lxx,
                                       const double* lu, const double* luu, double mu, const BX& bx, const double* ub,
                                       double* Vx, double* Vxx, double* k, double* K, double* dJ) {
  double Qx[N], Qu[M], Qxx[N * N], Qux[M * N], Quu[M * M], VA[N * N], VB[N * M];
#pragma unroll
  for (int r = 0; r < N; ++r) {
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < N; ++c) s += A[c * N + r] * Vx[c];
    Qx[r] = lx[r] + s;
  }
#pragma unroll
  for (int j = 0; j < M; ++j) {
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < N; ++c) s += B[c * M + j] * Vx[c];
    Qu[j] = lu[j] + s;
  }
#pragma unroll
  for (int r = 0; r < N; ++r) {
#pragma unroll
    for (int c = 0; c < N; ++c) {
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < N; ++q) s += Vxx[r * N + q] * A[q * N + c];
      VA[r * N + c] = s;
    }
#pragma unroll
    for (int c = 0; c < M; ++c) {
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < N; ++q) s += Vxx[r * N + q] * B[q * M + c];
      VB[r * M + c] = s;
    }
  }
#pragma unroll
  for (int r = 0; r < N; ++r)
#pragma unroll
    for (int c = 0; c < N; ++c) {
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < N; ++q) s += A[q * N + r] * VA[q * N + c];
      Qxx[r * N + c] = lxx[r * N + c] + s;
    }
#pragma unroll
  for (int j = 0; j < M; ++j) {
#pragma unroll
    for (int c = 0; c < N; ++c) {
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < N; ++q) s += B[q * M + j] * VA[q * N + c];
      Qux[j * N + c] = s;
    }
#pragma unroll
    for (int c = 0; c < M; ++c) {
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < N; ++q) s += B[q * M + j] * VB[q * M + c];
      Quu[j * M + c] = (j == c ? luu[j] : 0.0) + s;
    }
  }
  double L[M * M];
#pragma unroll
  for (int j = 0; j < M; ++j)
#pragma unroll
    for (int c = 0; c < M; ++c) L[j * M + c] = Quu[j * M + c] + (j == c ? mu : 0.0);
  if (!to_chol<M>(L)) return false;
  if constexpr (BX::on) {
    unsigned fm;
    if (!to_box_gain<M>(bx, Quu, mu, Qu, ub, k, &fm, L)) return false;
#pragma unroll
    for (int j = 0; j < M; ++j)
#pragma unroll
      for (int c = 0; c < N; ++c) K[j * N + c] = ((fm >> j) & 1u) ? -Qux[j * N + c] : 0.0;
#pragma unroll
    for (int c = 0; c < N; ++c) to_chol_solve<M>(L, K + c, N);
#pragma unroll
    for (int j = 0; j < M; ++j)
      if (!((fm >> j) & 1u))
#pragma unroll
        for (int c = 0; c < N; ++c) K[j * N + c] = 0.0;
  } else {
#pragma unroll
    for (int j = 0; j < M; ++j) k[j] = -Qu[j];
    to_chol_solve<M>(L, k, 1);
#pragma unroll
    for (int q = 0; q < M * N; ++q) K[q] = -Qux[q];
#pragma unroll
    for (int c = 0; c < N; ++c) to_chol_solve<M>(L, K + c, N);
  }
  double Tk[M], T[M * N], d0 = 0.0, d1 = 0.0, d2 = dJ[2];
#pragma unroll
  for (int j = 0; j < M; ++j) {
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < M; ++c) s += Quu[j * M + c] * k[c];
    Tk[j] = s;
#pragma unroll
    for (int c = 0; c < N; ++c) {
      double v = 0.0;
#pragma unroll
      for (int q = 0; q < M; ++q) v += Quu[j * M + q] * K[q * N + c];
      T[j * N + c] = v;
    }
  }
#pragma unroll
  for (int j = 0; j < M; ++j) {
    d0 += k[j] * Qu[j];
    d1 += k[j] * Tk[j];
    if constexpr (BX::on) {
      if (!bx.held(j, ub[j], Qu[j])) d2 = fmax(d2, fabs(Qu[j]));
    } else {
      d2 = fmax(d2, fabs(Qu[j]));
    }
  }
  dJ[0] += d0;
  dJ[1] += 0.5 * d1;
  dJ[2] = d2;
#pragma unroll
  for (int r = 0; r < N; ++r) {
    double s = Qx[r];
#pragma unroll
    for (int j = 0; j < M; ++j) s += K[j * N + r] * (Tk[j] + Qu[j]) + Qux[j * N + r] * k[j];
    Vx[r] = s;
  }
  double W[N * N];
#pragma unroll
  for (int r = 0; r < N; ++r)
#pragma unroll
    for (int c = 0; c < N; ++c) {
      double s = Qxx[r * N + c];
#pragma unroll
      for (int j = 0; j < M; ++j) s += K[j * N + r] * (T[j * N + c] + Qux[j * N + c]) + Qux[j * N + r] * K[j * N + c];
      W[r * N + c] = s;
    }
#pragma unroll
  for (int r = 0; r < N; ++r)
#pragma unroll
    for (int c = 0; c < N; ++c) Vxx[r * N + c] = 0.5 * (W[r * N + c] + W[c * N + r]);
  return true;
}

// M^-1 of a constant-M chain (the double integrator) at the episode's first node, once per episode
template <int NJ>
struct ToMinv {
  double a[NJ > 0 ? NJ * NJ : 1];
  __device__ __forceinline__ ToMinv(const SysDevice& sd, const Traj& cur) {
    if constexpr (NJ > 0) {
      double q0[NJ], Mm[NJ * NJ];
#pragma unroll
      for (int i = 0; i < NJ; ++i) q0[i] = cur.S.at(0, i);
      chain_mass<NJ>(sd, q0, Mm);
      small_inverse<NJ>(Mm, a);
    }
  }
};

// Per-node record of a closed-form episode: DdpRec's A, B, l_x, l_xx (here in the cost
// convention, the signs already flipped) followed by l_u [M] and the diagonal of l_uu [M]. The
// wave solver keeps them [e][t][k]: one episode's records are contiguous, a node's record is what
// the recursion reads in one go.
template <int NJ>
struct ToRec {
  using RC = DdpRec<NJ>;
  static constexpr int N = RC::N, M = RC::M;
  static constexpr int LU = RC::R, LUU = LU + M, R = LUU + M;
};

// The record of node t of one closed-form episode (terminal, t == Te: l_x, l_xx of the terminal
// weights only). A caller that knows terminal at compile time keeps the weights uniform. PSD: l_xx is
// replaced by its projection onto the positive semidefinite cone (the "psd" Hessian mode).
template <int NJ, bool PSD>
__device__ inline void to_node_record(const SysDevice& sd, const double* Minv, const Traj& cur, int t, bool terminal,
                                      double* r) {
  using TR = ToRec<NJ>;
  using RC = DdpRec<NJ>;
  constexpr int N = TR::N, M = TR::M;
  const cacto_sys_params& p = sd.p;
  double w[7], x[N], lx[N], lxx[N * N];
#pragma unroll
  for (int k = 0; k < 7; ++k) w[k] = terminal ? p.w_terminal[k] : p.w_running[k];
#pragma unroll
  for (int k = 0; k < N; ++k) x[k] = cur.S.at(t, k);
  ddp_lx<NJ>(sd, w, x, lx, lxx);
#pragma unroll
  for (int k = 0; k < N; ++k) r[RC::LX + k] = -lx[k];
  if constexpr (PSD) {
#pragma unroll
    for (int k = 0; k < N * N; ++k) lxx[k] = -lxx[k];
    psd_project<N>(lxx);
#pragma unroll
    for (int k = 0; k < N * N; ++k) r[RC::LXX + k] = lxx[k];
  } else {
#pragma unroll
    for (int k = 0; k < N * N; ++k) r[RC::LXX + k] = -lxx[k];
  }
  if (terminal) return;
  double A[N * N], B[N * M];
  ddp_jacobians<NJ>(sd, x, Minv, A, B);
#pragma unroll
  for (int k = 0; k < N * N; ++k) r[RC::A + k] = A[k];
#pragma unroll
  for (int k = 0; k < N * M; ++k) r[RC::B + k] = B[k];
#pragma unroll
  for (int j = 0; j < M; ++j) {
    double lu, luu;  // the reward's, as l_x, l_xx above
    ddp_lu(p, w[6], cur.U.at(t, j), j, &lu, &luu);
    r[TR::LU + j] = -lu;
    r[TR::LUU + j] = -luu;
  }
}

// The backward pass of one closed-form episode on one thread. node(t, terminal, buf) is node t's
// record: evaluated into buf [ToRec::R] on the spot (k_to_solve_thread, k_to_gains_thread) or read from
// where the lanes of k_to_solve_wave left it. Returns -1, or the step at which Qbar_uu was not
// positive definite. dJ [3] is reset here. U: the episode's nominal controls (read under bounds only).
template <int NJ, class BX, class Node>
__device__ inline int to_backward_thread(Node node, int Te, double mu, const BX& bx, const View& U, const Gains& g,
                                         double* dJ) {
  using TR = ToRec<NJ>;
  using RC = DdpRec<NJ>;
  constexpr int N = TR::N, M = TR::M;
  double buf[TR::R], Vx[N], Vxx[N * N];
  {
    const double* r = node(Te, true, buf);
#pragma unroll
    for (int k = 0; k < N; ++k) Vx[k] = r[RC::LX + k];
#pragma unroll
    for (int k = 0; k < N * N; ++k) Vxx[k] = r[RC::LXX + k];
  }
  dJ[0] = dJ[1] = dJ[2] = 0.0;
  for (int i = Te - 1; i >= 0; --i) {
    const double* r = node(i, false, buf);
    double kk[M], KK[M * N], ub[M];
    if constexpr (BX::on)
#pragma unroll
      for (int j = 0; j < M; ++j) ub[j] = U.at(i, j);
    if (!to_riccati_step<N, M>(r + RC::A, r + RC::B, r + RC::LX, r + RC::LXX, r + TR::LU, r + TR::LUU, mu, bx, ub, Vx, Vxx,
                               kk, KK, dJ))
      return i;
#pragma unroll
    for (int j = 0; j < M; ++j) g.k.at(i, j) = kk[j];
#pragma unroll
    for (int q = 0; q < M * N; ++q) g.K.at(i, q) = KK[q];
  }
  return -1;
}
// ... with every node evaluated on this thread
template <int NJ, bool PSD, class BX>
__device__ inline int to_backward_eval(const SysDevice& sd, const double* Minv, const Traj& cur, int Te, double mu,
                                       const BX& bx, const Gains& g, double* dJ) {
  return to_backward_thread<NJ, BX>(
      [&](int t, bool terminal, double* buf) -> const double* {
        to_node_record<NJ, PSD>(sd, Minv, cur, t, terminal, buf);
        return buf;
      },
      Te, mu, bx, cur.U, g, dJ);
}

// One roll-out of one episode on one thread: closed loop around (cur, g) with step size alpha, or
// open loop (g.k.p == nullptr). STORE: the new trajectory goes to nw and the node costs to cost
// (element t at cost.at(t, 0)); nw may be cur itself, since node t+1 of cur is read before node
// t+1 of nw is written. Returns the total cost. Under bounds every control is clamped to them before
// it is applied, the open-loop ones (a warm start's) included.
template <int NJ, bool STORE, class BX>
__device__ inline double to_forward_thread(const SysDevice& sd, const Traj& cur, const Gains& g, int Te, double alpha,
                                           const BX& bx, const Traj& nw, const View& cost) {
  constexpr int N = DdpDims<NJ>::N, M = DdpDims<NJ>::M, ns = N + 1;
  const cacto_sys_params& p = sd.p;
  double w_run[7], w_term[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    w_run[k] = p.w_running[k];
    w_term[k] = p.w_terminal[k];
  }
  double x[ns], xb[N], xn[ns], u[M];
#pragma unroll
  for (int k = 0; k < ns; ++k) x[k] = cur.S.at(0, k);
#pragma unroll
  for (int k = 0; k < N; ++k) xb[k] = x[k];
  const double t0 = x[N];
  if (STORE)
#pragma unroll
    for (int k = 0; k < ns; ++k) nw.S.at(0, k) = x[k];
  double J = 0.0;
  for (int t = 0; t < Te; ++t) {
#pragma unroll
    for (int j = 0; j < M; ++j) {
      double v = cur.U.at(t, j);
      if (g.k.p) {
        v += alpha * g.k.at(t, j);
#pragma unroll
        for (int c = 0; c < N; ++c) v += g.K.at(t, j * N + c) * (x[c] - xb[c]);
      }
      u[j] = bx.clamp(j, v);
    }
    const double c = to_cost<NJ>(sd, w_run, x, u);
    J += c;
    env_simulate<NJ>(sd, x, u, false, xn);
    xn[N] = t0 + p.dt * (double)(t + 1);  // TO.py:115: t0 + dt * t, by multiplication
#pragma unroll
    for (int k = 0; k < N; ++k) xb[k] = cur.S.at(t + 1, k);
    if (STORE) {
#pragma unroll
      for (int j = 0; j < M; ++j) nw.U.at(t, j) = u[j];
      cost.at(t, 0) = c;
#pragma unroll
      for (int k = 0; k < ns; ++k) nw.S.at(t + 1, k) = xn[k];
    }
#pragma unroll
    for (int k = 0; k < ns; ++k) x[k] = xn[k];
  }
  const double c = to_cost<NJ>(sd, w_term, x, nullptr);
  J += c;
  if (STORE) cost.at(Te, 0) = c;
  return J;
}

__device__ __forceinline__ bool to_valid_len(int Te, int64_t ldS, int64_t ldU) { return Te >= 0 && Te < ldS && Te <= ldU; }

// views of episode e in the caller's layout
template <int NJ>
__device__ __forceinline__ Traj api_traj(double* S, int64_t ldS, double* U, int64_t ldU, int e) {
  constexpr int ns = Dims<NJ>::NS, na = Dims<NJ>::NA;
  return Traj{View{S + (size_t)e * ldS * ns, (size_t)ns, 1}, View{U + (size_t)e * ldU * na, (size_t)na, 1}};
}
template <int NJ>
__device__ __forceinline__ Gains api_gains(double* k, double* K, int64_t ldU, int e) {
  constexpr int N = DdpDims<NJ>::N, na = Dims<NJ>::NA;
  return Gains{View{k ? k + (size_t)e * ldU * na : nullptr, (size_t)na, 1},
               View{K ? K + (size_t)e * ldU * na * N : nullptr, (size_t)na * N, 1}};
}

// cacto_to_backward_gains, closed-form family: one thread per episode.
template <int NJ, bool PSD, class BX>
__global__ void __launch_bounds__(64) k_to_gains_thread(const SysDevice* __restrict__ sdp, const double* S, int64_t ldS,
                                                         const double* U, int64_t ldU,
                                                         const int32_t* __restrict__ nsteps, int n_ep, double mu,
                                                         double* k_out, double* K_out, double* __restrict__ dJ_out,
                                                         int32_t* __restrict__ pd_out, BX bx) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_ep) return;
  const int Te = nsteps[e];
  if (!to_valid_len(Te, ldS, ldU)) return;
  const SysDevice& sd = *sdp;
  const Traj cur = api_traj<NJ>(const_cast<double*>(S), ldS, const_cast<double*>(U), ldU, e);
  const ToMinv<NJ> Minv(sd, cur);
  double dJ[3];
  const int pd = to_backward_eval<NJ, PSD>(sd, Minv.a, cur, Te, mu, bx, api_gains<NJ>(k_out, K_out, ldU, e), dJ);
  pd_out[e] = pd;
#pragma unroll
  for (int k = 0; k < 3; ++k) dJ_out[(size_t)e * 3 + k] = dJ[k];
}

// cacto_to_forward, every system: one thread per episode.
template <int NJ, class BX>
__global__ void __launch_bounds__(64) k_to_forward(const SysDevice* __restrict__ sdp, const double* S, int64_t ldS,
                                                    const double* U, int64_t ldU, const double* k_in,
                                                    const double* K_in, const int32_t* __restrict__ nsteps, int n_ep,
                                                    double alpha, double* S_new, double* U_new, double* cost_new, BX bx) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_ep) return;
  const int Te = nsteps[e];
  if (!to_valid_len(Te, ldS, ldU)) return;
  const Traj cur = api_traj<NJ>(const_cast<double*>(S), ldS, const_cast<double*>(U), ldU, e);
  const Traj nw = api_traj<NJ>(S_new, ldS, U_new, ldU, e);
  const Gains g = api_gains<NJ>(const_cast<double*>(k_in), const_cast<double*>(K_in), ldU, e);
  to_forward_thread<NJ, true>(*sdp, cur, g, Te, alpha, bx, nw, View{cost_new + (size_t)e * ldS, 1, 1});
}

struct ToCfgDev {
  int max_iter, max_ls;
  double gtol, armijo, mu_min, mu_up, mu_down, mu_max;
};

// ---------------------------------------------------------------------------------------------
// The iteration loop every solver runs, as the state of one episode and its transitions:
//   to_enter -> to_iter_begin(warm start's cost) -> while running and pass < max_iter:
//     backward pass -> to_verdict -> [TO_SEARCH: line search] -> to_decide
//   -> to_iter_store
// A solver's lanes that hold the state hold it alike, so every branch on it is uniform.
// ---------------------------------------------------------------------------------------------
struct ToOut {  // cacto_to_solve's per-episode results
  int32_t *status, *iters;
  double* J;  // [n_ep][2]: the warm start's cost, the final cost
};
struct ToIter {
  int status, iters;  // status MAXITER: still running
  double mu, J, J0;
  __device__ __forceinline__ bool running() const { return status == CACTO_TO_MAXITER; }
};

// mu after a failed factorisation or line search; true: past mu_max
__device__ __forceinline__ bool to_raise_mu(const ToCfgDev& c, double* mu) {
  *mu = fmax(*mu * c.mu_up, c.mu_min);
  return *mu > c.mu_max;
}
__device__ __forceinline__ void to_lower_mu(const ToCfgDev& c, double* mu) {
  *mu = *mu / c.mu_down;
  if (*mu < c.mu_min) *mu = 0.0;
}
__device__ __forceinline__ bool to_admissible(const ToCfgDev& c, double J, double Jc, double alpha, const double* dJ) {
  return isfinite(Jc) && (J - Jc >= c.armijo * -(alpha * dJ[0] + alpha * alpha * dJ[1])) && Jc <= J;
}

// Entry. false: there is nothing to optimise — the episode is skipped (Te < 0: no output is
// touched), or its length does not fit the caller's buffers (FAILED after 0 passes, written by
// the thread(s) with writer set).
__device__ __forceinline__ bool to_enter(int Te, int64_t ldS, int64_t ldU, const ToOut& out, int e, bool writer) {
  if (Te < 0) return false;
  if (to_valid_len(Te, ldS, ldU)) return true;
  if (writer) {
    out.status[e] = CACTO_TO_FAILED;
    out.iters[e] = 0;
  }
  return false;
}
// The state before the first pass, from the warm start's cost
__device__ __forceinline__ ToIter to_iter_begin(int Te, double J) {
  ToIter s{CACTO_TO_MAXITER, 0, 0.0, J, J};
  if (Te == 0) s.status = CACTO_TO_CONVERGED;
  if (!isfinite(J)) s.status = CACTO_TO_FAILED;
  return s;
}
// What a backward pass that returned pd (-1, or the step that was not positive definite) and dJ
// asks for: mu raised, nothing more (the stopping rule), or a line search along its gains
enum ToVerdict { TO_RAISE, TO_STOP, TO_SEARCH };
__device__ __forceinline__ ToVerdict to_verdict(const ToCfgDev& c, int pd, const double* dJ) {
  if (pd >= 0) return TO_RAISE;
  return dJ[2] <= c.gtol ? TO_STOP : TO_SEARCH;
}
// The end of a pass: after that verdict and, with TO_SEARCH, a line search that picked
// alpha = 2^-sel, whose roll-out costs Jsel, or nothing (sel < 0). A pass that gave no step
// raises mu (the retry counts as a pass; FAILED past mu_max), an accepted step lowers it.
__device__ __forceinline__ void to_decide(const ToCfgDev& c, ToIter& s, ToVerdict v, int sel, double Jsel) {
  ++s.iters;
  if (v == TO_STOP) {
    s.status = CACTO_TO_CONVERGED;
  } else if (v == TO_SEARCH && sel >= 0) {
    s.J = Jsel;
    to_lower_mu(c, &s.mu);
  } else if (to_raise_mu(c, &s.mu)) {
    s.status = CACTO_TO_FAILED;
  }
}
__device__ __forceinline__ void to_iter_store(const ToIter& s, const ToOut& out, int e) {
  out.status[e] = s.status;
  out.iters[e] = s.iters;
  out.J[(size_t)e * 2] = s.J0;
  out.J[(size_t)e * 2 + 1] = s.J;
}

// The host-issued solver keeps the state in global memory between its launches: live (Te while
// the episode is being optimised, -1 once finished or skipped: the derivative and gains kernels
// skip it), mu, J; pass count, status and J0 in the outputs; done counts the finished episodes
// (the host's poll).
struct ToState {
  int32_t* live;
  double* mu;
  double* J;
  int32_t* done;
};
__device__ __forceinline__ ToIter to_state_load(const ToState& st, const ToOut& out, int e) {
  return ToIter{CACTO_TO_MAXITER, out.iters[e], st.mu[e], st.J[e], out.J[(size_t)e * 2]};
}
__device__ __forceinline__ void to_state_store(const ToIter& s, int Te, const ToState& st, const ToOut& out, int e) {
  to_iter_store(s, out, e);
  st.mu[e] = s.mu;
  st.J[e] = s.J;
  st.live[e] = s.running() ? Te : -1;
  if (!s.running()) atomicAdd(st.done, 1);
}

// The warm start of one episode, in place in cur: the copy of s0 and of the controls of nodes
// first, first + stride, ... of U_init, then (on one thread, after the copy) the roll-out, which
// leaves the node costs in cost and returns their sum. Under bounds the roll-out clamps the controls
// it stores: the warm start the loop begins from, and whose cost is J[0], is the clamped one.
template <int NJ>
__device__ __forceinline__ void to_warm_copy(const double* S0, const double* U_init, int64_t ldU, int e, int Te,
                                             const Traj& cur, int first, int stride) {
  constexpr int ns = Dims<NJ>::NS, na = Dims<NJ>::NA;
  if (first == 0)
#pragma unroll
    for (int k = 0; k < ns; ++k) cur.S.at(0, k) = S0[(size_t)e * ns + k];
  for (int t = first; t < Te; t += stride)
#pragma unroll
    for (int j = 0; j < na; ++j) cur.U.at(t, j) = U_init[((size_t)e * ldU + t) * na + j];
}
template <int NJ, class BX>
__device__ __forceinline__ double to_warm_rollout(const SysDevice& sd, int Te, const BX& bx, const Traj& cur, const View& cost) {
  const Gains none{View{nullptr, 0, 0}, View{nullptr, 0, 0}};
  return to_forward_thread<NJ, true>(sd, cur, none, Te, 0.0, bx, cur, cost);
}
template <int NJ, class BX>
__device__ __forceinline__ double to_warm_start_thread(const SysDevice& sd, const double* S0, const double* U_init, int64_t ldU,
                                                       int e, int Te, const BX& bx, const Traj& cur, const View& cost) {
  to_warm_copy<NJ>(S0, U_init, ldU, e, Te, cur, 0, 1);
  return to_warm_rollout<NJ>(sd, Te, bx, cur, cost);
}

// One candidate of the line search on one thread: the cost of alpha = 2^-j rolled out without
// storing it, or NaN when the step is not admissible.
template <int NJ, class BX>
__device__ __forceinline__ double to_ls_candidate(const SysDevice& sd, const ToCfgDev& cfg, const Traj& cur, const Gains& g, int Te,
                                                  int j, double J, const double* dJ, const BX& bx, const View& cost) {
  const double alpha = ldexp(1.0, -j);
  const double Jc = to_forward_thread<NJ, false>(sd, cur, g, Te, alpha, bx, cur, cost);
  return to_admissible(cfg, J, Jc, alpha, dJ) ? Jc : __builtin_nan("");
}
// The smallest admissible j among to_ls_candidate's values cand [0..max_ls] — by definition what
// sequential backtracking picks — or -1 (always, where no search was asked for: all are NaN)
__device__ __forceinline__ int to_pick(const ToCfgDev& cfg, const double* cand) {
  for (int q = 0; q <= cfg.max_ls; ++q)
    if (cand[q] == cand[q]) return q;
  return -1;
}

// ---------------------------------------------------------------------------------------------
// Which solver runs a (system, path), and the one map of cacto_to_solve's workspace
// ---------------------------------------------------------------------------------------------
// The systems whose node derivatives come as records of the label pass's kernels (car_park,
// manipulator, UR5); the others (single integrator, car, double integrator) have closed forms
template <int NJ>
constexpr bool to_split() {
  return NJ > 2 || NJ == -2;
}
// Of those, car_park has a persistent kernel; the revolute chains have none
template <int NJ>
constexpr bool to_persistent() {
  return NJ == -2;
}
enum ToSolver {
  TO_SOLVER_THREAD,  // k_to_solve_thread
  TO_SOLVER_WAVE,    // k_to_solve_wave
  TO_SOLVER_HOST,    // k_to_init, then per pass the derivative kernels, k_to_gains_wave, k_to_linesearch
  TO_SOLVER_SPLIT,   // k_to_solve_split
};
template <int NJ>
constexpr ToSolver to_route(int path) {
  const bool wave = path == CACTO_TO_PATH_WAVE;
  if (!to_split<NJ>()) return wave ? TO_SOLVER_WAVE : TO_SOLVER_THREAD;
  return wave && to_persistent<NJ>() ? TO_SOLVER_SPLIT : TO_SOLVER_HOST;
}
// Threads per workgroup of k_to_solve_split: car_park's phases hold no per-thread LDS and a
// 100-step episode's nodes fit one stride
constexpr int TO_SPLIT_THREADS = 256;

inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }

// The workspace of cacto_to_solve as a solver sees it: 256-byte aligned blocks, carved in the
// constructor and nowhere else (ws may be null: bytes alone is wanted). E = n_ep, L = ldS.
//   thread  order [E] + hist [L + 1] | lanes: S [L][ns][E], U [L][na][E], cost [L][E], k [L][na][E],
//           K [L][na*nx][E], handed out by lanes_views
//   wave    order [E] + hist [L + 1] | a block of the thread solver's size, at its head per episode the
//           gains k [L][na], K [L][na*nx] | per episode the records [L][ToRec::R]
//   split   per episode the gains k [L][na], K [L][na*nx] | per episode the records [L][DdpRec::R]
//   host    live [E], pd [E], done | mu [E], J [E], dJ [E][3], k [E][L][na], K [E][L][na*nx] (indexed
//           with ldU <= L by the kernels) | the records [t][k][e] (+ the chains' primal workspace)
// The wave and split solvers keep trajectory and node costs in the caller's S / U / step_cost.
template <int NJ>
struct ToWs {
  static constexpr int N = DdpDims<NJ>::N, M = DdpDims<NJ>::M;
  size_t E, L, bytes;
  int32_t *order, *hist;  // k_to_order's output and scratch
  double* lanes;
  double *k, *K, *rec;
  ToState st;
  int32_t* pd;
  double* dJ;

  ToWs(void* ws, int n_ep, int64_t ldS, ToSolver solver) : E((size_t)n_ep), L((size_t)ldS), bytes(0) {
    order = hist = st.live = st.done = pd = nullptr;
    lanes = k = K = rec = st.mu = st.J = dJ = nullptr;
    const size_t g = E * L * M, G = g * N;
    if (solver == TO_SOLVER_THREAD || solver == TO_SOLVER_WAVE) {
      order = take<int32_t>(ws, E);
      hist = take<int32_t>(ws, L + 1);
      close();
      if (solver == TO_SOLVER_THREAD) {
        lanes = take<double>(ws, lanes_doubles(E, L));
        close();
      } else {
        k = take<double>(ws, lanes_doubles(E, L));
        close();
        rec = take<double>(ws, E * L * ToRec<NJ>::R);
        close();
      }
    } else {
      if (solver == TO_SOLVER_SPLIT) {
        k = take<double>(ws, g + G);
      } else {
        st.live = take<int32_t>(ws, E);
        pd = take<int32_t>(ws, E);
        st.done = take<int32_t>(ws, 1);
        close();
        st.mu = take<double>(ws, E);
        st.J = take<double>(ws, E);
        dJ = take<double>(ws, 3 * E);
        k = take<double>(ws, g);
        K = take<double>(ws, G);
      }
      close();
      rec = take<double>(ws, ddp_rec_doubles<NJ>(n_ep, ldS));
      close();
    }
  }
  // The thread solver's block, [t][k][e] (a wave's lanes touch consecutive addresses), and episode
  // e's views into it. k_to_solve_thread is given the block as one __restrict__ pointer, not this
  // struct: with the five arrays as pointers the compiler cannot tell from its other arguments it
  // ran a third slower at 4096 episodes (2.9 s against 2.1 s on the double integrator).
  static constexpr size_t lanes_doubles(size_t E, size_t L) { return E * L * (size_t)(N + 1 + M + 1 + M + M * N); }
  __device__ static __forceinline__ void lanes_views(double* blk, size_t E, size_t L, int e, Traj* cur, View* cost, Gains* g) {
    double* S = blk + e;
    double* U = S + L * (N + 1) * E;
    double* C = U + L * M * E;
    double* k = C + L * E;
    double* K = k + L * M * E;
    *cur = Traj{View{S, (N + 1) * E, E}, View{U, M * E, E}};
    *cost = View{C, E, E};
    *g = Gains{View{k, M * E, E}, View{K, (size_t)M * N * E, E}};
  }
  // episode e's gains (k [L][na], then K [L][na*nx], from this->k) and records (R doubles per
  // node), wave and split solvers
  __device__ __forceinline__ Gains episode_gains(int e) const {
    double* p = k + (size_t)e * L * (M + M * N);
    return Gains{View{p, (size_t)M, 1}, View{p + L * M, (size_t)M * N, 1}};
  }
  __device__ __forceinline__ double* episode_rec(int e, int R) const { return rec + (size_t)e * L * R; }

 private:
  template <class T>
  T* take(void* ws, size_t n) {
    T* p = ws ? reinterpret_cast<T*>(static_cast<char*>(ws) + bytes) : nullptr;
    bytes += n * sizeof(T);
    return p;
  }
  void close() { bytes = align256(bytes); }
};

// Episodes sorted by decreasing length (counting sort over Te; one workgroup). order [n_ep],
// hist [ldS + 1] scratch. The place of an episode among those of its own length depends on the
// atomics' order; it only decides which lane runs it.
__global__ void __launch_bounds__(256) k_to_order(const int32_t* __restrict__ nsteps, int n_ep, int64_t ldS,
                                                  int32_t* __restrict__ order, int32_t* __restrict__ hist) {
  const int nb = (int)ldS + 1;  // bucket 0: skipped or invalid, bucket b: Te = ldS - b
  for (int b = threadIdx.x; b < nb; b += blockDim.x) hist[b] = 0;
  __syncthreads();
  for (int e = threadIdx.x; e < n_ep; e += blockDim.x) {
    const int Te = nsteps[e];
    atomicAdd(&hist[(Te < 0 || Te >= ldS) ? 0 : (int)ldS - Te], 1);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    // longest first; bucket 0 (nothing to do) last
    int acc = 0;
    for (int b = 1; b < nb; ++b) {
      const int c = hist[b];
      hist[b] = acc;
      acc += c;
    }
    hist[0] = acc;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < n_ep; e += blockDim.x) {
    const int Te = nsteps[e];
    order[atomicAdd(&hist[(Te < 0 || Te >= ldS) ? 0 : (int)ldS - Te], 1)] = e;
  }
}

// The thread solver (closed-form systems, path 0): one thread per episode, the whole loop on the
// device; trajectory, node costs and gains in the workspace (ToWs::lanes_views), copied out at the
// end. Its own phases: the backward pass with every node evaluated on the spot, and sequential
// backtracking that stops at the first admissible step — a candidate's cost is evaluated without
// storing it, and the accepted one is rolled out again in place.
template <int NJ, bool PSD, class BX>
__global__ void __launch_bounds__(64) k_to_solve_thread(const SysDevice* __restrict__ sdp, const double* __restrict__ S0,
                                                         const double* __restrict__ U_init, int64_t ldU,
                                                         const int32_t* __restrict__ nsteps, int n_ep, int64_t ldS,
                                                         ToCfgDev cfg, const int32_t* __restrict__ order,
                                                         double* __restrict__ lanes, double* __restrict__ S_out,
                                                         double* __restrict__ U_out, double* __restrict__ cost_out,
                                                         int32_t* __restrict__ status_out, int32_t* __restrict__ iters_out,
                                                         double* __restrict__ J_out, BX bx) {
  constexpr int N = DdpDims<NJ>::N, M = DdpDims<NJ>::M, ns = N + 1;
  const int slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= n_ep) return;
  const int e = order[slot];
  const int Te = nsteps[e];
  const ToOut out{status_out, iters_out, J_out};
  if (!to_enter(Te, ldS, ldU, out, e, true)) return;
  const SysDevice& sd = *sdp;
  Traj cur;
  View cost;
  Gains g;
  ToWs<NJ>::lanes_views(lanes, (size_t)n_ep, (size_t)ldS, e, &cur, &cost, &g);
  ToIter s = to_iter_begin(Te, to_warm_start_thread<NJ>(sd, S0, U_init, ldU, e, Te, bx, cur, cost));
  if (s.running()) {
    const ToMinv<NJ> Minv(sd, cur);
    double dJ[3];
    for (int it = 0; it < cfg.max_iter && s.running(); ++it) {
      const ToVerdict v = to_verdict(cfg, to_backward_eval<NJ, PSD>(sd, Minv.a, cur, Te, s.mu, bx, g, dJ), dJ);
      int sel = -1;
      for (int j = 0; v == TO_SEARCH && j <= cfg.max_ls && sel < 0; ++j)
        if (!isnan(to_ls_candidate<NJ>(sd, cfg, cur, g, Te, j, s.J, dJ, bx, cost))) sel = j;
      to_decide(cfg, s, v, sel, sel >= 0 ? to_forward_thread<NJ, true>(sd, cur, g, Te, ldexp(1.0, -sel), bx, cur, cost) : s.J);
    }
  }
  for (int t = 0; t <= Te; ++t) {
#pragma unroll
    for (int k = 0; k < ns; ++k) S_out[((size_t)e * ldS + t) * ns + k] = cur.S.at(t, k);
    cost_out[(size_t)e * ldS + t] = cost.at(t, 0);
    if (t < Te)
#pragma unroll
      for (int j = 0; j < M; ++j) U_out[((size_t)e * ldU + t) * M + j] = cur.U.at(t, j);
  }
  to_iter_store(s, out, e);
}

// LDS of k_to_solve_wave: what lane 0 (the backward pass) and the lane of the accepted step hand
// to the others
struct ToWaveLds {
  double pass[4];  // dJ [3] of the backward pass; the cost of the roll-out just stored
  int pd;
};

// The wave solver (closed-form systems, path 1): one 64-lane workgroup per episode, for
// per-episode calls and batches too small to fill the device with one thread per episode. The
// trajectory and the node costs live in the caller's S / U / step_cost (rows past Te are never
// touched); gains and node records in the workspace (ToWs: episode_*). Its own phases: the lanes
// stride over the nodes for the records and lane 0 runs the recursion from them; lane
// j <= max_ls evaluates the cost of alpha = 2^-j without storing it, and the lane of the
// smallest admissible j rolls that step out in place.
template <int NJ, bool PSD, class BX>
__global__ void __launch_bounds__(64) k_to_solve_wave(const SysDevice* __restrict__ sdp, const double* __restrict__ S0,
                                                       const double* U_init, int64_t ldU,
                                                       const int32_t* __restrict__ nsteps, int n_ep, int64_t ldS,
                                                       ToCfgDev cfg, ToWs<NJ> lay, double* S_out, double* U_out,
                                                       double* cost_out, int32_t* __restrict__ status_out,
                                                       int32_t* __restrict__ iters_out, double* __restrict__ J_out, BX bx) {
  using TR = ToRec<NJ>;
  __shared__ ToWaveLds lds;
  const int lane = threadIdx.x;
  const int e = lay.order[blockIdx.x];
  const int Te = nsteps[e];
  const ToOut out{status_out, iters_out, J_out};
  if (!to_enter(Te, ldS, ldU, out, e, lane == 0)) return;  // uniform over the workgroup
  const SysDevice& sd = *sdp;
  const Traj cur = api_traj<NJ>(S_out, ldS, U_out, ldU, e);
  const View cost{cost_out + (size_t)e * ldS, 1, 1};
  const Gains g = lay.episode_gains(e);
  double* rec = lay.episode_rec(e, TR::R);
  to_warm_copy<NJ>(S0, U_init, ldU, e, Te, cur, lane, 64);
  __syncthreads();
  if (lane == 0) lds.pass[3] = to_warm_rollout<NJ>(sd, Te, bx, cur, cost);
  __syncthreads();
  ToIter s = to_iter_begin(Te, lds.pass[3]);
  if (s.running()) {
    const ToMinv<NJ> Minv(sd, cur);
    for (int it = 0; it < cfg.max_iter && s.running(); ++it) {
      for (int t = lane; t <= Te; t += 64) to_node_record<NJ, PSD>(sd, Minv.a, cur, t, t == Te, rec + (size_t)t * TR::R);
      __syncthreads();
      if (lane == 0) {
        double d[3];
        lds.pd = to_backward_thread<NJ, BX>([rec](int t, bool, double*) { return (const double*)(rec + (size_t)t * TR::R); },
                                            Te, s.mu, bx, cur.U, g, d);
#pragma unroll
        for (int k = 0; k < 3; ++k) lds.pass[k] = d[k];
      }
      __syncthreads();
      const double dJ[3] = {lds.pass[0], lds.pass[1], lds.pass[2]};
      const ToVerdict v = to_verdict(cfg, lds.pd, dJ);
      int sel = -1;
      if (v == TO_SEARCH) {
        const bool ok = lane <= cfg.max_ls && !isnan(to_ls_candidate<NJ>(sd, cfg, cur, g, Te, lane, s.J, dJ, bx, cost));
        sel = __ffsll(__ballot(ok)) - 1;
        if (lane == sel) lds.pass[3] = to_forward_thread<NJ, true>(sd, cur, g, Te, ldexp(1.0, -sel), bx, cur, cost);
        __syncthreads();
      }
      to_decide(cfg, s, v, sel, lds.pass[3]);
    }
  }
  if (lane == 0) to_iter_store(s, out, e);
}

// The "psd" Hessian mode on a split-family node's record: the l_xx block (the reward's, as the
// derivative kernels leave it) replaced by -P(-l_xx), the projection taken in the cost convention.
// rec, es as ddp_derivs_node.
template <int NJ>
__device__ __forceinline__ void to_psd_record(double* rec, size_t es) {
  using RC = DdpRec<NJ>;
  constexpr int N = RC::N;
  double h[N * N];
#pragma unroll
  for (int k = 0; k < N * N; ++k) h[k] = -rec[(size_t)(RC::LXX + k) * es];
  psd_project<N>(h);
#pragma unroll
  for (int k = 0; k < N * N; ++k) rec[(size_t)(RC::LXX + k) * es] = -h[k];
}

// ... as a kernel of its own over the [t][k][e] records of the label pass's derivative kernels
// (the host-issued solver and cacto_to_backward_gains), one thread per (episode, step), run after
// them: k_ddp_lx<3/6> already spills, and the label pass must keep the exact Hessian.
template <int NJ>
__global__ void __launch_bounds__(64) k_to_psd_records(const int32_t* __restrict__ nsteps, int n_ep, double* __restrict__ ws) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const int t = blockIdx.y;
  if (e >= n_ep) return;
  if (t > nsteps[e]) return;  // also Te < 0: skipped, as k_ddp_derivs
  to_psd_record<NJ>(ws + (size_t)t * DdpRec<NJ>::R * n_ep + e, (size_t)n_ep);
}

// LDS of the backward pass of one split-family episode (operands, products, gains of one step)
template <int NJ>
struct ToGainsLds {
  static constexpr int N = DdpRec<NJ>::N, M = DdpRec<NJ>::M;
  double sA[N * N], sB[N * M], sLx[N], sLxx[N * N], sVx[N], sVxx[N * N], sU[M];
  double sVA[N * N], sVB[N * M], sQx[N], sQu[M], sQxx[N * N], sQux[M * N], sQuu[M * M];
  double sk[M], sK[M * N], sTk[M], sT[M * N], sW[N * N];
  int sFail;
};

// The backward pass of one split-family episode with gains, run by a whole workgroup of BT threads
// (lane: the thread's index in it): every product's outputs spread over the threads (one thread
// forms one output, always in the same summation order, so the width does not change a number),
// operands in LDS, the M x M Cholesky and its solves on thread 0. Every thread of the workgroup must
// call it: the step loop's barriers are workgroup barriers and every branch around them is uniform.
// rec: the episode's derivative records (the reward's: l_x, l_xx change sign on load), element k of
// node t at rec[t * ts + k * es]. Ue, ke, Ke: the episode's controls [.][na] and gains [.][na],
// [.][na][N]. Returns, on thread 0, pd = -1 or the step at which Qbar_uu was not positive definite,
// and dJ [3]; the other threads' values mean nothing. The LDS is free again once every thread has left
// and passed a barrier. No pointer here is __restrict__: the persistent solver reads what its own
// workgroup wrote earlier in the same kernel.
struct ToPass {
  int pd;
  double dJ[3];
};
template <int NJ, int BT, class BX>
__device__ __forceinline__ ToPass to_gains_episode(ToGainsLds<NJ>& L, const cacto_sys_params& p, const double* Ue, int Te, double mu,
                                        const BX& bx, const double* rec_e, size_t ts, size_t es, double* ke, double* Ke,
                                        int lane) {
  using RC = DdpRec<NJ>;
  constexpr int N = RC::N, M = RC::M, na = Dims<NJ>::NA;
  const double w6 = p.w_running[6];
  {
    const double* rec = rec_e + (size_t)Te * ts;
    for (int k = lane; k < N; k += BT) L.sVx[k] = -rec[(size_t)(RC::LX + k) * es];
    for (int k = lane; k < N * N; k += BT) L.sVxx[k] = -rec[(size_t)(RC::LXX + k) * es];
    if (lane == 0) L.sFail = 0;
  }
  double d0 = 0.0, d1 = 0.0, d2 = 0.0;  // lane 0's
  int pd = -1;
  __syncthreads();
  for (int i = Te - 1; i >= 0; --i) {
    const double* rec = rec_e + (size_t)i * ts;
    for (int k = lane; k < N * N; k += BT) {
      L.sA[k] = rec[(size_t)(RC::A + k) * es];
      L.sLxx[k] = -rec[(size_t)(RC::LXX + k) * es];
    }
    for (int k = lane; k < N * M; k += BT) L.sB[k] = rec[(size_t)(RC::B + k) * es];
    for (int k = lane; k < N; k += BT) L.sLx[k] = -rec[(size_t)(RC::LX + k) * es];
    for (int k = lane; k < M; k += BT) L.sU[k] = Ue[(size_t)i * na + k];
    __syncthreads();
    // V_xx A, V_xx B, Q_x = l_x + A^T V_x, Q_u = l_u + B^T V_x
    for (int o = lane; o < N * N + N * M + N + M; o += BT) {
      double s = 0.0;
      if (o < N * N) {
        const int r = o / N, c = o - r * N;
#pragma unroll
        for (int k = 0; k < N; ++k) s += L.sVxx[r * N + k] * L.sA[k * N + c];
        L.sVA[o] = s;
      } else if (o < N * N + N * M) {
        const int q = o - N * N, r = q / M, c = q - r * M;
#pragma unroll
        for (int k = 0; k < N; ++k) s += L.sVxx[r * N + k] * L.sB[k * M + c];
        L.sVB[q] = s;
      } else if (o < N * N + N * M + N) {
        const int r = o - N * N - N * M;
#pragma unroll
        for (int k = 0; k < N; ++k) s += L.sA[k * N + r] * L.sVx[k];
        L.sQx[r] = L.sLx[r] + s;
      } else {
        const int j = o - N * N - N * M - N;
        double lu, luu;  // the reward's: negated
        ddp_lu(p, w6, L.sU[j], j, &lu, &luu);
#pragma unroll
        for (int k = 0; k < N; ++k) s += L.sB[k * M + j] * L.sVx[k];
        L.sQu[j] = -lu + s;
      }
    }
    __syncthreads();
    // Q_xx = l_xx + A^T V_xx A, Q_ux = B^T V_xx A, Q_uu = l_uu + B^T V_xx B
    for (int o = lane; o < N * N + M * N + M * M; o += BT) {
      double s = 0.0;
      if (o < N * N) {
        const int r = o / N, c = o - r * N;
#pragma unroll
        for (int k = 0; k < N; ++k) s += L.sA[k * N + r] * L.sVA[k * N + c];
        L.sQxx[o] = L.sLxx[o] + s;
      } else if (o < N * N + M * N) {
        const int q = o - N * N, j = q / N, c = q - j * N;
#pragma unroll
        for (int k = 0; k < N; ++k) s += L.sB[k * M + j] * L.sVA[k * N + c];
        L.sQux[q] = s;
      } else {
        const int q = o - N * N - M * N, r = q / M, c = q - r * M;
#pragma unroll
        for (int k = 0; k < N; ++k) s += L.sB[k * M + r] * L.sVB[k * M + c];
        double lu, luu = 0.0;
        if (r == c) {
          ddp_lu(p, w6, L.sU[r], r, &lu, &luu);
          luu = -luu;
        }
        L.sQuu[q] = luu + s;
      }
    }
    __syncthreads();
    if (lane == 0) {
      double Lm[M * M], kk[M];
#pragma unroll
      for (int q = 0; q < M * M; ++q) Lm[q] = L.sQuu[q] + (q % (M + 1) == 0 ? mu : 0.0);
      // under bounds, after the same verdict on the full Qbar_uu: k from the box QP, Lm the factor of
      // its free block, K's clamped rows exactly 0 (to_riccati_step's rule)
      unsigned fm = ~0u;
      bool ok = to_chol<M>(Lm);
      if constexpr (BX::on) {
        if (ok) {
          double qu[M], ub[M];
#pragma unroll
          for (int j = 0; j < M; ++j) {
            qu[j] = L.sQu[j];
            ub[j] = L.sU[j];
          }
          ok = to_box_gain<M>(bx, L.sQuu, mu, qu, ub, kk, &fm, Lm);
        }
      }
      if (!ok) {
        L.sFail = 1;
        pd = i;
      } else {
        if constexpr (!BX::on) {
#pragma unroll
          for (int j = 0; j < M; ++j) kk[j] = -L.sQu[j];
          to_chol_solve<M>(Lm, kk, 1);
        }
#pragma unroll 1
        for (int c = 0; c < N; ++c) {
          double col[M];
#pragma unroll
          for (int j = 0; j < M; ++j) col[j] = ((fm >> j) & 1u) ? -L.sQux[j * N + c] : 0.0;
          to_chol_solve<M>(Lm, col, 1);
#pragma unroll
          for (int j = 0; j < M; ++j) L.sK[j * N + c] = ((fm >> j) & 1u) ? col[j] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < M; ++j) {
          double s = 0.0;
#pragma unroll
          for (int c = 0; c < M; ++c) s += L.sQuu[j * M + c] * kk[c];
          L.sTk[j] = s;
          L.sk[j] = kk[j];
          d0 += kk[j] * L.sQu[j];
          d1 += kk[j] * s;
          if constexpr (BX::on) {
            if (!bx.held(j, L.sU[j], L.sQu[j])) d2 = fmax(d2, fabs(L.sQu[j]));
          } else {
            d2 = fmax(d2, fabs(L.sQu[j]));
          }
        }
      }
    }
    __syncthreads();
    if (L.sFail) break;  // uniform
    // T = Q_uu K; the gains to memory
    for (int o = lane; o < M * N; o += BT) {
      const int j = o / N, c = o - j * N;
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < M; ++q) s += L.sQuu[j * M + q] * L.sK[q * N + c];
      L.sT[o] = s;
      Ke[(size_t)i * na * N + o] = L.sK[o];
    }
    for (int j = lane; j < M; j += BT) ke[(size_t)i * na + j] = L.sk[j];
    __syncthreads();
    // V_x, and V_xx before symmetrisation
    for (int o = lane; o < N * N + N; o += BT) {
      if (o < N * N) {
        const int r = o / N, c = o - r * N;
        double s = L.sQxx[o];
#pragma unroll
        for (int j = 0; j < M; ++j)
          s += L.sK[j * N + r] * (L.sT[j * N + c] + L.sQux[j * N + c]) + L.sQux[j * N + r] * L.sK[j * N + c];
        L.sW[o] = s;
      } else {
        const int r = o - N * N;
        double s = L.sQx[r];
#pragma unroll
        for (int j = 0; j < M; ++j) s += L.sK[j * N + r] * (L.sTk[j] + L.sQu[j]) + L.sQux[j * N + r] * L.sk[j];
        L.sVx[r] = s;
      }
    }
    __syncthreads();
    for (int o = lane; o < N * N; o += BT) {
      const int r = o / N, c = o - r * N;
      L.sVxx[o] = 0.5 * (L.sW[o] + L.sW[c * N + r]);
    }
    __syncthreads();
  }
  return ToPass{pd, {d0, 0.5 * d1, d2}};
}

// cacto_to_backward_gains and the host-issued solver of the split family: one wavefront per
// episode. rec_ws: the derivative records of k_ddp_derivs / k_ddp_prim + k_ddp_tan + k_ddp_lx,
// [t][k][e]. mu_ep: per-episode mu (the solver) or nullptr (mu).
template <int NJ, class BX>
__global__ void __launch_bounds__(64) k_to_gains_wave(const SysDevice* __restrict__ sdp, const double* __restrict__ U,
                                                      int64_t ldU, const int32_t* __restrict__ nsteps, int n_ep,
                                                      int64_t ldS, double mu, const double* __restrict__ mu_ep,
                                                      const double* __restrict__ rec_ws, double* __restrict__ k_out,
                                                      double* __restrict__ K_out, double* __restrict__ dJ_out,
                                                      int32_t* __restrict__ pd_out, BX bx) {
  using RC = DdpRec<NJ>;
  constexpr int N = RC::N, na = Dims<NJ>::NA;
  __shared__ ToGainsLds<NJ> lds;
  const int e = blockIdx.x, lane = threadIdx.x;
  const int Te = nsteps[e];
  if (!to_valid_len(Te, ldS, ldU)) return;  // uniform over the workgroup
  if (mu_ep) mu = mu_ep[e];
  const ToPass bp = to_gains_episode<NJ, 64>(lds, sdp->p, U + (size_t)e * ldU * na, Te, mu, bx, rec_ws + e,
                                             (size_t)RC::R * n_ep, (size_t)n_ep, k_out + (size_t)e * ldU * na,
                                             K_out + (size_t)e * ldU * na * N, lane);
  if (lane == 0) {
    pd_out[e] = bp.pd;
    dJ_out[(size_t)e * 3] = bp.dJ[0];
    dJ_out[(size_t)e * 3 + 1] = bp.dJ[1];
    dJ_out[(size_t)e * 3 + 2] = bp.dJ[2];
  }
}

// The host-issued solver (car_park, manipulator and UR5 on path 0; the chains also on path 1):
// k_to_init, then per pass the derivative kernels of the label pass (fed ToState::live as nsteps),
// k_to_gains_wave and k_to_linesearch, the state in ToState in between. k_to_init: the warm
// start, rolled out into the caller's S / U / step_cost, one thread per episode.
template <int NJ, class BX>
__global__ void __launch_bounds__(64) k_to_init(const SysDevice* __restrict__ sdp, const double* __restrict__ S0,
                                                const double* __restrict__ U_init, int64_t ldU,
                                                const int32_t* __restrict__ nsteps, int n_ep, int64_t ldS, ToState st,
                                                double* S_out, double* U_out, double* cost_out,
                                                int32_t* __restrict__ status_out, int32_t* __restrict__ iters_out,
                                                double* __restrict__ J_out, BX bx) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_ep) return;
  const int Te = nsteps[e];
  const ToOut out{status_out, iters_out, J_out};
  if (!to_enter(Te, ldS, ldU, out, e, true)) {
    st.live[e] = -1;
    atomicAdd(st.done, 1);
    return;
  }
  const ToIter s = to_iter_begin(Te, to_warm_start_thread<NJ>(*sdp, S0, U_init, ldU, e, Te, bx, api_traj<NJ>(S_out, ldS, U_out, ldU, e),
                                                              View{cost_out + (size_t)e * ldS, 1, 1}));
  to_state_store(s, Te, st, out, e);
}

// One pass's decision and line search of the host-issued solver. A workgroup of 64 threads holds
// 64 / LSP episodes (LSP: the power of two >= max_ls + 1), thread (episode, j) evaluates the cost
// of alpha = 2^-j without storing the trajectory, the episode's first thread picks the smallest
// admissible j and stores the episode's state, and thread j rolls the accepted step out in place.
template <int NJ, class BX>
__global__ void __launch_bounds__(64) k_to_linesearch(const SysDevice* __restrict__ sdp, double* S, int64_t ldS, double* U,
                                                       int64_t ldU, double* k_in, double* K_in,
                                                       const double* __restrict__ dJ_in, const int32_t* __restrict__ pd_in,
                                                       int n_ep, ToCfgDev cfg, int LSP, ToState st, double* cost_out,
                                                       int32_t* __restrict__ status_out, int32_t* __restrict__ iters_out,
                                                       double* __restrict__ J_out, BX bx) {
  __shared__ double sJ[64];
  __shared__ int sSel[64];
  const int G = 64 / LSP, tid = threadIdx.x;
  const int grp = tid / LSP, j = tid - grp * LSP;
  const int e = blockIdx.x * G + grp;
  const int Te = e < n_ep ? st.live[e] : -1;
  const bool live = Te >= 0;
  const ToOut out{status_out, iters_out, J_out};
  double dJ[3] = {0.0, 0.0, 0.0}, J = 0.0;
  Traj cur{};
  Gains g{};
  View cost{};
  ToVerdict v = TO_STOP;
  if (live) {
#pragma unroll
    for (int k = 0; k < 3; ++k) dJ[k] = dJ_in[(size_t)e * 3 + k];
    v = to_verdict(cfg, pd_in[e], dJ);
    J = st.J[e];
    cur = api_traj<NJ>(S, ldS, U, ldU, e);
    g = api_gains<NJ>(k_in, K_in, ldU, e);
    cost = View{cost_out + (size_t)e * ldS, 1, 1};
  }
  const bool search = live && v == TO_SEARCH;
  sJ[tid] = search && j <= cfg.max_ls ? to_ls_candidate<NJ>(*sdp, cfg, cur, g, Te, j, J, dJ, bx, cost) : __builtin_nan("");
  __syncthreads();
  if (j == 0) {
    const int sel = to_pick(cfg, sJ + grp * LSP);
    if (live) {
      ToIter s = to_state_load(st, out, e);
      to_decide(cfg, s, v, sel, sJ[grp * LSP + max(sel, 0)]);
      to_state_store(s, Te, st, out, e);
    }
    sSel[grp] = sel;
  }
  __syncthreads();
  if (search && j == sSel[grp]) to_forward_thread<NJ, true>(*sdp, cur, g, Te, ldexp(1.0, -j), bx, cur, cost);
}

// LDS of k_to_solve_split: the backward pass's operands, and the scalars the phases hand to every
// thread (dJ [3] and the warm start's cost, the verdict, the candidates' costs).
template <int NJ>
struct ToSplitLds {
  ToGainsLds<NJ> gains;
  double pass[4];
  double cand[64];
  int pd;
};

// The split solver (car_park, path 1): one workgroup of BT threads per episode, the whole loop on
// the device, with the phases of the host-issued solver as device functions (contraction is off,
// so the numbers are that solver's bit for bit). Its own phases: the threads stride over the
// nodes for the derivative records; every wave runs the backward pass's step loop and takes
// outputs in it (one output per thread, the same summation order per output: the first of the
// two arrangements a wider workgroup allows, so its barriers are workgroup barriers reached by
// all waves); thread j <= max_ls evaluates alpha = 2^-j into LDS, every thread takes the pick
// from there, and thread sel rolls the accepted step out in place. The phases hand records,
// gains and trajectory to each other through global memory inside the workgroup: the barrier
// between them is the ordering (nothing crosses a workgroup), and no pointer they go through is
// __restrict__. The trajectory and the node costs live in the caller's S / U / step_cost (rows
// past Te, and a skipped episode's, are never touched); gains and records in the workspace
// (ToWs: episode_*, the records' element stride 1).
// The revolute chains are not instantiated: their derivative phase needs the tangent pass's LDS
// slabs and the bodies of k_ddp_prim / k_ddp_tan / k_ddp_lx, and a build of this kernel with them
// faulted on the GPU for a reason that has not been found.
template <int NJ, int BT, bool PSD, class BX>
__global__ void __launch_bounds__(BT) k_to_solve_split(const SysDevice* __restrict__ sdp, const double* __restrict__ S0,
                                                        const double* U_init, int64_t ldU,
                                                        const int32_t* __restrict__ nsteps, int n_ep, int64_t ldS,
                                                        ToCfgDev cfg, ToWs<NJ> lay, double* S_out, double* U_out,
                                                        double* cost_out, int32_t* __restrict__ status_out,
                                                        int32_t* __restrict__ iters_out, double* __restrict__ J_out, BX bx) {
  static_assert(NJ == -2, "k_to_solve_split: car_park only");
  using RC = DdpRec<NJ>;
  __shared__ ToSplitLds<NJ> lds;
  const int tid = threadIdx.x, e = blockIdx.x;
  const int Te = nsteps[e];
  const ToOut out{status_out, iters_out, J_out};
  if (!to_enter(Te, ldS, ldU, out, e, tid == 0)) return;  // uniform over the workgroup
  const SysDevice& sd = *sdp;
  const Traj cur = api_traj<NJ>(S_out, ldS, U_out, ldU, e);
  const View cost{cost_out + (size_t)e * ldS, 1, 1};
  const Gains g = lay.episode_gains(e);
  double* rec = lay.episode_rec(e, RC::R);
  if (tid == 0) lds.pass[3] = to_warm_start_thread<NJ>(sd, S0, U_init, ldU, e, Te, bx, cur, cost);
  __syncthreads();
  ToIter s = to_iter_begin(Te, lds.pass[3]);
  for (int it = 0; it < cfg.max_iter && s.running(); ++it) {
    for (int t = tid; t <= Te; t += BT) {
      ddp_derivs_node<NJ>(sd, &cur.S.at(t, 0), t < Te ? &cur.U.at(t, 0) : nullptr, t == Te, rec + (size_t)t * RC::R, 1);
      if constexpr (PSD) to_psd_record<NJ>(rec + (size_t)t * RC::R, 1);
    }
    __syncthreads();
    const ToPass bp = to_gains_episode<NJ, BT>(lds.gains, sd.p, cur.U.p, Te, s.mu, bx, rec, (size_t)RC::R, 1, g.k.p, g.K.p, tid);
    if (tid == 0) {
      lds.pd = bp.pd;
#pragma unroll
      for (int k = 0; k < 3; ++k) lds.pass[k] = bp.dJ[k];
    }
    __syncthreads();
    const double dJ[3] = {lds.pass[0], lds.pass[1], lds.pass[2]};
    const ToVerdict v = to_verdict(cfg, lds.pd, dJ);
    if (tid < 64)
      lds.cand[tid] = v == TO_SEARCH && tid <= cfg.max_ls ? to_ls_candidate<NJ>(sd, cfg, cur, g, Te, tid, s.J, dJ, bx, cost)
                                                          : __builtin_nan("");
    __syncthreads();
    const int sel = to_pick(cfg, lds.cand);
    to_decide(cfg, s, v, sel, lds.cand[max(sel, 0)]);
    if (tid == sel) to_forward_thread<NJ, true>(sd, cur, g, Te, ldexp(1.0, -sel), bx, cur, cost);
    __syncthreads();
  }
  if (tid == 0) to_iter_store(s, out, e);
}

}  // namespace cacto

using namespace cacto;

namespace {

inline bool to_path_ok(int path) { return path == CACTO_TO_PATH_DEFAULT || path == CACTO_TO_PATH_WAVE; }

// cacto_to_opts: NULL means the defaults; anything but a known hessian and zero reserved words is refused
inline bool to_opts_ok(const cacto_to_opts* o) {
  return !o || ((o->hessian == CACTO_TO_HESS_EXACT || o->hessian == CACTO_TO_HESS_PSD) && o->reserved[0] == 0 &&
                o->reserved[1] == 0 && o->reserved[2] == 0);
}
inline bool to_opts_psd(const cacto_to_opts* o) { return o && o->hessian == CACTO_TO_HESS_PSD; }

// the label pass's derivative records over (episode, step) (cacto_ddp_launch_derivs,
// ddp_kernels.hip); psd: then the projection of the records' l_xx blocks, on the launcher's grid
template <int NJ>
int to_launch_derivs(const cacto_sys* sys, const double* S, int64_t ldS, const double* U, int64_t ldU, const int32_t* n,
                     int n_ep, double* rec, bool psd, hipStream_t st) {
  const int rc = cacto_ddp_launch_derivs(sys, S, ldS, U, ldU, n, n_ep, rec, ldS, true, st);
  if (rc != CACTO_OK || !psd) return rc;
  hipLaunchKernelGGL(k_to_psd_records<NJ>, dim3(ceil_div(n_ep, 64), (unsigned)ldS), dim3(64), 0, st, n, n_ep, rec);
  CACTO_CHECK_HIP(hipGetLastError());
  return CACTO_OK;
}

template <int NJ>
struct LaunchToGains {
  static int run(const cacto_sys* sys, const double* S, int64_t ldS, const double* U, int64_t ldU, const int32_t* n,
                 int n_ep, double mu, bool psd, const cacto_to_box* box, double* k, double* K, double* dJ, int32_t* pd,
                 hipStream_t st) {
    if (!ddp_supported<NJ>(sys, "cacto_to_backward_gains")) return CACTO_EUNSUPPORTED;
    return to_with_box(box, [&](auto bx) { return go(sys, S, ldS, U, ldU, n, n_ep, mu, psd, bx, k, K, dJ, pd, st); });
  }
  template <class BX>
  static int go(const cacto_sys* sys, const double* S, int64_t ldS, const double* U, int64_t ldU, const int32_t* n,
                int n_ep, double mu, bool psd, BX bx, double* k, double* K, double* dJ, int32_t* pd, hipStream_t st) {
    if constexpr (DdpDims<NJ>::ok) {
      if constexpr (to_split<NJ>()) {
        double* rec = nullptr;
        const int rc = cacto_ddp_workspace(const_cast<cacto_sys*>(sys), ddp_rec_doubles<NJ>(n_ep, ldS) * sizeof(double), &rec);
        if (rc != CACTO_OK) return rc;
        const int rc2 = to_launch_derivs<NJ>(sys, S, ldS, U, ldU, n, n_ep, rec, psd, st);
        if (rc2 != CACTO_OK) return rc2;
        hipLaunchKernelGGL((k_to_gains_wave<NJ, BX>), dim3(n_ep), dim3(64), 0, st, sys->dev, U, ldU, n, n_ep, ldS, mu,
                           (const double*)nullptr, rec, k, K, dJ, pd, bx);
      } else {
        if (psd)
          hipLaunchKernelGGL((k_to_gains_thread<NJ, true, BX>), dim3(ceil_div(n_ep, 64)), dim3(64), 0, st, sys->dev, S, ldS,
                             U, ldU, n, n_ep, mu, k, K, dJ, pd, bx);
        else
          hipLaunchKernelGGL((k_to_gains_thread<NJ, false, BX>), dim3(ceil_div(n_ep, 64)), dim3(64), 0, st, sys->dev, S, ldS,
                             U, ldU, n, n_ep, mu, k, K, dJ, pd, bx);
      }
      CACTO_CHECK_HIP(hipGetLastError());
    }
    return CACTO_OK;
  }
};

template <int NJ>
struct LaunchToForward {
  static int run(const cacto_sys* sys, const double* S, int64_t ldS, const double* U, int64_t ldU, const double* k,
                 const double* K, const int32_t* n, int n_ep, double alpha, const cacto_to_box* box, double* Sn, double* Un,
                 double* cost, hipStream_t st) {
    if (!ddp_supported<NJ>(sys, "cacto_to_forward")) return CACTO_EUNSUPPORTED;
    return to_with_box(box, [&](auto bx) -> int {
      if constexpr (DdpDims<NJ>::ok) {
        hipLaunchKernelGGL((k_to_forward<NJ, decltype(bx)>), dim3(ceil_div(n_ep, 64)), dim3(64), 0, st, sys->dev, S, ldS, U,
                           ldU, k, K, n, n_ep, alpha, Sn, Un, cost, bx);
        CACTO_CHECK_HIP(hipGetLastError());
      }
      return CACTO_OK;
    });
  }
};

template <int NJ>
struct LaunchToBytes {
  static int run(int n_ep, int64_t ldS, int path, size_t* out) {
    if constexpr (DdpDims<NJ>::ok) *out = ToWs<NJ>(nullptr, n_ep, ldS, to_route<NJ>(path)).bytes;
    return CACTO_OK;
  }
};

// The solvers' launches. A solver is instantiated for the systems to_route can give it, once per
// Hessian mode and once per bounds mode: both are template parameters of the solving kernels, so the
// exact-mode kernels carry no trace of the projection and the unbounded ones none of the box QP.
template <int NJ>
struct LaunchToSolve {
  template <bool PSD, class BX>
  static void launch_closed_form(ToSolver solver, const cacto_sys* sys, const double* S0, const double* U_init, int64_t ldU,
                                 const int32_t* n, int n_ep, int64_t ldS, const ToCfgDev& c, const ToWs<NJ>& lay, double* S,
                                 double* U, double* cost, int32_t* status, int32_t* iters, double* J, BX bx, hipStream_t st) {
    if (solver == TO_SOLVER_WAVE)
      hipLaunchKernelGGL((k_to_solve_wave<NJ, PSD, BX>), dim3(n_ep), dim3(64), 0, st, sys->dev, S0, U_init, ldU, n, n_ep, ldS,
                         c, lay, S, U, cost, status, iters, J, bx);
    else
      hipLaunchKernelGGL((k_to_solve_thread<NJ, PSD, BX>), dim3(ceil_div(n_ep, 64)), dim3(64), 0, st, sys->dev, S0, U_init,
                         ldU, n, n_ep, ldS, c, (const int32_t*)lay.order, lay.lanes, S, U, cost, status, iters, J, bx);
  }
  static int run(const cacto_sys* sys, const double* S0, const double* U_init, int64_t ldU, const int32_t* n, int n_ep,
                 int64_t ldS, const cacto_to_cfg* cfg, bool psd, const cacto_to_box* box, double* S, double* U, double* cost,
                 int32_t* status, int32_t* iters, double* J, void* ws, size_t ws_bytes, hipStream_t st) {
    if (!ddp_supported<NJ>(sys, "cacto_to_solve")) return CACTO_EUNSUPPORTED;
    return to_with_box(box, [&](auto bx) {
      return go(sys, S0, U_init, ldU, n, n_ep, ldS, cfg, psd, bx, S, U, cost, status, iters, J, ws, ws_bytes, st);
    });
  }
  template <class BX>
  static int go(const cacto_sys* sys, const double* S0, const double* U_init, int64_t ldU, const int32_t* n, int n_ep,
                int64_t ldS, const cacto_to_cfg* cfg, bool psd, BX bx, double* S, double* U, double* cost, int32_t* status,
                int32_t* iters, double* J, void* ws, size_t ws_bytes, hipStream_t st) {
    if constexpr (DdpDims<NJ>::ok) {
      const ToSolver solver = to_route<NJ>(cfg->path);
      const ToWs<NJ> lay(ws, n_ep, ldS, solver);
      CACTO_REQUIRE(ws_bytes >= lay.bytes,
                    "cacto_to_solve: workspace smaller than cacto_to_workspace_bytes_cfg for this path "
                    "(path 0: cacto_to_workspace_bytes)");
      const ToCfgDev c{cfg->max_iter, cfg->max_ls, cfg->gtol, cfg->armijo, cfg->mu_min, cfg->mu_up, cfg->mu_down, cfg->mu_max};
      if constexpr (!to_split<NJ>()) {
        hipLaunchKernelGGL(k_to_order, dim3(1), dim3(256), 0, st, n, n_ep, ldS, lay.order, lay.hist);
        CACTO_CHECK_HIP(hipGetLastError());
        if (psd)
          launch_closed_form<true>(solver, sys, S0, U_init, ldU, n, n_ep, ldS, c, lay, S, U, cost, status, iters, J, bx, st);
        else
          launch_closed_form<false>(solver, sys, S0, U_init, ldU, n, n_ep, ldS, c, lay, S, U, cost, status, iters, J, bx, st);
        CACTO_CHECK_HIP(hipGetLastError());
      } else if (solver == TO_SOLVER_SPLIT) {
        if constexpr (to_persistent<NJ>()) {
          constexpr int BT = TO_SPLIT_THREADS;
          if (psd)
            hipLaunchKernelGGL((k_to_solve_split<NJ, BT, true, BX>), dim3(n_ep), dim3(BT), 0, st, sys->dev, S0, U_init, ldU,
                               n, n_ep, ldS, c, lay, S, U, cost, status, iters, J, bx);
          else
            hipLaunchKernelGGL((k_to_solve_split<NJ, BT, false, BX>), dim3(n_ep), dim3(BT), 0, st, sys->dev, S0, U_init, ldU,
                               n, n_ep, ldS, c, lay, S, U, cost, status, iters, J, bx);
          CACTO_CHECK_HIP(hipGetLastError());
        }
      } else {
        // the gains kernel indexes the gains with ldU; the workspace holds ldS rows of them
        CACTO_REQUIRE(ldU <= ldS, "cacto_to_solve: ldU > ldS");
        CACTO_CHECK_HIP(hipMemsetAsync(lay.st.done, 0, sizeof(int32_t), st));
        hipLaunchKernelGGL((k_to_init<NJ, BX>), dim3(ceil_div(n_ep, 64)), dim3(64), 0, st, sys->dev, S0, U_init, ldU, n, n_ep,
                           ldS, lay.st, S, U, cost, status, iters, J, bx);
        CACTO_CHECK_HIP(hipGetLastError());
        int LSP = 1;
        while (LSP < c.max_ls + 1) LSP *= 2;
        const int G = 64 / LSP;
        for (int it = 0; it < c.max_iter; ++it) {
          if (cfg->poll_every > 0 && it % cfg->poll_every == 0) {
            int32_t d = 0;
            CACTO_CHECK_HIP(hipMemcpyAsync(&d, lay.st.done, sizeof(int32_t), hipMemcpyDeviceToHost, st));
            CACTO_CHECK_HIP(hipStreamSynchronize(st));
            if (d >= n_ep) break;
          }
          const int rc = to_launch_derivs<NJ>(sys, S, ldS, U, ldU, lay.st.live, n_ep, lay.rec, psd, st);
          if (rc != CACTO_OK) return rc;
          hipLaunchKernelGGL((k_to_gains_wave<NJ, BX>), dim3(n_ep), dim3(64), 0, st, sys->dev, U, ldU, lay.st.live, n_ep, ldS,
                             0.0, (const double*)lay.st.mu, lay.rec, lay.k, lay.K, lay.dJ, lay.pd, bx);
          CACTO_CHECK_HIP(hipGetLastError());
          hipLaunchKernelGGL((k_to_linesearch<NJ, BX>), dim3(ceil_div(n_ep, G)), dim3(64), 0, st, sys->dev, S, ldS, U, ldU,
                             lay.k, lay.K, lay.dJ, lay.pd, n_ep, c, LSP, lay.st, cost, status, iters, J, bx);
          CACTO_CHECK_HIP(hipGetLastError());
        }
      }
    }
    return CACTO_OK;
  }
};

// cacto_to_solve_plan: what LaunchToSolve runs for a path
template <int NJ>
struct LaunchToPlan {
  static int run(const cacto_sys* sys, int path, bool psd, cacto_to_plan* out) {
    if (!ddp_supported<NJ>(sys, "cacto_to_solve_plan")) return CACTO_EUNSUPPORTED;
    if constexpr (DdpDims<NJ>::ok) {
      switch (to_route<NJ>(path)) {
        case TO_SOLVER_THREAD: *out = cacto_to_plan{1, 64, 0, 0}; break;
        case TO_SOLVER_WAVE: *out = cacto_to_plan{1, 64, (int32_t)sizeof(ToWaveLds), 0}; break;
        case TO_SOLVER_SPLIT: *out = cacto_to_plan{1, TO_SPLIT_THREADS, (int32_t)sizeof(ToSplitLds<NJ>), 0}; break;
        // the kernel described is the one-wave-per-episode backward pass; psd: one launch more, the
        // projection of the records
        case TO_SOLVER_HOST:
          *out = cacto_to_plan{0, 64, (int32_t)sizeof(ToGainsLds<NJ>), (NJ > 2 ? 5 : 3) + (psd ? 1 : 0)};
          break;
      }
    }
    return CACTO_OK;
  }
};

}  // namespace

// The options are a property of the call alone: like an unknown path they are reported before the
// other arguments are looked at.
#define CACTO_TO_REQUIRE_OPTS(opts, who) \
  CACTO_REQUIRE(to_opts_ok(opts), who ": bad options (hessian: CACTO_TO_HESS_EXACT or CACTO_TO_HESS_PSD; reserved words 0)")
// ... and so are the bounds, right after them (CACTO_TO_REQUIRE_BOX, ddp_device.h)

// The kernels a plan describes are the same with and without bounds (the box QP needs no LDS and no
// launch of its own)
extern "C" int cacto_to_solve_plan_box(const cacto_sys* sys, const cacto_to_cfg* cfg_h, cacto_to_plan* out,
                                       const cacto_to_opts* opts, const cacto_to_box* box) {
  CACTO_REQUIRE(cfg_h, "cacto_to_solve_plan: null config");
  CACTO_REQUIRE(to_path_ok(cfg_h->path),
                "cacto_to_solve_plan: bad config (path: CACTO_TO_PATH_DEFAULT or CACTO_TO_PATH_WAVE)");
  CACTO_TO_REQUIRE_OPTS(opts, "cacto_to_solve_plan");
  CACTO_TO_REQUIRE_BOX(box, sys, "cacto_to_solve_plan");
  CACTO_REQUIRE(sys && out, "cacto_to_solve_plan: bad arguments (null pointer)");
  return dispatch_nj<LaunchToPlan>(sys->host.p, sys, (int)cfg_h->path, to_opts_psd(opts), out);
}

extern "C" int cacto_to_solve_plan_opts(const cacto_sys* sys, const cacto_to_cfg* cfg_h, cacto_to_plan* out,
                                        const cacto_to_opts* opts) {
  return cacto_to_solve_plan_box(sys, cfg_h, out, opts, nullptr);
}

extern "C" int cacto_to_solve_plan(const cacto_sys* sys, const cacto_to_cfg* cfg_h, cacto_to_plan* out) {
  return cacto_to_solve_plan_opts(sys, cfg_h, out, nullptr);
}

extern "C" int cacto_to_backward_gains_box(const cacto_sys* sys, const double* S_d, int64_t ldS, const double* U_d,
                                           int64_t ldU, const int32_t* nsteps_d, int n_ep, double mu, double* k_d,
                                           double* K_d, double* dJ_d, int32_t* pd_d, void* stream,
                                           const cacto_to_opts* opts, const cacto_to_box* box) {
  CACTO_TO_REQUIRE_OPTS(opts, "cacto_to_backward_gains");
  CACTO_TO_REQUIRE_BOX(box, sys, "cacto_to_backward_gains");
  CACTO_REQUIRE(sys && S_d && U_d && nsteps_d && k_d && K_d && dJ_d && pd_d && n_ep >= 0 && ldS >= 1 && ldU >= 0,
                "cacto_to_backward_gains: bad arguments");
  if (n_ep == 0) return CACTO_OK;
  return dispatch_nj<LaunchToGains>(sys->host.p, sys, S_d, ldS, U_d, ldU, nsteps_d, n_ep, mu, to_opts_psd(opts), box, k_d,
                                    K_d, dJ_d, pd_d, as_stream(stream));
}

extern "C" int cacto_to_backward_gains_opts(const cacto_sys* sys, const double* S_d, int64_t ldS, const double* U_d,
                                            int64_t ldU, const int32_t* nsteps_d, int n_ep, double mu, double* k_d,
                                            double* K_d, double* dJ_d, int32_t* pd_d, void* stream,
                                            const cacto_to_opts* opts) {
  return cacto_to_backward_gains_box(sys, S_d, ldS, U_d, ldU, nsteps_d, n_ep, mu, k_d, K_d, dJ_d, pd_d, stream, opts,
                                     nullptr);
}

extern "C" int cacto_to_backward_gains(const cacto_sys* sys, const double* S_d, int64_t ldS, const double* U_d,
                                       int64_t ldU, const int32_t* nsteps_d, int n_ep, double mu, double* k_d,
                                       double* K_d, double* dJ_d, int32_t* pd_d, void* stream) {
  return cacto_to_backward_gains_opts(sys, S_d, ldS, U_d, ldU, nsteps_d, n_ep, mu, k_d, K_d, dJ_d, pd_d, stream, nullptr);
}

extern "C" int cacto_to_forward_box(const cacto_sys* sys, const double* S_d, int64_t ldS, const double* U_d, int64_t ldU,
                                    const double* k_d, const double* K_d, const int32_t* nsteps_d, int n_ep, double alpha,
                                    double* S_new_d, double* U_new_d, double* cost_new_d, void* stream,
                                    const cacto_to_box* box) {
  CACTO_TO_REQUIRE_BOX(box, sys, "cacto_to_forward");
  CACTO_REQUIRE(sys && S_d && U_d && nsteps_d && S_new_d && U_new_d && cost_new_d && n_ep >= 0 && ldS >= 1 && ldU >= 0 &&
                    (k_d == nullptr) == (K_d == nullptr),
                "cacto_to_forward: bad arguments");
  if (n_ep == 0) return CACTO_OK;
  return dispatch_nj<LaunchToForward>(sys->host.p, sys, S_d, ldS, U_d, ldU, k_d, K_d, nsteps_d, n_ep, alpha, box, S_new_d,
                                      U_new_d, cost_new_d, as_stream(stream));
}

extern "C" int cacto_to_forward(const cacto_sys* sys, const double* S_d, int64_t ldS, const double* U_d, int64_t ldU,
                                const double* k_d, const double* K_d, const int32_t* nsteps_d, int n_ep, double alpha,
                                double* S_new_d, double* U_new_d, double* cost_new_d, void* stream) {
  return cacto_to_forward_box(sys, S_d, ldS, U_d, ldU, k_d, K_d, nsteps_d, n_ep, alpha, S_new_d, U_new_d, cost_new_d, stream,
                              nullptr);
}

// The projection works in place on the records, so the workspace is the same in both Hessian modes;
// the box QP lives in registers, so it is the same with and without bounds
extern "C" size_t cacto_to_workspace_bytes_box(const cacto_sys* sys, int n_ep, int64_t ldS, const cacto_to_cfg* cfg_h,
                                               const cacto_to_opts* opts, const cacto_to_box* box) {
  const int path = cfg_h ? (int)cfg_h->path : (int)CACTO_TO_PATH_DEFAULT;
  if (!to_box_ok(box, to_box_na(sys))) return 0;
  if (!sys || n_ep < 0 || ldS < 1 || !to_path_ok(path) || !to_opts_ok(opts)) return 0;
  size_t out = 0;
  if (dispatch_nj<LaunchToBytes>(sys->host.p, n_ep, ldS, path, &out) != CACTO_OK) return 0;
  return out;
}

extern "C" size_t cacto_to_workspace_bytes_opts(const cacto_sys* sys, int n_ep, int64_t ldS, const cacto_to_cfg* cfg_h,
                                                const cacto_to_opts* opts) {
  return cacto_to_workspace_bytes_box(sys, n_ep, ldS, cfg_h, opts, nullptr);
}

extern "C" size_t cacto_to_workspace_bytes(const cacto_sys* sys, int n_ep, int64_t ldS) {
  return cacto_to_workspace_bytes_opts(sys, n_ep, ldS, nullptr, nullptr);
}

extern "C" size_t cacto_to_workspace_bytes_cfg(const cacto_sys* sys, int n_ep, int64_t ldS, const cacto_to_cfg* cfg_h) {
  if (!cfg_h) return 0;
  return cacto_to_workspace_bytes_opts(sys, n_ep, ldS, cfg_h, nullptr);
}

extern "C" int cacto_to_solve_box(const cacto_sys* sys, const double* S0_d, const double* U_init_d, int64_t ldU,
                                  const int32_t* nsteps_d, int n_ep, int64_t ldS, const cacto_to_cfg* cfg_h, double* S_d,
                                  double* U_d, double* step_cost_d, int32_t* status_d, int32_t* iters_d, double* J_d,
                                  void* ws_d, size_t ws_bytes, void* stream, const cacto_to_opts* opts,
                                  const cacto_to_box* box) {
  CACTO_REQUIRE(cfg_h, "cacto_to_solve: null config");
  // an unknown path is a property of the config alone: reported before the arguments are looked at
  CACTO_REQUIRE(to_path_ok(cfg_h->path), "cacto_to_solve: bad config (path: CACTO_TO_PATH_DEFAULT or CACTO_TO_PATH_WAVE)");
  CACTO_TO_REQUIRE_OPTS(opts, "cacto_to_solve");
  CACTO_TO_REQUIRE_BOX(box, sys, "cacto_to_solve");
  CACTO_REQUIRE(sys && S0_d && U_init_d && nsteps_d && S_d && U_d && step_cost_d && status_d && iters_d && J_d && ws_d &&
                    n_ep >= 0 && ldS >= 1 && ldU >= 0 && ldU <= ldS,
                "cacto_to_solve: bad arguments (null pointer, n_ep < 0, ldS < 1, ldU < 0 or ldU > ldS)");
  CACTO_REQUIRE(cfg_h->max_iter >= 0 && cfg_h->max_ls >= 0 && cfg_h->max_ls <= 63 && cfg_h->mu_up > 1.0 &&
                    cfg_h->mu_down > 1.0 && cfg_h->mu_min > 0.0 && cfg_h->poll_every >= 0,
                "cacto_to_solve: bad config (max_iter >= 0, 0 <= max_ls <= 63, mu_up > 1, mu_down > 1, mu_min > 0)");
  if (sys->host.p.w_terminal[6] != 0.0) {
    set_error("cacto_to_solve: w_terminal[6] != 0 (the reference adds u_{T-1} to the terminal cost through it, TO.py:60)");
    return CACTO_EUNSUPPORTED;
  }
  if (n_ep == 0) return CACTO_OK;
  return dispatch_nj<LaunchToSolve>(sys->host.p, sys, S0_d, U_init_d, ldU, nsteps_d, n_ep, ldS, cfg_h, to_opts_psd(opts),
                                    box, S_d, U_d, step_cost_d, status_d, iters_d, J_d, ws_d, ws_bytes, as_stream(stream));
}

extern "C" int cacto_to_solve_opts(const cacto_sys* sys, const double* S0_d, const double* U_init_d, int64_t ldU,
                                   const int32_t* nsteps_d, int n_ep, int64_t ldS, const cacto_to_cfg* cfg_h, double* S_d,
                                   double* U_d, double* step_cost_d, int32_t* status_d, int32_t* iters_d, double* J_d,
                                   void* ws_d, size_t ws_bytes, void* stream, const cacto_to_opts* opts) {
  return cacto_to_solve_box(sys, S0_d, U_init_d, ldU, nsteps_d, n_ep, ldS, cfg_h, S_d, U_d, step_cost_d, status_d, iters_d,
                            J_d, ws_d, ws_bytes, stream, opts, nullptr);
}

extern "C" int cacto_to_solve(const cacto_sys* sys, const double* S0_d, const double* U_init_d, int64_t ldU,
                              const int32_t* nsteps_d, int n_ep, int64_t ldS, const cacto_to_cfg* cfg_h, double* S_d,
                              double* U_d, double* step_cost_d, int32_t* status_d, int32_t* iters_d, double* J_d,
                              void* ws_d, size_t ws_bytes, void* stream) {
  return cacto_to_solve_opts(sys, S0_d, U_init_d, ldU, nsteps_d, n_ep, ldS, cfg_h, S_d, U_d, step_cost_d, status_d,
                             iters_d, J_d, ws_d, ws_bytes, stream, nullptr);
}
