// The box-constrained quadratic programme of control-limited DDP (Tassa, Mansard, Todorov, ICRA 2014),
//   minimise 1/2 x^T H x + q^T x  subject to  lo <= x <= hi,   H = Q_uu + mu I positive definite,
// by projected Newton in float64 on one thread: the trajectory optimiser's bounds mode (to_kernels.hip)
// solves one per node of the backward pass, with the box [lo - ubar, hi - ubar] around the nominal
// control. Every solver calls this one function, and the library is built with -ffp-contract=off, so
// the solvers of a system see the same solution bit for bit. No LDS, no global memory; M <= 6 keeps
// every array in registers (all indices are compile-time constants after unrolling).
#pragma once
#include <hip/hip_runtime.h>

namespace cacto {

// Iterations of the outer loop and halvings of the step. An iteration either leaves the clamped set
// as it is (the next one then ends with the exact solution on that set) or changes it, and a strictly
// convex QP in M <= 6 unknowns changes it a handful of times: the caps are far above what the random
// problems of tests/test_to_box_cpu.py need (every one of them is solved). Past a cap the caller is
// told (false) and treats the node as not positive definite: a larger mu makes H more diagonal, where
// one projected step is the solution.
constexpr int BOX_QP_ITERS = 32;
constexpr int BOX_QP_HALVINGS = 40;
constexpr double BOX_QP_ARMIJO = 0.1;

// element (i, j) of the symmetric h, of which the lower triangle is what is read (as to_chol does)
template <int M>
__host__ __device__ __forceinline__ double box_sym(const double* h, int i, int j) {
  return i >= j ? h[i * M + j] : h[j * M + i];
}

// Cholesky factor (lower triangle of L, L L^T) of h with the rows and columns outside `free` replaced
// by those of the identity: its free block is a factor of the free block of h, its other rows are
// the identity's, so a solve with a right-hand side that is 0 outside `free` is the free block's
// solve and leaves 0 there. false at a pivot <= 0 or a non-finite one.
template <int M>
__host__ __device__ inline bool box_chol_free(const double* h, unsigned free, double* L) {
#pragma unroll
  for (int j = 0; j < M; ++j) {
    const bool fj = (free >> j) & 1u;
    double d = fj ? h[j * M + j] : 1.0;
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[j * M + k] * L[j * M + k];
    if (!(d > 0.0) || !(d <= 1.79769313486231570815e308)) return false;
    const double l = sqrt(d);
    L[j * M + j] = l;
#pragma unroll
    for (int i = j + 1; i < M; ++i) {
      double s = (fj && ((free >> i) & 1u)) ? h[i * M + j] : 0.0;
#pragma unroll
      for (int k = 0; k < j; ++k) s -= L[i * M + k] * L[j * M + k];
      L[i * M + j] = s / l;
    }
#pragma unroll
    for (int i = 0; i < j; ++i) L[i * M + j] = 0.0;
  }
  return true;
}
// x <- (L L^T)^-1 x
template <int M>
__host__ __device__ inline void box_chol_solve(const double* L, double* x) {
#pragma unroll
  for (int i = 0; i < M; ++i) {
    double s = x[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= L[i * M + k] * x[k];
    x[i] = s / L[i * M + i];
  }
#pragma unroll
  for (int i = M - 1; i >= 0; --i) {
    double s = x[i];
#pragma unroll
    for (int k = i + 1; k < M; ++k) s -= L[k * M + i] * x[k];
    x[i] = s / L[i * M + i];
  }
}

// The box of a node around its nominal control u: the offsets (lo - u, hi - u), each moved outward by one
// unit in the last place where u + offset would otherwise stop short of the bound in float64. One unit
// is enough: the rounded difference d has u + d within half a unit of d of the bound (and equal to it
// wherever u is within a factor of two of the bound, where the difference is exact), so the next
// double carries the exact sum, and with it the rounded one, to the bound or past it. A control the QP
// clamps then lands on its bound exactly when the roll-out applies the full step and clamps, where
// fl(u + fl(hi - u)) can stop one rounding error short of hi and the next pass would count that
// control as free. An infinite bound gives an infinite offset.
__host__ __device__ __forceinline__ double box_offset_hi(double u, double hi) {
  const double d = hi - u;
  return u + d < hi ? nextafter(d, 1.79769313486231570815e308) : d;
}
__host__ __device__ __forceinline__ double box_offset_lo(double u, double lo) {
  const double d = lo - u;
  return u + d > lo ? nextafter(d, -1.79769313486231570815e308) : d;
}

// H [M * M] row-major symmetric positive definite (lower triangle read), q, lo < hi [M] (an infinite
// entry: that side is open), all unchanged. Out: x [M] the minimiser, *free_mask bit j set where x_j
// is free (clear: x_j sits on a bound and the gradient points out of the box), Lf [M * M] the factor
// box_chol_free(H, *free_mask). The iteration starts at the projection of 0 and repeats:
//   g = q + H x;  free = all but { j : x_j = lo_j and g_j > 0, or x_j = hi_j and g_j < 0 };
//   nothing free, or g = 0 on the free set, or the last step was the full Newton step on this very
//   set (it solved the set's equations: the free gradient has vanished to rounding): done;
//   the working set w: the free set less, repeatedly, the components on a bound that the Newton
//   step d = -H_ww^-1 g_w of the rest would push out of the box (without this the projected step
//   need not descend; a single component is never pushed out, so w is not empty);
//   x <- P(x + s d), the largest s = 2^-i with f(P(x + s d)) - f(x) <= BOX_QP_ARMIJO g^T (P(x + s d) - x)
//   (P the projection onto the box; the difference of f evaluated as g^T D + 1/2 D^T H D, which keeps
//   its sign where f itself would round it away). A step that no longer changes x in floating point
//   (D = 0 with w the whole free set) also ends the iteration: x is as good as float64 holds.
// false: a block has no Cholesky factor, no step gave the decrease, or BOX_QP_ITERS ran out; x,
// *free_mask and Lf then mean nothing.
template <int M>
__host__ __device__ inline bool to_box_qp(const double* H, const double* q, const double* lo, const double* hi, double* x,
                                          unsigned* free_mask, double* Lf) {
  unsigned fr = ~0u;     // the set Lf is the factor of; none yet
  unsigned wlast = ~0u;  // the working set of the last step, when that was an unprojected Newton step
#pragma unroll
  for (int j = 0; j < M; ++j) x[j] = fmin(fmax(0.0, lo[j]), hi[j]);
#pragma unroll 1
  for (int it = 0; it < BOX_QP_ITERS; ++it) {
    double g[M], gmax = 0.0;
    unsigned f = 0u;
#pragma unroll
    for (int j = 0; j < M; ++j) {
      double s = q[j];
#pragma unroll
      for (int c = 0; c < M; ++c) s += box_sym<M>(H, j, c) * x[c];
      g[j] = s;
      if (!(s == s)) return false;
      const bool clamped = (x[j] == lo[j] && s > 0.0) || (x[j] == hi[j] && s < 0.0);
      if (!clamped) {
        f |= 1u << j;
        gmax = fmax(gmax, fabs(s));
      }
    }
    bool done = f == 0u || gmax == 0.0 || f == wlast;
    unsigned w = f;
    double d[M];
    if (!done) {
#pragma unroll 1
      for (int r = 0; r < M; ++r) {
        if (w != fr) {
          if (!box_chol_free<M>(H, w, Lf)) return false;
          fr = w;
        }
#pragma unroll
        for (int j = 0; j < M; ++j) d[j] = ((w >> j) & 1u) ? -g[j] : 0.0;
        box_chol_solve<M>(Lf, d);
        unsigned out = 0u;
#pragma unroll
        for (int j = 0; j < M; ++j)
          if (((w >> j) & 1u) && ((x[j] == lo[j] && d[j] < 0.0) || (x[j] == hi[j] && d[j] > 0.0))) out |= 1u << j;
        if (out == 0u) break;
        w &= ~out;
      }
      double step = 1.0;
      bool ok = false;
#pragma unroll 1
      for (int h = 0; h <= BOX_QP_HALVINGS && !ok && !done; ++h) {
        double D[M], gD = 0.0, DHD = 0.0;
        bool inside = true, moved = false;
#pragma unroll
        for (int j = 0; j < M; ++j) {
          const double xn = x[j] + step * d[j], xc = fmin(fmax(xn, lo[j]), hi[j]);
          inside = inside && xc == xn;
          D[j] = xc - x[j];
          moved = moved || D[j] != 0.0;
          gD += g[j] * D[j];
        }
        if (!moved) {
          if (w != f) return false;
          done = true;
        } else {
#pragma unroll
          for (int j = 0; j < M; ++j) {
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < M; ++c) s += box_sym<M>(H, j, c) * D[c];
            DHD += D[j] * s;
          }
          if (gD < 0.0 && gD + 0.5 * DHD <= BOX_QP_ARMIJO * gD) {
            ok = true;
            wlast = (inside && h == 0) ? w : ~0u;
#pragma unroll
            for (int j = 0; j < M; ++j) x[j] = fmin(fmax(x[j] + step * d[j], lo[j]), hi[j]);  // a bound is met exactly
          }
        }
        step *= 0.5;
      }
      if (!ok && !done) return false;
    }
    if (done) {
      if (f != fr && !box_chol_free<M>(H, f, Lf)) return false;
      *free_mask = f;
      return true;
    }
  }
  return false;
}

}  // namespace cacto
