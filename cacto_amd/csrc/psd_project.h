// Projection of a small symmetric matrix onto the positive semidefinite cone, P(H) = V max(L, 0) V^T
// with H = V L V^T, by a cyclic Jacobi eigenvalue iteration in float64 on one thread. The trajectory
// optimiser's "psd" Hessian mode (to_kernels.hip) passes every node's l_xx (cost convention) through
// it; the label pass never does. Every solver calls this one function, and the library is built
// with -ffp-contract=off, so the solvers of a system see the same projected matrix bit for bit.
#pragma once
#include <hip/hip_runtime.h>

namespace cacto {

// Sweeps over the N (N - 1) / 2 pivots. Measured in numpy on 200 random symmetric matrices per size
// with eigenvalues spread over 1e-6..1e3: N <= 6 reaches off(A) / |H| ~ 1e-16 in 6 sweeps, N = 12 in
// 8. A sweep that met no non-zero pivot ends the iteration early (a diagonal matrix after none, a
// 2 x 2 one after its single rotation): the count of sweeps depends on the matrix alone.
template <int N>
struct PsdSweeps {
  static constexpr int value = N > 6 ? 8 : 6;
};

// One rotation in the (p, q) plane, p < q, of the symmetric a (both triangles kept) with the
// eigenvector accumulation v <- v J. A zero pivot is skipped (returns false). theta =
// (a_qq - a_pp) / (2 a_pq), t = sgn(theta) / (|theta| + hypot(theta, 1)) is the smaller root of
// t^2 + 2 theta t - 1; hypot does not overflow where theta^2 would, and an infinite theta (a
// denormal pivot) gives t = 0, the identity.
template <int N>
__host__ __device__ __forceinline__ bool psd_rotate(double* a, double* v, int p, int q) {
  const double apq = a[p * N + q];
  if (apq == 0.0) return false;
  const double app = a[p * N + p], aqq = a[q * N + q];
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = copysign(1.0, theta) / (fabs(theta) + hypot(theta, 1.0));
  const double c = 1.0 / hypot(t, 1.0), s = t * c;
  a[p * N + p] = app - t * apq;
  a[q * N + q] = aqq + t * apq;
  a[p * N + q] = a[q * N + p] = 0.0;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    if (k != p && k != q) {
      const double akp = a[k * N + p], akq = a[k * N + q];
      const double np_ = c * akp - s * akq, nq_ = s * akp + c * akq;
      a[k * N + p] = a[p * N + k] = np_;
      a[k * N + q] = a[q * N + k] = nq_;
    }
    const double vkp = v[k * N + p], vkq = v[k * N + q];
    v[k * N + p] = c * vkp - s * vkq;
    v[k * N + q] = s * vkp + c * vkq;
  }
  return true;
}

// h [N * N] row-major, symmetric (the upper triangle is what is read), replaced by P(h): pivots in
// row order (p, q), p < q; the diagonal clipped at 0; V max(L, 0) V^T rebuilt on the upper triangle
// and mirrored, so the result is symmetric exactly. N <= 6: the pivot loops are unrolled and a, v
// stay in registers; larger N keeps them rolled (a, v indexed at run time, in scratch): 2 N^2
// doubles are more registers than a lane has.
template <int N>
__host__ __device__ inline void psd_project(double* h) {
  double a[N * N], v[N * N];
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) {
      a[i * N + j] = i <= j ? h[i * N + j] : h[j * N + i];
      v[i * N + j] = i == j ? 1.0 : 0.0;
    }
#pragma unroll 1
  for (int sweep = 0; sweep < PsdSweeps<N>::value; ++sweep) {
    bool rotated = false;
    if constexpr (N <= 6) {
#pragma unroll
      for (int p = 0; p < N - 1; ++p)
#pragma unroll
        for (int q = p + 1; q < N; ++q) rotated |= psd_rotate<N>(a, v, p, q);
    } else {
#pragma unroll 1
      for (int p = 0; p < N - 1; ++p)
#pragma unroll 1
        for (int q = p + 1; q < N; ++q) rotated |= psd_rotate<N>(a, v, p, q);
    }
    if (!rotated) break;
  }
  if constexpr (N <= 6) {
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
      for (int j = i; j < N; ++j) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k) s += (v[i * N + k] * fmax(a[k * N + k], 0.0)) * v[j * N + k];
        h[i * N + j] = h[j * N + i] = s;
      }
  } else {
#pragma unroll 1
    for (int i = 0; i < N; ++i)
#pragma unroll 1
      for (int j = i; j < N; ++j) {
        double s = 0.0;
#pragma unroll 1
        for (int k = 0; k < N; ++k) s += (v[i * N + k] * fmax(a[k * N + k], 0.0)) * v[j * N + k];
        h[i * N + j] = h[j * N + i] = s;
      }
  }
}

}  // namespace cacto
