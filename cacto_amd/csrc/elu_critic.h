// The elu critic (critic_type 'elu', NeuralNetwork.py:65-78: Dense 16, 32, 256, 256 with elu, then
// Dense 1) over a 16-sample tile held in LDS: forward pass and input gradient, the tile machinery of
// mlp.h on this network's shape.
//
// Out tiles per hidden layer: 1, 2, 16, 16 (35 tiles; one kept array is 35 KiB). Only h_l is kept:
// elu' = h < 0 ? h + 1 : 1 and elu'' = h < 0 ? h + 1 : 0 both follow from the stored h (elu_pair /
// act_d2 of common.h give the same values), so no pass keeps a second array per layer.
//
// Per layer (forward blocks OT x KT, transposed blocks KT x OT):
//   l0 ns -> 16   1 x 1    mm_layer_t<1>, one wave
//   l1 16 -> 32   2 x 1    mm_layer_t<1>, two waves
//   l2 32 -> 256  16 x 2   mm_layer_t<2>, 4 out tiles per wave
//   l3 256 -> 256 16 x 16  mm_layer_t<16>: 64 fragment blocks per wave do not fit in registers, so
//                          they stream from L2 one out tile ahead (as the actor's W2 does)
//   l4 256 -> 1   1 x 16   split-K over the 4 waves (mm_single_tile)
#pragma once

#include "net_common.h"

namespace cacto {

constexpr int ELU_DIMS[4] = {16, 32, 256, 256};
constexpr int ELU_ZOFF[4] = {0, 1, 3, 19};  // hidden-layer tile offsets; G_l (l = 1..3) sits at ELU_ZOFF[l - 1]
constexpr int ELU_OT[4] = {1, 2, 16, 16};
constexpr int ELU_TILES = 35;
constexpr int ELU_GTILES = 19;  // G_1 .. G_3

__device__ __forceinline__ float4 elu_d1(const float4 h) {
  return make_float4(h.x < 0.f ? fadd(h.x, 1.f) : 1.f, h.y < 0.f ? fadd(h.y, 1.f) : 1.f,
                     h.z < 0.f ? fadd(h.z, 1.f) : 1.f, h.w < 0.f ? fadd(h.w, 1.f) : 1.f);
}
__device__ __forceinline__ float4 elu_d2(const float4 h) {
  return make_float4(act_d2(true, h.x), act_d2(true, h.y), act_d2(true, h.z), act_d2(true, h.w));
}
__device__ __forceinline__ float4 mul4(const float4 a, const float4 b) {
  return make_float4(fmul(a.x, b.x), fmul(a.y, b.y), fmul(a.z, b.z), fmul(a.w, b.w));
}

// W5[:, 0] (256 floats) into LDS: the backward passes read the lane's 4 rows of an out tile from it.
// The caller's next barrier publishes it.
__device__ __forceinline__ void elu_stage_w5(const NetView& N, float* w5s, const Lane& L) {
  w5s[L.tid] = N.flat[N.t.woff[4] + L.tid];
}
__device__ __forceinline__ float4 elu_w5(const float* w5s, int ot, const Lane& L) {
  return reinterpret_cast<const float4*>(w5s)[4 * ot + L.g];
}

// One layer on its shape, BIAS or not (the Sobolev adjoint runs the forward fragments without
// bias). TR: the transposed pass G_l = D_l W_l^T (in tiles out, K = the layer's out tiles).
template <int l, bool BIAS, bool TR, typename Epi>
__device__ __forceinline__ void elu_layer(const NetView& N, const float4* X, const Lane& L, Epi&& epi) {
  const float* b = BIAS ? N.biasp(l) : nullptr;
  if constexpr (!TR) {
    if constexpr (l == 0) mm_layer_t<1>(N.fwd(0), 1, X, L.wave, L.lane, epi, b);
    if constexpr (l == 1) mm_layer_t<1>(N.fwd(1), 2, X, L.wave, L.lane, epi, b);
    if constexpr (l == 2) mm_layer_t<2>(N.fwd(2), 16, X, L.wave, L.lane, epi, b);
    if constexpr (l == 3) mm_layer_t<16>(N.fwd(3), 16, X, L.wave, L.lane, epi, b);
  } else {
    if constexpr (l == 0) mm_layer_t<1>(N.bwd(0), 1, X, L.wave, L.lane, epi, nullptr);
    if constexpr (l == 1) mm_layer_t<2>(N.bwd(1), 1, X, L.wave, L.lane, epi, nullptr);
    if constexpr (l == 2) mm_layer_t<16>(N.bwd(2), 2, X, L.wave, L.lane, epi, nullptr);
    if constexpr (l == 3) mm_layer_t<16>(N.bwd(3), 16, X, L.wave, L.lane, epi, nullptr);
  }
}

// Forward over the input tile X0: h_l = elu(z_l) into Hs (35 tiles at ELU_ZOFF), hook(l, ot, h4) for
// every hidden out tile, V[c] (LDS, 16 floats) the output for sample c. Ends with a barrier.
template <bool WANT_V = true, typename Hook>
__device__ __forceinline__ void elu_forward_tile(const NetView& N, const float4* X0, float4* Hs, float4* red, float* V,
                                                 const Lane& L, Hook&& hook) {
  auto epi = [&](int l) {
    return [&, l](int ot, floatx4 acc) {
      float h[4], c[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) elu_pair(acc[r], &h[r], &c[r]);  // acc = x W + b
      const float4 h4 = make_float4(h[0], h[1], h[2], h[3]);
      Hs[(ELU_ZOFF[l] + ot) * 64 + L.lane] = h4;
      hook(l, ot, h4);
    };
  };
  elu_layer<0, true, false>(N, X0, L, epi(0));
  __syncthreads();
  elu_layer<1, true, false>(N, Hs + ELU_ZOFF[0] * 64, L, epi(1));
  __syncthreads();
  elu_layer<2, true, false>(N, Hs + ELU_ZOFF[1] * 64, L, epi(2));
  __syncthreads();
  elu_layer<3, true, false>(N, Hs + ELU_ZOFF[2] * 64, L, epi(3));
  __syncthreads();
  if (WANT_V) {
    mm_single_tile(N.fwd(4), 16, Hs + ELU_ZOFF[3] * 64, red, L, [&](int, floatx4 acc) {
      if (L.g == 0) V[L.c] = acc[0];
    }, N.biasp(4), 1);
    __syncthreads();
  }
}

// Input gradient (first backward pass) from the kept h tiles: G[4] = W5, D[l] = G[l+1] elu'(z_l),
// G[l] = D[l] W_l^T. D tiles go to D (35 tiles at ELU_ZOFF; D may be Hs itself: each lane reads the
// h of its element, then writes the D over it, and no later step of this pass reads that h), G_1..G_3
// to Gs (19 tiles) when non-null, D via hookD(l, ot, lane, d4), dV/dx0 in G0 (1 tile). w5s: W5[:, 0]
// staged by elu_stage_w5 before the caller's last barrier. Ends with a barrier.
template <typename HookD>
__device__ __forceinline__ void elu_first_backward(const NetView& N, const float4* Hs, float4* D, float4* Gs,
                                                   float4* G0, const float* w5s, const Lane& L, HookD&& hookD) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int ot = L.wave + 4 * t;
    const float4 d4 = mul4(elu_w5(w5s, ot, L), elu_d1(Hs[(ELU_ZOFF[3] + ot) * 64 + L.lane]));
    D[(ELU_ZOFF[3] + ot) * 64 + L.lane] = d4;
    hookD(3, ot, L.lane, d4);
  }
  __syncthreads();
  auto epi = [&](int l) {
    return [&, l](int it, floatx4 acc) {
      const float4 gl = f4(acc);
      if (Gs) Gs[(ELU_ZOFF[l - 1] + it) * 64 + L.lane] = gl;
      const float4 d4 = mul4(gl, elu_d1(Hs[(ELU_ZOFF[l - 1] + it) * 64 + L.lane]));
      D[(ELU_ZOFF[l - 1] + it) * 64 + L.lane] = d4;
      hookD(l - 1, it, L.lane, d4);
    };
  };
  elu_layer<3, false, true>(N, D + ELU_ZOFF[3] * 64, L, epi(3));
  __syncthreads();
  elu_layer<2, false, true>(N, D + ELU_ZOFF[2] * 64, L, epi(2));
  __syncthreads();
  elu_layer<1, false, true>(N, D + ELU_ZOFF[1] * 64, L, epi(1));
  __syncthreads();
  elu_layer<0, false, true>(N, D + ELU_ZOFF[0] * 64, L, [&](int, floatx4 acc) { G0[L.lane] = f4(acc); });
  __syncthreads();
}

}  // namespace cacto
