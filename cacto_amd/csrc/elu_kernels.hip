// The elu critic's kernels (critic_type 'elu': 16, 32, 256, 256 wide, elu_critic.h): inference and
// dV/ds, the critic chain, and the actor chain / paired grid with the critic pass at s' on this
// shape. A translation unit of its own: the sine critics' kernels (learn_kernels.hip,
// net_kernels.hip) are compiled from unchanged code beside it, and a handle's critic topology picks
// between the two at the launch_* level. 16-sample tiles at every batch size.
//
// The in-kernel phase stamps of the diagnostic builds cover the sine chains only.
#undef CACTO_STAMPS
#define CSTAMP(k) \
  do {            \
  } while (0)
#define CSTAMP_DECL
#define CSTAMP_FLUSH \
  do {               \
  } while (0)

#include "chains.h"

namespace cacto {

// ---------------------------------------------------------------- inference
// V = critic(s); optionally dV/ds (w.r.t. the raw state, through the normalisation). 43 KiB of LDS.
__global__ void __launch_bounds__(CACTO_THREADS)
    k_critic_forward_elu(const SysDevice* __restrict__ sdp, NetView N, const float* __restrict__ S,
                         float* __restrict__ Vout, float* __restrict__ dVdS, int B) {
  __shared__ float4 X0[64];
  __shared__ float4 Hs[ELU_TILES * 64];
  __shared__ float4 G0[64];
  __shared__ float4 red[4 * 64];
  __shared__ float st[16 * 16];
  __shared__ __attribute__((aligned(16))) float w5s[256];  // read as float4 (elu_w5)
  __shared__ float V[16];
  const cacto_sys_params& p = sdp->p;
  const Lane L;
  const int ns = p.nb_state, s0 = blockIdx.x * CACTO_TILE;
  {
    const int c = L.tid >> 4, f = L.tid & 15;
    st[L.tid] = (s0 + c < B && f < ns) ? S[(size_t)(s0 + c) * ns + f] : 0.f;
  }
  elu_stage_w5(N, w5s, L);
  __syncthreads();
  if (L.wave == 0) fill_input_tile(p, st, X0, L);
  __syncthreads();
  elu_forward_tile(N, X0, Hs, red, V, L, [](int, int, float4) {});
  if (L.tid < 16 && s0 + L.tid < B && Vout) Vout[s0 + L.tid] = V[L.tid];
  if (!dVdS) return;
  elu_first_backward(N, Hs, Hs, nullptr, G0, w5s, L, [](int, int, int, float4) {});
  if (L.wave == 0) {
    const float4 g = G0[L.lane];
    const float gv[4] = {g.x, g.y, g.z, g.w};
    for (int r = 0; r < 4; ++r) {
      const int f = 4 * L.g + r;
      if (f < ns && s0 + L.c < B) dVdS[(size_t)(s0 + L.c) * ns + f] = normalize_backward(p, f, gv[r]);
    }
  }
}

// ---------------------------------------------------------------- critic chain
// 96.5 KiB: with the actor chain's 62.2 KiB one critic and one actor workgroup share a CU (160 KiB),
// as the sine chains do (the pipelined large-batch update runs critic(t+1) and actor(t) side by
// side; with 4 KiB more they took turns on a CU: DI B = 4096 5.2 k -> 6.9 k updates/s).
// Kept arrays: Hs (h_l, 35 tiles), DZ (35 tiles: the target passes' h, then D_l of the first
// backward, then zbar_l from the Sobolev adjoint on) and G (G_1..G_3 of the first backward, 19
// tiles; the adjoint writes its forward-mode tile of layer l over G_{l+1} once it has read it). The
// sine chain keeps cos z_l beside sin z_l; here elu' and elu'' come from h_l.
// Two short-lived arrays share storage with later ones: the split-K partials `red`
// of the forward passes' last layer are G's first 4 tiles (G is first written by the first
// backward, after every forward pass), and the Sobolev adjoint's input tile GB is XT (the s' input
// tile, dead after the target pass).
struct CriticLdsElu {
  float4 X0[64], XT[64], G0[64];
  float4 Hs[ELU_TILES * 64];
  float4 DZ[ELU_TILES * 64];
  float4 G[ELU_GTILES * 64];
  float st[256], stn[256], dvdx[256], w5s[256];
  float Rs[16], ds[16], ws[16], Vn[16], V[16], y[16], Vb[16], Vt2[16];
};

// one 16-sample tile of the critic chain (workgroup-wide; S in LDS): critic_chain's five phases and
// panels (chains.h) on the elu shape
__device__ __forceinline__ void critic_chain_elu(CriticLdsElu& S, const int tile, const SysDevice* __restrict__ sdp,
                                                 const NetView& C, const NetView& Tg, const ChainScalars& cs,
                                                 const double* __restrict__ storage, const int32_t* __restrict__ idx,
                                                 const float* __restrict__ isw, int B, const GradBufs& gb,
                                                 float* __restrict__ y_out, float* __restrict__ V_out,
                                                 float* __restrict__ Vt_out, int32_t* __restrict__ step) {
  float4 *X0 = S.X0, *XT = S.XT, *G0 = S.G0, *GB = S.XT, *Hs = S.Hs, *DZ = S.DZ, *ZB = S.DZ, *G = S.G, *red = S.G;
  static_assert(ELU_GTILES >= 4, "red (4 tiles) inside G");
  float *st = S.st, *stn = S.stn, *dvdx = S.dvdx, *w5s = S.w5s, *Rs = S.Rs, *ds = S.ds, *ws = S.ws, *Vn = S.Vn,
        *V = S.V, *y = S.y, *Vb = S.Vb, *Vt2 = S.Vt2;
  const cacto_sys_params& p = sdp->p;
  const Lane L;
  const int ns = p.nb_state, cols = 3 * ns + 3, s0 = tile * CACTO_TILE;
  const int ld = gb.ld, Bp = gb.Bp;
  const bool sob = cs.w_S != 0.f;
  if (tile == 0 && L.tid == 0 && step) step[0] += 1;  // Keras critic optimizer iterations

  const Norm4 nrm(p, L);
  {  // one (sample, feature) per thread, branch-free gathers (clamped indices, then zeroed)
    const int c = L.tid >> 4, f = L.tid & 15;
    const bool valid = s0 + c < B, in = valid && f < ns;
    const int sc = min(s0 + c, B - 1), fc = min(f, ns - 1);
    const int32_t row = idx[sc];
    elu_stage_w5(C, w5s, L);
    const double* rp = storage + (size_t)row * cols;
    const double x = rp[fc], xn = rp[ns + 1 + fc], xd = rp[2 * ns + 1 + fc];
    const double r = rp[ns], d = rp[3 * ns + 1];
    const float wv = isw ? isw[sc] : 1.f;
    st[c * 16 + f] = in ? (float)x : 0.f;
    stn[c * 16 + f] = in ? (float)xn : 0.f;
    dvdx[c * 16 + f] = in ? (float)xd : 0.f;
    if (f == 0) {
      Rs[c] = valid ? (float)r : 0.f;
      ds[c] = valid ? (float)d : 0.f;
      ws[c] = valid ? wv : 0.f;
    }
  }
  __syncthreads();
  if (L.wave == 0) {
    nrm.fill(st, X0, L);
    nrm.fill(stn, XT, L);
  }
  __syncthreads();

  // y = R + (1 - d) * V_tgt(s_next)   (NeuralNetwork.py:153-158)
  if (!cs.MC) elu_forward_tile(Tg, XT, DZ, red, Vn, L, [](int, int, float4) {});
  if (L.tid < 16) y[L.tid] = cs.MC ? Rs[L.tid] : fadd(Rs[L.tid], fmul(fsub(1.f, ds[L.tid]), Vn[L.tid]));
  if (cs.want_vt) elu_forward_tile(Tg, X0, DZ, red, Vt2, L, [](int, int, float4) {});  // NeuralNetwork.py:178

  // forward at s, keeping h_l; h_l -> LT_{l+1} second half
  if (L.wave == 0) store_panel(gb.LT[0], ld, Bp + s0 + L.c, 0, L.g, X0[L.lane]);
  elu_forward_tile(C, X0, Hs, red, V, L, [&](int l, int ot, float4 h4) {
    store_panel(gb.LT[l + 1], ld, Bp + s0 + L.c, ot, L.g, h4);
  });

  if (sob) {
    // first backward: D_l -> RT_l first half; G_l kept in LDS; G_0 = dV/dx0
    elu_first_backward(C, Hs, DZ, G, G0, w5s, L, [&](int l, int ot, int lane, float4 d4) {
      store_panel(gb.RT[l], ld, s0 + (lane & 15), ot, lane >> 4, d4);
    });
    // Sobolev loss gradient w.r.t. dV/ds, then w.r.t. G_0 (NeuralNetwork.py:167-170): one
    // (sample c, feature f) element per thread
    {
      const int c = L.tid >> 4, f = L.tid & 15;
      float gb0 = 0.f;
      if (f < ns - 1) {
        const float nf = (float)p.state_norm[f];
        auto nback = [&](float g) { return !p.normalize ? g : fdiv(g, nf); };  // f < ns - 1: not the time column
        const float gsq = fdiv(fmul(fdiv(1.f, (float)cs.B_global), ws[c]), (float)(ns - 1));
        const float dvds = nback(reinterpret_cast<const float*>(G0)[((f >> 2) * 16 + c) * 4 + (f & 3)]);
        const float yp = clog(dvds), yt = clog(dvdx[c * 16 + f]);
        const float gyp = fmul(fmul(2.f, gsq), fsub(yp, yt));
        gb0 = nback(clog_backward(dvds, gyp));
      }
      reinterpret_cast<float*>(GB)[((f >> 2) * 16 + c) * 4 + (f & 3)] = gb0;
      gb.LT[0][(size_t)f * ld + s0 + c] = gb0;  // the panel row of feature f (store_panel's layout)
    }
    __syncthreads();
    // backward of the first backward, l = 0..3 (oracle/nn.py compute_critic_grad), on the forward
    // fragments without bias: t_l = in_l W_l; zbar_l = (t_l G_{l+1}) elu''(z_l) (EluGrad's grad);
    // in_{l+1} = t_l elu'(z_l) -> LT_{l+1} first half, and over G_{l+1} in LDS (this lane's element,
    // just read). zbar_l goes over D_l (dead: its panel is written, its G pass done).
    auto sp_epi = [&](int l) {
      return [&, l](int ot, floatx4 acc) {
        const float4 h = Hs[(ELU_ZOFF[l] + ot) * 64 + L.lane];
        const float4 gu = l < 3 ? G[(ELU_ZOFF[l] + ot) * 64 + L.lane] : elu_w5(w5s, ot, L);
        const float4 t4 = f4(acc);
        ZB[(ELU_ZOFF[l] + ot) * 64 + L.lane] = mul4(mul4(t4, gu), elu_d2(h));
        const float4 g4 = mul4(t4, elu_d1(h));  // MulGrad into the upstream grad
        if (l < 3) G[(ELU_ZOFF[l] + ot) * 64 + L.lane] = g4;
        store_panel(gb.LT[l + 1], ld, s0 + L.c, ot, L.g, g4);
      };
    };
    elu_layer<0, false, false>(C, GB, L, sp_epi(0));
    __syncthreads();
    elu_layer<1, false, false>(C, G + ELU_ZOFF[0] * 64, L, sp_epi(1));
    __syncthreads();
    elu_layer<2, false, false>(C, G + ELU_ZOFF[1] * 64, L, sp_epi(2));
    __syncthreads();
    elu_layer<3, false, false>(C, G + ELU_ZOFF[2] * 64, L, sp_epi(3));
    __syncthreads();
    if (L.tid < 16) gb.RT[4][s0 + L.tid] = 1.f;  // dW5 += Gbar_4 (G_4 = W5[:, 0])
  } else {
    for (int k = L.tid; k < ELU_TILES * 64; k += CACTO_THREADS) ZB[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();

  // value loss: Vbar = (2 * ((wS/B) * w)) * (V - y)   (Keras MSE, SUM_OVER_BATCH_SIZE)
  if (L.tid < 16) {
    const int c = L.tid;
    const float wv = sob ? cs.w_S : 1.f;
    const float gl = fmul(fdiv(wv, (float)cs.B_global), ws[c]);
    Vb[c] = fmul(fmul(2.f, gl), fsub(V[c], y[c]));
    gb.RT[4][Bp + s0 + c] = Vb[c];
    if (s0 + c < B) {
      if (y_out) y_out[s0 + c] = y[c];
      if (V_out) V_out[s0 + c] = V[c];
      if (Vt_out && cs.want_vt) Vt_out[s0 + c] = Vt2[c];
    }
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < 4; ++t) {  // zbar_3 += (Vbar * W5) * elu'(z3): out tiles wave + 4 t
    const int ot = L.wave + 4 * t;
    const float4 c = elu_d1(Hs[(ELU_ZOFF[3] + ot) * 64 + L.lane]);
    float4 zb = ZB[(ELU_ZOFF[3] + ot) * 64 + L.lane];
    const float4 w = elu_w5(w5s, ot, L);
    const float vb = Vb[L.c];
    zb.x = fadd(zb.x, fmul(fmul(vb, w.x), c.x));
    zb.y = fadd(zb.y, fmul(fmul(vb, w.y), c.y));
    zb.z = fadd(zb.z, fmul(fmul(vb, w.z), c.z));
    zb.w = fadd(zb.w, fmul(fmul(vb, w.w), c.w));
    ZB[(ELU_ZOFF[3] + ot) * 64 + L.lane] = zb;
  }
  __syncthreads();
  // backward through the forward graph: zbar_{l-1} += (zbar_l W_l^T) * elu'(z_{l-1})
  auto hb_epi = [&](int l) {
    return [&, l](int it, floatx4 acc) {
      const float4 c = elu_d1(Hs[(ELU_ZOFF[l - 1] + it) * 64 + L.lane]);
      float4 zb = ZB[(ELU_ZOFF[l - 1] + it) * 64 + L.lane];
      zb.x = fadd(zb.x, fmul(acc[0], c.x));
      zb.y = fadd(zb.y, fmul(acc[1], c.y));
      zb.z = fadd(zb.z, fmul(acc[2], c.z));
      zb.w = fadd(zb.w, fmul(acc[3], c.w));
      ZB[(ELU_ZOFF[l - 1] + it) * 64 + L.lane] = zb;
    };
  };
  auto store_rt = [&](int l) {
    for (int k = L.tid; k < ELU_OT[l] * 64; k += CACTO_THREADS) {
      const int ot = k >> 6, lane = k & 63;
      store_panel(gb.RT[l], ld, Bp + s0 + (lane & 15), ot, lane >> 4, ZB[(ELU_ZOFF[l] + ot) * 64 + lane]);
    }
  };
  store_rt(3);
  elu_layer<3, false, true>(C, ZB + ELU_ZOFF[3] * 64, L, hb_epi(3));
  __syncthreads();
  store_rt(2);
  elu_layer<2, false, true>(C, ZB + ELU_ZOFF[2] * 64, L, hb_epi(2));
  __syncthreads();
  store_rt(1);
  elu_layer<1, false, true>(C, ZB + ELU_ZOFF[1] * 64, L, hb_epi(1));
  __syncthreads();
  store_rt(0);
  __syncthreads();
}

__global__ void __launch_bounds__(CACTO_THREADS)
    k_critic_grad_elu(const SysDevice* __restrict__ sdp, NetView C, NetView Tg, ChainScalars cs,
                      const double* __restrict__ storage, const int32_t* __restrict__ idx,
                      const float* __restrict__ isw, int B, GradBufs gb, float* __restrict__ y_out,
                      float* __restrict__ V_out, float* __restrict__ Vt_out, int32_t* __restrict__ step) {
  __shared__ CriticLdsElu S;
  critic_chain_elu(S, chain_tile_of(blockIdx.x, gridDim.x, cs.xcd_tiles), sdp, C, Tg, cs, storage, idx, isw, B, gb,
                   y_out, V_out, Vt_out, step);
}

// ---------------------------------------------------------------- actor chain against the elu critic
// k_actor_grad / k_chain_pair (learn_kernels.hip) with actor_chain's critic pass at s' on the elu shape
template <int NJ>
__global__ void __launch_bounds__(CACTO_THREADS) __attribute__((amdgpu_waves_per_eu(actor_grad_wpe<NJ>(), 8)))
    k_actor_grad_elu(const SysDevice* __restrict__ sdp, NetView Ac, NetView C, ChainScalars cs,
                     const double* __restrict__ storage, const int32_t* __restrict__ idx, int B, GradBufs gb,
                     int32_t* __restrict__ step) {
  __shared__ ActorLds S;
  ChainScalars c = cs;
  if (cs.wait_p && cs.wait_at_start) {
    if (threadIdx.x == 0) pipe_wait(cs.wait_p, cs.wait_v, const_cast<unsigned long long*>(cs.wait_p) - 1);
    __syncthreads();
    c.wait_p = nullptr;
  }
  actor_chain<NJ, true>(S, chain_tile_of(blockIdx.x, gridDim.x, cs.xcd_tiles), sdp, Ac, C, c, storage, idx, B, gb,
                        step);
}

template <int NJ>
__global__ void __launch_bounds__(CACTO_THREADS)
    k_chain_pair_elu(const SysDevice* __restrict__ sdp, NetView C, NetView Tg, NetView Ac, ChainScalars cs,
                     const double* __restrict__ storage, const int32_t* __restrict__ idx_c,
                     const float* __restrict__ isw, const int32_t* __restrict__ idx_a, int B, int nct, GradBufs gbc,
                     GradBufs gba, float* __restrict__ y_out, float* __restrict__ V_out, int32_t* __restrict__ step) {
  constexpr size_t bytes = sizeof(CriticLdsElu) > sizeof(ActorLds) ? sizeof(CriticLdsElu) : sizeof(ActorLds);
  __shared__ __attribute__((aligned(16))) unsigned char smem[bytes];
  if ((int)blockIdx.x < nct) {
    critic_chain_elu(*reinterpret_cast<CriticLdsElu*>(smem), blockIdx.x, sdp, C, Tg, cs, storage, idx_c, isw, B, gbc,
                     y_out, V_out, nullptr, step);
  } else {
    actor_chain<NJ, true>(*reinterpret_cast<ActorLds*>(smem), blockIdx.x - nct, sdp, Ac, C, cs, storage, idx_a, B,
                          gba, step);
  }
}

template <int NJ>
struct LaunchActorChainElu {
  static int run(const cacto_sys* sys, NetView Ac, NetView C, ChainScalars cs, const double* storage,
                 const int32_t* idx, int B, GradBufs gb, int32_t* step, hipStream_t st) {
    hipLaunchKernelGGL(k_actor_grad_elu<NJ>, dim3(gb.Bp / CACTO_TILE), dim3(CACTO_THREADS), 0, st, sys->dev, Ac, C,
                       cs, storage, idx, B, gb, step);
    CACTO_CHECK_HIP(hipGetLastError());
    return CACTO_OK;
  }
};

template <int NJ>
struct LaunchChainPairElu {
  static int run(const cacto_sys* sys, NetView C, NetView Tg, NetView Ac, ChainScalars cs, const double* storage,
                 const int32_t* idx_c, const float* isw, const int32_t* idx_a, int B, GradBufs gbc, GradBufs gba,
                 float* y, float* V, int32_t* step, hipStream_t st) {
    const int nct = gbc.Bp / CACTO_TILE;
    hipLaunchKernelGGL(k_chain_pair_elu<NJ>, dim3(2 * nct), dim3(CACTO_THREADS), 0, st, sys->dev, C, Tg, Ac, cs,
                       storage, idx_c, isw, idx_a, B, nct, gbc, gba, y, V, step);
    CACTO_CHECK_HIP(hipGetLastError());
    return CACTO_OK;
  }
};

int launch_critic_forward_elu(const cacto_sys* sys, const NetView& N, const float* S, float* V, float* dVdS, int B,
                              hipStream_t st) {
  hipLaunchKernelGGL(k_critic_forward_elu, dim3(ceil_div(B, CACTO_TILE)), dim3(CACTO_THREADS), 0, st, sys->dev, N, S,
                     V, dVdS, B);
  CACTO_CHECK_HIP(hipGetLastError());
  return CACTO_OK;
}

int launch_critic_chain_elu(const cacto_sys* sys, const NetView& C, const NetView& Tg, const ChainScalars& cs,
                            const double* storage, const int32_t* idx, const float* isw, int B, const GradBufs& gb,
                            float* y, float* V, float* Vt, int32_t* step, hipStream_t st) {
  hipLaunchKernelGGL(k_critic_grad_elu, dim3(gb.Bp / CACTO_TILE), dim3(CACTO_THREADS), 0, st, sys->dev, C, Tg, cs,
                     storage, idx, isw, B, gb, y, V, Vt, step);
  CACTO_CHECK_HIP(hipGetLastError());
  return CACTO_OK;
}

int launch_actor_chain_elu(const cacto_sys* sys, const NetView& Ac, const NetView& C, const ChainScalars& cs,
                           const double* storage, const int32_t* idx, int B, const GradBufs& gb, int32_t* step,
                           hipStream_t st) {
  return dispatch_nj<LaunchActorChainElu>(sys->host.p, sys, Ac, C, cs, storage, idx, B, gb, step, st);
}

int launch_chain_pair_elu(const cacto_sys* sys, const NetView& C, const NetView& Tg, const NetView& Ac,
                          const ChainScalars& cs, const double* storage, const int32_t* idx_c, const float* isw,
                          const int32_t* idx_a, int B, const GradBufs& gbc, const GradBufs& gba, float* y, float* V,
                          int32_t* step, hipStream_t st) {
  return dispatch_nj<LaunchChainPairElu>(sys->host.p, sys, C, Tg, Ac, cs, storage, idx_c, isw, idx_a, B, gbc, gba, y,
                                         V, step, st);
}

}  // namespace cacto
