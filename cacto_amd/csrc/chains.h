// The per-sample chain device functions (one tile of a critic or an actor chain per workgroup) and
// their LDS layouts, shared by the translation units that instantiate chain kernels:
// learn_kernels.hip (the sine / sine-elu critics) and elu_kernels.hip (the elu critic). The includer
// defines the CSTAMP / CSTAMP_DECL / CSTAMP_FLUSH macros (no-ops outside the stamped builds).
#pragma once

#include "learn.h"
#include "net_common.h"
#include "elu_critic.h"

namespace cacto {

// Block b -> tile of a 16-sample chain grid. xcd_tiles (ntiles % 128 == 0): block b runs on XCD
// b % 8 (the dispatcher's round robin), which k_wgrad_big gives the 256-row chunks x, x + 8, ... —
// 16 tiles each — so XCD x takes the tiles of exactly those chunks and their panel rows are written
// into the L2 the GEMM reads them from. Which block runs a tile changes no value.
__device__ __forceinline__ int chain_tile_of(int b, int ntiles, int xcd_tiles) {
  if (!xcd_tiles) return b;
  const int x = b & 7, j = b >> 3;
  return ((j >> 4) * 8 + x) * 16 + (j & 15);
}

// The device-side waits of the pipeline: until *wait_p >= wait_v (normally already true: one load).
// Bounded: after ~2^22 polls (seconds) the wait gives up and latches the timeout word, so an
// ordering bug cannot hang the GPU; the host then fails the call (cacto_pipeline_check). The signal
// words live in cacto_sys::pipe_sig: [0] actor chains finished, [1] timeout latch, [2] critic Adam
// steps finished, [3] k_adam's last-workgroup counter, [4..7] the concurrency probe's words. Relaxed
// polls: the write-after-read order (the critic's Adam may overwrite what an actor chain read once
// that chain has finished) carries no data; for the read-after-write order (the actor chain reads
// what the critic's Adam wrote) the Adam's stores went through to memory before it published (see
// ChainScalars and DESIGN §3's memory-ordering contract).
// ("Memory-ordering contract", sites 2 and 3)
__device__ __forceinline__ void pipe_wait(const unsigned long long* wait_p, unsigned long long wait_v,
                                          unsigned long long* latch) {
  if (!wait_p) return;
  for (int k = 0; k < (1 << 22); ++k) {
    if (__hip_atomic_load(wait_p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= wait_v) return;
    __builtin_amdgcn_s_sleep(2);
  }
  __hip_atomic_store(latch, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void store_panel(float* base, int ld, int row, int t, int g, float4 v) {
  float* p = base + (size_t)(16 * t + 4 * g) * ld + row;
  p[0] = v.x;
  p[ld] = v.y;
  p[2 * (size_t)ld] = v.z;
  p[3 * (size_t)ld] = v.w;
}

// custom_logarithm (NeuralNetwork.py:140-148) and its TF gradient (tf.where / tf.maximum / Log).
__device__ __forceinline__ float clog(float x) {
  const float eps = 1e-7f;
  return x > 0.f ? logf(fadd(fmaxf(x, eps), 1.f)) : -logf(fadd(fmaxf(-x, eps), 1.f));
}
__device__ __forceinline__ float clog_backward(float x, float g) {
  const float eps = 1e-7f;
  const float ax = x > 0.f ? x : -x;
  if (!(ax >= eps)) return 0.f;  // Maximum grad goes to the constant when |x| < eps
  return fmul(g, fdiv(1.f, fadd(ax, 1.f)));
}

// ---------------------------------------------------------------- critic chain (a11)
// 92.7 KB: with the actor chain's 65 KB one critic and one actor workgroup share a CU (the
// pipelined large-batch update runs critic(t+1) and actor(t) side by side)
struct CriticLds {
  float4 X0[64], XT[64], G0[64];
  float4 Cs[24 * 64];  // cos z_l
  float4 Hs[24 * 64];  // h_l = sin z_l; zbar_l from the Sobolev backward on (the same slot: read, then written)
  float4 G[16 * 64];
  float4 GB[16 * 64];
  float4 red[4 * 64];
  float st[256], stn[256], dvdx[256];
  float Rs[16], ds[16], ws[16], Vn[16], V[16], y[16], Vb[16], Vt2[16];
};

// one 16-sample tile of the critic chain (workgroup-wide; S in LDS)
__device__ __forceinline__ void critic_chain(CriticLds& S, const int tile, const SysDevice* __restrict__ sdp,
                                             const NetView& C, const NetView& Tg, const ChainScalars& cs,
                                             const double* __restrict__ storage, const int32_t* __restrict__ idx,
                                             const float* __restrict__ isw, int B, const GradBufs& gb,
                                             float* __restrict__ y_out, float* __restrict__ V_out,
                                             float* __restrict__ Vt_out, int32_t* __restrict__ step) {
  float4 *X0 = S.X0, *XT = S.XT, *G0 = S.G0, *Cs = S.Cs, *Hs = S.Hs, *G = S.G, *ZB = S.Hs, *GB = S.GB, *red = S.red;
  float *st = S.st, *stn = S.stn, *dvdx = S.dvdx, *Rs = S.Rs, *ds = S.ds, *ws = S.ws, *Vn = S.Vn, *V = S.V, *y = S.y,
        *Vb = S.Vb, *Vt2 = S.Vt2;
  CSTAMP_DECL;
  CSTAMP(0);
  const cacto_sys_params& p = sdp->p;
  const Lane L;
  const int ns = p.nb_state, cols = 3 * ns + 3, s0 = tile * CACTO_TILE;
  const int ld = gb.ld, Bp = gb.Bp;
  const bool sob = cs.w_S != 0.f;
  const int zoff[4] = {0, 4, 8, 16};
  const int goff[4] = {0, 0, 4, 8};
  if (tile == 0 && L.tid == 0 && step) step[0] += 1;  // Keras critic optimizer iterations

  // the target network's fragments for the first pass (loaded during the row gathers, below)
  CriticFwdFrags TF;
  float4 w5[2];  // W5[:, 0] at this lane's rows of layer-3 out tiles wave, wave + 4
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const float* w = C.flat + C.t.woff[4] + 16 * (L.wave + 4 * t) + 4 * L.g;
    w5[t] = make_float4(w[0], w[1], w[2], w[3]);
  }
  const Norm4 nrm(p, L);  // state_norm of this lane's features, loaded with the rows
  {  // one (sample, feature) per thread: the row gathers overlap
    // branch-free gathers (clamped sample and feature indices, then zeroed): no load sits under
    // a branch, so the waits stay exact
    const int c = L.tid >> 4, f = L.tid & 15;
    const bool valid = s0 + c < B, in = valid && f < ns;
    const int sc = min(s0 + c, B - 1), fc = min(f, ns - 1);
    const int32_t row = idx[sc];
    // issued between the index load and the dependent row loads: the wait for the index (in-order
    // vmcnt) does not cover them, and they have both latencies to land
    TF.load<true>(Tg, L);
    TF.load_last(Tg, L);
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
  CSTAMP(1);

  // y = R + (1 - d) * V_tgt(s_next)   (NeuralNetwork.py:153-158)
  if (!cs.MC) critic_forward_tile_f(TF, Tg, XT, nullptr, nullptr, Hs, red, Vn, L, [](int, int, float4) {});
  __syncthreads();
  CSTAMP(2);
  if (L.tid < 16) y[L.tid] = cs.MC ? Rs[L.tid] : fadd(Rs[L.tid], fmul(fsub(1.f, ds[L.tid]), Vn[L.tid]));
  if (cs.want_vt) {  // the extra V_tgt(s) of NeuralNetwork.py:178
    critic_forward_tile_f(TF, Tg, X0, nullptr, nullptr, Hs, red, Vt2, L, [](int, int, float4) {});
    __syncthreads();
  }

  // forward at s, keeping sin z and cos z; h_l -> LT_l second half
  if (L.wave == 0) store_panel(gb.LT[0], ld, Bp + s0 + L.c, 0, L.g, X0[L.lane]);
  critic_forward_tile(C, X0, Cs, Hs, Hs, red, V, L, [&](int l, int ot, float4 h4) {
    store_panel(gb.LT[l + 1], ld, Bp + s0 + L.c, ot, L.g, h4);
  });
  __syncthreads();
  CSTAMP(3);

  CriticFwdFrags SF;
  if (sob) {
    // first backward: D_l -> RT_l first half; G_l kept in LDS; G_0 = dV/dx0
    critic_first_backward(C, Cs, GB, G, G0, red, L, [&](int l, int ot, int lane, float4 d4) {
      store_panel(gb.RT[l], ld, s0 + (lane & 15), ot, lane >> 4, d4);
    });
    __syncthreads();
    CSTAMP(4);
    SF.load<false>(C, L);
    // Sobolev loss gradient w.r.t. dV/ds, then w.r.t. G_0 (NeuralNetwork.py:167-170): one
    // (sample c, feature f) element per thread (the same ops as per lane and feature)
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
    CSTAMP(5);
    // backward of the first backward, l = 0..3 (see oracle/nn.py compute_critic_grad), on the
    // forward fragments (no bias, loaded before the Sobolev loss above)
    // ZB aliases Hs: each lane reads sin z_l of its element, then writes zbar_l over it (no other
    // reader of that element is left: later passes read other layers' slots)
    auto sp_epi = [&](int l, float4* nxt) {
      return [&, l, nxt](int ot, floatx4 acc) {
        const float4 sz = Hs[(zoff[l] + ot) * 64 + L.lane], cz = Cs[(zoff[l] + ot) * 64 + L.lane];
        const float4 gu = l < 3 ? G[(goff[l + 1] + ot) * 64 + L.lane] : (ot >= 4 ? w5[1] : w5[0]);
        const float sv[4] = {sz.x, sz.y, sz.z, sz.w}, cv[4] = {cz.x, cz.y, cz.z, cz.w};
        const float gg[4] = {gu.x, gu.y, gu.z, gu.w};
        float zb[4], gn[4];
#ifdef CACTO_CRITIC_ELU
        const bool elu = (C.t.act >> l) & 1;
#else
        constexpr bool elu = false;
#endif
        for (int r = 0; r < 4; ++r) {
          // CosGrad: -grad * sin(x) (an elu layer: grad * exp(z) below zero)
          zb[r] = elu ? fmul(fmul(acc[r], gg[r]), act_d2(true, sv[r])) : fmul(-fmul(acc[r], gg[r]), sv[r]);
          gn[r] = fmul(acc[r], cv[r]);                 // MulGrad into the upstream grad
        }
        ZB[(zoff[l] + ot) * 64 + L.lane] = make_float4(zb[0], zb[1], zb[2], zb[3]);
        const float4 g4 = make_float4(gn[0], gn[1], gn[2], gn[3]);
        nxt[ot * 64 + L.lane] = g4;
        store_panel(gb.LT[l + 1], ld, s0 + L.c, ot, L.g, g4);
      };
    };
    float4* nA = GB + 8 * 64;
    SF.f0.run(GB, nullptr, 4, L.wave, L.lane, sp_epi(0, nA));
    __syncthreads();
    CSTAMP(6);
    SF.f1.run(nA, nullptr, 4, L.wave, L.lane, sp_epi(1, GB));
    __syncthreads();
    CSTAMP(7);
    SF.f2.run(GB, nullptr, 8, L.wave, L.lane, sp_epi(2, nA));
    __syncthreads();
    CSTAMP(8);
    SF.f3.run(nA, nullptr, 8, L.wave, L.lane, sp_epi(3, GB));
    __syncthreads();
    CSTAMP(9);
    if (L.tid < 16) gb.RT[4][s0 + L.tid] = 1.f;  // dW5 += Gbar_4 (G_4 = W5[:, 0])
  } else {
    for (int k = L.tid; k < 24 * 64; k += CACTO_THREADS) ZB[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();
  CSTAMP(10);

  // the transposed fragments of the last backward pass, in flight during the value loss
  CriticBwdFrags HB;
  HB.load(C, L);
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
  for (int t = 0; t < 2; ++t) {  // zbar_3 += (Vbar * W5) * cos(z3): out tiles wave, wave + 4
    const int ot = L.wave + 4 * t;
    const float4 z = Cs[(zoff[3] + ot) * 64 + L.lane];
    float4 zb = ZB[(zoff[3] + ot) * 64 + L.lane];
    const float4 w = w5[t];
    const float vb = Vb[L.c];
    zb.x = fadd(zb.x, fmul(fmul(vb, w.x), z.x));
    zb.y = fadd(zb.y, fmul(fmul(vb, w.y), z.y));
    zb.z = fadd(zb.z, fmul(fmul(vb, w.z), z.z));
    zb.w = fadd(zb.w, fmul(fmul(vb, w.w), z.w));
    ZB[(zoff[3] + ot) * 64 + L.lane] = zb;
  }
  __syncthreads();
  CSTAMP(11);
  // backward through the forward graph: zbar_{l-1} += (zbar_l W_l^T) * cos(z_{l-1})
  auto hb_epi = [&](int l) {
    return [&, l](int it, floatx4 acc) {
      const float4 z = Cs[(zoff[l - 1] + it) * 64 + L.lane];
      float4 zb = ZB[(zoff[l - 1] + it) * 64 + L.lane];
      zb.x = fadd(zb.x, fmul(acc[0], z.x));
      zb.y = fadd(zb.y, fmul(acc[1], z.y));
      zb.z = fadd(zb.z, fmul(acc[2], z.z));
      zb.w = fadd(zb.w, fmul(acc[3], z.w));
      ZB[(zoff[l - 1] + it) * 64 + L.lane] = zb;
    };
  };
  auto store_rt = [&](int l) {
    for (int k = L.tid; k < C.t.OT[l] * 64; k += CACTO_THREADS) {
      const int ot = k >> 6, lane = k & 63;
      store_panel(gb.RT[l], ld, Bp + s0 + (lane & 15), ot, lane >> 4, ZB[(zoff[l] + ot) * 64 + lane]);
    }
  };
  store_rt(3);
  HB.g3.run(ZB + zoff[3] * 64, nullptr, 8, L.wave, L.lane, hb_epi(3));
  __syncthreads();
  CSTAMP(12);
  store_rt(2);
  HB.g2.run(ZB + zoff[2] * 64, nullptr, 4, L.wave, L.lane, hb_epi(2));
  __syncthreads();
  CSTAMP(13);
  store_rt(1);
  HB.g1.run(ZB + zoff[1] * 64, nullptr, 4, L.wave, L.lane, hb_epi(1));
  __syncthreads();
  CSTAMP(14);
  store_rt(0);
  CSTAMP(15);
  __syncthreads();
  CSTAMP_FLUSH;
}

// env_simulate_derivative (env.h) of a revolute chain for a tile's T samples, spread over threads
// (a tile leaves most of the workgroup idle during the float64 dynamics): M(q) by CRBA (wave 1)
// beside h(q, v) by RNEA (wave 0) — chain_mass / chain_nle, the two halves of chain_terms in its
// operation order — then per sample NJ + 1 threads each factor M and solve one right-hand side:
// a - h (the step) or e_j (column j of M^-1, a column of Fu). The same operations on the same values
// as the one-thread path, so s' and Fu are bit-identical to it. st / stn: [T][16] floats, A: [T][NA],
// Fu: [T][CACTO_MAX_STATE * CACTO_MAX_ACTION], dM / dh: float64 scratch. Contains two barriers.
template <int NJ, int T>
__device__ __forceinline__ void chain_dynamics_spread(const SysDevice& sd, const float* st, const float* A,
                                                      double* dM, double* dh, float* stn, float* Fu, int tid) {
  constexpr int NS = Dims<NJ>::NS, NA = Dims<NJ>::NA;
  const cacto_sys_params& p = sd.p;
  const int wave = tid >> 6, lane = tid & 63;
  if constexpr (NJ == 3) {
    if (sd.pl[0] != 0.0) {
      // the planar 3R chain (the manipulator): the closed form is short, one thread per sample
      // (env_simulate_derivative's planar path, as the 16-sample chain's)
      if (tid < T) {
        const int c = tid;
        double s[NS], a[NA], sn[NS], F[NS * NA];
#pragma unroll
        for (int f = 0; f < NS; ++f) s[f] = (double)st[c * 16 + f];
#pragma unroll
        for (int i = 0; i < NA; ++i) a[i] = (double)A[c * NA + i];
        (void)env_simulate_derivative_planar3(sd, s, a, true, sn, F);
#pragma unroll
        for (int f = 0; f < 16; ++f) stn[c * 16 + f] = f < NS ? (float)sn[f] : 0.f;
#pragma unroll
        for (int k = 0; k < NS * NA; ++k) Fu[c * CACTO_MAX_STATE * CACTO_MAX_ACTION + k] = (float)F[k];
      }
      __syncthreads();
      __syncthreads();
      return;
    }
  }
  if (wave < 2 && lane < T) {
    const int c = lane;
    double q[NJ], v[NJ];
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
      q[i] = (double)st[c * 16 + i];
      v[i] = (double)st[c * 16 + NJ + i];
    }
    if (wave == 0) {
      double h[NJ];
      chain_nle<NJ>(sd, q, v, h);
#pragma unroll
      for (int i = 0; i < NJ; ++i) dh[c * NJ + i] = h[i];
    } else {
      double M[NJ * NJ];
      chain_mass<NJ>(sd, q, M);
#pragma unroll
      for (int k = 0; k < NJ * NJ; ++k) dM[c * NJ * NJ + k] = M[k];
    }
  }
  __syncthreads();
  CSTAMP(12);
  if (tid < T * (NJ + 1)) {
    const int c = tid / (NJ + 1), j = tid - c * (NJ + 1);
    const double dt = p.dt;
    double L[NJ * NJ], x[NJ];
#pragma unroll
    for (int k = 0; k < NJ * NJ; ++k) L[k] = dM[c * NJ * NJ + k];
    (void)cholesky<NJ>(L);
    if (j == 0) {
#pragma unroll
      for (int i = 0; i < NJ; ++i) x[i] = (double)A[c * NA + i] - dh[c * NJ + i];
      chol_solve<NJ>(L, x);
      float* sn = stn + c * 16;
#pragma unroll
      for (int i = 0; i < NJ; ++i) {  // env_simulate_derivative's f32in update
        const double s = (double)st[c * 16 + i], vv = (double)st[c * 16 + NJ + i];
        const float vdt = __fmul_rn((float)vv, (float)dt);
        sn[i] = (float)(s + (double)vdt);
        sn[NJ + i] = (float)(double)(float)(vv + x[i] * dt);
      }
      sn[2 * NJ] = (float)((double)st[c * 16 + 2 * NJ] + dt);
#pragma unroll
      for (int f = NS; f < 16; ++f) sn[f] = 0.f;
    } else {
      const int col = j - 1;
#pragma unroll
      for (int i = 0; i < NJ; ++i) x[i] = (i == col) ? 1.0 : 0.0;
      chol_solve<NJ>(L, x);
      float* F = Fu + c * CACTO_MAX_STATE * CACTO_MAX_ACTION;
#pragma unroll
      for (int r = 0; r < NS; ++r) {
        double v = 0.0;
        if (r >= NJ && r < 2 * NJ) {
          v = x[r - NJ] * dt;
          if (p.normalize) v *= sd.inv_norm[r];
        }
        F[r * NA + col] = (float)v;
      }
    }
  }
  __syncthreads();
}

// ---------------------------------------------------------------- actor chain (a12)
// Waves per SIMD the large-batch actor chain is compiled for. 2 (<= 256 registers, some spilled)
// lets one actor and one critic workgroup share a CU: manipulator B = 8192 5.86 k -> 7.14 k
// updates/s, car_park 8.78 k -> 8.99 k; the DI (10.84 k -> 10.53 k) and UR5 (10.6 k -> 9.1 k:
// 1.9 KB of spills) keep 1. AG_WPE overrides it for every system (A/B builds).
#ifndef AG_SPREAD_NJ
#define AG_SPREAD_NJ 4  // chains from this many joints take chain_dynamics_spread in the actor chain
#endif
#ifndef AG_RING
#define AG_RING 24  // fragments in flight in the actor's W2^T pass (mm_layer_ring)
#endif
template <int NJ>
constexpr int actor_grad_wpe() {
#ifdef AG_WPE
  return AG_WPE;
#else
  return NJ == 6 ? 1 : 2;
#endif
}
// 65 KB (see CriticLds). The 40-tile region W holds, in turn: the actor's h1, h2 (tiles 0-31); the
// critic pass at s' — its h ping-pong (0-15) and cos z (16-39); the actor's zbar2 (16-31).
struct ActorLds {
  float4 X0[64], XS[64], G0[64], ZB3[64];
  float4 W[40 * 64];
  unsigned char ZS[32 * 64];  // sign bits (z > 0) of the actor's z1, z2: bit r of [(l * 16 + ot) * 64 + lane]
  float4 red[4 * 64];
  float st[256], stn[256], gn[256];
  float A[16 * CACTO_MAX_ACTION];
  float Fu[16 * CACTO_MAX_STATE * CACTO_MAX_ACTION];
  float dra[16 * CACTO_MAX_ACTION];
  float Vn[16];
  double term_s[16];
};

// one 16-sample tile of the actor chain (workgroup-wide; S in LDS)
// ELU: the critic pass at s' on the elu critic's shape (elu_critic.h) instead of the sine critics'
template <int NJ, bool ELU = false>
__device__ __forceinline__ void actor_chain(ActorLds& S, const int tile, const SysDevice* __restrict__ sdp,
                                            const NetView& Ac, const NetView& C, const ChainScalars& cs,
                                            const double* __restrict__ storage, const int32_t* __restrict__ idx, int B,
                                            const GradBufs& gb, int32_t* __restrict__ step) {
  float4 *X0 = S.X0, *XS = S.XS, *G0 = S.G0, *ZB3 = S.ZB3, *H = S.W, *ZC = S.W + 16 * 64, *red = S.red;
  unsigned char* ZS = S.ZS;
  float *st = S.st, *stn = S.stn, *gn = S.gn, *A = S.A, *Fu = S.Fu, *dra = S.dra, *Vn = S.Vn;
  double* term_s = S.term_s;
  CSTAMP(0);
  const SysDevice& sd = *sdp;
  const cacto_sys_params& p = sd.p;
  const Lane L;
  const int ns = p.nb_state, na = p.nb_action, cols = 3 * ns + 3, s0 = tile * CACTO_TILE;
  const int ld = gb.ld;
  if (tile == 0 && L.tid == 0 && step) step[1] += 1;  // Keras actor optimizer iterations
  Frag1<4> F1;  // actor layer 1 (ns -> 256), in flight during the row gathers
  F1.load(Ac.fwd(0), Ac.biasp(0), L.wave, L.lane);
  {
    const int c = L.tid >> 4, f = L.tid & 15;
    const bool valid = s0 + c < B;
    const double* rp = storage + (size_t)(valid ? idx[s0 + c] : 0) * cols;
    st[c * 16 + f] = (valid && f < ns) ? (float)rp[f] : 0.f;
    if (f == 0) term_s[c] = valid ? rp[3 * ns + 2] : 0.0;
  }
  __syncthreads();
  if (L.wave == 0) {
    fill_input_tile(p, st, X0, L);
    store_panel(gb.LT[0], ld, s0 + L.c, 0, L.g, X0[L.lane]);  // input of layer 0 (normalised)
  }
  __syncthreads();
  // actor forward; h1 -> LT_1, h2 -> LT_2
  CSTAMP(1);
  actor_forward_tile(Ac, na, X0, nullptr, H, red, A, L, [&](int l, int ot, float4 z4, float4 h4) {
    ZS[(l * 16 + ot) * 64 + L.lane] = (z4.x > 0.f) | (z4.y > 0.f) << 1 | (z4.z > 0.f) << 2 | (z4.w > 0.f) << 3;
    store_panel(gb.LT[l + 1], ld, s0 + L.c, ot, L.g, h4);
  }, &F1);
  __syncthreads();
  CSTAMP(2);
  // dynamics at (s, a) in float64 from float32 tensors (environment.py:134-144, :353-362)
  if constexpr (NJ >= AG_SPREAD_NJ) {
    // revolute chains spread over the workgroup (one thread per sample held all of it; UR5
    // spilled); d reward / d a on wave 2 alongside. Its float64 scratch takes the start of the W
    // region: the actor's h1 / h2 there are dead after the action layer, the critic pass at s'
    // that fills it comes after.
    if (L.tid >= 128 && L.tid < 144) {
      constexpr int NA = Dims<NJ>::NA;
      const int c = L.tid - 128;
      float af[NA], g[NA];
#pragma unroll
      for (int i = 0; i < NA; ++i) af[i] = A[c * na + i];
      const double tc = term_s[c];
      const double w6 = 6 >= p.n_weights ? 0.0 : tc * p.w_terminal[6] + (1.0 - tc) * p.w_running[6];
      (void)reward_batch_f32<NA>(p, w6, af, 0.0, g);
#pragma unroll
      for (int i = 0; i < NA; ++i) dra[c * na + i] = g[i];
    }
    double* dM = reinterpret_cast<double*>(S.W);
    static_assert(sizeof(double) * CACTO_TILE * (NJ * NJ + NJ) <= sizeof(S.W), "chain scratch in W");
    chain_dynamics_spread<NJ, CACTO_TILE>(sd, st, A, dM, dM + CACTO_TILE * NJ * NJ, stn, Fu, L.tid);
  } else if (L.tid < 16) {
    constexpr int NS = Dims<NJ>::NS, NA = Dims<NJ>::NA;
    const int c = L.tid;
    double s[NS], a[NA], sn[NS], F[NS * NA];
    float af[NA];
#pragma unroll
    for (int f = 0; f < NS; ++f) s[f] = (double)st[c * 16 + f];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      af[i] = A[c * na + i];
      a[i] = (double)af[i];
    }
    if constexpr (NJ > 0 && NJ <= 3) {
      if (p.const_dyn) env_simulate_derivative_const<NJ>(sd, s, a, true, sn, F);
      else env_simulate_derivative<NJ>(sd, s, a, true, sn, F);
    } else {
      env_simulate_derivative<NJ>(sd, s, a, true, sn, F);
    }
#pragma unroll
    for (int f = 0; f < 16; ++f) stn[c * 16 + f] = f < NS ? (float)sn[f] : 0.f;
#pragma unroll
    for (int k = 0; k < NS * NA; ++k) Fu[c * CACTO_MAX_STATE * CACTO_MAX_ACTION + k] = (float)F[k];
  } else if (L.tid >= 64 && L.tid < 80) {
    // wave 1, alongside the dynamics: only d reward / d a enters the actor gradient
    // (NeuralNetwork.py:199-204), and only the control cost depends on a, so the state terms of the
    // reward are not evaluated here
    constexpr int NA = Dims<NJ>::NA;
    const int c = L.tid - 64;
    float af[NA], g[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) af[i] = A[c * na + i];
    const double tc = term_s[c];
    const double w6 = 6 >= p.n_weights ? 0.0 : tc * p.w_terminal[6] + (1.0 - tc) * p.w_running[6];
    (void)reward_batch_f32<NA>(p, w6, af, 0.0, g);
#pragma unroll
    for (int i = 0; i < NA; ++i) dra[c * na + i] = g[i];
  }
  __syncthreads();
  CSTAMP(3);
  if (L.wave == 0) fill_input_tile(p, stn, XS, L);
  // pipeline: the critic this pass reads is written by the other stream's Adam
  if (cs.wait_p && L.tid == 0) pipe_wait(cs.wait_p, cs.wait_v, const_cast<unsigned long long*>(cs.wait_p) - 1);
  __syncthreads();
  // critic (already updated) at s': V and dV/dx0 (NeuralNetwork.py:190-195)
  float4* HC = H;            // 16 tiles
  float4* ZB2 = H + 16 * 64;  // 16 tiles
  CSTAMP(4);
  if constexpr (ELU) {
    // h_l in tiles 0-34 of W, each D_l then written over its h_l; W5 staged in gn (free until dQ/da)
    static_assert(ELU_TILES <= 40, "elu critic pass in W");
    elu_stage_w5(C, gn, L);
    elu_forward_tile<false>(C, XS, H, red, Vn, L, [](int, int, float4) {});  // V(s') unused
    __syncthreads();
    CSTAMP(5);
    elu_first_backward(C, H, H, nullptr, G0, gn, L, [](int, int, int, float4) {});
  } else {
  critic_forward_tile<false>(C, XS, ZC, nullptr, HC, red, Vn, L, [](int, int, float4) {});  // V(s') unused
  __syncthreads();
  CSTAMP(5);
  critic_first_backward(C, ZC, HC, nullptr, G0, red, L, [](int, int, int, float4) {});
  }
  __syncthreads();
  CSTAMP(6);
  // dQ/da = dV/ds' Fu + dr/da ; abar = -dQ/da / B  (NeuralNetwork.py:206-231)
  {  // d normalize / d s of every (sample, state) element at once, one per thread
    const int c = L.tid >> 4, i = L.tid & 15;
    if (i < ns) gn[c * 16 + i] = normalize_backward(p, i, reinterpret_cast<const float*>(G0)[((i >> 2) * 16 + c) * 4 + (i & 3)]);
  }
  // the two backward layers' first fragments, in flight during the rest of the dQ/da phase (W3^T:
  // KT = 1, every tile; W2^T: the first tile's 16 blocks); issued after the loads above waited on
  Frag1<4> B2;
  FragTile<16> B1;
  B2.load(Ac.bwd(2), nullptr, L.wave, L.lane);
  B1.load(Ac.bwd(1), L.wave, L.lane);
  __syncthreads();
  if (L.wave == 0) {
    const int c = L.c;
    float abar[4];
    for (int r = 0; r < 4; ++r) {
      const int j = 4 * L.g + r;
      abar[r] = 0.f;
      if (j < na && s0 + c < B) {
        float q = 0.f;
        for (int i = 0; i < ns; ++i) {
          const float t = fmul(gn[c * 16 + i], Fu[c * CACTO_MAX_STATE * CACTO_MAX_ACTION + i * na + j]);
          q = (i == 0) ? t : fadd(q, t);
        }
        q = fadd(q, dra[c * na + j]);
        abar[r] = fmul(-q, fdiv(1.f, (float)cs.B_global));
      }
    }
    const float4 v = make_float4(abar[0], abar[1], abar[2], abar[3]);
    ZB3[L.lane] = v;
    store_panel(gb.RT[2], ld, s0 + c, 0, L.g, v);
  }
  __syncthreads();
  CSTAMP(7);
  // zbar2 = (abar W3^T) * lrelu'(z2) ; zbar1 = (zbar2 W2^T) * lrelu'(z1)
  auto epi2 = [&](int it, floatx4 acc) {
    const unsigned zs = ZS[(16 + it) * 64 + L.lane];
    float o[4];
    for (int r = 0; r < 4; ++r) o[r] = (zs >> r & 1) ? acc[r] : fmul(acc[r], 0.3f);
    const float4 v = make_float4(o[0], o[1], o[2], o[3]);
    ZB2[it * 64 + L.lane] = v;
    store_panel(gb.RT[1], ld, s0 + L.c, it, L.g, v);
  };
  auto epi1 = [&](int it, floatx4 acc) {
    const unsigned zs = ZS[it * 64 + L.lane];
    float o[4];
    for (int r = 0; r < 4; ++r) o[r] = (zs >> r & 1) ? acc[r] : fmul(acc[r], 0.3f);
    store_panel(gb.RT[0], ld, s0 + L.c, it, L.g, make_float4(o[0], o[1], o[2], o[3]));
  };
  // the actor's fixed shape (see actor_forward_tile): W3^T KT = 1, W2^T KT = 16, 16 out tiles each
  mm_layer1_pre<4>(B2, ZB3, L.wave, L.lane, epi2, nullptr);
  __syncthreads();
  CSTAMP(8);
  mm_layer_ring<16, 4, AG_RING>(B1, Ac.bwd(1), ZB2, L.wave, L.lane, epi1);
  __syncthreads();
  CSTAMP(9);
  __syncthreads();
  CSTAMP_FLUSH;
#ifdef CACTO_STAMPS
  if (tile == 0 && L.tid == 0)
    for (int k_ = 0; k_ < 32; ++k_) g_astamps[k_] = cacto_stamp_s[k_];
#endif
}

}  // namespace cacto
