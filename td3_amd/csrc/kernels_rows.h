// Part of kernels.hip: the row kernels (one batch row per wave): row_policy_head, the TD3_particles heads,
// the unit / target loss rows, row_lnbwd, row_dispatch, row_kernel and the two-kind row_kernel2.
// Needs row_actor.h (RowCtx, the wide-head stage, the actor-head backward row) and kernels_prologues.h.
#pragma once
#include "dev.h"
#include "kernels.h"
#include "row_actor.h"
#include "kernels_prologues.h"

namespace td3 {

// ================================================================== row kernels
// One batch row per wave (grid: Bp/4 x nprob, 256 threads): the head / loss work between the
// GEMM stages.  Every operand of the row (and the head weights) is requested up front, the
// reductions are DPP wave sums; a wave's serial chain is a single row.
template <bool NORM, int RW = 1>
__device__ __forceinline__ void row_policy_head(const GemmProb& P, const RowCtx& c) {
  using namespace policy_head;
  // every field in one scalar-load batch, and the step counter (Philox noise) requested with
  // the row: left alone, the compiler fetched fields where used (a chain of kernel-argument round
  // trips) and the counter after the head's dot products (one more memory round trip at the tail)
  asm volatile("" ::"s"(P.ex[kH3]), "s"(P.ex[kGamma3]), "s"(P.ex[kBeta3]), "s"(P.ex[kW4]), "s"(P.ex[kB4]),
               "s"(P.ex[kNoise]), "s"(P.ex[kOut]), "s"(P.ex[kTanh]), "s"(P.ex[kU3]), "s"(P.ex[kStats3]),
               "s"(P.ex[kOut2]), "s"(P.exi[kK3]), "s"(P.exi[kLd3]), "s"(P.exi[kLdw4]), "s"(P.exi[kLdOut]),
               "s"(P.exi[kGenNoise]), "s"(P.exi[kAd]), "s"(P.exi[kActCol]), "s"(P.exi[kLdNoise]), "s"(P.exi[kTarget]),
               "s"(P.exi[kClamp]), "s"(P.exf[kMaxAction]), "s"(P.exf[kPolicyNoise]), "s"(P.exf[kNoiseClip]),
               "s"(P.seed), "s"(P.ctr), "s"(P.B), "s"(P.tile_begin));
  const int K3 = P.exi[kK3], ld3 = P.exi[kLd3], ldw4 = P.exi[kLdw4];
  const int ad = P.exi[kAd], sd = P.exi[kActCol];
  const bool target = P.exi[kTarget] != 0;
  const float ma = P.exf[kMaxAction];
  const bool gen = target && P.exi[kGenNoise];
  // the counter (ctr is always set, step.hip policy_head_prob) by an ordinary relaxed load whose address carries a
  // lane-dependent zero (mbcnt with an empty mask): a divergent load, so the value lands in VGPRs
  // and the compiler's own wait placement defers it to the Philox draw.  Left uniform, it is a
  // scalar load waited for ahead of the row's loads.
  const int64_t* ctrp = &P.ctr->total_it + __builtin_amdgcn_mbcnt_lo(0u, 0u);
  const uint64_t stepv = (uint64_t)__hip_atomic_load(ctrp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  float x[1][8], g[8], bb[8], mean[1], rstd[1];
  rv_load(x[0], P.ex[kH3] + (size_t)c.row * ld3, ld3, c.lane);
  if (NORM) {
    rv_load(g, P.ex[kGamma3], ld3, c.lane);
    rv_load(bb, P.ex[kBeta3], ld3, c.lane);
  }
  float nz = 0.f;
  if (target && !P.exi[kGenNoise] && c.lane < ad) nz = gld(P.ex[kNoise] + ((size_t)c.row * P.exi[kLdNoise] + c.lane));
  float mine = 0.f;                       // lane o keeps head output o
  if (RW > 1 && P.tile_begin) {           // wide head: W4's ad rows staged in LDS (wide_stage)
    extern __shared__ float4 row_lds4[];
    const float bl = gld(P.ex[kB4] + (c.lane < ad ? c.lane : 0));
    wide_stage<64 * RW>(row_lds4, reinterpret_cast<const float4*>(P.ex[kW4]), ad * ldw4 / 4,
               reinterpret_cast<const float4*>(P.ex[kW4]), 0);
    const float* hw = reinterpret_cast<const float*>(row_lds4);
    opaque8(x[0]); opaque8(g); opaque8(bb);
    TL_MARK(5);
    if (NORM) ln_fwd_rows<1>(x, g, bb, K3, c.lane, mean, rstd);
    for (int ob = 0; ob < ad; ob += kHeadRegs) {
      float pb[kHeadRegs];
#pragma unroll
      for (int o = 0; o < kHeadRegs; ++o) {
        float w[8];
        rv_load_lds(w, hw + (size_t)(ob + o < ad ? ob + o : 0) * ldw4, ldw4, c.lane);
        pb[o] = rv_pdot(x[0], w, K3, c.lane);
      }
#pragma unroll
      for (int o = 0; o < kHeadRegs; ++o)
        if (ob + o < ad) {
          const float z = wsum(pb[o]) + bl;   // lane ob + o holds b4[ob + o]
          if (c.lane == ob + o) mine = z;
        }
    }
  } else {
  float w4[kHeadRegs][8], b4v[kHeadRegs];
#pragma unroll
  for (int o = 0; o < kHeadRegs; ++o) {
    const int oo = o < ad ? o : 0;
    rv_load(w4[o], P.ex[kW4] + (size_t)oo * ldw4, ldw4, c.lane);
    b4v[o] = gld(P.ex[kB4] + oo);
  }
  TL_MARK(5);
  TL_FINE(6);
  if (NORM) ln_fwd_rows<1>(x, g, bb, K3, c.lane, mean, rstd);
  float part[kHeadRegs];
#pragma unroll
  for (int o = 0; o < kHeadRegs; ++o) part[o] = rv_pdot(x[0], w4[o], K3, c.lane);
#pragma unroll
  for (int o = 0; o < kHeadRegs; ++o)
    if (o < ad) {
      const float z = wsum(part[o]) + b4v[o];
      if (c.lane == o) mine = z;
    }
  // wide action spaces without the LDS stage: further blocks of kHeadRegs outputs, each block's
  // W4 rows and biases requested in one batch (one load round trip per block)
  for (int ob = kHeadRegs; ob < ad; ob += kHeadRegs) {
    float wb[kHeadRegs][8], bv[kHeadRegs];
#pragma unroll
    for (int o = 0; o < kHeadRegs; ++o) {
      const int oo = ob + o < ad ? ob + o : 0;
      rv_load(wb[o], P.ex[kW4] + (size_t)oo * ldw4, ldw4, c.lane);
      bv[o] = gld(P.ex[kB4] + oo);
    }
    float pb[kHeadRegs];
#pragma unroll
    for (int o = 0; o < kHeadRegs; ++o) pb[o] = rv_pdot(x[0], wb[o], K3, c.lane);
#pragma unroll
    for (int o = 0; o < kHeadRegs; ++o)
      if (ob + o < ad) {
        const float z = wsum(pb[o]) + bv[o];
        if (c.lane == ob + o) mine = z;
      }
  }
  }
  if (!target) {
    if (NORM) rv_store(P.ex[kU3] + (size_t)c.row * ld3, ld3, c.lane, x[0]);
    if (NORM && c.lane == 0) {
      gst(P.ex[kStats3] + c.row, mean[0]);
      gst(P.ex[kStats3] + (c.Bp + c.row), rstd[0]);
    }
  }
  TL_MARK(7);
  if (c.lane >= ad) return;
  const int o = c.lane;
  const bool live = c.row < P.B;
  const float th = tanhf(mine);
  float a;
  if (target) {
    float z = nz;
    if (gen) {                                               // Philox N(0,1) (randn_like, :132)
      float g4[4];
      philox_normal4(P.seed, stepv, kStreamNoise, (uint32_t)(c.row * 8 + (o >> 2)), g4);
      z = g4[o & 3];
      gst(P.ex[kNoise] + ((size_t)c.row * P.exi[kLdNoise] + o), z);
    }
    float n = z * P.exf[kPolicyNoise];
    n = fminf(fmaxf(n, -P.exf[kNoiseClip]), P.exf[kNoiseClip]);
    const float v = ma * th + n;
    a = P.exi[kClamp] ? fminf(fmaxf(v, -ma), ma) : v;
  } else {
    a = ma * th;
    gst(P.ex[kTanh] + ((size_t)c.row * 32 + o), th);
  }
  gst(P.ex[kOut] + ((size_t)c.row * P.exi[kLdOut] + sd + o), live ? a : 0.f);
  if (P.ex[kOut2]) gst(P.ex[kOut2] + ((size_t)c.row * P.exi[kLdOut] + sd + o), live ? a : 0.f);
}

// ================================================================== TD3_particles heads
// The Q networks of TD3_particles output one value per action dimension (Q head [A, 300],
// TD3_particles.py:91); y = r + not_done*discount*min(Q1', Q2') broadcasts over them (:183-189)
// and F.mse_loss averages over B*A.  Values / targets are kept as [Bp][32] rows.
// Each squared error carries its row's importance weight w (one per transition, shared by its A
// outputs; 1 unless the step is prioritized, and then exact): dL/dQ_j,r,o = 2/(B*A) w_r (Q_j,r,o - y_r,o).
// Each critic's problem also leaves its rows' sum over o of |Q_j - y| (kTd): the prioritized step
// combines the critics' rows into the |TD error| it writes back (per_td_combine_kernel, step.hip).

// (operands: critic_loss_p, kernels.h)
template <bool NORM>
__device__ __forceinline__ void row_critic_loss_p(const GemmProb& P, const RowCtx& c) {
  using namespace critic_loss_p;
  const int K3 = P.exi[kK3], ld3 = P.exi[kLd3], j = P.exi[kJ], nq = P.exi[kNq], ldw4 = P.exi[kLdw4];
  const bool cdq = P.exi[kCdq] != 0;
  float x0[1][8], x1[1][8], xq[1][8], h[1][8], g[3][8], bb[3][8];
  rv_load(x0[0], P.ex[kH3] + (size_t)c.row * ld3, ld3, c.lane);
  rv_load(x1[0], P.ex[kH3 + 1] + (size_t)c.row * ld3, ld3, c.lane);
  rv_load(xq[0], P.ex[kH3 + 2] + (size_t)c.row * ld3, ld3, c.lane);
  if (NORM) {
#pragma unroll
    for (int n = 0; n < 3; ++n) {
      rv_load(g[n], P.ex[kGamma3 + n], ld3, c.lane);
      rv_load(bb[n], P.ex[kBeta3 + n], ld3, c.lane);
    }
  }
  const float rw = gld(P.ex[kReward] + c.row), nd = gld(P.ex[kNotDone] + c.row);
  const float iw = gld(P.ex[kW] + c.row);      // with the row's other loads: one round trip
#pragma unroll
  for (int jj = 0; jj < 8; ++jj) h[0][jj] = xq[0][jj];
  float m0[1], s0[1], m1[1], s1[1], mq[1], sq[1];
  if (NORM) {
    ln_fwd_rows<1>(x0, g[0], bb[0], K3, c.lane, m0, s0);
    ln_fwd_rows<1>(x1, g[1], bb[1], K3, c.lane, m1, s1);
    ln_fwd_rows<1>(xq, g[2], bb[2], K3, c.lane, mq, sq);
  } else {
    mq[0] = 0.f;
    sq[0] = 1.f;
  }
  const bool live = c.row < P.B;
  float gu[1][8];
#pragma unroll
  for (int jj = 0; jj < 8; ++jj) gu[0][jj] = 0.f;
  // mse over B*A, times the row's importance weight (1 unless the step is prioritized, and then exact)
  const float gs = P.exf[kGradScale] * iw;
  float se = 0.f, ta = 0.f;
  for (int o = 0; o < nq; ++o) {
    float w0[8], w1[8], wq[8];
    rv_load(w0, P.ex[kW4] + (size_t)o * ldw4, ld3, c.lane);
    rv_load(w1, P.ex[kW4 + 1] + (size_t)o * ldw4, ld3, c.lane);
    rv_load(wq, P.ex[kW4 + 2] + (size_t)o * ldw4, ld3, c.lane);
    const float tq0 = wsum(rv_pdot(x0[0], w0, K3, c.lane)) + gld(P.ex[kW4] + (P.exi[kB4Off] + o));
    const float tq1 = cdq ? wsum(rv_pdot(x1[0], w1, K3, c.lane)) + gld(P.ex[kW4 + 1] + (P.exi[kB4Off + 1] + o)) : tq0;
    const float q = wsum(rv_pdot(xq[0], wq, K3, c.lane)) + gld(P.ex[kW4 + 2] + (P.exi[kB4Off + 2] + o));
    const float y = rw + (nd * P.exf[kDiscount]) * fminf(tq0, tq1);          // TD3_particles.py:183-189
    const float d = q - y;
    const float gq = live ? gs * d : 0.f;
    se += live ? d * d : 0.f;
    ta += live ? fabsf(d) : 0.f;
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) gu[0][jj] += gq * wq[jj];
    if (c.lane == 0) {
      gst(P.ex[kDZ4] + ((size_t)c.row * 32 + o), gq);
      gst(P.ex[kQ] + ((size_t)c.row * 32 + o), q);
      if (j == 0) gst(P.ex[kY] + ((size_t)c.row * 32 + o), y);
    }
  }
  if (c.lane == 0) {
    gst(P.ex[kSqErr] + c.row, iw * se);
    gst(P.ex[kTd] + c.row, ta);
    if (NORM) {
      gst(P.ex[kStats3] + c.row, mq[0]);
      gst(P.ex[kStats3] + (c.Bp + c.row), sq[0]);
    }
  }
  rv_store(P.ex[kDU3] + (size_t)c.row * ld3, ld3, c.lane, gu[0]);
  if (NORM) rv_store(P.ex[kU3] + (size_t)c.row * ld3, ld3, c.lane, xq[0]);
  ln_bwd_rows<1>(gu, h, g[2], mq, sq, K3, c.lane, NORM);
  rv_store(P.Aout + (size_t)c.row * P.ldao, P.ldao, c.lane, gu[0]);
}

// -mean over B*nq of Q1(s, pi(s)) (TD3_particles.py:211-212), head + LN3 backward of Q1.
// (operands: actor_loss_p, kernels.h)
template <bool NORM>
__device__ __forceinline__ void row_actor_loss_p(const GemmProb& P, const RowCtx& c) {
  using namespace actor_loss_p;
  const int K3 = P.exi[kK3], ld3 = P.exi[kLd3], nq = P.exi[kNq], ldw4 = P.exi[kLdw4];
  float x[1][8], h[1][8], g[8], bb[8], mean[1], rstd[1];
  rv_load(x[0], P.ex[kH3] + (size_t)c.row * ld3, ld3, c.lane);
  if (NORM) {
    rv_load(g, P.ex[kGamma3], ld3, c.lane);
    rv_load(bb, P.ex[kBeta3], ld3, c.lane);
  }
#pragma unroll
  for (int jj = 0; jj < 8; ++jj) h[0][jj] = x[0][jj];
  if (NORM) ln_fwd_rows<1>(x, g, bb, K3, c.lane, mean, rstd);
  const float gq = c.row < P.B ? P.exf[kGradScale] : 0.f;
  float gu[1][8];
#pragma unroll
  for (int jj = 0; jj < 8; ++jj) gu[0][jj] = 0.f;
  for (int o = 0; o < nq; ++o) {
    float w[8];
    rv_load(w, P.ex[kW4] + (size_t)o * ldw4, ld3, c.lane);
    const float q = wsum(rv_pdot(x[0], w, K3, c.lane)) + gld(P.ex[kB4] + o);
    if (c.lane == 0) gst(P.ex[kQ] + ((size_t)c.row * 32 + o), q);
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) gu[0][jj] += gq * w[jj];
  }
  ln_bwd_rows<1>(gu, h, g, mean, rstd, K3, c.lane, NORM);
  rv_store(P.Aout + (size_t)c.row * P.ldao, P.ldao, c.lane, gu[0]);
}

// dQ1/da through lnorm1 (the Q input LayerNorm, no ReLU before it), tanh backward (no
// max_action, TD3_particles.py:68), then the actor head and LN3 backward.
// (operands: actor_head_bwd_p, kernels.h)
template <bool NORM>
__device__ __forceinline__ void row_actor_head_bwd_p(const GemmProb& P, const RowCtx& c) {
  using namespace actor_head_bwd_p;
  const int Kin = P.exi[kKin], ldin = P.exi[kLdIn], acol = P.exi[kActCol], ad = P.exi[kAd];
  const int K3 = P.exi[kK3], ld3 = P.exi[kLd3], ldw4 = P.exi[kLdw4];
  const float ma = P.exf[kMaxAction];
  float gu[1][8], xr[1][8], gi[8], h3[1][8], g3[8], mi[1], ri[1], mn3[1], rs3[1];
  rv_load(gu[0], P.ex[kDUin] + (size_t)c.row * ldin, ldin, c.lane);
  rv_load(xr[0], P.ex[kXin] + (size_t)c.row * ldin, ldin, c.lane);
  rv_load(h3[0], P.ex[kH3] + (size_t)c.row * ld3, ld3, c.lane);
  if (NORM) {
    rv_load(gi, P.ex[kGammaIn], ldin, c.lane);
    rv_load(g3, P.ex[kGamma3], ld3, c.lane);
    mi[0] = gld(P.ex[kStatsIn] + c.row);
    ri[0] = gld(P.ex[kStatsIn] + (c.Bp + c.row));
    mn3[0] = gld(P.ex[kStats3] + c.row);
    rs3[0] = gld(P.ex[kStats3] + (c.Bp + c.row));
  } else {
    mi[0] = mn3[0] = 0.f;
    ri[0] = rs3[0] = 1.f;
  }
  const float tl = c.lane < ad ? gld(P.ex[kTanh] + ((size_t)c.row * 32 + c.lane)) : 0.f;
  ln_bwd_rows<1, false>(gu, xr, gi, mi, ri, Kin, c.lane, NORM);     // grad of the Q input row
  const bool live = c.row < P.B;
  float gu3[1][8];
#pragma unroll
  for (int jj = 0; jj < 8; ++jj) gu3[0][jj] = 0.f;
  for (int o = 0; o < ad; ++o) {
    const int col = acol + o;                                         // rcol^-1: lane, register
    const int jsel = ((col >> 8) << 2) + (col & 3);
    float v = 0.f;
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) v = jj == jsel ? gu[0][jj] : v;
    const float ga = __shfl(v, (col & 255) >> 2, 64);
    const float t = __shfl(tl, o, 64);
    const float gz4 = live ? (ga * ma) * (1.f - t * t) : 0.f;
    if (c.lane == 0) gst(P.ex[kDZ4] + ((size_t)c.row * 32 + o), gz4);
    float w4[8];
    rv_load(w4, P.ex[kW4] + (size_t)o * ldw4, ld3, c.lane);
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) gu3[0][jj] += gz4 * w4[jj];
  }
  rv_store(P.ex[kDU3] + (size_t)c.row * ld3, ld3, c.lane, gu3[0]);
  ln_bwd_rows<1>(gu3, h3, g3, mn3, rs3, K3, c.lane, NORM);
  rv_store(P.Aout + (size_t)c.row * P.ldao, P.ldao, c.lane, gu3[0]);
}

// ---- unit-gradient critic head (kRowUnitLoss) ----------------------------------------------
// The Q_j head (TD3_featured.py:145, Q.forward :74-81) and the backward of its mse term with
// dL/dQ_j = 1: every per-row gradient vector of the MLP backward is linear in the row's
// dL/dQ_j (LayerNorm backward and relu' are linear in the incoming gradient for fixed forward
// activations), so the input-grad chain runs on these unit rows while the target path is still
// computing y; the dW stage scales row r by g_r = 2/B (Q_j,r - y_r) (kRowTargetLoss).
// (operands: unit_loss, kernels.h)
template <bool NORM>
__device__ __forceinline__ void row_unit_loss(const GemmProb& P, const RowCtx& c) {
  using namespace unit_loss;
  asm volatile("" ::"s"(P.ex[kH3]), "s"(P.ex[kGamma3]), "s"(P.ex[kBeta3]), "s"(P.ex[kW4]), "s"(P.ex[kB4]),
               "s"(P.ex[kQ]), "s"(P.ex[kU3]), "s"(P.ex[kStats3]), "s"(P.ex[kDU3]), "s"(P.exi[kK3]), "s"(P.exi[kLd3]),
               "s"(P.Aout), "s"(P.ldao));
  const int K3 = P.exi[kK3], ld3 = P.exi[kLd3];
  float x[1][8], h[1][8], g[8], bb[8], w[8], mean[1] = {0.f}, rstd[1] = {1.f};
  rv_load(x[0], P.ex[kH3] + (size_t)c.row * ld3, ld3, c.lane);
  if (NORM) {
    rv_load(g, P.ex[kGamma3], ld3, c.lane);
    rv_load(bb, P.ex[kBeta3], ld3, c.lane);
  } else {
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) g[jj] = bb[jj] = 0.f;
  }
  rv_load(w, P.ex[kW4], ld3, c.lane);
  const float b4 = gld(P.ex[kB4]);
  __builtin_amdgcn_sched_barrier(0);     // every load requested before the first use
#pragma unroll
  for (int jj = 0; jj < 8; ++jj) h[0][jj] = x[0][jj];
  if (NORM) ln_fwd_rows<1>(x, g, bb, K3, c.lane, mean, rstd);
  const float q = wsum(rv_pdot(x[0], w, K3, c.lane)) + b4;
  if (c.lane == 0) {
    gst(P.ex[kQ] + c.row, q);
    if (NORM) {
      gst(P.ex[kStats3] + c.row, mean[0]);
      gst(P.ex[kStats3] + (c.Bp + c.row), rstd[0]);
    }
  }
  if (NORM) rv_store(P.ex[kU3] + (size_t)c.row * ld3, ld3, c.lane, x[0]);
  float gu[1][8];
#pragma unroll
  for (int jj = 0; jj < 8; ++jj) gu[0][jj] = w[jj];
  rv_store(P.ex[kDU3] + (size_t)c.row * ld3, ld3, c.lane, gu[0]);
  ln_bwd_rows<1>(gu, h, g, mean, rstd, K3, c.lane, NORM);
  rv_store(P.Aout + (size_t)c.row * P.ldao, P.ldao, c.lane, gu[0]);
}

// ---- clipped double-Q target and the rows' loss gradients (kRowTargetLoss) -----------------
// y = r + not_done * discount * min(Q1'(s',a'), Q2'(s',a')) (TD3_featured.py:140-142) and for both
// online critics g_j = 2/B w (Q_j - y) (F.mse_loss backward, :148, times the row's importance weight
// w: 1 unless the step is prioritized, and then exact): the head's dZ4_j and the row scale of Q_j's
// unit backward in the dW stage; the weighted squared errors for the loss read-back; the row's
// |TD error|, the mean over the twin, for the priority write-back.
// (operands: target_loss, kernels.h)
template <bool NORM>
__device__ __forceinline__ void row_target_loss(const GemmProb& P, const RowCtx& c) {
  using namespace target_loss;
  asm volatile("" ::"s"(P.ex[kH3]), "s"(P.ex[kH3 + 1]), "s"(P.ex[kGamma3]), "s"(P.ex[kGamma3 + 1]), "s"(P.ex[kBeta3]),
               "s"(P.ex[kBeta3 + 1]), "s"(P.ex[kW4]), "s"(P.ex[kW4 + 1]), "s"(P.ex[kB4]), "s"(P.ex[kB4 + 1]),
               "s"(P.ex[kReward]), "s"(P.ex[kNotDone]), "s"(P.ex[kQ]), "s"(P.ex[kQ + 1]), "s"(P.exi[kK3]),
               "s"(P.exi[kLd3]));
  asm volatile("" ::"s"(P.ex[kY]), "s"(P.ex[kDZ4]), "s"(P.ex[kDZ4 + 1]), "s"(P.ex[kSqErr]), "s"(P.ex[kG]),
               "s"(P.ex[kG + 1]), "s"(P.ex[kW]), "s"(P.ex[kTd]), "s"(P.exf[kDiscount]), "s"(P.exf[kGradScale]),
               "s"(P.B));
  const int K3 = P.exi[kK3], ld3 = P.exi[kLd3];
  float x0[1][8], x1[1][8], g[2][8], bb[2][8], w[2][8];
  rv_load(x0[0], P.ex[kH3] + (size_t)c.row * ld3, ld3, c.lane);
  rv_load(x1[0], P.ex[kH3 + 1] + (size_t)c.row * ld3, ld3, c.lane);
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    if (NORM) {
      rv_load(g[n], P.ex[kGamma3 + n], ld3, c.lane);
      rv_load(bb[n], P.ex[kBeta3 + n], ld3, c.lane);
    }
    rv_load(w[n], P.ex[kW4 + n], ld3, c.lane);
  }
  const float b40 = gld(P.ex[kB4]), b41 = gld(P.ex[kB4 + 1]);
  const float rw = gld(P.ex[kReward] + c.row), nd = gld(P.ex[kNotDone] + c.row);
  const float q1 = gld(P.ex[kQ] + c.row), q2 = gld(P.ex[kQ + 1] + c.row);
  const float iw = gld(P.ex[kW] + c.row);
  __builtin_amdgcn_sched_barrier(0);     // every load requested before the first use
  float m0[1], s0[1], m1[1], s1[1];
  if (NORM) {
    ln_fwd_rows<1>(x0, g[0], bb[0], K3, c.lane, m0, s0);
    ln_fwd_rows<1>(x1, g[1], bb[1], K3, c.lane, m1, s1);
  }
  const float d0 = rv_pdot(x0[0], w[0], K3, c.lane);
  const float d1 = rv_pdot(x1[0], w[1], K3, c.lane);
  const float tq0 = wsum(d0) + b40, tq1 = wsum(d1) + b41;
  const float y = rw + (nd * P.exf[kDiscount]) * fminf(tq0, tq1);                  // :141-142
  const bool live = c.row < P.B;
  const float e1 = q1 - y, e2 = q2 - y;
  // mse_loss bwd (:148)
  const float gs = P.exf[kGradScale] * iw;
  const float g1 = live ? gs * e1 : 0.f, g2 = live ? gs * e2 : 0.f;
  if (c.lane == 0) {
    gst(P.ex[kY] + c.row, y);
    gst(P.ex[kDZ4] + ((size_t)c.row * 32), g1);
    gst(P.ex[kDZ4 + 1] + ((size_t)c.row * 32), g2);
    gst(P.ex[kSqErr] + c.row, live ? iw * e1 * e1 : 0.f);
    gst(P.ex[kSqErr] + (c.Bp + c.row), live ? iw * e2 * e2 : 0.f);
    gst(P.ex[kG] + c.row, g1);
    gst(P.ex[kG + 1] + c.row, g2);
    gst(P.ex[kTd] + c.row, live ? 0.5f * (fabsf(e1) + fabsf(e2)) : 0.f);
  }
}

// ---- dZ = relu'(LN_bwd(dU)) of full rows (kRowLnBwd): lnbwd_rows_kernel's row as a row kind,
// so it can share a launch with another row stage.
// (operands: ln_bwd, kernels.h)
template <bool NORM>
__device__ __forceinline__ void row_lnbwd(const GemmProb& P, const RowCtx& c) {
  using namespace ln_bwd;
  asm volatile("" ::"s"(P.ex[kDU]), "s"(P.ex[kH]), "s"(P.ex[kStats]), "s"(P.ex[kGamma]), "s"(P.ex[kDZ]),
               "s"(P.exi[kLd]), "s"(P.exi[kK]));
  const int ld = P.exi[kLd];
  float gu[1][8], h[1][8], g[8], mean[1], rstd[1];
  float4 qg[2], qu[2], qh[2];
  if constexpr (NORM) rv_load_raw(qg, P.ex[kGamma], ld, c.lane);
  rv_load_raw(qu, P.ex[kDU] + (size_t)c.row * ld, ld, c.lane);
  rv_load_raw(qh, P.ex[kH] + (size_t)c.row * ld, ld, c.lane);
  mean[0] = NORM ? gld(P.ex[kStats] + c.row) : 0.f;
  rstd[0] = NORM ? gld(P.ex[kStats] + (c.Bp + c.row)) : 1.f;
  __builtin_amdgcn_sched_barrier(0);     // every load requested before the first use
  if constexpr (NORM) rv_from_raw(g, qg, ld, c.lane);
  else {
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) g[jj] = 0.f;
  }
  rv_from_raw(gu[0], qu, ld, c.lane);
  rv_from_raw(h[0], qh, ld, c.lane);
  if constexpr (NORM) ln_bwd_rows_pk<1>(gu, h, g, mean, rstd, 1.0f / (float)P.exi[kK]);
  else ln_bwd_rows<1>(gu, h, g, mean, rstd, P.exi[kK], c.lane, 0);
  rv_store(P.ex[kDZ] + (size_t)c.row * ld, ld, c.lane, gu[0]);
}

template <int KIND, bool NORM, int RW>
__device__ __forceinline__ void row_dispatch(const GemmProb& P, const RowCtx& c) {
  if constexpr (KIND == kRowPolicyHead) row_policy_head<NORM, RW>(P, c);
  else if constexpr (KIND == kRowActorHeadBwd) row_actor_head_bwd<NORM, RW>(P, c);
  else if constexpr (KIND == kRowCriticLossP) row_critic_loss_p<NORM>(P, c);
  else if constexpr (KIND == kRowActorLossP) row_actor_loss_p<NORM>(P, c);
  else if constexpr (KIND == kRowActorHeadBwdP) row_actor_head_bwd_p<NORM>(P, c);
  else if constexpr (KIND == kRowUnitLoss) row_unit_loss<NORM>(P, c);
  else if constexpr (KIND == kRowTargetLoss) row_target_loss<NORM>(P, c);
  else if constexpr (KIND == kRowLnBwd) row_lnbwd<NORM>(P, c);
}

template <int KIND, bool NORM, int RW = kRowWaves>
__global__ __launch_bounds__(64 * RW) void row_kernel(int Bp, GemmTable tab) {   // Bp first: preloaded
  const GemmProb& P = tab.p[blockIdx.y];
  // grid.x = Bp / RW exactly (launch_rows): every wave owns a row, no bounds check (which would put
  // a kernel-argument round trip ahead of the row's loads)
  const RowCtx c{(int)(blockIdx.x * RW + (threadIdx.x >> 6)), (int)(threadIdx.x & 63), Bp};
  TL_MARK(0);
  row_dispatch<KIND, NORM, RW>(P, c);
  TL_MARK(3);
}

// Two independent row stages in one launch (problems [0, n1) of kind K1, the rest K2): the
// branch is on blockIdx.y, uniform per workgroup.
template <int K1, int K2, bool NORM, int RW = kRowWaves>
__global__ __launch_bounds__(64 * RW) void row_kernel2(int Bp, int n1, GemmTable tab) {
  const GemmProb& P = tab.p[blockIdx.y];
  const RowCtx c{(int)(blockIdx.x * RW + (threadIdx.x >> 6)), (int)(threadIdx.x & 63), Bp};
  TL_MARK(0);
  if ((int)blockIdx.y < n1) row_dispatch<K1, NORM, RW>(P, c);
  else row_dispatch<K2, NORM, RW>(P, c);
  TL_MARK(3);
}

}  // namespace td3
