// The device code shared by kernels.hip, bc.hip and bcf.hip: the row kernels' context, the wide-head LDS
// stage and the actor-head backward row (plain: kRowActorHeadBwd, instantiated in kernels.hip; BC:
// kRowActorHeadBwdBc, instantiated in bc.hip; BC on the kept rows only: kRowActorHeadBwdBcF, instantiated in
// bcf.hip -- the kernels of each form a code object of their own and leave the others' as they are).
#pragma once
#include "dev.h"
#include "kernels.h"

namespace td3 {

// Workgroup barrier for LDS hand-offs: s_waitcnt lgkmcnt(0) + s_barrier, without the vmcnt(0) drain
// __syncthreads() adds (no workgroup reads global data another of its waves stored).
// TD3_SYNC_BARRIERS=1 restores __syncthreads() (A/B builds).
#ifndef TD3_SYNC_BARRIERS
#define TD3_SYNC_BARRIERS 0
#endif
__device__ __forceinline__ void lds_barrier() {
#if TD3_SYNC_BARRIERS
  __syncthreads();
#else
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#endif
}

#ifndef TD3_ROW_WAVES
#define TD3_ROW_WAVES 1
#endif
constexpr int kRowWaves = TD3_ROW_WAVES;   // waves (rows) per row-kernel workgroup: 1 (A/B 4 / 2 / 1: C2 8.93k / 9.03k / 9.09k; the waves of a row stage spread over 4x the CUs, whose load units they no longer share)

struct RowCtx {
  int row, lane, Bp;
};

// ---- policy heads: target smoothing (TD3_featured.py:131-137) / pi(s) = ma*tanh (:47-48) --
// (operands: policy_head, kernels.h)
constexpr int kHeadRegs = 8;   // head outputs kept in registers (wider heads loop)

// Wide heads (action width > kHeadRegs; Humanoid: 17).  Requested block by block, the head weight
// rows cost one dependent load round trip per kHeadRegs outputs (actor_head_bwd: a wave's chain
// 8 us at Humanoid B = 1024, profiles/r05_timeline_humanoid.txt).  Instead the workgroup stages
// every row once in (dynamic) LDS, all requests in one round trip, shared by its kWideRows rows
// (RW: the launch's rows per workgroup); launch_rows sizes the LDS, launches the RW = kWideRows
// variant and marks the problems (GemmProb::tile_begin = 1, otherwise unused by the row kernels).
// The LDS rows are the same values, used in the same order: bit-identical results.
constexpr int kWideStage = 16;   // float4 per thread: up to 64 KB staged by kWideRows waves
constexpr int kWideRows = 4;     // rows (waves) per workgroup of the wide-head row launches
// The row operands, re-defined after the stage: the wide and narrow paths' identical LayerNorm math
// on them was hoisted above the branch, i.e. waited for the rows before the stage was requested
__device__ __forceinline__ void opaque8(float (&v)[8]) {
  asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]));
}
__device__ __forceinline__ void opaque1(float& v) { asm volatile("" : "+v"(v)); }
template <int NT>
__device__ __forceinline__ void wide_stage(float4* dst, const float4* a, int n1, const float4* b, int n2) {
  const int n = n1 + n2;
  // surplus slots re-copy element `spare` (distinct per lane): unconditional loads and stores, so
  // the compiler cannot sink the loads into per-slot branches (one round trip per slot)
  const int spare = (int)threadIdx.x < n ? (int)threadIdx.x : 0;
  float4 v[kWideStage];
  int at[kWideStage];
#pragma unroll
  for (int i = 0; i < kWideStage; ++i) {
    const int e = (int)threadIdx.x + NT * i;
    at[i] = e < n ? e : spare;
    v[i] = at[i] < n1 ? a[at[i]] : b[at[i] - n1];
  }
#pragma unroll
  for (int i = 0; i < kWideStage; ++i) dst[at[i]] = v[i];
  lds_barrier();
}

// W[:, s0 .. s0+kHeadRegs): those columns of the 8 W rows a lane owns (rcol), as two float4 loads
// per row at the (4-B aligned) column s0 itself; columns at or past `lim` are 0.  (Aligned loads
// from below s0 needed a select on the uniform offset, which compiled to branches with a full
// load drain per row: 8 dependent load round trips.)
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
__device__ __forceinline__ void head_cols(const float* W, int ldw, int s0, int lim, int lane,
                                          float (&out)[kHeadRegs][8]) {
  static_assert(kHeadRegs == 8, "two float4 per row");
#pragma unroll
  for (int jj = 0; jj < 8; ++jj) {
    const float* wp = W + ((size_t)rcol(lane, jj) * ldw + s0);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const f32x4u t = *reinterpret_cast<const f32x4u*>(wp + 4 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e) out[4 * q + e][jj] = 4 * q + e < lim ? t[e] : 0.f;
    }
  }
}

// ---- TD3+BC (Fujimoto & Gu 2021; td3_set_bc): lambda = alpha / mean_r |Q1(s_r, pi(s_r))| -------
// sum over r < B of |Qv[r]| in ONE order, whatever the grid and whichever path asks: lane l adds rows
// l, l + 64, l + 128, .. ascending (rows at or past B add 0), then wsum's fixed tree over the 64
// lanes.  Eight rows' loads per lane are requested before the first add.  Every lane returns the sum.
__device__ __forceinline__ float bc_qabs_sum(const float* Qv, int B, int lane) {
  float s = 0.f;
  for (int r0 = 0; r0 < B; r0 += 64 * 8) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int r = r0 + 64 * k + lane;
      const float q = gld(Qv + (r < B ? r : 0));
      v[k] = r < B ? fabsf(q) : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) s += v[k];
  }
  return wsum(s);
}
// (lambda, mean |Q|) of that sum: no guard, a zero mean gives lambda = inf as the paper's code does
__device__ __forceinline__ float bc_lambda(float qsum, int B, float alpha, float* qabs) {
  *qabs = qsum / (float)B;
  return alpha / *qabs;
}
// dL/dpi_o = lambda g_o + 2/(B A) (pi_o - a_o): g_o = dQ1/da_o as the plain actor step has it (it
// carries -1/B), pi_o = max_action tanh_o; *se accumulates (pi_o - a_o)^2 in output order
__device__ __forceinline__ float bc_grad(float ga, float lam, float bcs, float ma, float t, float a, float* se) {
  const float d = ma * t - a;
  *se += d * d;
  return lam * ga + bcs * d;
}

// The row mask of the filtered BC term (td3_set_bc_filter; operands actor_head_bwd_bcf): row r keeps its
// term while r < n_d (the step's candidate rows: its demonstration rows, or all B) and, with the Q-filter
// (Nair et al. 2018), Q1(s_r, a_r) > Q1(s_r, pi_r) -- a strict fp32 compare, so a NaN on either side drops
// the row.  Each wave decides its own row and forms c = (float)(2.0 / ((double)n_d * A)) from the device
// word once; a row that is not kept gets c = 0 (n_d = 0 never uses the quotient).  Lane 0 writes keep[row].
__device__ __forceinline__ bool bcf_keep(const GemmProb& P, const RowCtx& c, int ad, float* bcs) {
  namespace bf = actor_head_bwd_bcf;
  asm volatile("" ::"s"(P.ex[bf::kQ1sa]), "s"(P.ex[bf::kNDemo]), "s"(P.ex[bf::kKeep]), "s"(P.exi[bf::kQFilter]));
  const float qsa = gld(P.ex[bf::kQ1sa] + c.row), qpi = gld(P.ex[bf::kQv] + c.row);
  const int nd = *(const GAS int*)P.ex[bf::kNDemo];
  const bool keep = c.row < nd && c.row < P.B && (!P.exi[bf::kQFilter] || qsa > qpi);
  *bcs = keep ? (float)(2.0 / ((double)nd * (double)ad)) : 0.f;
  if (c.lane == 0) gst(P.ex[bf::kKeep] + c.row, keep ? 1.f : 0.f);
  return keep;
}

// ---- dQ1/da through Q1's first layer, then the actor's head and LN3 backward -------------
// (operands: actor_head_bwd, kernels.h; BC: the TD3+BC row kind kRowActorHeadBwdBc, operands
// actor_head_bwd_bc -- the two extra terms of dL/dpi, the row's squared BC error, and lambda; kBcFiltered:
// kRowActorHeadBwdBcF, the same arithmetic with the row's c from bcf_keep and 0 as the squared error of a
// row that is not kept)
constexpr int kBcOff = 0, kBcAll = 1, kBcFiltered = 2;
template <bool NORM, int RW = 1, int BC = kBcOff>
__device__ __forceinline__ void row_actor_head_bwd(const GemmProb& P, const RowCtx& c) {
  using namespace actor_head_bwd;
  namespace bc = actor_head_bwd_bc;
  // every field in one scalar-load batch (left alone, the compiler requested them where used, in
  // dependent kernel-argument round trips between the row's loads)
  asm volatile("" ::"s"(P.ex[kDU0]), "s"(P.ex[kH0]), "s"(P.ex[kStats0]), "s"(P.ex[kGamma0]), "s"(P.ex[kW1]),
               "s"(P.ex[kTanh]), "s"(P.ex[kW4]), "s"(P.ex[kH3]), "s"(P.ex[kStats3]), "s"(P.ex[kGamma3]),
               "s"(P.ex[kDZ4]), "s"(P.ex[kDU3]), "s"(P.ex[kW1T]), "s"(P.exi[kK0]), "s"(P.exi[kLd0]),
               "s"(P.exi[kLdw1]), "s"(P.exi[kActCol]), "s"(P.exi[kAd]), "s"(P.exi[kK3]), "s"(P.exi[kLd3]),
               "s"(P.exi[kLdw4]), "s"(P.exi[kLdW1T]), "s"(P.exf[kMaxAction]), "s"(P.Aout), "s"(P.ldao), "s"(P.B),
               "s"(P.tile_begin));
  const int K0 = P.exi[kK0], ld0 = P.exi[kLd0], ldw1 = P.exi[kLdw1], sd = P.exi[kActCol], ad = P.exi[kAd];
  const int K3 = P.exi[kK3], ld3 = P.exi[kLd3], ldw4 = P.exi[kLdw4];
  const float ma = P.exf[kMaxAction];
  float gu0[1][8], h0[1][8], h3[1][8], g0[8], g3[8], mn0[1], rs0[1], mn3[1], rs3[1];
  float w1[kHeadRegs][8], w4[kHeadRegs][8];
  rv_load(gu0[0], P.ex[kDU0] + (size_t)c.row * ld0, ld0, c.lane);
  rv_load(h0[0], P.ex[kH0] + (size_t)c.row * ld0, ld0, c.lane);
  rv_load(h3[0], P.ex[kH3] + (size_t)c.row * ld3, ld3, c.lane);
  if (NORM) {
    rv_load(g0, P.ex[kGamma0], ld0, c.lane);
    rv_load(g3, P.ex[kGamma3], ld3, c.lane);
    mn0[0] = gld(P.ex[kStats0] + c.row);
    rs0[0] = gld(P.ex[kStats0] + (c.Bp + c.row));
    mn3[0] = gld(P.ex[kStats3] + c.row);
    rs3[0] = gld(P.ex[kStats3] + (c.Bp + c.row));
  } else {
    mn0[0] = mn3[0] = 0.f;
    rs0[0] = rs3[0] = 1.f;
  }
  const float tl = c.lane < ad ? gld(P.ex[kTanh] + ((size_t)c.row * 32 + c.lane)) : 0.f;
  float al = 0.f, lam = 0.f, bcs = 0.f, se = 0.f;   // BC: lane o's stored action a_o, lambda, 2/(B A), sum of (pi - a)^2
  bool keep = true;                                 // kBcFiltered: the row keeps its BC term
  if constexpr (BC) {
    asm volatile("" ::"s"(P.ex[bc::kQv]), "s"(P.ex[bc::kAct]), "s"(P.ex[bc::kRowSe]), "s"(P.ex[bc::kLam]),
                 "s"(P.exi[bc::kLdAct]), "s"(P.exf[bc::kAlpha]), "s"(P.exf[bc::kBcScale]));
    if (c.lane < ad) al = gld(P.ex[bc::kAct] + ((size_t)c.row * P.exi[bc::kLdAct] + sd + c.lane));
    if constexpr (BC == kBcFiltered) keep = bcf_keep(P, c, ad, &bcs);
    else bcs = P.exf[bc::kBcScale];
    float qabs;
    lam = bc_lambda(bc_qabs_sum(P.ex[bc::kQv], P.B, c.lane), P.B, P.exf[bc::kAlpha], &qabs);
    if (c.row == 0 && c.lane == 0) {
      gst(P.ex[bc::kLam], lam);
      gst(P.ex[bc::kLam] + 1, qabs);
    }
  }
  // W1[:, sd+o], the action columns: rows of the transposed copy when the step keeps one (kW1T,
  // row length kLdW1T: coalesced, the same elements per lane), else strided column reads
  const float* w1t = P.ex[kW1T];
  if (RW > 1 && P.tile_begin) {     // wide head (wide_stage): the transposed W1 rows, then W4's, in LDS
    extern __shared__ float4 row_lds4[];
    const int n1 = ad * P.exi[kLdW1T] / 4;
    wide_stage<64 * RW>(row_lds4, reinterpret_cast<const float4*>(w1t), n1, reinterpret_cast<const float4*>(P.ex[kW4]),
               ad * ldw4 / 4);
    const float* hw1 = reinterpret_cast<const float*>(row_lds4);
    const float* hw4 = hw1 + (size_t)4 * n1;
    opaque8(gu0[0]); opaque8(h0[0]); opaque8(h3[0]); opaque8(g0); opaque8(g3);
    opaque1(mn0[0]); opaque1(rs0[0]); opaque1(mn3[0]); opaque1(rs3[0]);
    ln_bwd_rows<1>(gu0, h0, g0, mn0, rs0, K0, c.lane, NORM);       // dZ0 of Q1 (pads -> 0)
    const bool live = c.row < P.B;
    float gu3[1][8];
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) gu3[0][jj] = 0.f;
    for (int ob = 0; ob < ad; ob += kHeadRegs) {
      float pb[kHeadRegs];
#pragma unroll
      for (int o = 0; o < kHeadRegs; ++o) {
        float w[8];
        rv_load_lds(w, hw1 + (size_t)(ob + o < ad ? ob + o : 0) * P.exi[kLdW1T], K0, c.lane);
        pb[o] = rv_pdot(gu0[0], w, K0, c.lane);
      }
#pragma unroll
      for (int o = 0; o < kHeadRegs; ++o)
        if (ob + o < ad) {
          float ga = wsum(pb[o]);                                     // dL/da_o
          const float t = __shfl(tl, ob + o, 64);
          if constexpr (BC) ga = bc_grad(ga, lam, bcs, ma, t, __shfl(al, ob + o, 64), &se);
          const float gz4 = live ? (ga * ma) * (1.f - t * t) : 0.f;   // max_action*tanh bwd
          if (c.lane == 0) gst(P.ex[kDZ4] + ((size_t)c.row * 32 + ob + o), gz4);
          float w4r[8];
          rv_load_lds(w4r, hw4 + (size_t)(ob + o) * ldw4, ldw4, c.lane);
#pragma unroll
          for (int jj = 0; jj < 8; ++jj) gu3[0][jj] += gz4 * w4r[jj];
        }
    }
    if constexpr (BC)
      if (c.lane == 0) gst(P.ex[bc::kRowSe] + c.row, live && keep ? se : 0.f);
    rv_store(P.ex[kDU3] + (size_t)c.row * ld3, ld3, c.lane, gu3[0]);
    ln_bwd_rows<1>(gu3, h3, g3, mn3, rs3, K3, c.lane, NORM);        // dZ3 of the actor
    rv_store(P.Aout + (size_t)c.row * P.ldao, P.ldao, c.lane, gu3[0]);
    return;
  }
  if (w1t) {
#pragma unroll
    for (int o = 0; o < kHeadRegs; ++o) rv_load(w1[o], w1t + (size_t)(o < ad ? o : 0) * P.exi[kLdW1T], K0, c.lane);
  } else {
    head_cols(P.ex[kW1], ldw1, sd, ad, c.lane, w1);
  }
#pragma unroll
  for (int o = 0; o < kHeadRegs; ++o) {
    const int oo = o < ad ? o : 0;
    rv_load(w4[o], P.ex[kW4] + (size_t)oo * ldw4, ldw4, c.lane);
  }
  ln_bwd_rows<1>(gu0, h0, g0, mn0, rs0, K0, c.lane, NORM);       // dZ0 of Q1 (pads -> 0)
  const bool live = c.row < P.B;
  float gu3[1][8];
#pragma unroll
  for (int jj = 0; jj < 8; ++jj) gu3[0][jj] = 0.f;
  float part[kHeadRegs];
#pragma unroll
  for (int o = 0; o < kHeadRegs; ++o) part[o] = rv_pdot(gu0[0], w1[o], K0, c.lane);
#pragma unroll
  for (int o = 0; o < kHeadRegs; ++o)
    if (o < ad) {
      float ga = wsum(part[o]);                                       // dL/da_o
      const float t = __shfl(tl, o, 64);
      if constexpr (BC) ga = bc_grad(ga, lam, bcs, ma, t, __shfl(al, o, 64), &se);
      const float gz4 = live ? (ga * ma) * (1.f - t * t) : 0.f;       // max_action*tanh bwd
      if (c.lane == 0) gst(P.ex[kDZ4] + ((size_t)c.row * 32 + o), gz4);
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) gu3[0][jj] += gz4 * w4[o][jj];
    }
  // wide action spaces (Humanoid: 17): further blocks of kHeadRegs outputs, each block's W1
  // columns and W4 rows requested in one batch (one load round trip per block, not per output)
  for (int ob = kHeadRegs; ob < ad; ob += kHeadRegs) {
    float w1b[kHeadRegs][8], w4b[kHeadRegs][8];
    if (w1t) {
#pragma unroll
      for (int o = 0; o < kHeadRegs; ++o)
        rv_load(w1b[o], w1t + (size_t)(ob + o < ad ? ob + o : 0) * P.exi[kLdW1T], K0, c.lane);
    } else {
      head_cols(P.ex[kW1], ldw1, sd + ob, ad - ob, c.lane, w1b);
    }
#pragma unroll
    for (int o = 0; o < kHeadRegs; ++o) {
      const int oo = ob + o < ad ? ob + o : 0;
      rv_load(w4b[o], P.ex[kW4] + (size_t)oo * ldw4, ldw4, c.lane);
    }
    float pb[kHeadRegs];
#pragma unroll
    for (int o = 0; o < kHeadRegs; ++o) pb[o] = rv_pdot(gu0[0], w1b[o], K0, c.lane);
#pragma unroll
    for (int o = 0; o < kHeadRegs; ++o)
      if (ob + o < ad) {
        float ga = wsum(pb[o]);
        const float t = __shfl(tl, ob + o, 64);
        if constexpr (BC) ga = bc_grad(ga, lam, bcs, ma, t, __shfl(al, ob + o, 64), &se);
        const float gz4 = live ? (ga * ma) * (1.f - t * t) : 0.f;
        if (c.lane == 0) gst(P.ex[kDZ4] + ((size_t)c.row * 32 + ob + o), gz4);
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) gu3[0][jj] += gz4 * w4b[o][jj];
      }
  }
  if constexpr (BC)
    if (c.lane == 0) gst(P.ex[bc::kRowSe] + c.row, live && keep ? se : 0.f);
  rv_store(P.ex[kDU3] + (size_t)c.row * ld3, ld3, c.lane, gu3[0]);
  ln_bwd_rows<1>(gu3, h3, g3, mn3, rs3, K3, c.lane, NORM);        // dZ3 of the actor
  rv_store(P.Aout + (size_t)c.row * P.ldao, P.ldao, c.lane, gu3[0]);
}

}  // namespace td3
