// Part of kernels.hip: the weight-gradient stage with one tile per workgroup: lnbwd_rows_kernel, the Adam /
// Polyak state helpers (AdamState, apply_grads), dw_kernel, dw64_kernel and dw64g_kernel.
// Needs dev.h (AdamK, adam_elem, the LN backward rows) and kernels.h (DwArgs, LnBwdTable); row_actor.h for
// kRowWaves; xcd_tile of kernels_gemm.h; kernels_timeline.h for the marks.
#pragma once
#include "dev.h"
#include "kernels.h"
#include "row_actor.h"
#include "kernels_timeline.h"
#include "kernels_gemm.h"

namespace td3 {

// templated on NORM and with the problems in the kernel arguments: a runtime `norm` select on
// the statistics loads compiled to a branch and a load drain per row (5 dependent load rounds)
#ifndef TD3_LNBWD_RB
#define TD3_LNBWD_RB 1
#endif
constexpr int kLnBwdRB = TD3_LNBWD_RB;   // rows per wave: 1 (4: 4.0 us per launch, 2: 3.4, 1: 3.2)
template <bool NORM>
__global__ __launch_bounds__(64 * kRowWaves) void lnbwd_rows_kernel(int Bp, LnBwdTable tab) {   // Bp first: preloaded
  constexpr int RB = kLnBwdRB;
  const LnBwdProb& P = tab.p[blockIdx.y];
  const int lane = threadIdx.x & 63;
  // grid.x = Bp / (kRowWaves RB) exactly (Bp is a multiple of 32): no bounds check, which would put a
  // kernel-argument round trip ahead of the table's
  const int row0 = (blockIdx.x * kRowWaves + (threadIdx.x >> 6)) * RB;
  float gu[RB][8], h[RB][8], g[8], mean[RB], rstd[RB];
  float4 qg[2], qu[RB][2], qh[RB][2];
  if constexpr (NORM) rv_load_raw(qg, P.lng, P.ld, lane);
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    rv_load_raw(qu[r], P.GU + (size_t)(row0 + r) * P.ld, P.ld, lane);
    rv_load_raw(qh[r], P.H + (size_t)(row0 + r) * P.ld, P.ld, lane);
    mean[r] = NORM ? gld(P.stats + (row0 + r)) : 0.f;
    rstd[r] = NORM ? gld(P.stats + (Bp + row0 + r)) : 1.f;
  }
  __builtin_amdgcn_sched_barrier(0);     // every load requested before the first use
  if constexpr (NORM) rv_from_raw(g, qg, P.ld, lane);
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    rv_from_raw(gu[r], qu[r], P.ld, lane);
    rv_from_raw(h[r], qh[r], P.ld, lane);
  }
  if constexpr (NORM) ln_bwd_rows_pk<RB>(gu, h, g, mean, rstd, 1.0f / (float)P.K);
  else ln_bwd_rows<RB>(gu, h, g, mean, rstd, P.K, lane, 0);
#pragma unroll
  for (int r = 0; r < RB; ++r) rv_store(P.GZ + (size_t)(row0 + r) * P.ld, P.ld, lane, gu[r]);
}

// ================================================================== Adam / Polyak (AdamK, adam_elem: dev.h)
// N optimizer updates at once: every P/M/V(/T) load is issued before the first store, so the
// element chain costs one memory round trip instead of N (the stores of one element could alias
// the next element's loads for the compiler).
// The optimizer state of N elements (P, M, V and, with Polyak, T), requested without waiting.
template <int N>
struct AdamState {
  float mm[N], vv[N], pp[N], tt[N];
};
template <int N>
__device__ __forceinline__ void adam_state_load(const DwArgs& a, const int64_t (&idx)[N], const bool (&ok)[N],
                                                AdamState<N>& st) {
  if (a.mode == kDwGrad) return;
  const bool pol = a.mode == kDwAdamPolyak;
  int64_t any = -1;                                 // a valid index for the masked lanes' loads
#pragma unroll
  for (int e = N - 1; e >= 0; --e)
    if (ok[e]) any = idx[e];
  if (any < 0) return;
#pragma unroll
  for (int e = 0; e < N; ++e) {
    const int64_t j = ok[e] ? idx[e] : any;
    st.mm[e] = gld(a.adam.M + j);
    st.vv[e] = gld(a.adam.V + j);
    st.pp[e] = gld(a.adam.P + j);
    st.tt[e] = pol ? gld(a.adam.T + j) : 0.f;
  }
}

// qidx (nullable): the elements' k-quad image indices (AdamArgs::P4 / T4), for weight matrices
template <int N>
__device__ __forceinline__ void apply_grads_loaded(const DwArgs& a, const AdamK& k, const int64_t (&idx)[N],
                                                   const float (&g)[N], const bool (&ok)[N], AdamState<N>& st,
                                                   const int64_t* qidx = nullptr) {
  if (a.mode == kDwGrad) {
#pragma unroll
    for (int e = 0; e < N; ++e)
      if (ok[e]) gst(a.adam.G + idx[e], g[e]);
    return;
  }
  const bool pol = a.mode == kDwAdamPolyak;
  float (&mm)[N] = st.mm;
  float (&vv)[N] = st.vv;
  float (&pp)[N] = st.pp;
  float (&tt)[N] = st.tt;
#pragma unroll
  for (int e = 0; e < N; ++e) {                    // torch _single_tensor_adam, as adam_elem
    mm[e] = __fmaf_rn(k.w1, g[e] - mm[e], mm[e]);
    vv[e] = vv[e] * k.b2;
    vv[e] = vv[e] + (k.c2 * g[e]) * g[e];
    const float denom = sqrtf(vv[e]) / k.bc2s + k.eps;
    pp[e] = pp[e] + (k.negss * mm[e]) / denom;
    tt[e] = k.tau * pp[e] + k.omt * tt[e];
  }
#pragma unroll
  for (int e = 0; e < N; ++e) {
    if (!ok[e]) continue;
    sst(a.adam.M + idx[e], mm[e]);
    sst(a.adam.V + idx[e], vv[e]);
    pst(a.adam.P + idx[e], pp[e]);
    if (pol) pst(a.adam.T + idx[e], tt[e]);
    if (qidx && a.adam.P4) {
      pst(a.adam.P4 + qidx[e], pp[e]);
      if (pol) pst(a.adam.T4 + qidx[e], tt[e]);
    }
  }
}

template <int N>
__device__ __forceinline__ void apply_grads(const DwArgs& a, const AdamK& k, const int64_t (&idx)[N],
                                            const float (&g)[N], const bool (&ok)[N], const int64_t* qidx = nullptr) {
  AdamState<N> st;
  adam_state_load<N>(a, idx, ok, st);
  apply_grads_loaded<N>(a, k, idx, g, ok, st, qidx);
}

// The dZ rows' scale (unit-gradient rows: g_r; otherwise 1.0 from ldrs = 0) is requested with the
// chunk, as 4 float4 (rows rb .. rb+15 of the dense scale array), so its wait is the chunk's own.
template <bool SC>
__device__ __forceinline__ void dw_load_chunk(const DwProb& P, int rc, int h, int n0, int k0, int i,
                                              float (&av)[16], float (&bv)[16], float4 (&sc)[4]) {
  const int rb = rc * 32 + 16 * h;
  const float* gp = P.G + (size_t)rb * P.ldg + n0 + i;
  const float* up = P.U + (size_t)rb * P.ldu + k0 + i;
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    av[s] = gld(gp + (size_t)s * P.ldg);
    bv[s] = gld(up + (size_t)s * P.ldu);
  }
  if constexpr (SC) {
#pragma unroll
    for (int q = 0; q < 4; ++q) sc[q] = gld4(P.rs + (size_t)(rb + 4 * q) * P.ldrs);
  }
}
template <bool SC>
__device__ __forceinline__ void dw_scale(float (&av)[16], const float4 (&sc)[4]) {
  if constexpr (!SC) return;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    av[4 * q + 0] *= sc[q].x; av[4 * q + 1] *= sc[q].y; av[4 * q + 2] *= sc[q].z; av[4 * q + 3] *= sc[q].w;
  }
}

// dw64_kernel's vector tile (Bp >= 512): one column per thread, NT/32 row groups of 8-row strides
// (the float4 form below measured slower there: Humanoid C_dw 52 -> 61 us).
template <int NT, bool SC>
__device__ __forceinline__ void dw_vector_tile_cols(const DwArgs& a, const DwProb& P, const AdamK& k, int j,
                                               float* red) {
  constexpr int NG = NT / 32;
  const int n0 = j * 32;
  const int c = threadIdx.x & 31, rg = threadIdx.x >> 5;
  const bool ln = P.offg >= 0;
  const bool hasb = P.offb >= 0;                    // false: a LayerNorm-only problem (lnorm1)
  float sb = 0.f, sg = 0.f, sbeta = 0.f;
  for (int r0 = rg; r0 < a.Bp; r0 += 8 * NG) {
    float gz[8], gu[8], hh[8], mu[8], rs[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int r = min(r0 + NG * u, a.Bp - 1);     // clamped: loads stay unconditional
      const float sc = SC ? gld(P.rs + (size_t)r * P.ldrs) : 1.f;   // dZ / dU row scale (unit rows)
      gz[u] = hasb ? gld(P.G + ((size_t)r * P.ldg + n0 + c)) * sc : 0.f;
      if (ln) {
        gu[u] = gld(P.GU + ((size_t)r * P.ldgu + n0 + c)) * sc;
        hh[u] = gld(P.H + ((size_t)r * P.ldh + n0 + c));
        mu[u] = gld(P.stats + r);
        rs[u] = gld(P.stats + (a.Bp + r));
      }
      if (r0 + NG * u >= a.Bp) {
        gz[u] = 0.f;
        gu[u] = 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      sb += gz[u];
      if (ln) {
        sg += gu[u] * ((hh[u] - mu[u]) * rs[u]);
        sbeta += gu[u];
      }
    }
  }
  red[(0 * NG + rg) * 32 + c] = sb;
  red[(1 * NG + rg) * 32 + c] = sg;
  red[(2 * NG + rg) * 32 + c] = sbeta;
  __syncthreads();
  if (threadIdx.x < 32) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      s0 += red[(0 * NG + g) * 32 + c];
      s1 += red[(1 * NG + g) * 32 + c];
      s2 += red[(2 * NG + g) * 32 + c];
    }
    const int64_t idx[3] = {P.offb + n0 + c, P.offg + n0 + c, P.offbeta + n0 + c};
    const float gq[3] = {s0, s1, s2};
    const bool ok[3] = {hasb, ln, ln};
    apply_grads<3>(a, k, idx, gq, ok);
  }
}

// Vector tile j of a problem: db = sum dZ, dgamma = sum dU*xhat, dbeta = sum dU over 32 columns,
// then the optimizer update of those 32 columns.  A thread owns 4 adjacent columns (float4 loads)
// of every (NT/8)-th row: at Bp = 256 all of a thread's rows are requested in one batch, and the
// optimizer state of the 32 x 3 elements is requested behind them.
template <int NT, bool SC, int U = 8>               // U: rows per group and batch
__device__ __forceinline__ void dw_vector_tile(const DwArgs& a, const DwProb& P, const AdamPw& pw, int j,
                                               float* red) {
  constexpr int RG = NT / 8;                        // row groups
  const int n0 = j * 32;
  const int c4 = (threadIdx.x & 7) * 4, rg = threadIdx.x >> 3;
  const bool ln = P.offg >= 0;
  const bool hasb = P.offb >= 0;                    // false: a LayerNorm-only problem (lnorm1)
  const int c = threadIdx.x & 31;
  const int64_t idx[3] = {P.offb + n0 + c, P.offg + n0 + c, P.offbeta + n0 + c};
  const bool ok[3] = {hasb, ln, ln};
  AdamState<3> st;
  float sb[4] = {0.f, 0.f, 0.f, 0.f}, sg[4] = {0.f, 0.f, 0.f, 0.f}, sbeta[4] = {0.f, 0.f, 0.f, 0.f};
  // every operand read unconditionally from a valid address (the bias-less / LN-less operands
  // alias a present one) and masked at use: `hasb ?` / `if (ln)` on the loads compiled to
  // branches whose joins drained the loads in flight
  const float* gzp = hasb ? P.G : P.GU;
  const float* gup = ln ? P.GU : P.G;
  const float* hp = ln ? P.H : P.G;
  const float* stp = ln ? P.stats : P.G;
  const int ldz = hasb ? P.ldg : P.ldgu, ldu = ln ? P.ldgu : P.ldg, ldh = ln ? P.ldh : P.ldg;
  for (int r0 = rg; r0 < a.Bp; r0 += RG * U) {
    float4 gz[U], gu[U], hh[U];
    float mu[U], rs[U], sc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int r = min(r0 + RG * u, a.Bp - 1);     // clamped: loads stay unconditional
      gz[u] = gld4(gzp + ((size_t)r * ldz + n0 + c4));
      gu[u] = gld4(gup + ((size_t)r * ldu + n0 + c4));
      hh[u] = gld4(hp + ((size_t)r * ldh + n0 + c4));
      mu[u] = gld(stp + r);
      rs[u] = gld(stp + (a.Bp + r));
      sc[u] = SC ? gld(P.rs + (size_t)r * P.ldrs) : 1.f;   // dZ / dU row scale (unit rows)
    }
    if (r0 == rg && threadIdx.x < 32) adam_state_load<3>(a, idx, ok, st);
    __builtin_amdgcn_sched_barrier(0);
    if (!hasb) {
#pragma unroll
      for (int u = 0; u < U; ++u) gz[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (r0 + RG * u >= a.Bp) continue;
      const float z[4] = {gz[u].x * sc[u], gz[u].y * sc[u], gz[u].z * sc[u], gz[u].w * sc[u]};
      sb[0] += z[0]; sb[1] += z[1]; sb[2] += z[2]; sb[3] += z[3];
      if (ln) {
        const float g4[4] = {gu[u].x * sc[u], gu[u].y * sc[u], gu[u].z * sc[u], gu[u].w * sc[u]};
        const float h4[4] = {hh[u].x, hh[u].y, hh[u].z, hh[u].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          sg[e] += g4[e] * ((h4[e] - mu[u]) * rs[u]);
          sbeta[e] += g4[e];
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    red[(0 * RG + rg) * 33 + c4 + e] = sb[e];
    red[(1 * RG + rg) * 33 + c4 + e] = sg[e];
    red[(2 * RG + rg) * 33 + c4 + e] = sbeta[e];
  }
  __syncthreads();
  TL_MARK(1);
  TL_MARK(2);
  if (threadIdx.x < 32) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll 8
    for (int g = 0; g < RG; ++g) {
      s0 += red[(0 * RG + g) * 33 + c];
      s1 += red[(1 * RG + g) * 33 + c];
      s2 += red[(2 * RG + g) * 33 + c];
    }
    const float gq[3] = {s0, s1, s2};
    apply_grads_loaded<3>(a, make_adam(a.adam, pw), idx, gq, ok, st);
  }
  TL_MARK(3);
}

// Matrix tiles: dW[n][k] = sum_r dZ[r][n] * U[r][k] (32x32 per workgroup, rows split over the
// 4 waves, operands of the next row chunk in flight while the current one is multiplied).
// Vector tiles: db = sum dZ, dgamma = sum dU*xhat, dbeta = sum dU over 32 columns.
// Both end in the fused optimizer update of the elements they own.
#ifndef TD3_DW_OCC
#define TD3_DW_OCC 3
#endif
// SC: the launch scales dZ / dU rows (DwProb::rs; the unit-gradient critic backward)
template <bool SC>
__global__ __launch_bounds__(256, TD3_DW_OCC) void dw_kernel(DwArgs a, int nb) {
  __shared__ float red[4 * 32 * 33];
  const int b = xcd_tile(nb);
  TL_MARK(0);
  if (b >= nb) return;
  int pi = 0;
#pragma unroll
  for (int i = 1; i < kMaxDwProbs; ++i)
    if (i < a.nprob && b >= a.probs[i].tile_begin) pi = i;
  const DwProb& P = a.probs[pi];
  const int t = b - P.tile_begin;
  const int nmat = (P.Np >> 5) * P.ntk;
  const AdamPw pw = adam_pw(a.adam);            // requested now, used after the MFMA loop
  if (t < nmat) {
    const int kt = t % P.ntk, nt = t / P.ntk;
    const int n0 = nt * 32, k0 = kt * 32;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = lane & 31, h = lane >> 5;
    const int nrc = a.Bp >> 5;
    const int cb = wave * nrc / 4, ce = (wave + 1) * nrc / 4;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float a0[16], b0[16], a1[16], b1[16];
    float4 c0[4], c1[4];
    if (cb < ce) dw_load_chunk<SC>(P, cb, h, n0, k0, i, a0, b0, c0);
    if (cb + 1 < ce) dw_load_chunk<SC>(P, cb + 1, h, n0, k0, i, a1, b1, c1);
    // the optimizer state of this thread's 4 elements (row tn, columns tq..tq+3 of the tile: one
    // float4 per array, a quarter of the memory instructions of 4 scalar elements), requested
    // behind the first two operand chunks (their MFMA waits do not include it) and landing during
    // the MFMA chain.  T is read from a valid address whatever the mode (a `pol ?` select on it
    // compiled to a branch whose join drained the loads in flight).
    const int tn = threadIdx.x >> 3, tq = (threadIdx.x & 7) * 4;
    const int64_t ix = P.offW + (int64_t)(n0 + tn) * P.Kp + k0 + tq;
    const bool grad_only = a.mode == kDwGrad, pol = a.mode == kDwAdamPolyak;
    float4 sm4 = make_float4(0.f, 0.f, 0.f, 0.f), sv4 = sm4, sp4 = sm4, st4 = sm4;
    if (!grad_only) {
      sm4 = gld4(a.adam.M + ix);
      sv4 = gld4(a.adam.V + ix);
      sp4 = gld4(a.adam.P + ix);
      st4 = gld4((pol ? a.adam.T : a.adam.P) + ix);
    }
    for (int rc = cb; rc < ce; rc += 2) {
      dw_scale<SC>(a0, c0);
#pragma unroll
      for (int s = 0; s < 16; ++s) acc = mfma32x32x2(a0[s], b0[s], acc);
      if (rc + 2 < ce) dw_load_chunk<SC>(P, rc + 2, h, n0, k0, i, a0, b0, c0);
      if (rc + 1 >= ce) break;
      dw_scale<SC>(a1, c1);
#pragma unroll
      for (int s = 0; s < 16; ++s) acc = mfma32x32x2(a1[s], b1[s], acc);
      if (rc + 3 < ce) dw_load_chunk<SC>(P, rc + 3, h, n0, k0, i, a1, b1, c1);
    }
    TL_MARK(5);
#pragma unroll
    for (int r = 0; r < 16; ++r) red[(wave * 32 + mfma_row(r, lane)) * 33 + i] = acc[r];
    __syncthreads();
    TL_MARK(1);
    TL_MARK(2);
    const AdamK k = make_adam(a.adam, pw);
    float gq[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float g = red[tn * 33 + tq + q];
#pragma unroll
      for (int w = 1; w < 4; ++w) g = g + red[(w * 32 + tn) * 33 + tq + q];
      gq[q] = k0 + tq + q < P.kvalid ? g : 0.f;     // zero gradient, zero moments: the pad stays 0
    }
    if (grad_only) {
      gst4(a.adam.G + ix, make_float4(gq[0], gq[1], gq[2], gq[3]));
    } else {
      float mm[4] = {sm4.x, sm4.y, sm4.z, sm4.w}, vv[4] = {sv4.x, sv4.y, sv4.z, sv4.w};
      float pp[4] = {sp4.x, sp4.y, sp4.z, sp4.w}, tt[4] = {st4.x, st4.y, st4.z, st4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {                // torch _single_tensor_adam, as adam_elem
        mm[e] = __fmaf_rn(k.w1, gq[e] - mm[e], mm[e]);
        vv[e] = vv[e] * k.b2;
        vv[e] = vv[e] + (k.c2 * gq[e]) * gq[e];
        const float denom = sqrtf(vv[e]) / k.bc2s + k.eps;
        pp[e] = pp[e] + (k.negss * mm[e]) / denom;
        tt[e] = k.tau * pp[e] + k.omt * tt[e];
      }
      sst4(a.adam.M + ix, make_float4(mm[0], mm[1], mm[2], mm[3]));
      sst4(a.adam.V + ix, make_float4(vv[0], vv[1], vv[2], vv[3]));
      pst4(a.adam.P + ix, make_float4(pp[0], pp[1], pp[2], pp[3]));
      if (pol) pst4(a.adam.T + ix, make_float4(tt[0], tt[1], tt[2], tt[3]));
      if (a.adam.P4) {        // the k-quad images: this thread's 4 elements are one 16-B piece
        const int64_t iq = P.offW + ((int64_t)((k0 + tq) >> 2) * P.Np + n0 + tn) * 4;
        pst4(a.adam.P4 + iq, make_float4(pp[0], pp[1], pp[2], pp[3]));
        if (pol) pst4(a.adam.T4 + iq, make_float4(tt[0], tt[1], tt[2], tt[3]));
      }
    }
    TL_MARK(3);
    return;
  }
  dw_vector_tile<256, SC>(a, P, pw, t - nmat, red);
}

// Large batches (Bp >= 512): 64x64 weight tiles per workgroup of 8 waves.  Each step stages 64
// rows of dZ[:, n0:n0+64] and U[:, k0:k0+64] in LDS (one float4 per thread and operand, the next
// 64 rows in flight in registers); wave w multiplies quadrant (w&3) over the 32-row half w>>2.
// Per 32x32 output this reads half the operand bytes of dw_kernel's register tiles, the bound
// at B >= 512.  The two row halves meet in LDS; the rh=0 waves apply the optimizer update.
constexpr int kDw64S = 66;                          // LDS row stride: rows 16 apart 32 banks apart
constexpr int kDw64Depth = 2;                       // 64-row steps in flight (1, 3, 5: no change)
#ifndef TD3_DW64_VEC4
#define TD3_DW64_VEC4 1
#endif
template <bool SC>
__global__ __launch_bounds__(512) void dw64_kernel(DwArgs a, int nb) {
  __shared__ float sm[2 * 2 * 64 * kDw64S];         // [buf][operand][64 rows][kDw64S]
  __shared__ float4 ssl4[2][16];                     // SC: [buf] the 64 rows' dZ scales
  const int b = xcd_tile(nb);
  TL_MARK(0);
  if (b >= nb) return;
  int pi = 0;
#pragma unroll
  for (int i = 1; i < kMaxDwProbs; ++i)
    if (i < a.nprob && b >= a.probs[i].tile_begin) pi = i;
  const DwProb& P = a.probs[pi];
  const int t = b - P.tile_begin;
  const int ntn = (P.Np + 63) >> 6;
  const int nmat = ntn * P.ntk;                      // ntk = k tiles of 64 in this mode
  const AdamPw pw = adam_pw(a.adam);
  if (t >= nmat) {
#if TD3_DW64_VEC4
    dw_vector_tile<512, SC, 4>(a, P, pw, t - nmat, sm);   // 4-row batches: <= 128 VGPRs
#else
    dw_vector_tile_cols<512, SC>(a, P, make_adam(a.adam, pw), t - nmat, sm);
#endif
#ifdef TD3_TL
    if (threadIdx.x == 0 && blockIdx.x < 8192) td3_tl[blockIdx.x][6] = 1;   // vector tile (tl_probe)
#endif
    TL_MARK(3);
    return;
  }
  const int kt = t % P.ntk, nt = t / P.ntk;
  const int n0 = nt * 64, k0 = kt * 64;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 31, h = lane >> 5;
  const int qn = (wave >> 1) & 1, qk = wave & 1, rh = wave >> 2;
  // staging: float4 e = tid and tid + 512 of each operand's 64x64 block: row e>>4, cols 4(e&15);
  // kDw64Depth steps of 64 rows are in flight in registers (HBM latency > one step's 16 MFMAs)
  constexpr int D = kDw64Depth;
  float4 sg[D][2], su[D][2];
  float ssc[D];
  // SC: the step's 64 row scales ride along with the operands (thread t loads row t & 63's, the
  // first wave puts them in LDS) and scale the dZ operand at the MFMA (16 per lane half and step)
  auto fetch = [&](int r0, float4 (&g)[2], float4 (&u)[2], float& sc) {
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int e = tid + 512 * v, row = r0 + (e >> 4), c4 = (e & 15) * 4;
      const bool live = row < a.Bp;
      g[v] = (live && n0 + c4 < P.Np) ? gld4(P.G + (size_t)row * P.ldg + n0 + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
      u[v] = (live && k0 + c4 < P.Kp) ? gld4(P.U + (size_t)row * P.ldu + k0 + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if constexpr (SC) sc = gld(P.rs + (size_t)min(r0 + (tid & 63), a.Bp - 1) * P.ldrs);
  };
  auto put = [&](int buf, const float4 (&gq)[2], const float4 (&uq)[2], float sc) {
    float* g = sm + buf * 2 * 64 * kDw64S;
    float* uu = g + 64 * kDw64S;
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int e = tid + 512 * v, row = e >> 4, c4 = (e & 15) * 4;
      float* gp = g + row * kDw64S + c4;
      float* up = uu + row * kDw64S + c4;
      gp[0] = gq[v].x; gp[1] = gq[v].y; gp[2] = gq[v].z; gp[3] = gq[v].w;
      up[0] = uq[v].x; up[1] = uq[v].y; up[2] = uq[v].z; up[3] = uq[v].w;
    }
    if constexpr (SC) {
      if (tid < 64) reinterpret_cast<float*>(ssl4[buf])[tid] = sc;
    }
  };
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const int nstep = (a.Bp + 63) >> 6;
#pragma unroll
  for (int d = 0; d < D; ++d)
    if (d < nstep) fetch(d * 64, sg[d], su[d], ssc[d]);
  for (int st0 = 0; st0 < nstep; st0 += D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int st = st0 + d;
      if (st >= nstep) break;
      const int buf = st & 1;
      put(buf, sg[d], su[d], ssc[d]);
      __syncthreads();
      if (st + D < nstep) fetch((st + D) * 64, sg[d], su[d], ssc[d]);
      const float* g = sm + buf * 2 * 64 * kDw64S + (rh * 32 + 16 * h) * kDw64S;
      const float* uu = g + 64 * kDw64S;
      float scl[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 v4 = SC ? ssl4[buf][(rh * 32 + 16 * h) / 4 + q] : make_float4(1.f, 1.f, 1.f, 1.f);
        scl[4 * q + 0] = v4.x; scl[4 * q + 1] = v4.y; scl[4 * q + 2] = v4.z; scl[4 * q + 3] = v4.w;
      }
#pragma unroll
      for (int s2 = 0; s2 < 16; ++s2) {
        const float ga = g[s2 * kDw64S + qn * 32 + i];
        acc = mfma32x32x2(SC ? ga * scl[s2] : ga, uu[s2 * kDw64S + qk * 32 + i], acc);
      }
    }
  }
  __syncthreads();                                   // staging buffers become the reduction tile
  TL_MARK(1);
  float* red = sm + (wave & 3) * 32 * 33;
  if (rh == 1) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[mfma_row(r, lane) * 33 + i] = acc[r];
  }
  __syncthreads();
  // (the optimizer state is requested here, not behind the first operand steps: there its 64
  // loads per lane sat in front of the later steps' operand loads in the in-order vmcnt queue,
  // Humanoid C_dw 49 -> 60 us)
  if (rh == 0) {
    const int kk = k0 + qk * 32 + i;
    int64_t idx[16], qidx[16];
    float gq[16];
    bool ok[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = n0 + qn * 32 + mfma_row(r, lane);
      gq[r] = acc[r] + red[mfma_row(r, lane) * 33 + i];
      ok[r] = n < P.Np && kk < P.kvalid;           // kvalid <= Kp: columns past it keep their 0
      idx[r] = P.offW + (int64_t)n * P.Kp + kk;
      qidx[r] = P.offW + ((int64_t)(kk >> 2) * P.Np + n) * 4 + (kk & 3);
    }
    TL_MARK(2);
    apply_grads<16>(a, make_adam(a.adam, pw), idx, gq, ok, qidx);
    TL_MARK(3);
  }
}

// dw64_kernel with the operand steps staged by LDS-DMA (global_load_lds_dwordx4: no register
// round trip, no LDS-write pass) when Bp is a multiple of 64.  LDS image per buffer and operand:
// [64 rows][64 cols] unpadded, the two 32-column halves swapped on rows with bit 4 set (the DMA
// destination is lane-linear, so the swizzle is applied to the per-lane SOURCE column; an MFMA
// operand read takes rows 16 apart in its two lane halves, which then hit the other 32 banks).
// Columns past Np / Kp are read from a clamped valid column: they only feed outputs the
// epilogue masks.  One step is in flight while the previous one is multiplied.
typedef __attribute__((address_space(3))) void* td3_lptr;
// The DMA is issued by inline asm: through the builtin, hipcc cannot tell which LDS buffer a DMA
// writes and waits vmcnt(0) before the first operand read of every step (draining the next
// step's DMA); the waits are therefore placed by hand (vmcnt(0) before each step's barrier).
__device__ __forceinline__ void glds16(const float* src, float* lds_wave_base) {
  const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(td3_lptr)lds_wave_base);
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
}
__device__ __forceinline__ void glds4(const float* src, float* lds_wave_base) {
  const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(td3_lptr)lds_wave_base);
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
}
template <bool SC>
// (launch bounds: 2 workgroups per CU, <= 128 VGPRs)
__global__ __launch_bounds__(512, 4) void dw64g_kernel(DwArgs a, int nb) {
  // ONE __shared__ object (a second one made hipcc drain the DMA, vmcnt(0), before the first
  // operand read of every step): [buf][operand][64 rows][64 cols (swizzled)], then SC's
  // [buf][64] row scales
  __shared__ float sm[2 * 2 * 64 * 64 + 2 * 64];
  float* const ssl = sm + 2 * 2 * 64 * 64;
  const int b = xcd_tile(nb);
  TL_MARK(0);
  if (b >= nb) return;
  int pi = 0;
#pragma unroll
  for (int i = 1; i < kMaxDwProbs; ++i)
    if (i < a.nprob && b >= a.probs[i].tile_begin) pi = i;
  const DwProb& P = a.probs[pi];
  const int t = b - P.tile_begin;
  const int nmat = ((P.Np + 63) >> 6) * P.ntk;       // ntk = k tiles of 64 in this mode
  const AdamPw pw = adam_pw(a.adam);
  if (t >= nmat) {
    dw_vector_tile<512, SC, 4>(a, P, pw, t - nmat, sm);   // 4-row batches: <= 128 VGPRs
#ifdef TD3_TL
    if (threadIdx.x == 0 && blockIdx.x < 8192) td3_tl[blockIdx.x][6] = 1;   // vector tile (tl_probe)
#endif
    TL_MARK(3);
    return;
  }
  const int kt = t % P.ntk, nt = t / P.ntk;
  const int n0 = nt * 64, k0 = kt * 64;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 31, h = lane >> 5;
  const int qn = (wave >> 1) & 1, qk = wave & 1, rh = wave >> 2;
  // DMA lanes: wave w fills rows 8w .. 8w+7 of both operands (two 4-row wave-instructions each);
  // lane L -> row 8w + 4j + L/16, LDS columns 4(L&15) .. +3 <- source columns of the swizzle
  const int lr = lane >> 4, lc = (lane & 15) * 4;
  int gcol[2], ucol[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int row = 8 * wave + 4 * j + lr;
    const int c = lc ^ (((row >> 4) & 1) << 5);
    gcol[j] = min(n0 + c, P.Np - 4);
    ucol[j] = min(k0 + c, P.Kp - 4);
  }
  auto issue = [&](int st, int buf) {
    float* g = sm + buf * 2 * 4096;
    float* u = g + 4096;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int rl = 8 * wave + 4 * j;               // first LDS row of this wave-instruction
      const size_t row = (size_t)(st * 64 + rl + lr);
      glds16(P.G + row * P.ldg + gcol[j], g + rl * 64);
      glds16(P.U + row * P.ldu + ucol[j], u + rl * 64);
    }
    if constexpr (SC) {
      if (wave == 0)
        glds4(P.rs + (size_t)(st * 64 + lane) * P.ldrs, ssl + buf * 64);
    }
  };
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const int nstep = a.Bp >> 6;
  issue(0, 0);
  const int ca = (qn ^ h) * 32 + i, cb = (qk ^ h) * 32 + i;   // swizzled operand columns of this lane
  // a quadrant past Np / Kp (the 32-wide edge tiles of a padded 32-multiple) only feeds masked
  // outputs: its waves keep staging and synchronising but leave the MFMA pipe to a co-resident
  // workgroup
  const bool live = n0 + qn * 32 < P.Np && k0 + qk * 32 < P.Kp;
  for (int st = 0; st < nstep; ++st) {
    const int buf = st & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's DMA of step st has landed
    __syncthreads();                                 // everyone's has; every wave is done with buffer buf ^ 1
    if (st + 1 < nstep) issue(st + 1, buf ^ 1);
    if (!live) continue;
    const float* g = sm + buf * 2 * 4096 + (rh * 32 + 16 * h) * 64;
    const float* u = g + 4096;
    float scl[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 v4 = SC ? *reinterpret_cast<const float4*>(ssl + buf * 64 + rh * 32 + 16 * h + 4 * q)
                           : make_float4(1.f, 1.f, 1.f, 1.f);
      scl[4 * q + 0] = v4.x; scl[4 * q + 1] = v4.y; scl[4 * q + 2] = v4.z; scl[4 * q + 3] = v4.w;
    }
#pragma unroll
    for (int s2 = 0; s2 < 16; ++s2) {
      const float ga = g[s2 * 64 + ca];
      acc = mfma32x32x2(SC ? ga * scl[s2] : ga, u[s2 * 64 + cb], acc);
    }
  }
  __syncthreads();                                   // staging buffers become the reduction tile
  TL_MARK(1);
  float* red = sm + (wave & 3) * 32 * 33;
  if (rh == 1) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[mfma_row(r, lane) * 33 + i] = acc[r];
  }
  __syncthreads();
  if (rh == 0) {
    const int kk = k0 + qk * 32 + i;
    int64_t idx[16], qidx[16];
    float gq[16];
    bool ok[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = n0 + qn * 32 + mfma_row(r, lane);
      gq[r] = acc[r] + red[mfma_row(r, lane) * 33 + i];
      ok[r] = n < P.Np && kk < P.kvalid;           // kvalid <= Kp: columns past it keep their 0
      idx[r] = P.offW + (int64_t)n * P.Kp + kk;
      qidx[r] = P.offW + ((int64_t)(kk >> 2) * P.Np + n) * 4 + (kk & 3);
    }
    TL_MARK(2);
    apply_grads<16>(a, make_adam(a.adam, pw), idx, gq, ok, qidx);
    TL_MARK(3);
  }
}

}  // namespace td3
