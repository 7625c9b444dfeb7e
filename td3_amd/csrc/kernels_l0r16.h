// Part of kernels.hip: l0r16_kernel, the fused layer 0-1 stage on 16-row tiles.
// Needs the l0_* helpers and Ctx of kernels_prologues.h and xcd_tile and the chunk loads of kernels_gemm.h.
#pragma once
#include "dev.h"
#include "kernels.h"
#include "row_actor.h"
#include "kernels_prologues.h"
#include "kernels_gemm.h"

namespace td3 {

// ================================================================== 16-row fused layer 0-1
// The fused layer-0 stages (kProL0 / kProL0G: F_fwd01 with the step's sample, AF_fwd01) on 16-row
// tiles (VERDICT r04 #1a).  A 32-row workgroup spends most of its span on row-serial work before its
// first layer-1 MFMA (F_fwd01, profiles/r04_timeline_halfcheetah.txt: 8.4 of 14.9 us = records,
// layer 0 over 512 columns, LayerNorm 0); half the rows halve the layer-0 MFMAs and the LayerNorm
// rows per wave, and the 16 x 16*NCT output tile (v_mfma_f32_16x16x4_f32) halves the layer-1 chain
// of a 32 x 64 tile at NCT = 4.  Workgroup = NW = NCT * WK waves (8 .. 16), tile (16 rows, 16*NCT
// layer-1 columns) of one network; the problem directory, XCD-aware tile order and every output
// (H1, H0 / U0 slices, LN0 statistics, the sample's copies, reward / not_done, drawn rows) are
// gemm_body's kProL0 / kProL0G contract (kernels.h), so the planner swaps the launch only.
//  1. input rows: thread t (< 512) stages x[t / 32][t % 32] (kProL0G: the Philox row drawn per
//     thread, the record read unconditionally and masked at the LDS put), then W0 / b0 / LN0 affine
//     requests; kProL0G requests the layer-1 weights after the records landed (TD3_L0G_LATE_B),
//  2. layer 0: 16 x 16 tiles tau = wave + NW*q of Z0 = X W0^T on v_mfma_f32_16x16x4_f32, min(K0, 8)
//     MFMAs per tile (lane group g supplies k = 8g + s), + b0, ReLU into the A buffer,
//  3. LayerNorm 0 in place (rows w and w + NW of wave w),
//  4. layer 1: wave (c = w % NCT, kq = w / NCT): 16 x 16 columns 16c.., K range kq of WK, chunks of
//     32 (lane group g: k = kb + 8g + s, 2 ds_read_b128 per row chunk), partials summed through LDS.
constexpr int kR16XS = 36;      // LDS row stride of the staged 16 input rows
#ifndef TD3_L0R16_KS8
#define TD3_L0R16_KS8 1
#endif

template <int NCT, int WK, bool GATHER>
__global__ __launch_bounds__(64 * NCT * WK) void l0r16_kernel(int nb, int nprob, int tb1, int tb2, int tb3, int Bp,
                                                              GemmTable tab, Counters* bump, int bump_actor) {
  using namespace ring_l0;
  constexpr int NW = NCT * WK, NT = 64 * NW, OUTW = 16 * NCT;
  static_assert(NW >= 8 && NW <= 16 && NT % OUTW == 0, "l0r16: 8 .. 16 waves, whole output rows per pass");
  extern __shared__ float4 smem4[];
  float* smem = reinterpret_cast<float*>(smem4);
  const int b = xcd_tile(nb);
  TL_MARK(0);
  if (b >= nb) return;
  int pi = 0;
  if (nprob > 1 && b >= tb1) pi = 1;
  if (nprob > 2 && b >= tb2) pi = 2;
  if (nprob > 3 && b >= tb3) pi = 3;
  pi = __builtin_amdgcn_readfirstlane(pi);
  const GemmProb& P = tab.p[pi];
  if constexpr (GATHER)
    asm volatile("" ::"s"(P.A), "s"(P.lda), "s"(P.ex[kW0]), "s"(P.ex[kB0]), "s"(P.exi[kN0p]), "s"(P.exi[kK0]), "s"(P.W),
                 "s"(P.ldw), "s"(P.Kp), "s"(P.lng), "s"(P.lnb), "s"(P.bias), "s"(P.Nout), "s"(P.tile_begin),
                 "s"(P.norm), "s"(P.B), "s"(tab.rs.data), "s"(tab.rs.rec), "s"(tab.rs.d_size), "s"(tab.rs.seed),
                 "s"(tab.rs.ctr), "s"(P.exi[kRecOff]), "s"(P.exi[kRecOffRw]), "s"(P.wsk), "s"(P.w0sk));
  else
    asm volatile("" ::"s"(P.A), "s"(P.lda), "s"(P.ex[kW0]), "s"(P.ex[kB0]), "s"(P.exi[kN0p]), "s"(P.exi[kK0]), "s"(P.W),
                 "s"(P.ldw), "s"(P.Kp), "s"(P.lng), "s"(P.lnb), "s"(P.bias), "s"(P.Nout), "s"(P.tile_begin),
                 "s"(P.norm), "s"(P.B), "s"(P.wsk), "s"(P.w0sk));
  const int mtiles = Bp >> 4;
  const int t = b - P.tile_begin;
  const int mt = t % mtiles, nt = t / mtiles;
  const int m0 = mt * 16, n0 = nt * OUTW;
  const int Kp = P.Kp;                          // layer-1 K = layer-0 padded width (<= 512)
  const int S = lds_stride(Kp);
  float* abuf = smem;                           // [16][S]: H0, then U0 = LN0(H0): layer 1's A rows
  float* xs = abuf + 16 * S;                    // [16][kR16XS]: the input rows
  float* h0s = xs + 16 * kR16XS;                // [16][S]: H0 kept for its store when LN0 overwrites abuf
  float* red = h0s + 16 * S;                    // [NW][16][17]: layer-1 K-split partials
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int j16 = lane & 15, g = lane >> 4;
  const int K0 = P.exi[kK0], N0p = P.exi[kN0p];
  const bool t0 = nt == 0;
  // ---- 1. input rows (loads first: the record reads are the latency-critical ones)
  const int xrow = (threadIdx.x >> 5) & 15, xcol = threadIdx.x & 31;
  const bool xown = threadIdx.x < 512;
  const int grow_x = m0 + xrow;
  int64_t idx = 0;
  float xv, rw = 0.f;
  if constexpr (GATHER) {
    const uint64_t step = (uint64_t)(tab.rs.ctr->total_it + 1);
    const uint64_t n = (uint64_t)*tab.rs.d_size;
    idx = grow_x < P.B ? (int64_t)philox_index(tab.rs.seed, step, (uint32_t)grow_x, n) : -1;
    __builtin_amdgcn_sched_barrier(0);
    const float* rec = tab.rs.data + (size_t)(idx >= 0 ? idx : 0) * tab.rs.rec;
    xv = gld(rec + P.exi[kRecOff] + (xcol < K0 ? xcol : 0));
    rw = t0 ? gld(rec + P.exi[kRecOffRw] + (xcol & 1)) : 0.f;
  } else {
    xv = gld(P.A + (size_t)grow_x * P.lda + xcol);   // input rows are >= 32 wide (zero pads)
  }
  // layer-0 weights of this wave's tiles (B operand: W0[tau*16 + j16][8g + s], two float4 per tile:
  // element-wise loads at k = KS*g + s were 16 scattered lines per instruction and held the record
  // reads' landing ~3 us behind the 32-row kernel's) and biases.  MFMA s covers k = 8g + s, g = 0..3
  // (x and W0 pads past K0 are zero): MFMAs s >= K0 read only pads and are skipped
  const int n0t = N0p >> 4;                     // layer-0 column tiles of 16
  constexpr int kQ0 = (32 + NW - 1) / NW;       // tiles per wave (N0p <= 512)
  float w0[kQ0][8], b0v[kQ0];
#pragma unroll
  for (int q = 0; q < kQ0; ++q) {
    const int tau = min(wave + NW * q, n0t - 1);
    const float* wp = P.ex[kW0] + (size_t)(tau * 16 + j16) * w0_sn(P.w0sk) + (size_t)(2 * g) * w0_sk(P.w0sk);
    const float4 u = gld4(wp), v = gld4(wp + w0_sk(P.w0sk));
    w0[q][0] = u.x; w0[q][1] = u.y; w0[q][2] = u.z; w0[q][3] = u.w;
    w0[q][4] = v.x; w0[q][5] = v.y; w0[q][6] = v.z; w0[q][7] = v.w;
    b0v[q] = gld(P.ex[kB0] + tau * 16 + j16);
  }
  float lg[8], lb[8];
  if (P.norm) {
    rv_load(lg, P.lng, Kp, lane);
    rv_load(lb, P.lnb, Kp, lane);
  }
  // layer-1 weights: wave (c, kq) streams W1[n0 + 16c + j16][k] over its K range in 32-deep chunks
  const int c = wave % NCT, kq = wave / NCT;
  const int nch = Kp >> 5;
  const int cb = kq * nch / WK, ce = (kq + 1) * nch / WK;
  constexpr int kMaxCh = (16 + WK - 1) / WK;    // chunks of a wave at Kp = 512
  const int ncol = n0 + 16 * c + j16;
  const bool cact = n0 + 16 * c < P.Nout;
  const int wrow = cact ? ncol : 0;
  float bw[kMaxCh][8];
  auto load_w1 = [&]() {
#pragma unroll
    for (int q = 0; q < kMaxCh; ++q) {
      const int ch = min(cb + q, ce - 1);
      const int sk = w_sk(P.wsk);
      const float* wp = P.W + (size_t)wrow * P.ldw + (size_t)(ch * 8 + 2 * g) * sk;
      const float4 u = gld4(wp), v = gld4(wp + sk);
      bw[q][0] = u.x; bw[q][1] = u.y; bw[q][2] = u.z; bw[q][3] = u.w;
      bw[q][4] = v.x; bw[q][5] = v.y; bw[q][6] = v.z; bw[q][7] = v.w;
    }
  };
  constexpr bool kLateB = GATHER && TD3_L0G_LATE_B;
  if constexpr (!kLateB) load_w1();
  const int ocol = threadIdx.x % OUTW;          // the epilogue's column (NT % OUTW == 0)
  const float bias = P.bias && n0 + ocol < P.Nout ? gld(P.bias + n0 + ocol) : 0.f;
  TL_MARK(5);
  // put the input rows; n-tile 0 stores the sample's copies / reward / not_done / drawn rows
  if (xown) {
    const bool valid = xcol < K0;
    const float x = (!GATHER || (idx >= 0 && valid)) ? xv : 0.f;
    xs[xrow * kR16XS + xcol] = x;
    if constexpr (GATHER) {
      if (t0) {
        if (valid) {
          if (P.ex[kRowCopy]) gst(P.ex[kRowCopy] + (size_t)grow_x * P.exi[kLdRowCopy] + xcol, x);
          if (P.ex[kRowCopy2]) gst(P.ex[kRowCopy2] + (size_t)grow_x * P.exi[kLdRowCopy2] + xcol, x);
        }
        if (xcol < 2 && rw_ptr(P, xcol)) gst(rw_ptr(P, xcol) + grow_x, idx >= 0 ? rw : 0.f);
        if (pi == 0 && tab.rs.idx_out && xcol == 0 && grow_x < P.B) tab.rs.idx_out[grow_x] = idx;
      }
    }
  }
  lds_barrier();
  TL_MARK(6);
  // kProL0G: the layer-1 weights (160 KB per workgroup at 80 columns) are requested only now, behind
  // the staged rows: issued before the put, they shared the CU's ~70 GB/s L2 rate with the records
  // and W0 and the put landed ~2.7 us later (tools/tl_probe.py); they are not needed before the
  // LayerNorm, and the LDS-only barriers do not drain them
  if constexpr (kLateB) {
    load_w1();
    __builtin_amdgcn_sched_barrier(0);
  }
  // ---- 2. layer 0 on MFMA: A = the staged rows (lane (j16, g) supplies x[j16][8g + s])
  const bool keep = P.ex[kH0] && P.norm;
  {
    const float4 x0 = *reinterpret_cast<const float4*>(xs + j16 * kR16XS + 8 * g);
    const float4 x1 = *reinterpret_cast<const float4*>(xs + j16 * kR16XS + 8 * g + 4);
    const float av[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
    const int ks = min(K0, 8);                  // MFMA s reads k = 8g + s: all past K0 when s >= K0
    f32x4 acc0[kQ0];
#pragma unroll
    for (int q = 0; q < kQ0; ++q) acc0[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (TD3_L0R16_KS8 && ks == 8) {             // inputs of >= 8 features: no per-MFMA branches
#pragma unroll
      for (int q = 0; q < kQ0; ++q) {
        if (wave + NW * q >= n0t) continue;
#pragma unroll
        for (int s2 = 0; s2 < 8; ++s2)
          acc0[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s2], w0[q][s2], acc0[q], 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int q = 0; q < kQ0; ++q) {
        if (wave + NW * q >= n0t) continue;
#pragma unroll
        for (int s2 = 0; s2 < 8; ++s2)
          if (s2 < ks) acc0[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s2], w0[q][s2], acc0[q], 0, 0, 0);
      }
    }
#pragma unroll
    for (int q = 0; q < kQ0; ++q) {
      const int tau = wave + NW * q;
      if (tau >= n0t) continue;
      const int col = tau * 16 + j16;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const float h = fmaxf(acc0[q][v] + b0v[q], 0.f);
        abuf[(4 * g + v) * S + col] = h;
        if (keep) h0s[(4 * g + v) * S + col] = h;
      }
    }
  }
  // ---- 3. LayerNorm 0 in place (wave w: rows w and w + NW)
  if (P.norm) {
    lds_barrier();
    TL_MARK(7);
    const int r0 = wave, r1 = wave + NW < 16 ? wave + NW : wave;
    float x[2][8], mean[2], rstd[2], rm[8];
    rv_load_lds(x[0], abuf + r0 * S, Kp, lane);
    rv_load_lds(x[1], abuf + r1 * S, Kp, lane);
    real_mask(rm, P.Kreal, lane);
    ln_fwd_rows_pk<2>(x, lg, lb, rm, 1.0f / (float)P.Kreal, mean, rstd);
    lds_store8(abuf + r0 * S, Kp, lane, x[0]);
    if (wave + NW < 16) lds_store8(abuf + r1 * S, Kp, lane, x[1]);
    if (t0 && P.stats && lane == 0) {
      gst(P.stats + (m0 + r0), mean[0]);
      gst(P.stats + (Bp + m0 + r0), rstd[0]);
      if (wave + NW < 16) {
        gst(P.stats + (m0 + r1), mean[1]);
        gst(P.stats + (Bp + m0 + r1), rstd[1]);
      }
    }
  }
  lds_barrier();
  TL_MARK(1);
  TL_CLK_BEGIN();
  // ---- 4. layer 1: 16 x 16 output of column tile c over chunks [cb, ce)
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (cact) {
    const float* ar = abuf + j16 * S + 8 * g;
#pragma unroll
    for (int q = 0; q < kMaxCh; ++q) {
      if (cb + q < ce) {
        const int kb = (cb + q) * 32;
        const float4 u = *reinterpret_cast<const float4*>(ar + kb);
        const float4 v = *reinterpret_cast<const float4*>(ar + kb + 4);
        const float a8[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
#pragma unroll
        for (int s2 = 0; s2 < 8; ++s2) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a8[s2], bw[q][s2], acc, 0, 0, 0);
      }
    }
  }
  TL_CLK_END();
  // H0 / U0 rows of the tile, each n-tile workgroup its slice of the columns (after the MFMA loop:
  // in the prologue they queued ahead of the weight stream)
  {
    float* H0 = P.ex[kH0];
    float* U0 = P.norm ? P.Aout : nullptr;
    const float* hsrc = P.norm ? h0s : abuf;
    if (H0 || U0) {
      const int nq = Kp >> 2;
      const int q0 = nt * nq / P.ntiles, per = (nt + 1) * nq / P.ntiles - q0;
      for (int e = threadIdx.x; e < 16 * per; e += NT) {
        const int row = e / per, q4 = 4 * (q0 + e % per);
        const size_t grow = (size_t)(m0 + row);
        if (H0) gst4(H0 + grow * P.exi[kN0p] + q4, *reinterpret_cast<const float4*>(hsrc + row * S + q4));
        if (U0) gst4(U0 + grow * P.ldao + q4, *reinterpret_cast<const float4*>(abuf + row * S + q4));
      }
    }
  }
  // K-split partials through LDS (16 x 16 C map: column j16, rows 4g + v), bias, ReLU, store
#pragma unroll
  for (int v = 0; v < 4; ++v) red[(wave * 16 + 4 * g + v) * 17 + j16] = acc[v];
  lds_barrier();
  TL_MARK(2);
#pragma unroll
  for (int e0 = 0; e0 < 16 * OUTW; e0 += NT) {
    const int e = e0 + threadIdx.x;
    const int row = e / OUTW, cc = ocol >> 4, jj = ocol & 15;
    float v = red[((0 * NCT + cc) * 16 + row) * 17 + jj];
#pragma unroll
    for (int w = 1; w < WK; ++w) v = v + red[((w * NCT + cc) * 16 + row) * 17 + jj];
    if (P.bias) v = v + bias;
    if (P.relu) v = fmaxf(v, 0.f);
    if (n0 + ocol < P.Nout) gst(P.C + ((size_t)(m0 + row) * P.ldc + n0 + ocol), v);
  }
  TL_MARK(3);
  if (bump && blockIdx.x == 0 && threadIdx.x == 0) {
    if (bump_actor != kBumpActorOnly) {
      bump->total_it += 1;
      bump->critic_step += 1;
      bump->pw[0] *= bump->beta[0];
      bump->pw[1] *= bump->beta[1];
    }
    if (bump_actor) {
      bump->actor_step += 1;
      bump->pw[2] *= bump->beta[2];
      bump->pw[3] *= bump->beta[3];
    }
  }
}

}  // namespace td3
