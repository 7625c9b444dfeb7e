// Part of kernels.hip: the GEMM-stage prologues, which build a workgroup's A tile in LDS (lds_put_row, Ctx,
// pro_copy / pro_ln / pro_lnbwd / pro_headbwd / pro_gather) and the l0_* helpers of the fused first layer.
// Needs dev.h and kernels.h (the operand slots of each prologue); kernels_timeline.h for the marks.
#pragma once
#include "dev.h"
#include "kernels.h"
#include "kernels_timeline.h"

namespace td3 {

// A workgroup barrier for LDS hand-offs only: this wave's LDS accesses complete, then s_barrier.
// __syncthreads() is a workgroup-scope release + acquire, which on gfx950 waits vmcnt(0): every
// load the wave has in flight (the streamed weights) drains at each prologue barrier.  The asm's
// memory clobber keeps the compiler from moving LDS accesses across it; global memory needs no
// ordering at these barriers (no workgroup reads global data another of its waves stored).
// TD3_SYNC_BARRIERS=1 restores __syncthreads() (A/B builds).

__device__ __forceinline__ void lds_put_row(float* smem, int S, int row, int Kp, int lane, const float (&v)[8]) {
  lds_store8(smem + row * S, Kp, lane, v);
}

// ================================================================== prologues
// GEMM workgroups are kNW waves; each prologue writes rows wave*kRPW .. +kRPW-1 of the
// workgroup's A tile (LDS, [32][S]).
constexpr int kNW = kGemmWaves;
constexpr int kRPW = 32 / kNW;
struct Ctx {
  int m0, wave, lane, nt, Bp, S;
};

template <int RPW, int RB = RPW>
__device__ __forceinline__ void pro_copy(const GemmProb& P, float* smem, const Ctx& c) {
#pragma unroll
  for (int r0 = 0; r0 < RPW; r0 += RB) {
    float x[RB][8];
#pragma unroll
    for (int r = 0; r < RB; ++r)
      rv_load(x[r], P.A + (size_t)(c.m0 + c.wave * RPW + r0 + r) * P.lda, P.Kp, c.lane);
#pragma unroll
    for (int r = 0; r < RB; ++r) lds_put_row(smem, c.S, c.wave * RPW + r0 + r, P.Kp, c.lane, x[r]);
  }
}

struct NoOp {
  __device__ __forceinline__ void operator()() const {}
};

template <int RPW, class AfterIssue = NoOp>
__device__ __forceinline__ void pro_ln(const GemmProb& P, float* smem, const Ctx& c,
                                       const AfterIssue& after_issue = AfterIssue()) {
  constexpr int RB = RPW;
  float x[RB][8], g[8], bb[8], mean[RB], rstd[RB];
#pragma unroll
  for (int r = 0; r < RB; ++r)
    rv_load(x[r], P.A + (size_t)(c.m0 + c.wave * RPW + r) * P.lda, P.Kp, c.lane);
  rv_load(g, P.lng, P.Kp, c.lane);
  rv_load(bb, P.lnb, P.Kp, c.lane);
  after_issue();
  TL_FINE(6);
  float rm[8];
  real_mask(rm, P.Kreal, c.lane);
  ln_fwd_rows_pk<RB>(x, g, bb, rm, 1.0f / (float)P.Kreal, mean, rstd);
  TL_FINE(7);
  const bool t0 = c.nt == 0;
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    const int row = c.wave * RPW + r, grow = c.m0 + row;
    lds_put_row(smem, c.S, row, P.Kp, c.lane, x[r]);
    if (t0 && P.Aout) rv_store(P.Aout + (size_t)grow * P.ldao, P.Kp, c.lane, x[r]);
    if (t0 && P.stats && c.lane == 0) {
      gst(P.stats + (grow), mean[r]);
      gst(P.stats + (c.Bp + grow), rstd[r]);
    }
  }
}

template <int RPW>
__device__ __forceinline__ void pro_lnbwd(const GemmProb& P, float* smem, const Ctx& c) {
  constexpr int RB = 2;
  float g[8];
  rv_load(g, P.lng, P.Kp, c.lane);
  const bool t0 = c.nt == 0;
#pragma unroll
  for (int r0 = 0; r0 < RPW; r0 += RB) {
    float gu[RB][8], h[RB][8], mean[RB], rstd[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      const int grow = c.m0 + c.wave * RPW + r0 + r;
      rv_load(gu[r], P.A + (size_t)grow * P.lda, P.Kp, c.lane);
      rv_load(h[r], P.H + (size_t)grow * P.ldh, P.Kp, c.lane);
      mean[r] = P.norm ? gld(P.stats + (grow)) : 0.f;
      rstd[r] = P.norm ? gld(P.stats + (c.Bp + grow)) : 1.f;
    }
    if (P.norm) ln_bwd_rows_pk<RB>(gu, h, g, mean, rstd, 1.0f / (float)P.Kreal);
    else ln_bwd_rows<RB>(gu, h, g, mean, rstd, P.Kreal, c.lane, 0);
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      const int row = c.wave * RPW + r0 + r;
      lds_put_row(smem, c.S, row, P.Kp, c.lane, gu[r]);
      if (t0 && P.Aout) rv_store(P.Aout + (size_t)(c.m0 + row) * P.ldao, P.Kp, c.lane, gu[r]);
    }
  }
}

// The actor loss -mean Q1(s, pi(s)) (TD3_featured.py:159) backward into Q1's head as the prologue
// of the first input-grad stage (kProHeadBwd): dL/dQ_r = -1/B for every live row, so dU3 = -w4/B
// is the same row everywhere and each column-tile workgroup forms dZ3 of its 32 rows from H3
// alone: LN3 statistics, Q1 = w4 . LN3(H3) + b4 (stored by n-tile 0 for the loss value), then
// relu'(LN3_bwd(dU3)).  Row work is 3 wave reductions per row on top of pro_lnbwd's 2, so the
// repetition over column tiles costs less than the row launch it replaces.
template <int RPW>
__device__ __forceinline__ void pro_headbwd(const GemmProb& P, float* smem, const Ctx& c) {
  constexpr int RB = 2;
  float g[8], w[8], rm[8], bb[8];
  rv_load(w, P.ex[head_bwd_pro::kW4], P.Kp, c.lane);
  if (P.norm) {
    rv_load(g, P.lng, P.Kp, c.lane);
    rv_load(bb, P.lnb, P.Kp, c.lane);
  }
  const float b4 = gld(P.ex[head_bwd_pro::kB4]);
  real_mask(rm, P.Kreal, c.lane);
  const float invK = 1.0f / (float)P.Kreal;
  const bool t0 = c.nt == 0;
  float hall[RPW][8];          // all of the wave's rows in one load round
#pragma unroll
  for (int r = 0; r < RPW; ++r) rv_load(hall[r], P.A + (size_t)(c.m0 + c.wave * RPW + r) * P.lda, P.Kp, c.lane);
#pragma unroll
  for (int r0 = 0; r0 < RPW; r0 += RB) {
    float h[RB][8], gu[RB][8], mean[RB], rstd[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
      for (int j = 0; j < 8; ++j) h[r][j] = hall[r0 + r][j];
    if (P.norm) {   // LN3 statistics (ln_fwd_rows_pk's two passes; the normalised row is not needed)
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        const f32x2 a = (pk2(h[r], 0) + pk2(h[r], 1)) + (pk2(h[r], 2) + pk2(h[r], 3));
        mean[r] = wsum(a.x + a.y) * invK;
      }
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        const f32x2 nm = splat2(-mean[r]);
        f32x2 v = splat2(0.f);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x2 d = pkfma(nm, pk2(rm, q), pk2(h[r], q));
          v = pkfma(d, d, v);
        }
        rstd[r] = __builtin_amdgcn_rsqf(wsum(v.x + v.y) * invK + 1e-5f);
      }
    }
    if (t0) {       // Q1 = w4 . LN3(H3) + b4, for the loss value
      float x[RB][8];
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        const float nb = -mean[r] * rstd[r];
#pragma unroll
        for (int j = 0; j < 8; ++j)
          x[r][j] = P.norm ? __fmaf_rn(__fmaf_rn(h[r][j], rstd[r], nb), g[j], bb[j]) : h[r][j];
        const float q = wsum(rv_pdot(x[r], w, P.Kreal, c.lane)) + b4;
        if (c.lane == 0) gst(P.ex[head_bwd_pro::kQ] + (c.m0 + c.wave * RPW + r0 + r), q);
      }
    }
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      const float gq = c.m0 + c.wave * RPW + r0 + r < P.B ? P.exf[head_bwd_pro::kGradScale] : 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) gu[r][j] = gq * w[j];
    }
    if (P.norm) ln_bwd_rows_pk<RB>(gu, h, g, mean, rstd, invK);
    else ln_bwd_rows<RB>(gu, h, g, mean, rstd, P.Kreal, c.lane, 0);
#pragma unroll
    for (int r = 0; r < RB; ++r) lds_put_row(smem, c.S, c.wave * RPW + r0 + r, P.Kp, c.lane, gu[r]);
  }
}

// Replay-ring rows (kProGather): the step's sample (my_replay_buffer.py:119-128) drawn and read
// by the first layer itself.  Row indices: Philox(seed, total_it + 1, row) over [0, size), the
// same draw as gather_kernel; padded rows (>= B) are zero.  Record fields are not 16-B aligned,
// so the lane slices are dword loads.
__device__ __forceinline__ void rv_load_u(float (&v)[8], const float* __restrict__ p, int len, int lane) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int col = rcol(lane, j);
    v[j] = col < len ? gld(p + col) : 0.f;
  }
}

// A problem's first column tile also stores its rows for the later stages (no extra loads): the
// A row to Aout and ring_l0::kRowCopy2, reward / not_done to kReward / kNotDone; problem 0 records
// the drawn rows.

// reward (lane 0) / not_done (lane 1) destination of the sample: a select between the two
// scalar fields.  Indexed as P.ex[kReward + lane], the pointer was fetched by a VECTOR load of the
// kernel arguments whose vmcnt(0) drained every weight load in flight (the n-tile-0 workgroups
// of F_fwd01 ran ~3 us behind the rest).
__device__ __forceinline__ float* rw_ptr(const GemmProb& P, int lane) {
  using namespace ring_l0;
  float* r0 = P.ex[kReward];
  float* r1 = P.ex[kNotDone];
  asm volatile("" : "+s"(r0), "+s"(r1));   // pinned in SGPRs: the select below is a v_cndmask
  return lane == 0 ? r0 : r1;
}
template <int RPW>
__device__ __forceinline__ void pro_gather(const GemmProb& P, const RingSide& rs, float* smem, const Ctx& c,
                                           int pi) {
  using namespace ring_l0;
  const uint64_t step = (uint64_t)(rs.ctr->total_it + 1);
  const uint64_t n = (uint64_t)*rs.d_size;
  int64_t idx[RPW];
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const int grow = c.m0 + c.wave * RPW + r;
    idx[r] = grow < P.B ? (int64_t)philox_index(rs.seed, step, (uint32_t)grow, n) : -1;
  }
  const bool t0 = c.nt == 0;
  float x[RPW][8], rw[RPW];
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    rw[r] = 0.f;
    if (idx[r] >= 0) {
      const float* rec = rs.data + (size_t)idx[r] * rs.rec;
      rv_load_u(x[r], rec + P.exi[kRecOff], P.Kreal, c.lane);
      if (t0 && c.lane < 2 && rw_ptr(P, c.lane)) rw[r] = gld(rec + P.exi[kRecOffRw] + c.lane);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) x[r][j] = 0.f;
    }
  }
#pragma unroll
  for (int r = 0; r < RPW; ++r) lds_put_row(smem, c.S, c.wave * RPW + r, P.Kp, c.lane, x[r]);
  if (!t0) return;
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const int grow = c.m0 + c.wave * RPW + r;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int col = rcol(c.lane, j);
      if (col < P.Kreal) {
        if (P.Aout) gst(P.Aout + (size_t)grow * P.ldao + col, x[r][j]);
        if (P.ex[kRowCopy2]) gst(P.ex[kRowCopy2] + (size_t)grow * P.exi[kLdRowCopy2] + col, x[r][j]);
      }
    }
    if (c.lane < 2 && rw_ptr(P, c.lane)) gst(rw_ptr(P, c.lane) + grow, rw[r]);
    if (pi == 0 && rs.idx_out && c.lane == 0 && grow < P.B) rs.idx_out[grow] = idx[r];
  }
}

// ---- kProL0 / kProL0G: layer 0 inside the layer-1 launch --------------------------------
// Stage 1: the workgroup's 32 input rows (<= 32 wide) into LDS xs[32][kL0XS], each wave its
// kRPW rows (lane half h = row parity, lane i = column).  l0_load_x requests them FIRST in the
// kernel (ahead of the weights: vmcnt retires in order); kProL0G draws them from the ring exactly
// as pro_gather.  l0_put_x writes them to LDS and, in n-tile 0, stores the copies / reward /
// not_done / drawn rows.
constexpr int kL0R = kRPW / 2;
struct L0X {
  float x[kL0R], rw[kL0R];
  int64_t idx[kL0R];
};
template <bool GATHER>
__device__ __forceinline__ void l0_load_x(const GemmProb& P, const RingSide& rs, const Ctx& c, L0X& X) {
  using namespace ring_l0;
  const int K0 = P.exi[kK0];
  const int i = c.lane & 31, h = c.lane >> 5;
  const bool t0 = c.nt == 0;
  uint64_t step = 0, n = 0;
  if constexpr (GATHER) {
    step = (uint64_t)(rs.ctr->total_it + 1);
    n = (uint64_t)*rs.d_size;
  }
  const int col = i;
  const bool valid = i < K0;
  // every row's index is drawn before the first record load: drawn row by row, the second draw
  // (which reads the loaded step / ring size) sat behind a vmcnt(0) that also drained the first
  // row's record load
  if constexpr (GATHER) {
#pragma unroll
    for (int rr = 0; rr < kL0R; ++rr) {
      const int grow = c.m0 + c.wave * kRPW + 2 * rr + h;
      X.idx[rr] = grow < P.B ? (int64_t)philox_index(rs.seed, step, (uint32_t)grow, n) : -1;
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  // unconditional loads (padding rows read ring row 0, padding columns a real column) masked in
  // l0_put_x: conditional loads put the waitcnt pass's vmcnt(0) at their control-flow joins,
  // draining the record loads before the weights were even requested
#pragma unroll
  for (int rr = 0; rr < kL0R; ++rr) {
    const int row = c.wave * kRPW + 2 * rr + h, grow = c.m0 + row;
    if constexpr (GATHER) {
      const int64_t idx = X.idx[rr] >= 0 ? X.idx[rr] : 0;
      const float* rec = rs.data + (size_t)idx * rs.rec;
      X.x[rr] = gld(rec + P.exi[kRecOff] + (valid ? col : 0));
      X.rw[rr] = t0 ? gld(rec + P.exi[kRecOffRw] + (i & 1)) : 0.f;
    } else {
      X.x[rr] = gld(P.A + (size_t)grow * P.lda + col);  // input rows are >= 32 wide (zero pads)
    }
  }
  (void)valid;
}

template <bool GATHER>
__device__ __forceinline__ void l0_put_x(const GemmProb& P, const RingSide& rs, float* xs, const Ctx& c, int pi,
                                         const L0X& X) {
  using namespace ring_l0;
  const int K0 = P.exi[kK0];
  const int i = c.lane & 31, h = c.lane >> 5;
  const bool t0 = c.nt == 0;
  const int col = i;
  const bool valid = i < K0;
#pragma unroll
  for (int rr = 0; rr < kL0R; ++rr) {
    const int row = c.wave * kRPW + 2 * rr + h, grow = c.m0 + row;
    const float xv = (!GATHER || (X.idx[rr] >= 0 && valid)) ? X.x[rr] : 0.f;
    xs[row * kL0XS + i] = xv;
    if constexpr (GATHER) {
      if (t0) {
        if (valid) {
          if (P.ex[kRowCopy]) gst(P.ex[kRowCopy] + (size_t)grow * P.exi[kLdRowCopy] + col, xv);
          if (P.ex[kRowCopy2]) gst(P.ex[kRowCopy2] + (size_t)grow * P.exi[kLdRowCopy2] + col, xv);
        }
        if (i < 2 && rw_ptr(P, i)) gst(rw_ptr(P, i) + grow, X.idx[rr] >= 0 ? X.rw[rr] : 0.f);
        if (pi == 0 && rs.idx_out && i == 0 && grow < P.B) rs.idx_out[grow] = X.idx[rr];
      }
    }
  }
}

// k offset of lane half h in the layer-0 operands: 12h when the input fits in 24 columns (the x
// rows' and W0 rows' columns 24..31 are zero pads, so a half's 16-wide read past k = 24 reads 0)
__device__ __forceinline__ int l0_koff(const GemmProb& P, int h) { return (P.exi[ring_l0::kK0] <= 24 ? 12 : 16) * h; }

// Stage 2: Z0 = X * W0^T on MFMA (wave w: layer-0 column tiles w and w + 8), + b0, ReLU, into the
// layer-1 A buffer (LDS, [32][S]); n-tile 0 also stores H0 (the backward's post-ReLU rows).
// K0 <= 24 (every featured input but the widest): lane half h supplies k = 12h + s, so 12 MFMAs
// cover the row instead of 16 -- only the operand offsets change (l0_koff), no shuffles.  (An
// earlier variant that selected between layouts on the loaded data waited early: slower.)
__device__ __forceinline__ void l0_mfma(const GemmProb& P, const float* xs, float* smem, float* h0s, const Ctx& c,
                                        const float (&w0)[2][16], const float (&b0)[2]) {
  using namespace ring_l0;
  const int i = c.lane & 31, h = c.lane >> 5;
  const int n0t = P.exi[kN0p] >> 5;
  const bool k24 = P.exi[kK0] <= 24;
  const float* arow = xs + i * kL0XS + l0_koff(P, h);
  float av[16];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 v = *reinterpret_cast<const float4*>(arow + 4 * q);
    av[4 * q + 0] = v.x; av[4 * q + 1] = v.y; av[4 * q + 2] = v.z; av[4 * q + 3] = v.w;
  }
  const bool keep = P.ex[kH0] && P.norm;   // H0 kept in LDS for l0_store_rows (LN overwrites smem)
  // both tiles' MFMA chains first (two accumulators), then the epilogues, with the uniform `keep`
  // hoisted out of the element loop (inside it, it compiled to a branch per element)
  f32x16 acc[2];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
    if (c.wave + kNW * ct >= n0t) continue;
#pragma unroll
    for (int s = 0; s < 12; ++s) acc[ct] = mfma32x32x2(av[s], w0[ct][s], acc[ct]);
    if (!k24) {
#pragma unroll
      for (int s = 12; s < 16; ++s) acc[ct] = mfma32x32x2(av[s], w0[ct][s], acc[ct]);
    }
  }
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    const int tile = c.wave + kNW * ct;
    if (tile >= n0t) continue;
    const int col = tile * 32 + i;
    float v[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = fmaxf(acc[ct][r] + b0[ct], 0.f);
#pragma unroll
    for (int r = 0; r < 16; ++r) smem[mfma_row(r, c.lane) * c.S + col] = v[r];
    if (keep) {
#pragma unroll
      for (int r = 0; r < 16; ++r) h0s[mfma_row(r, c.lane) * c.S + col] = v[r];
    }
  }
}

// Stage 3: LayerNorm 0 of the A buffer rows in place (each wave its kRPW rows); n-tile 0 stores
// the row statistics, as pro_ln (U0 is stored by l0_store_rows).
// (gamma / beta are requested at the kernel start: loaded here, their vmcnt wait also drained
// the n-tile-0 workgroup's sample-copy stores queued ahead of them, ~1 us)
__device__ __forceinline__ void l0_ln(const GemmProb& P, float* smem, const Ctx& c, const float (&g)[8],
                                      const float (&bb)[8]) {
  constexpr int RB = kRPW;
  float x[RB][8], mean[RB], rstd[RB], rm[8];
#pragma unroll
  for (int r = 0; r < RB; ++r) rv_load_lds(x[r], smem + (c.wave * kRPW + r) * c.S, P.Kp, c.lane);
  real_mask(rm, P.Kreal, c.lane);
  ln_fwd_rows_pk<RB>(x, g, bb, rm, 1.0f / (float)P.Kreal, mean, rstd);
  const bool t0 = c.nt == 0;
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    const int row = c.wave * kRPW + r, grow = c.m0 + row;
    lds_put_row(smem, c.S, row, P.Kp, c.lane, x[r]);
    if (t0 && P.stats && c.lane == 0) {
      gst(P.stats + (grow), mean[r]);
      gst(P.stats + (c.Bp + grow), rstd[r]);
    }
  }
}

// Stage 4 (after the layer-1 MFMA loop): H0 (post-ReLU, for LN0's backward) and U0 (post-LN, the
// layer-1 dW input) of the 32 rows, each n-tile workgroup of the row tile storing its 1/ntiles
// slice of the columns.  Stored from n-tile 0 during the prologue they were 128 KB of stores
// queued ahead of its weight stream (vmcnt retires in order): those workgroups ended ~3 us after
// the rest (F_fwd01, tools/tl_probe.py).
template <int NT>
__device__ __forceinline__ void l0_store_rows(const GemmProb& P, const float* smem, const float* h0s, const Ctx& c) {
  using namespace ring_l0;
  float* H0 = P.ex[kH0];
  float* U0 = P.norm ? P.Aout : nullptr;
  if (!H0 && !U0) return;
  const float* hsrc = P.norm ? h0s : smem;          // no LN: the A buffer is H0
  const int nq = P.Kp >> 2;
  const int q0 = c.nt * nq / P.ntiles, per = (c.nt + 1) * nq / P.ntiles - q0;
  for (int e = threadIdx.x; e < 32 * per; e += NT) {
    const int row = e / per, q = 4 * (q0 + e % per);
    const size_t grow = (size_t)(c.m0 + row);
    if (H0) gst4(H0 + grow * P.exi[kN0p] + q, *reinterpret_cast<const float4*>(hsrc + row * c.S + q));
    if (U0) gst4(U0 + grow * P.ldao + q, *reinterpret_cast<const float4*>(smem + row * c.S + q));
  }
}

}  // namespace td3
