// TD3 gradient-step kernels for gfx950 (MI355X).
//
// What each kernel restates (reference = /root/reference):
//   gemm_kernel<0,*,P>   nn.Linear forward + ReLU of one layer for several networks; the
//                        prologue P builds the input rows: copy, the previous layer's
//                        LayerNorm (ReLU -> LN order, TD3_featured.py:41-46 / :75-80), or a
//                        fused head (target smoothing :131-137, pi = max_action*tanh :47-48)
//   gemm_kernel<1,*,P>   dX = dZ * W of a Linear; the prologue forms dZ from dU
//                        (LN backward + ReLU backward) or from a fused loss head
//                        (clipped double-Q target + mse grads :139-148, -mean Q1 :159,
//                        dQ1/da -> tanh / max_action backward -> actor head)
//   dw_kernel            weight / bias / LN-affine grads (batch reductions, MFMA) fused
//                        with torch Adam (adam.py:457-547) and Polyak (:167-171)
//   lnbwd_rows_kernel    dZ of the first hidden layer (no GEMM follows it)
//   head_kernel          act / eval_q heads (TD3_featured.py:113-121)
//
// Latency rules applied everywhere (every kernel here is latency-bound at B=256):
// every operand a workgroup needs is requested before the first wait (weight fragments
// for all of a wave's K chunks, all rows of a batch, LN affines, head weights); wave
// reductions use DPP + readlane (no LDS round trips); rows are processed in batches so
// independent reductions interleave.
//
// Compute dtype: fp32 everywhere.  Matrix products use v_mfma_f32_32x32x2_f32
// (exact fp32 FMA chain, MI355X_MICROARCH.md § Matrix cores).
#include <math.h>
#include <stdlib.h>

#include "dev.h"
#include "kernels.h"
#include "row_actor.h"

namespace td3 {

// In-kernel phase timeline (experiment builds only: tools/build_exp.sh tl "-DTD3_TL"): per
// workgroup, s_memrealtime (100 MHz) at entry / after the prologue barrier / after the MFMA
// loop / after its own stores drained, plus the XCC id.  Read back with td3_tl_read.
#ifdef TD3_TL
__device__ unsigned long long td3_tl[8192][8];
// shader-clock counter (s_memtime) beside the 100 MHz marks 1 and 2 (prologue barrier, end of the
// MFMA loop): (clk[1] - clk[0]) / (tl[2] - tl[1]) * 100 MHz = the clock the MFMA phase ran at
__device__ unsigned long long td3_clk[8192][2];
__device__ __forceinline__ void tl_mark(int k) {
  const unsigned id = blockIdx.x + blockIdx.y * gridDim.x;
  if (threadIdx.x == 0 && id < 8192) {
    if (k == 3) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (k == 1 || k == 2) td3_clk[id][k - 1] = __builtin_amdgcn_s_memtime();
    td3_tl[id][k] = __builtin_amdgcn_s_memrealtime();
    if (k == 0) {
      unsigned x, hw;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
      td3_tl[id][4] = x | ((unsigned long long)hw << 32);
    }
  }
}
#define TL_MARK(k) tl_mark(k)
// every GEMM workgroup's MFMA phase (prologue barrier -> end of the MFMA loop) summed over launches:
// [0] shader-clock ticks (s_memtime), [1] 100 MHz ticks (s_memrealtime); read / cleared with
// td3_clk_sum_read (tools/clk_probe.py: the clock a run's MFMA phases ran at)
__device__ unsigned long long td3_clk_sum[2];
#define TL_CLK_BEGIN() const unsigned long long tl_c0 = __builtin_amdgcn_s_memtime(), tl_r0 = __builtin_amdgcn_s_memrealtime()
#define TL_CLK_END()                                                                             \
  do {                                                                                         \
    const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime(); \
    if (threadIdx.x == 0) {                                                                    \
      atomicAdd(&td3_clk_sum[0], c1 - tl_c0);                                                  \
      atomicAdd(&td3_clk_sum[1], r1 - tl_r0);                                                  \
    }                                                                                          \
  } while (0)
#else
#define TL_MARK(k)
#define TL_CLK_BEGIN()
#define TL_CLK_END()
#endif
#ifdef TD3_TL_FINE      // drain the loads at the mark (changes the overlap: phase attribution only)
#define TL_FINE(k) do { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); TL_MARK(k); } while (0)
#else
#define TL_FINE(k)
#endif

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

// ================================================================== batch-row GEMM stage
// Workgroup = 4 waves = one 32-row batch tile x (32*WN) output columns; each wave owns a
// 32x32 output tile and 1/WK of the K chunks (<= 4 chunks of 32 per wave).
//  1. weight fragments of every chunk of the wave are requested first (64 VGPRs),
//  2. the prologue builds the 32 A rows in LDS ([32][S], S == 4 mod 64 dwords: the
//     ds_read_b128 fragment reads are bank-conflict free),
//  3. per chunk a lane reads 16 A values (4x ds_read_b128) and issues 16
//     v_mfma_f32_32x32x2_f32 (lane half h supplies k = 16h + s of MFMA s),
//  4. WK > 1: the partial tiles are summed through LDS; bias / ReLU epilogue.
// With kNW waves, a wave holds at most 16 / kNW chunks of K <= 512 (WN = 1: WK = kNW;
// WN = 4 only runs K <= 128 with WK = kNW / 4).

// The k-quad stride of a MODE 0 weight image (GemmProb::wsk; 0: row-major)
__device__ __forceinline__ int w_sk(int wsk) { return wsk ? wsk : 4; }
// W0 of the fused layer-0 stages (ring_l0::kW0): row stride and k-quad stride (GemmProb::w0sk)
__device__ __forceinline__ int w0_sn(int w0sk) { return w0sk ? 4 : 32; }
__device__ __forceinline__ int w0_sk(int w0sk) { return w0sk ? w0sk : 4; }

template <int MODE>
__device__ __forceinline__ void load_chunk(const GemmProb& P, float (&b)[16], int ch, int ncol, int h) {
  const int kb = ch * 32 + 16 * h;
  if (MODE == 0) {
    const int sk = w_sk(P.wsk);
    const float* wp = P.W + (size_t)ncol * P.ldw + (size_t)(kb >> 2) * sk;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 v = gld4(wp + (size_t)q * sk);
      b[4 * q + 0] = v.x; b[4 * q + 1] = v.y; b[4 * q + 2] = v.z; b[4 * q + 3] = v.w;
    }
  } else {
    const float* wp = P.W + (size_t)kb * P.ldw + ncol;
#pragma unroll
    for (int s = 0; s < 16; ++s) b[s] = gld(wp + (size_t)s * P.ldw);
  }
}

template <int MODE, int NCH>
__device__ __forceinline__ void load_b(const GemmProb& P, float (&bv)[NCH][16], int cb, int nch,
                                       int ncol, int h) {
#pragma unroll
  for (int cc = 0; cc < NCH; ++cc) load_chunk<MODE>(P, bv[cc], min(cb + cc, nch - 1), ncol, h);
}

// WN = 0 (16 columns, v_mfma_f32_16x16x4_f32): lane (column ncol, k-group g) holds the weights
// k = ch*32 + 8g + s, s = 0..7, in b[0..7] (MODE 0: W[n][k], two float4; MODE 1: W[k][n]).
template <int MODE>
__device__ __forceinline__ void load_chunk16(const GemmProb& P, float (&b)[16], int ch, int ncol, int g) {
  const int kb = ch * 32 + 8 * g;
  if (MODE == 0) {
    const int sk = w_sk(P.wsk);
    const float* wp = P.W + (size_t)ncol * P.ldw + (size_t)(kb >> 2) * sk;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const float4 v = gld4(wp + (size_t)q * sk);
      b[4 * q + 0] = v.x; b[4 * q + 1] = v.y; b[4 * q + 2] = v.z; b[4 * q + 3] = v.w;
    }
  } else {
    const float* wp = P.W + (size_t)kb * P.ldw + ncol;
#pragma unroll
    for (int s = 0; s < 8; ++s) b[s] = gld(wp + (size_t)s * P.ldw);
  }
}

template <int MODE, int NCH>
__device__ __forceinline__ void load_b16(const GemmProb& P, float (&bv)[NCH][16], int cb, int nch,
                                         int ncol, int g) {
#pragma unroll
  for (int cc = 0; cc < NCH; ++cc) load_chunk16<MODE>(P, bv[cc], min(cb + cc, nch - 1), ncol, g);
}

// XCD-aware tile order (cdna_hip_programming.md §5.5 T1): the dispatcher deals blocks
// round-robin over the 8 XCDs, so block b runs on XCD b % 8.  Consecutive tiles (which share
// a weight column block: m is the fastest tile index) are given to blocks of one XCD, so a
// weight tile is fetched over the fabric once per XCD and then hit in that XCD's L2.
// `nb` is the real tile count; the grid is padded to a multiple of 8 (surplus blocks exit).
__device__ __forceinline__ int xcd_tile(int nb) {
  const int per = (nb + 7) >> 3;
  return (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
}



// Kernel arguments: the problem directory (nb, nprob, tile_begin of problems 1..3, Bp) comes
// first and is preloaded into SGPRs at wave launch (-amdgpu-kernarg-preload-count, build.py), so
// the problem select costs no memory round trip; the problem's fields are then the first and only
// kernel-argument round trip ahead of the operand loads.
#ifndef TD3_L0G_LATE_B
#define TD3_L0G_LATE_B 1
#endif
#ifndef TD3_L0_LATE_B
#define TD3_L0_LATE_B 0
#endif
// One workgroup's tile b of a GEMM stage (the body of gemm_kernel / gemm2_kernel).
template <int MODE, int WN, int PRO, int NW = kNW>
__device__ __forceinline__ void gemm_body(int b, int nprob, int tb1, int tb2, int tb3, int Bp, const GemmTable& tab,
                                          Counters* bump, int bump_actor, float* smem) {
  using namespace ring_l0;
  constexpr int RT = wn_rt(WN);                // 32-row tiles of the workgroup (kWn4x2: 2)
  constexpr int RPW = 32 * RT / NW;            // prologue rows per wave
  static_assert(NW == kNW || (PRO != kProL0 && PRO != kProL0G), "fused layer 0 runs kNW waves");
  static_assert(RT == 1 || (PRO != kProL0 && PRO != kProL0G && PRO != kProGather), "two row tiles: plain prologues");
  // WN = 0: 16 output columns per workgroup on v_mfma_f32_16x16x4_f32 (two 16-row halves of the
  // 32-row tile): half the MFMA chain of WN = 1 for stages of <= 128 32-column workgroups, which
  // otherwise leave half the CUs idle (stages.hip gemm_wn)
  constexpr int WNS = WN == 0 ? 1 : wn_cols(WN);   // waves per K group
  constexpr int WK = NW / WNS;
  constexpr int NT = 64 * NW;                  // threads
  constexpr int OUTW = WN == 0 ? 16 : 32 * wn_cols(WN);   // output columns of the workgroup
  constexpr bool kPrefetchB = true;
  int pi = 0;
  if (nprob > 1 && b >= tb1) pi = 1;
  if (nprob > 2 && b >= tb2) pi = 2;
  if (nprob > 3 && b >= tb3) pi = 3;
  pi = __builtin_amdgcn_readfirstlane(pi);     // one scalar index (not a select per field address)
  const GemmProb& P = tab.p[pi];
  // every field this workgroup reads, requested in ONE scalar-load batch: left to itself the
  // compiler requests each where first used, a chain of dependent kernarg round trips ahead of
  // the first operand load (tools/tl_probe.py)
  constexpr bool kL0 = PRO == kProL0 || PRO == kProL0G;
  if constexpr (kL0) {
    // fused layer 0: the fields the first operand requests need, in ONE batch (each asm
    // statement is a use, i.e. a wait: two statements were two dependent round trips); the rest
    // are batched behind the operand requests (l0_late_fields)
    if constexpr (PRO == kProL0G)
      asm volatile("" ::"s"(P.A), "s"(P.lda), "s"(P.ex[kW0]), "s"(P.ex[kB0]), "s"(P.exi[kN0p]), "s"(P.exi[kK0]),
                   "s"(P.W), "s"(P.ldw), "s"(P.Kp), "s"(P.lng), "s"(P.lnb), "s"(P.bias), "s"(P.Nout),
                   "s"(P.tile_begin), "s"(P.norm), "s"(P.B), "s"(tab.rs.data), "s"(tab.rs.rec), "s"(tab.rs.d_size),
                   "s"(tab.rs.seed), "s"(tab.rs.ctr), "s"(P.exi[kRecOff]), "s"(P.exi[kRecOffRw]), "s"(P.wsk),
                   "s"(P.w0sk));
    else
      asm volatile("" ::"s"(P.A), "s"(P.lda), "s"(P.ex[kW0]), "s"(P.ex[kB0]), "s"(P.exi[kN0p]), "s"(P.exi[kK0]),
                   "s"(P.W), "s"(P.ldw), "s"(P.Kp), "s"(P.lng), "s"(P.lnb), "s"(P.bias), "s"(P.Nout),
                   "s"(P.tile_begin), "s"(P.norm), "s"(P.B), "s"(P.wsk), "s"(P.w0sk));
  } else {
    if constexpr (PRO == kProHeadBwd)      // one batch with the head operands (a second asm would be a
      asm volatile("" ::"s"(P.A), "s"(P.lng), "s"(P.lnb), "s"(P.W), "s"(P.C), "s"(P.lda), "s"(P.Kreal), "s"(P.Kp),
                   "s"(P.ldw), "s"(P.Nout), "s"(P.ldc), "s"(P.ntiles), "s"(P.tile_begin), "s"(P.norm), "s"(P.B),
                   "s"(P.ex[head_bwd_pro::kW4]), "s"(P.ex[head_bwd_pro::kB4]), "s"(P.ex[head_bwd_pro::kQ]),
                   "s"(P.exf[head_bwd_pro::kGradScale]));
    else                                   // second dependent kernel-argument round trip)
      asm volatile("" ::"s"(P.A), "s"(P.lng), "s"(P.lnb), "s"(P.H), "s"(P.stats), "s"(P.Aout), "s"(P.W), "s"(P.bias),
                   "s"(P.C), "s"(P.lda), "s"(P.Kreal), "s"(P.Kp), "s"(P.ldh), "s"(P.ldao), "s"(P.ldw), "s"(P.Nout),
                   "s"(P.ldc), "s"(P.relu), "s"(P.ntiles), "s"(P.tile_begin), "s"(P.norm), "s"(P.B), "s"(P.wsk));
    if constexpr (PRO == kProGather)
      asm volatile("" ::"s"(P.ex[kRowCopy2]), "s"(P.ex[kReward]), "s"(P.ex[kNotDone]), "s"(P.exi[kRecOff]),
                   "s"(P.exi[kRecOffRw]), "s"(P.exi[kLdRowCopy2]), "s"(tab.rs.data), "s"(tab.rs.rec),
                   "s"(tab.rs.d_size), "s"(tab.rs.idx_out), "s"(tab.rs.seed), "s"(tab.rs.ctr));
  }
  const int mtiles = (Bp >> 5) / RT;
  const int t = b - P.tile_begin;
  const int mt = t % mtiles, nt = t / mtiles;
#if defined(TD3_TL) && !defined(TD3_TL_FINE)
  if (threadIdx.x == 0 && blockIdx.x < 8192) td3_tl[blockIdx.x][4] |= (unsigned long long)(nt + 1) << 16;
#endif
  const int m0 = mt * 32 * RT;
  const int n0 = nt * OUTW;
  const int Kp = P.Kp;
  const int S = lds_stride(Kp);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = lane & 31, h = lane >> 5;
  const int wn = wave % WNS, wk = wave / WNS;
  const int nch = Kp >> 5;
  const int cb = wk * nch / WK, ce = (wk + 1) * nch / WK;
  const int ncol0 = n0 + wn * 32;
  const bool active = ncol0 < P.Nout;
  const int ncol = (active ? ncol0 : 0) + (WN == 0 ? (lane & 15) : i);

  // weight chunks requested at the kernel start (the rest stream in the MFMA loop).  Prefetching
  // all 4 chunks of a WN=2 wave was no faster: the A-row loads then queue behind 16 weight loads.
  constexpr int kCh = 16 / NW;                // weight chunks a wave requests up front
  float bv[kCh][16];
  // bias of the epilogue's column, requested with the weights (off the tail of the chain)
  const int bcol = (WK == 1) ? ncol : n0 + (int)(threadIdx.x % OUTW);
  const float bias = (MODE == 0 && P.bias && (WK > 1 ? bcol < P.Nout : active)) ? gld(P.bias + bcol) : 0.f;
  const Ctx c{m0, wave, lane, nt, Bp, S};
  // kProL0*: the input rows first, then the wave's layer-0 weight tiles (B operand:
  // W0[tile*32 + i][16h .. 16h+15]) and biases, then the layer-1 weights
  L0X l0x;
  if constexpr (kL0) l0_load_x<PRO == kProL0G>(P, tab.rs, c, l0x);
  float w0[2][16], b0v[2];
  if constexpr (kL0) {
    const int koff = l0_koff(P, h);
    const int sn0 = w0_sn(P.w0sk), sk0 = w0_sk(P.w0sk);
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      const int tile = min(wave + kNW * ct, (P.exi[kN0p] >> 5) - 1);
      const float* wp = P.ex[kW0] + (size_t)(tile * 32 + i) * sn0 + (size_t)(koff >> 2) * sk0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 v = gld4(wp + (size_t)q * sk0);
        w0[ct][4 * q + 0] = v.x; w0[ct][4 * q + 1] = v.y; w0[ct][4 * q + 2] = v.z; w0[ct][4 * q + 3] = v.w;
      }
      b0v[ct] = gld(P.ex[kB0] + tile * 32 + i);
    }
  }
  float lg[8], lb[8];                          // kL0: LayerNorm-0 gamma / beta
  if constexpr (kL0) {
    if (P.norm) {
      rv_load(lg, P.lng, P.Kp, lane);
      rv_load(lb, P.lnb, P.Kp, lane);
    }
  }
  // the sampled-record stage (kProL0G) requests its layer-1 weights after the records landed:
  // in flight together, they delayed the latency-critical random record reads
  constexpr bool kLateB = (PRO == kProL0G && TD3_L0G_LATE_B) || (PRO == kProL0 && TD3_L0_LATE_B);
  if constexpr (kPrefetchB && !kLateB) {
    if constexpr (WN == 0) load_b16<MODE, kCh>(P, bv, cb, nch, ncol, lane >> 4);
    else load_b<MODE, kCh>(P, bv, cb, nch, ncol, h);
    __builtin_amdgcn_sched_barrier(0);     // keep the weight requests ahead of the prologue
  }

  if constexpr (kL0)         // l0_late_fields: requested behind the operand loads (waited for in their shadow)
    asm volatile("" ::"s"(P.ex[kH0]), "s"(P.Aout), "s"(P.ldao), "s"(P.stats), "s"(P.Kreal), "s"(P.C), "s"(P.ldc),
                 "s"(P.relu), "s"(P.ntiles), "s"(P.ex[kRowCopy2]), "s"(P.ex[kReward]), "s"(P.ex[kNotDone]),
                 "s"(P.ex[kRowCopy]), "s"(P.exi[kLdRowCopy2]), "s"(P.exi[kLdRowCopy]), "s"(tab.rs.idx_out));
  TL_MARK(5);
  // WN >= 2 waves own more chunks than kCh: the next two are requested right behind the A rows
  // (in flight during the LayerNorm, not queued ahead of it), the rest stream in the MFMA loop
  float bs0[16], bs1[16];
  const int s0 = cb + kCh;
  // WN = 4 (B >= 512, two workgroups per CU at <= 128 VGPRs) requests them after the prologue:
  // in flight during the LayerNorm they pushed the kernel past 128 VGPRs
  // The fused layer-0 stages (kL0) request the first two streamed chunks right before the MFMA
  // loop, unconditionally, the chunk index clamped to the wave's last chunk (a surplus load reads
  // that chunk again and is never multiplied): behind a branch, the waitcnt pass could not count
  // them and waited vmcnt(4) / vmcnt(0) before the first two chunks' MFMAs, i.e. for the chunks
  // just requested (F_fwd01 ISA; C2 +1 %).  The other prologues issue them early (pro_ln) or
  // measured slower unconditional (Humanoid MODE 1 stages: surplus strided loads).
  const int clast = max(ce - 1, 0);
  auto issue_stream = [&]() {
    if constexpr (WN == 2) {
      if constexpr (kL0) {
        load_chunk<MODE>(P, bs0, min(s0, clast), ncol, h);
        load_chunk<MODE>(P, bs1, min(s0 + 1, clast), ncol, h);
      } else {
        if (s0 < ce) load_chunk<MODE>(P, bs0, s0, ncol, h);
        if (s0 + 1 < ce) load_chunk<MODE>(P, bs1, s0 + 1, ncol, h);
      }
    }
  };

  if constexpr (PRO == kProCopy) pro_copy<RPW>(P, smem, c);
  else if constexpr (PRO == kProLN) pro_ln<RPW>(P, smem, c, issue_stream);
  else if constexpr (PRO == kProLNBwd) pro_lnbwd<RPW>(P, smem, c);
  else if constexpr (PRO == kProHeadBwd) pro_headbwd<RPW>(P, smem, c);
  else if constexpr (PRO == kProGather) pro_gather<RPW>(P, tab.rs, smem, c, pi);
  else if constexpr (kL0) {
    float* xs = smem + 32 * S;
    l0_put_x<PRO == kProL0G>(P, tab.rs, xs, c, pi, l0x);
    if constexpr (kLateB) {
      if constexpr (WN == 0) load_b16<MODE, kCh>(P, bv, cb, nch, ncol, lane >> 4);
      else load_b<MODE, kCh>(P, bv, cb, nch, ncol, h);
      __builtin_amdgcn_sched_barrier(0);
    }
    lds_barrier();
    TL_MARK(6);
    l0_mfma(P, xs, smem, xs + 32 * kL0XS, c, w0, b0v);
    if (P.norm) {
      lds_barrier();
      TL_MARK(7);
      l0_ln(P, smem, c, lg, lb);
    }
    issue_stream();
  }
  lds_barrier();
  TL_MARK(1);
  TL_CLK_BEGIN();
  if constexpr (PRO != kProLN && !kL0) issue_stream();
  if constexpr (wn_cols(WN) == 4) {
    if (s0 < ce) load_chunk<MODE>(P, bs0, s0, ncol, h);
    if (s0 + 1 < ce) load_chunk<MODE>(P, bs1, s0 + 1, ncol, h);
  }

  f32x4 acc16[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};   // WN = 0: rows 0-15, 16-31
  if constexpr (WN == 0) {
    if (active) {
      // lane (r = lane & 15, g = lane >> 4) supplies k = kb + 8g + s of MFMA s: its 8 A values
      // of a row are contiguous (2 ds_read_b128) and its 8 weights too; the two row halves are
      // independent accumulators (40-cycle dependent latency vs 32-cycle issue)
      const int g = lane >> 4;
      const float* ar0 = smem + (lane & 15) * S + 8 * g;
      const float* ar1 = ar0 + 16 * S;
#pragma unroll
      for (int cc = 0; cc < kCh; ++cc) {
        if (cb + cc < ce) {
          const int kb = (cb + cc) * 32;
          float x0[8], x1[8];
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            const float4 u = *reinterpret_cast<const float4*>(ar0 + kb + 4 * q);
            const float4 v = *reinterpret_cast<const float4*>(ar1 + kb + 4 * q);
            x0[4 * q + 0] = u.x; x0[4 * q + 1] = u.y; x0[4 * q + 2] = u.z; x0[4 * q + 3] = u.w;
            x1[4 * q + 0] = v.x; x1[4 * q + 1] = v.y; x1[4 * q + 2] = v.z; x1[4 * q + 3] = v.w;
          }
#pragma unroll
          for (int s = 0; s < 8; ++s) {
            acc16[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(x0[s], bv[cc][s], acc16[0], 0, 0, 0);
            acc16[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(x1[s], bv[cc][s], acc16[1], 0, 0, 0);
          }
        }
      }
    }
  }
  f32x16 acc[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[rt][r] = 0.f;
  // one 32-deep K chunk: per row tile, the lane's 16 A values (4 ds_read_b128) and 16 MFMAs on the
  // chunk's weight fragment (the row tiles' chains are independent: interleaved)
  auto chunk = [&](const float* arow, int kb, const float (&b)[16]) {
    float av[RT][16];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(arow + rt * 32 * S + kb + 4 * q);
        av[rt][4 * q + 0] = v.x; av[rt][4 * q + 1] = v.y; av[rt][4 * q + 2] = v.z; av[rt][4 * q + 3] = v.w;
      }
#pragma unroll
    for (int s = 0; s < 16; ++s)
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) acc[rt] = mfma32x32x2(av[rt][s], b[s], acc[rt]);
  };
  if (WN != 0 && active) {
    const float* arow = smem + i * S + 16 * h;
#pragma unroll
    for (int cc = 0; cc < kCh; ++cc)
      if (cb + cc < ce) chunk(arow, (cb + cc) * 32, bv[cc]);
    // the streamed chunks: two buffers, chunk ch+2 requested as chunk ch is multiplied
    if constexpr (wn_cols(WN) >= 2) {
      for (int ch = s0; ch < ce; ch += 2) {
        chunk(arow, ch * 32, bs0);
        if (ch + 2 < ce) load_chunk<MODE>(P, bs0, ch + 2, ncol, h);
        if (ch + 1 < ce) {
          chunk(arow, (ch + 1) * 32, bs1);
          if (ch + 3 < ce) load_chunk<MODE>(P, bs1, ch + 3, ncol, h);
        }
      }
    }
  }

  TL_CLK_END();
  if constexpr (kL0) l0_store_rows<NT>(P, smem, smem + 32 * S + 32 * kL0XS, c);
  if constexpr (WK == 1 && WN != 0) {
    if (active) {
      const int col = ncol0 + i;
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = rt * 32 + mfma_row(r, lane);
          float v = acc[rt][r];
          if (MODE == 0 && P.bias) v = v + bias;
          if (P.relu) v = fmaxf(v, 0.f);
          gst(P.C + ((size_t)(m0 + row) * P.ldc + col), v);
        }
    }
    TL_MARK(2);
  } else {
    float* red = smem;  // [NW][32][33]; wave = wk * WNS + wn; one row tile at a time
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      lds_barrier();
      if constexpr (WN == 0) {
        // 16x16 C/D map: column lane & 15, row 4 * (lane >> 4) + j
#pragma unroll
        for (int half = 0; half < 2; ++half)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            red[(wave * 32 + 16 * half + 4 * (lane >> 4) + j) * 33 + (lane & 15)] = acc16[half][j];
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) red[(wave * 32 + mfma_row(r, lane)) * 33 + i] = acc[rt][r];
      }
      lds_barrier();
      TL_MARK(2);
      // (32 x OUTW outputs over NT threads: 16 waves of a 16-column tile leave half the threads idle)
#pragma unroll
      for (int q = 0; q < (32 * OUTW + NT - 1) / NT; ++q) {
        const int e = threadIdx.x + NT * q;
        if (32 * OUTW % NT != 0 && e >= 32 * OUTW) break;
        const int row = e / OUTW, colw = e % OUTW;
        const int wnn = colw >> 5, ci = colw & 31;
        float v = red[(wnn * 32 + row) * 33 + ci];
#pragma unroll
        for (int w = 1; w < WK; ++w) v = v + red[((w * WNS + wnn) * 32 + row) * 33 + ci];
        if (MODE == 0 && P.bias) v = v + bias;
        if (P.relu) v = fmaxf(v, 0.f);
        if (n0 + colw < P.Nout) gst(P.C + ((size_t)(m0 + rt * 32 + row) * P.ldc + n0 + colw), v);
      }
    }
  }
  // a separate layer-0 forward stage of the actor phase (learner.h Plan::W1aT): the workgroups of column
  // tile nt also write its weight rows' columns [kTCol, kTCol + kTN), transposed, for
  // actor_head_bwd -- row n0 + r by row tile r % mtiles (done by row tile 0 alone, the copy was
  // that workgroup's tail: AF_fwd0 +0.9 us)
  if constexpr (MODE == 0 && PRO == kProCopy) {
    float* tc = P.ex[kTCopy];
    if (tc) {
      const int tcol = P.exi[kTCol], tn = P.exi[kTN];
      for (int e = threadIdx.x; e < OUTW * tn; e += NT) {
        const int r = e / tn, o = e % tn, n = n0 + r;
        if (r % mtiles == mt && n < P.Nout) gst(tc + ((size_t)o * P.Nout + n), gld(P.W + ((size_t)n * P.ldw + (size_t)((tcol + o) >> 2) * w_sk(P.wsk) + ((tcol + o) & 3))));
      }
    }
  }
  TL_MARK(3);
  // step counters (TD3_featured.py:124), off the head of the chain; the bumping stage never
  // reads them (the sample of this step drew its rows in the stage before)
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

template <int MODE, int WN, int PRO>
__global__ __launch_bounds__(64 * gemm_nw(MODE, WN, PRO), WN == 4 ? 4 : WN == kWn4x2 ? 2 : 1) void gemm_kernel(int nb, int nprob, int tb1, int tb2, int tb3, int Bp,
                                                        GemmTable tab, Counters* bump, int bump_actor) {
  extern __shared__ float4 smem4[];
  const int b = xcd_tile(nb);
  TL_MARK(0);
  if (b >= nb) return;
  gemm_body<MODE, WN, PRO, gemm_nw(MODE, WN, PRO)>(b, nprob, tb1, tb2, tb3, Bp, tab, bump, bump_actor,
                                                   reinterpret_cast<float*>(smem4));
}

// Two independent GEMM stages in one launch (the unit-gradient critic backward beside the target
// twin's forward, step.hip build_step): a uniform branch per workgroup picks the stage; the launch takes the
// larger LDS and register footprint of the two bodies.
// Tile placement: stage 1's tiles take the first 8*ceil(nb1/8) workgroup ids, dealt over the 8
// XCDs as xcd_tile does (consecutive tiles, which share weight columns, on one XCD); stage 2's
// follow the same way.  Dispatched in id order, stage 1 (the longer forward layer) gets a CU per
// workgroup and stage 2 starts on the CUs it leaves free, refilling them as its workgroups end.
#ifndef TD3_DUAL_OCC
#define TD3_DUAL_OCC 4
#endif
template <int M1, int W1, int P1, int M2, int W2, int P2>
__global__ __launch_bounds__(64 * kNW, (W1 == 4 || W2 == 4) ? 4 : (W1 == kWn4x2 || W2 == kWn4x2) ? 2 : TD3_DUAL_OCC) void gemm2_kernel(
    int nb1, int nb2, int Bp, int np1, int a1, int a2, int a3, int np2, int c1, int c2, int c3, GemmTable t1,
    GemmTable t2) {
  extern __shared__ float4 smem4[];
  TL_MARK(0);
  const int per1 = (nb1 + 7) >> 3, per2 = (nb2 + 7) >> 3;
  float* smem = reinterpret_cast<float*>(smem4);
  const int id = (int)blockIdx.x;
  if (id < 8 * per1) {
    const int b = (id & 7) * per1 + (id >> 3);
    if (b >= nb1) return;
    gemm_body<M1, W1, P1>(b, np1, a1, a2, a3, Bp, t1, nullptr, 0, smem);
  } else {
    const int l = id - 8 * per1, b = (l & 7) * per2 + (l >> 3);
    if (b >= nb2) return;
    gemm_body<M2, W2, P2>(b, np2, c1, c2, c3, Bp, t2, nullptr, 0, smem);
  }
}

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

// ================================================================== act / eval_q heads
__global__ __launch_bounds__(256) void head_kernel(HeadArgs a) {
  const HeadProb P = a.probs[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.Bp) return;
  float x[1][8], g[8], bb[8], mean[1], rstd[1];
  const int ld = P.ldh;
  rv_load(x[0], P.H3 + (size_t)row * ld, ld, lane);
  if (P.lng) {
    rv_load(g, P.lng, ld, lane);
    rv_load(bb, P.lnb, ld, lane);
    ln_fwd_rows<1>(x, g, bb, P.K3, lane, mean, rstd);
    if (P.stats && lane == 0) {
      gst(P.stats + (row), mean[0]);
      gst(P.stats + (a.Bp + row), rstd[0]);
    }
  }
  if (P.U3) rv_store(P.U3 + (size_t)row * P.ldu, P.ldu, lane, x[0]);
  float zl = 0.f;
  for (int o = 0; o < P.nout; ++o) {
    float w[8];
    rv_load(w, P.W4 + (size_t)o * P.ldw, P.ldw, lane);
    const float z = wsum(rv_pdot(x[0], w, P.K3, lane)) + gld(P.b4 + (o));
    if (lane == o) zl = z;
  }
  if (lane >= P.nout) return;
  const int o = lane;
  const bool live = row < a.B;
  if (P.mode == kHeadPolicy) {
    const float th = tanhf(zl);
    gst(P.out + ((size_t)row * P.ldo + P.out_col + o), live ? a.max_action * th : 0.f);
    if (P.tanh_out) gst(P.tanh_out + ((size_t)row * 32 + o), th);
  } else {
    gst(P.out + ((size_t)row * P.ldo + o), zl);          // Q values [row][nout]
  }
}

// ================================================================== small-query hidden layers
// One wave per 4 output columns of one network (blockIdx.y): the wave loads its 4 weight rows
// and the R query rows (lane-sliced, K <= 512), applies the input LayerNorm (the GEMM prologue's
// packed form: pads of X, gamma, beta are zero) and reduces the 4R dot products.
template <int R>
__global__ __launch_bounds__(256) void gemv_kernel(GemvArgs a) {
  const GemvProb& P = a.p[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int o0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 4;
  if (o0 >= P.N) return;
  float w[4][8], x[R][8];
#pragma unroll
  for (int j = 0; j < 4; ++j) rv_load(w[j], P.W + (size_t)min(o0 + j, P.N - 1) * P.ldw, P.K, lane);
#pragma unroll
  for (int r = 0; r < R; ++r) rv_load(x[r], P.X + (size_t)min(r, a.B - 1) * P.ldx, P.K, lane);
  if (P.lng) {
    float g[8], bb[8], rm[8], mean[R], rstd[R];
    rv_load(g, P.lng, P.K, lane);
    rv_load(bb, P.lnb, P.K, lane);
    real_mask(rm, P.K, lane);
    ln_fwd_rows_pk<R>(x, g, bb, rm, 1.0f / (float)P.K, mean, rstd);
  }
  float z[4][R];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < R; ++r) z[j][r] = wsum(rv_pdot(x[r], w[j], P.K, lane));
  // lane 4r + j stores column o0 + j of row r
  const int j = lane & 3, r = lane >> 2;
  if (r < R && r < a.B && o0 + j < P.N) {
    float v = 0.f;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
      for (int rr = 0; rr < R; ++rr)
        if (jj == j && rr == r) v = z[jj][rr];
    gst(P.Y + (size_t)r * P.ldy + o0 + j, fmaxf(v + gld(P.b + o0 + j), 0.f));
  }
}

template <int R>
__global__ __launch_bounds__(256) void gemv01_kernel(Gemv01Args a) {
  __shared__ float h0[R][512];
  const GemvProb& P = a.l1.p[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int o0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 4;
  float w[4][8], x[R][8];
#pragma unroll
  for (int j = 0; j < 4; ++j) rv_load(w[j], P.W + (size_t)min(o0 + j, P.N - 1) * P.ldw, P.K, lane);
  // H0 (all N0 columns, zero pads) into LDS; W0 pads past K0 are zero, so the float4 steps may
  // read past a row's K0 query values (xq is zero past B*K0 and padded by 4)
  const float* W0 = a.W0[blockIdx.y];
  const float* b0 = a.b0[blockIdx.y];
  for (int o = threadIdx.x; o < 512; o += 256) {
    float z[R];
#pragma unroll
    for (int r = 0; r < R; ++r) z[r] = 0.f;
    if (o < a.N0) {
      const float* wr = W0 + (size_t)o * a.ldw0;
      for (int c = 0; c < a.K0; c += 4) {
        const float4 wv = gld4(wr + c);
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const float* q = a.xq + r * a.K0 + c;
          z[r] += wv.x * q[0];
          z[r] += wv.y * q[1];
          z[r] += wv.z * q[2];
          z[r] += wv.w * q[3];
        }
      }
      const float bo = gld(b0 + o);
#pragma unroll
      for (int r = 0; r < R; ++r) z[r] = fmaxf(z[r] + bo, 0.f);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) h0[r][o] = z[r];
  }
  __syncthreads();
  if (o0 >= P.N) return;
#pragma unroll
  for (int r = 0; r < R; ++r) rv_load_lds(x[r], h0[r], P.K, lane);
  if (P.lng) {
    float g[8], bb[8], rm[8], mean[R], rstd[R];
    rv_load(g, P.lng, P.K, lane);
    rv_load(bb, P.lnb, P.K, lane);
    real_mask(rm, P.K, lane);
    ln_fwd_rows_pk<R>(x, g, bb, rm, 1.0f / (float)P.K, mean, rstd);
  }
  float z[4][R];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < R; ++r) z[j][r] = wsum(rv_pdot(x[r], w[j], P.K, lane));
  const int j = lane & 3, r = lane >> 2;
  if (r < R && r < a.l1.B && o0 + j < P.N) {
    float v = 0.f;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
      for (int rr = 0; rr < R; ++rr)
        if (jj == j && rr == r) v = z[jj][rr];
    gst(P.Y + (size_t)r * P.ldy + o0 + j, fmaxf(v + gld(P.b + o0 + j), 0.f));
  }
}

// ================================================================== one-launch query (select_action)
// select_action / eval_q of n <= kGemvRows rows as ONE launch (TD3_featured.py:113-121; VERDICT
// r04 #6).  Grid (nb, networks) of 256-thread workgroups; workgroup b of network k:
//   1. requests its layer-1 and layer-2 weight rows (4 + 4 per wave: nothing in the launch writes
//      them), computes all of H0 = relu(W0 x + b0) into LDS (the query is in the arguments),
//   2. layer 1, columns 16b .. 16b+15 (LN0 in the prologue), stored write-through (sc1),
//   3. hands off: every storing wave drains its stores, the workgroup meets at a barrier, one lane
//      adds to the network's layer-1 counter; one lane polls it (sc1 loads) up to nb arrivals,
//   4. layer 2, the same 16 columns, from the H1 rows read with sc1 loads (LN1), stored sc1,
//   5. arrives on the network's second counter; the LAST arriver (the value its add returned) reads
//      H2 with sc1 loads, applies LN2 and the head, writes the outputs and zeroes both counters
//      (every workgroup has passed its layer-1 poll before its second add).
// The hand-off is MI355X_MICROARCH.md's sc1 form (stores and loads of the handed-off rows all sc1,
// each storing wave's vmcnt(0) before the workgroup barrier, one agent-scope atomic per workgroup).
// A poll that sees no progress for ~2^22 rounds gives up and the outputs are NaN (no hang).
__device__ __forceinline__ float ald(const float* p) {
  return __hip_atomic_load((const GAS float*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void ast(float* p, float v) {
  __hip_atomic_store((GAS float*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void rv_load_sc1(float (&v)[8], const float* row, int n, int lane) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = rcol(lane, j);
    v[j] = c < n ? ald(row + c) : 0.f;
  }
}

template <int R, int KQ>    // KQ: float4 steps of a layer-0 row (K0 <= 4 * KQ)
__global__ __launch_bounds__(256) void act_kernel(ActArgs a) {
  __shared__ float h0[R][512];
  __shared__ int s_flag;
  TL_MARK(0);
  const int k = blockIdx.y;
  const GemvProb& P1 = a.g.l1.p[k];
  const GemvProb& P2 = a.l2[k];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int B = a.g.l1.B;
  const int o0 = (blockIdx.x * 4 + wave) * 4;            // this wave's 4 columns of layers 1 and 2
  int* c1 = a.ctr + 2 * k;
  int* c2 = c1 + 1;
  // layer 0's weights first (H0 waits for them alone: vmcnt retires in order), coalesced: thread t
  // holds columns 4*kg .. 4*kg + 3 (kg = t % TPR) of rows rsub + RPP*i, a wave's loads whole
  // contiguous rows (one row per thread was a 64-line scatter per load: ~2 us of H0, act_tl.py)
  const float* W0 = a.g.W0[k];
  const float* b0 = a.g.b0[k];
  constexpr int LW = 4 * KQ;                  // W0 row stride (floats): 32 or 64
  constexpr int TPR = LW / 4, RPP = 256 / TPR, NPASS = 512 / RPP;
  const int kg = threadIdx.x % TPR, rsub = threadIdx.x / TPR;
  float4 w0r[NPASS];
  float b0r[NPASS];
#pragma unroll
  for (int i = 0; i < NPASS; ++i) {           // unconditional (rows past N0 clamp; pads are zero)
    const int o = min(rsub + RPP * i, a.g.N0 - 1);
    w0r[i] = gld4(W0 + (size_t)o * LW + 4 * kg);
    b0r[i] = gld(b0 + o);
  }
  float xr[R][4];                             // the query values of this thread's 4 columns (xq is
#pragma unroll                                // zero past B*K0; past K0 the weights are zero)
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) xr[r][jj] = a.g.xq[min(r * a.g.K0 + 4 * kg + jj, kGemvQ - 1)];
  // layer 1's operands; layer 2's and the head's are requested after the layer-1 hand-off (in
  // flight together with W0 they held H0 ~3 us behind the CU's ~70 GB/s L2 rate, act_tl.py)
  float w1[4][8], w2[4][8];
#pragma unroll
  for (int j = 0; j < 4; ++j) rv_load(w1[j], P1.W + (size_t)min(o0 + j, P1.N - 1) * P1.ldw, P1.K, lane);
  float g1[8], bb1[8], g2[8], bb2[8], rm1[8], rm2[8];
  if (P1.lng) {
    rv_load(g1, P1.lng, P1.K, lane);
    rv_load(bb1, P1.lnb, P1.K, lane);
  }
  real_mask(rm1, P1.K, lane);
  real_mask(rm2, P2.K, lane);
  const float bia1 = gld(P1.b + min(o0 + (lane & 3), P1.N - 1));
  const HeadProb& H = a.head[k];
  constexpr int kPre = 8;
  float w4[kPre][8], hg[8], hb[8];
  // 1. H0 of every query row: 4-column partial dot products, summed over the TPR threads of a row
  //    (butterfly), + b0, ReLU; rows past N0 are zero
#pragma unroll
  for (int i = 0; i < NPASS; ++i) {
    const int o = rsub + RPP * i;
    const float4 w = w0r[i];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float z = w.x * xr[r][0];
      z = z + w.y * xr[r][1];
      z = z + w.z * xr[r][2];
      z = z + w.w * xr[r][3];
#pragma unroll
      for (int m = TPR / 2; m >= 1; m >>= 1) z = z + __shfl_xor(z, m);
      if (kg == 0) h0[r][o] = o < a.g.N0 ? fmaxf(z + b0r[i], 0.f) : 0.f;
    }
  }
  __syncthreads();
  TL_MARK(5);
  const int j = lane & 3, rr = lane >> 2;                // lane 4r + j: column o0 + j of row r
  // 2. layer 1
  if (o0 < P1.N) {
    float x[R][8];
#pragma unroll
    for (int r = 0; r < R; ++r) rv_load_lds(x[r], h0[r], P1.K, lane);
    if (P1.lng) {
      float mean[R], rstd[R];
      ln_fwd_rows_pk<R>(x, g1, bb1, rm1, 1.0f / (float)P1.K, mean, rstd);
    }
    float z[4][R];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
      for (int r = 0; r < R; ++r) z[jj][r] = wsum(rv_pdot(x[r], w1[jj], P1.K, lane));
    if (rr < R && rr < B && o0 + j < P1.N) {
      float v = 0.f;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int r = 0; r < R; ++r)
          if (jj == j && r == rr) v = z[jj][r];
      ast(P1.Y + (size_t)rr * P1.ldy + o0 + j, fmaxf(v + bia1, 0.f));
    }
  }
  // 3. hand-off of H1 (every wave's stores drained before the barrier; one add per workgroup)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  TL_MARK(6);
  const int nb = (int)gridDim.x;
  if (threadIdx.x == 0) __hip_atomic_fetch_add((GAS int*)c1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // layer 2's operands and the head's (any workgroup may arrive last: rows 0..7 of W4, LN2 affine,
  // biases; a head of more outputs loads the rest in its loop), in flight during the poll
#pragma unroll
  for (int j = 0; j < 4; ++j) rv_load(w2[j], P2.W + (size_t)min(o0 + j, P2.N - 1) * P2.ldw, P2.K, lane);
  if (P2.lng) {
    rv_load(g2, P2.lng, P2.K, lane);
    rv_load(bb2, P2.lnb, P2.K, lane);
  }
  const float bia2 = gld(P2.b + min(o0 + (lane & 3), P2.N - 1));
#pragma unroll
  for (int o = 0; o < kPre; ++o) rv_load(w4[o], H.W4 + (size_t)min(o, H.nout - 1) * H.ldw, H.ldw, lane);
  if (H.lng) {
    rv_load(hg, H.lng, H.ldh, lane);
    rv_load(hb, H.lnb, H.ldh, lane);
  }
  const float b4 = lane < H.nout ? gld(H.b4 + lane) : 0.f;
  if (threadIdx.x == 0) {
    int ok = !(a.fail_test && blockIdx.x == 0);
    for (int spin = 0; ok && __hip_atomic_load((GAS int*)c1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < nb; ++spin) {
      if (spin > (1 << 22)) {
        ok = 0;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    s_flag = ok;
  }
  __syncthreads();
  TL_MARK(7);
  const bool ok1 = s_flag != 0;
  // 4. layer 2 on the H1 rows
  if (o0 < P2.N) {
    float x[R][8];
#pragma unroll
    for (int r = 0; r < R; ++r) rv_load_sc1(x[r], P2.X + (size_t)min(r, B - 1) * P2.ldx, P2.K, lane);
    if (P2.lng) {
      float mean[R], rstd[R];
      ln_fwd_rows_pk<R>(x, g2, bb2, rm2, 1.0f / (float)P2.K, mean, rstd);
    }
    float z[4][R];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
      for (int r = 0; r < R; ++r) z[jj][r] = wsum(rv_pdot(x[r], w2[jj], P2.K, lane));
    if (rr < R && rr < B && o0 + j < P2.N) {
      float v = 0.f;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int r = 0; r < R; ++r)
          if (jj == j && r == rr) v = z[jj][r];
      ast(P2.Y + (size_t)rr * P2.ldy + o0 + j, ok1 ? fmaxf(v + bia2, 0.f) : __builtin_nanf(""));
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  TL_MARK(1);
  // arrival on the layer-2 counter; a workgroup whose poll gave up adds kActFailInc too, so the last
  // arriver knows the H2 rows are not all valid and publishes the flag with kActFailed (the host
  // then reports an error and re-zeroes the counters) instead of a valid-looking result
  if (threadIdx.x == 0) {
    const int old = __hip_atomic_fetch_add((GAS int*)c2, ok1 ? 1 : 1 + kActFailInc, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
    const bool last = (old & (kActFailInc - 1)) == nb - 1;
    s_flag = last ? ((old >= kActFailInc || !ok1) ? 2 : 1) : 0;
  }
  __syncthreads();
  TL_MARK(2);
  if (!s_flag) return;
  const bool failed = s_flag == 2;
  // 5. the last arriver: LN2 + head of row `wave` (head_kernel's arithmetic on sc1 loads)
  if (wave < B) {
    float x[1][8], mean[1], rstd[1];
    rv_load_sc1(x[0], H.H3 + (size_t)wave * H.ldh, H.K3, lane);
    if (H.lng) ln_fwd_rows<1>(x, hg, hb, H.K3, lane, mean, rstd);
    float zl = 0.f;
#pragma unroll
    for (int o = 0; o < kPre; ++o) {
      if (o >= H.nout) break;
      const float z = wsum(rv_pdot(x[0], w4[o], H.K3, lane)) + __shfl(b4, o);
      if (lane == o) zl = z;
    }
    for (int o = kPre; o < H.nout; ++o) {
      float w[8];
      rv_load(w, H.W4 + (size_t)o * H.ldw, H.ldw, lane);
      const float z = wsum(rv_pdot(x[0], w, H.K3, lane)) + __shfl(b4, o);
      if (lane == o) zl = z;
    }
    if (lane < H.nout) {
      if (H.mode == kHeadPolicy) gst(H.out + ((size_t)wave * H.ldo + H.out_col + lane), a.max_action * tanhf(zl));
      else gst(H.out + ((size_t)wave * H.ldo + lane), zl);
    }
  }
  // publish: the outputs (mapped host memory) complete, a system-scope release, then this network's
  // flag = the launch's sequence number, which the host polls instead of a stream synchronize
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __hip_atomic_store((GAS int*)c1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next
    __hip_atomic_store((GAS int*)c2, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // launch (stream order)
    if (a.flag) {
      __threadfence_system();
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(a.flag + k, failed ? (a.seq | kActFailed) : a.seq, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  TL_MARK(3);
}

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

// ================================================================== split-K dW (kernels.h DwSplit)
// Bp >= 512: one tile per workgroup (dw64g_kernel) did not fit the chip evenly -- Humanoid C_dw: 288
// 64x64 matrix tiles + 74 vector tiles on 256 CUs, so 32 CUs ran two tiles back to back (50 us; one
// tile alone 23.5).  Here every tile's 64-row steps are cut into ONE weighted list split evenly over
// one workgroup per CU; a workgroup walks its share tile by tile (LDS-DMA staging as dw64g_kernel)
// and stores one fp32 partial per tile it touched; the combine launch sums a tile's partials in
// workgroup order (fixed order: bitwise reproducible) and applies the optimizer.  Matrix tiles are
// 128 x 128 by default (dwsk_matrix128: 64 KB staged per step for 64 MFMA per wave -- a 64 x 64 step
// stages 32 KB for 16, and was bound by its DMA round trip, not the MFMA pipe).
__device__ __forceinline__ int dwsk_virtual(int g, int G) { return (g & 7) * (G >> 3) + (g >> 3); }

// Steps [s0, s1) of matrix tile (nt, kt) of P -> the 64x64 partial (row n - n0, column k - k0) at out.
template <bool SC>
__device__ __forceinline__ void dwsk_matrix(const DwArgs& a, const DwProb& P, int nt, int kt, int s0, int s1,
                                            float* sm, float* out) {
  float* const ssl = sm + 2 * 2 * 64 * 64;
  const int n0 = nt * 64, k0 = kt * 64;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 31, h = lane >> 5;
  const int qn = (wave >> 1) & 1, qk = wave & 1, rh = wave >> 2;
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
      const int rl = 8 * wave + 4 * j;
      const size_t row = (size_t)(st * 64 + rl + lr);
      glds16(P.G + row * P.ldg + gcol[j], g + rl * 64);
      glds16(P.U + row * P.ldu + ucol[j], u + rl * 64);
    }
    if constexpr (SC) {
      if (wave == 0) glds4(P.rs + (size_t)(st * 64 + lane) * P.ldrs, ssl + buf * 64);
    }
  };
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  issue(s0, 0);
  const int ca = (qn ^ h) * 32 + i, cb = (qk ^ h) * 32 + i;
  const bool live = n0 + qn * 32 < P.Np && k0 + qk * 32 < P.Kp;
  for (int st = s0; st < s1; ++st) {
    const int buf = (st - s0) & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's DMA of step st has landed
    __syncthreads();                                 // everyone's has; buffer buf ^ 1 is free
    if (st + 1 < s1) issue(st + 1, buf ^ 1);
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
  float* red = sm + (wave & 3) * 32 * 33;
  if (rh == 1) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[mfma_row(r, lane) * 33 + i] = acc[r];
  }
  __syncthreads();
  if (rh == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r)
      gst(out + (qn * 32 + mfma_row(r, lane)) * 64 + qk * 32 + i, acc[r] + red[mfma_row(r, lane) * 33 + i]);
  }
  __syncthreads();                                   // the next segment restages sm
}

// Steps [s0, s1) of 128 x 128 matrix tile (nt, kt) of P -> the partial (row n - n0, column k - k0,
// ld 128) at out; quadrants past Np / Kp are neither fetched, multiplied nor stored.  LDS per buffer
// and operand: [64 rows][128 cols], the 32-column groups 2c and 2c+1 swapped on rows with bit 4 set
// (an MFMA operand read takes rows 16 apart in its two lane halves, which then hit other banks).
// Wave w: n quadrant w >> 1 and k quadrants (w & 1), (w & 1) + 2, so the two waves of a SIMD (w, w + 4)
// own n quadrants {a, a + 2} x k quadrants {b, b + 2}: an edge tile's live quadrants stay spread
// over the four SIMDs.
template <bool SC>
__device__ __forceinline__ void dwsk_matrix128(const DwArgs& a, const DwProb& P, int nt, int kt, int s0, int s1,
                                               float* sm, float* out) {
  float* const ssl = sm + 2 * 2 * 64 * 128;
  const int n0 = nt * 128, k0 = kt * 128;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 31, h = lane >> 5;
  const int qn = wave >> 1, qk0 = wave & 1, qk1 = qk0 + 2;
  // DMA lanes: wave w fills rows 8w .. 8w+7 of both operands (four 2-row wave-instructions each);
  // lane L -> row 8w + 2j + L/32, LDS columns 4(L&31) .. +3 <- source columns of the swizzle
  const int lr = lane >> 5, lc = (lane & 31) * 4;
  int gcol[4], ucol[4];
  bool gl[4], ul[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = 8 * wave + 2 * j + lr;
    const int c = lc ^ (((row >> 4) & 1) << 5);
    gcol[j] = n0 + c;
    ucol[j] = k0 + c;
    gl[j] = gcol[j] < P.Np;                          // Np, Kp multiples of 32: whole column groups
    ul[j] = ucol[j] < P.Kp;
  }
  auto issue = [&](int st, int buf) {
    float* g = sm + buf * 2 * 8192;
    float* u = g + 8192;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int rl = 8 * wave + 2 * j;
      const size_t row = (size_t)(st * 64 + rl + lr);
      if (gl[j]) glds16(P.G + row * P.ldg + gcol[j], g + rl * 128);
      if (ul[j]) glds16(P.U + row * P.ldu + ucol[j], u + rl * 128);
    }
    if constexpr (SC) {
      if (wave == 0) glds4(P.rs + (size_t)(st * 64 + lane) * P.ldrs, ssl + buf * 64);
    }
  };
  f32x16 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    acc0[r] = 0.f;
    acc1[r] = 0.f;
  }
  issue(s0, 0);
  const int ca = (qn ^ h) * 32 + i, cb0 = (qk0 ^ h) * 32 + i, cb1 = (qk1 ^ h) * 32 + i;
  const bool live_n = n0 + qn * 32 < P.Np;
  const bool live0 = live_n && k0 + qk0 * 32 < P.Kp, live1 = live_n && k0 + qk1 * 32 < P.Kp;
  for (int st = s0; st < s1; ++st) {
    const int buf = (st - s0) & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's DMA of step st has landed
    __syncthreads();                                 // everyone's has; buffer buf ^ 1 is free
    if (st + 1 < s1) issue(st + 1, buf ^ 1);
    if (!live0) continue;
    // MFMA s (0..31) takes rows 32 (s >> 4) + 16 h + (s & 15): lane half h's rows have bit 4 = h
    const float* g = sm + buf * 2 * 8192 + 16 * h * 128;
    const float* u = g + 8192;
    float scl[32];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const float4 v4 = SC ? *reinterpret_cast<const float4*>(ssl + buf * 64 + 32 * (q >> 2) + 16 * h + 4 * (q & 3))
                           : make_float4(1.f, 1.f, 1.f, 1.f);
      scl[4 * q + 0] = v4.x; scl[4 * q + 1] = v4.y; scl[4 * q + 2] = v4.z; scl[4 * q + 3] = v4.w;
    }
    if (live1) {
#pragma unroll
      for (int s2 = 0; s2 < 32; ++s2) {
        const int r = 32 * (s2 >> 4) + (s2 & 15);
        const float ga = SC ? g[r * 128 + ca] * scl[s2] : g[r * 128 + ca];
        acc0 = mfma32x32x2(ga, u[r * 128 + cb0], acc0);
        acc1 = mfma32x32x2(ga, u[r * 128 + cb1], acc1);
      }
    } else {
#pragma unroll
      for (int s2 = 0; s2 < 32; ++s2) {
        const int r = 32 * (s2 >> 4) + (s2 & 15);
        const float ga = SC ? g[r * 128 + ca] * scl[s2] : g[r * 128 + ca];
        acc0 = mfma32x32x2(ga, u[r * 128 + cb0], acc0);
      }
    }
  }
  if (live0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) gst(out + (qn * 32 + mfma_row(r, lane)) * 128 + qk0 * 32 + i, acc0[r]);
  }
  if (live1) {
#pragma unroll
    for (int r = 0; r < 16; ++r) gst(out + (qn * 32 + mfma_row(r, lane)) * 128 + qk1 * 32 + i, acc1[r]);
  }
  __syncthreads();                                   // the next segment restages sm
}

// Steps [s0, s1) of vector tile j of P (32 columns): the partial db, dgamma, dbeta at out[0 / 32 / 64 + c].
// Thread = 4 adjacent columns x one row of each 64-row step (64 row groups), 4 steps per load batch.
template <bool SC>
__device__ __forceinline__ void dwsk_vector(const DwArgs& a, const DwProb& P, int j, int s0, int s1, float* red,
                                            float* out) {
  constexpr int U = 4;
  const int n0 = j * 32;
  const int c4 = (threadIdx.x & 7) * 4, rg = threadIdx.x >> 3;
  const bool ln = P.offg >= 0;
  const bool hasb = P.offb >= 0;
  const float* gzp = hasb ? P.G : P.GU;             // operands read from valid addresses, masked at use
  const float* gup = ln ? P.GU : P.G;
  const float* hp = ln ? P.H : P.G;
  const float* stp = ln ? P.stats : P.G;
  const int ldz = hasb ? P.ldg : P.ldgu, ldu = ln ? P.ldgu : P.ldg, ldh = ln ? P.ldh : P.ldg;
  float sb[4] = {0.f, 0.f, 0.f, 0.f}, sg[4] = {0.f, 0.f, 0.f, 0.f}, sbeta[4] = {0.f, 0.f, 0.f, 0.f};
  for (int st = s0; st < s1; st += U) {
    float4 gz[U], gu[U], hh[U];
    float mu[U], rs[U], sc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int r = min(st + u, s1 - 1) * 64 + rg;  // clamped: loads stay unconditional
      gz[u] = gld4(gzp + ((size_t)r * ldz + n0 + c4));
      gu[u] = gld4(gup + ((size_t)r * ldu + n0 + c4));
      hh[u] = gld4(hp + ((size_t)r * ldh + n0 + c4));
      mu[u] = gld(stp + r);
      rs[u] = gld(stp + (a.Bp + r));
      sc[u] = SC ? gld(P.rs + (size_t)r * P.ldrs) : 1.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (st + u >= s1) continue;
      if (hasb) {
        sb[0] += gz[u].x * sc[u]; sb[1] += gz[u].y * sc[u]; sb[2] += gz[u].z * sc[u]; sb[3] += gz[u].w * sc[u];
      }
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
    red[(0 * 64 + rg) * 33 + c4 + e] = sb[e];
    red[(1 * 64 + rg) * 33 + c4 + e] = sg[e];
    red[(2 * 64 + rg) * 33 + c4 + e] = sbeta[e];
  }
  __syncthreads();
  if (threadIdx.x < 96) {
    const int w = threadIdx.x >> 5, c = threadIdx.x & 31;
    float s = 0.f;
#pragma unroll 8
    for (int g = 0; g < 64; ++g) s += red[(w * 64 + g) * 33 + c];
    gst(out + w * 32 + c, s);
  }
  __syncthreads();
}

template <bool SC, bool T128>
__global__ __launch_bounds__(512, T128 ? 1 : 2) void dwsk_kernel(DwArgs a, DwSplit k) {
  // ONE __shared__ object (a second one made hipcc drain the DMA before every step's first operand
  // read, dw64g_kernel): [buf][operand][64 rows][tm cols (swizzled)], then SC's [buf][64] row scales
  __shared__ float sm[2 * 2 * 64 * (T128 ? 128 : 64) + 2 * 64];
  const int v = dwsk_virtual((int)blockIdx.x, k.G);
  TL_MARK(0);
  int u = k.wg_unit[v];
  const int u1 = k.wg_unit[v + 1];
  int j = 0;
#ifdef TD3_TL
  int nmat = 0, nvec = 0;
#endif
  while (u < u1) {
    const int t = __builtin_amdgcn_readfirstlane(u / k.S);
    const int s0 = u - t * k.S;
    const int s1 = (u1 - u) + s0 < k.S ? (u1 - u) + s0 : k.S;
    const DwTile T = k.tiles[t];
    const int pi = __builtin_amdgcn_readfirstlane(T.prob);
    const DwProb& P = a.probs[pi];
    float* out = k.slab + ((size_t)v * k.J + j) * k.slot;
    const int ta = __builtin_amdgcn_readfirstlane(T.a);
    if (__builtin_amdgcn_readfirstlane(T.kind) == 0) {
      if constexpr (T128) dwsk_matrix128<SC>(a, P, ta, __builtin_amdgcn_readfirstlane(T.b), s0, s1, sm, out);
      else dwsk_matrix<SC>(a, P, ta, __builtin_amdgcn_readfirstlane(T.b), s0, s1, sm, out);
    } else {
      dwsk_vector<SC>(a, P, ta, s0, s1, sm, out);
    }
    u += s1 - s0;
#ifdef TD3_TL
    if (T.kind == 0) nmat += s1 - s0;
    else nvec += s1 - s0;
    if (j == 0) TL_MARK(1);
    if (j == 1) TL_MARK(2);
#endif
    ++j;
  }
  TL_MARK(3);
#ifdef TD3_TL
  if (threadIdx.x == 0 && blockIdx.x < 8192) {
    td3_tl[blockIdx.x][5] = nmat;
    td3_tl[blockIdx.x][6] = nvec;
    td3_tl[blockIdx.x][7] = j;
  }
#endif
}

// Four workgroups per tile (a quarter of a matrix tile's rows each; a vector tile uses the first):
// the tile's partials summed in workgroup order, then the optimizer (or the gradient store of the
// data-parallel / weight-norm paths) on its elements.
__global__ __launch_bounds__(256) void dwsk_combine_kernel(DwArgs a, DwSplit k) {
  const int t = blockIdx.x >> 2, qtr = blockIdx.x & 3;
  const DwTile T = k.tiles[t];
  const DwProb& P = a.probs[__builtin_amdgcn_readfirstlane(T.prob)];
  const int v0 = k.tile_wg[2 * t], v1 = k.tile_wg[2 * t + 1];
  const AdamPw pw = adam_pw(a.adam);
  auto part = [&](int v) -> const float* {
    return k.slab + ((size_t)v * k.J + (t - k.wg_unit[v] / k.S)) * k.slot;
  };
  auto live = [&](int v) { return k.wg_unit[v] < k.wg_unit[v + 1]; };
  if (T.kind == 0) {
    const int tm = k.tm, c4 = tm >> 2;                // float4s per partial row
    const int n0 = T.a * tm, k0 = T.b * tm;
    const int per = tm * tm / (16 * 256);             // float4s per thread in a quarter: 1 or 4
    const bool grad_only = a.mode == kDwGrad, pol = a.mode == kDwAdamPolyak;
    const AdamK ak = make_adam(a.adam, pw);
    for (int q = 0; q < per; ++q) {
      const int e4 = (qtr * per + q) * 256 + threadIdx.x;
      const int row = e4 / c4, col = (e4 % c4) * 4;
      const int n = n0 + row, kk = k0 + col;
      if (n >= P.Np || kk >= P.Kp) continue;         // Kp is a multiple of 32: whole float4 in or out
      float4 g4 = gld4(part(v0) + row * tm + col);
      for (int v = v0 + 1; v <= v1; ++v) {
        if (!live(v)) continue;
        const float4 o = gld4(part(v) + row * tm + col);
        g4.x = g4.x + o.x; g4.y = g4.y + o.y; g4.z = g4.z + o.z; g4.w = g4.w + o.w;
      }
      const float gq[4] = {kk < P.kvalid ? g4.x : 0.f, kk + 1 < P.kvalid ? g4.y : 0.f,
                           kk + 2 < P.kvalid ? g4.z : 0.f, kk + 3 < P.kvalid ? g4.w : 0.f};
      const int64_t ix = P.offW + (int64_t)n * P.Kp + kk;
      if (grad_only) {
        gst4(a.adam.G + ix, make_float4(gq[0], gq[1], gq[2], gq[3]));
        continue;
      }
      const float4 m4 = gld4(a.adam.M + ix), v4 = gld4(a.adam.V + ix), p4 = gld4(a.adam.P + ix);
      const float4 t4 = gld4((pol ? a.adam.T : a.adam.P) + ix);
      float mm[4] = {m4.x, m4.y, m4.z, m4.w}, vv[4] = {v4.x, v4.y, v4.z, v4.w};
      float pp[4] = {p4.x, p4.y, p4.z, p4.w}, tt[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {                   // torch _single_tensor_adam, as adam_elem
        mm[e] = __fmaf_rn(ak.w1, gq[e] - mm[e], mm[e]);
        vv[e] = vv[e] * ak.b2;
        vv[e] = vv[e] + (ak.c2 * gq[e]) * gq[e];
        const float denom = sqrtf(vv[e]) / ak.bc2s + ak.eps;
        pp[e] = pp[e] + (ak.negss * mm[e]) / denom;
        tt[e] = ak.tau * pp[e] + ak.omt * tt[e];
      }
      sst4(a.adam.M + ix, make_float4(mm[0], mm[1], mm[2], mm[3]));
      sst4(a.adam.V + ix, make_float4(vv[0], vv[1], vv[2], vv[3]));
      pst4(a.adam.P + ix, make_float4(pp[0], pp[1], pp[2], pp[3]));
      if (pol) pst4(a.adam.T + ix, make_float4(tt[0], tt[1], tt[2], tt[3]));
      if (a.adam.P4) {                                // the k-quad images (one 16-B piece)
        const int64_t iq = P.offW + ((int64_t)(kk >> 2) * P.Np + n) * 4;
        pst4(a.adam.P4 + iq, make_float4(pp[0], pp[1], pp[2], pp[3]));
        if (pol) pst4(a.adam.T4 + iq, make_float4(tt[0], tt[1], tt[2], tt[3]));
      }
    }
    return;
  }
  if (qtr != 0 || threadIdx.x >= 32) return;
  const int c = threadIdx.x, n0 = T.a * 32;
  float gq[3];
#pragma unroll
  for (int w = 0; w < 3; ++w) {
    float s = gld(part(v0) + w * 32 + c);
    for (int v = v0 + 1; v <= v1; ++v)
      if (live(v)) s = s + gld(part(v) + w * 32 + c);
    gq[w] = s;
  }
  const bool ln = P.offg >= 0, hasb = P.offb >= 0;
  const int64_t idx[3] = {P.offb + n0 + c, P.offg + n0 + c, P.offbeta + n0 + c};
  const bool ok[3] = {hasb, ln, ln};
  apply_grads<3>(a, make_adam(a.adam, pw), idx, gq, ok);
}

// The flat optimizer pass of the data-parallel path (after the all-reduce): 4 elements per thread
// and array as one float4 (arenas and bucket ranges are multiples of 32 floats; launch_adam_flat
// checks), every load of the 4 elements requested before the first store.
__global__ __launch_bounds__(256) void adam_flat_kernel(AdamArgs a, int64_t n, int polyak, W4Map w) {
  const AdamK k = make_adam(a);
  const int64_t n4 = n >> 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const int64_t e = 4 * i;
    const float4 g4 = gld4(a.G + e), m4 = gld4(a.M + e), v4 = gld4(a.V + e), p4 = gld4(a.P + e);
    const float4 t4 = gld4((polyak ? a.T : a.P) + e);
    float g[4] = {g4.x * k.gscale, g4.y * k.gscale, g4.z * k.gscale, g4.w * k.gscale};
    float mm[4] = {m4.x, m4.y, m4.z, m4.w}, vv[4] = {v4.x, v4.y, v4.z, v4.w};
    float pp[4] = {p4.x, p4.y, p4.z, p4.w}, tt[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      adam_regs(pp[j], mm[j], vv[j], g[j], k);
      tt[j] = k.tau * pp[j] + k.omt * tt[j];           // TD3_featured.py:167-171
    }
    sst4(a.M + e, make_float4(mm[0], mm[1], mm[2], mm[3]));
    sst4(a.V + e, make_float4(vv[0], vv[1], vv[2], vv[3]));
    pst4(a.P + e, make_float4(pp[0], pp[1], pp[2], pp[3]));
    if (polyak) pst4(a.T + e, make_float4(tt[0], tt[1], tt[2], tt[3]));
    if (w.P4) {                                      // the k-quad images of the weight matrices
      const int64_t j = w.base + e;
      for (int m = 0; m < w.nmat; ++m) {
        const int64_t r = j - w.off[m];
        if (r < 0 || r >= (int64_t)w.Np[m] * w.Kp[m]) continue;
        const int nn = (int)(r / w.Kp[m]), kq = (int)(r - (int64_t)nn * w.Kp[m]) >> 2;
        const int64_t iq = w.off[m] + ((int64_t)kq * w.Np[m] + nn) * 4;
        pst4(w.P4 + iq, make_float4(pp[0], pp[1], pp[2], pp[3]));
        if (polyak) pst4(w.T4 + iq, make_float4(tt[0], tt[1], tt[2], tt[3]));
        break;
      }
    }
  }
}

__global__ __launch_bounds__(256) void local_sum_kernel(LocalSumArgs a) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.size; i += (int64_t)gridDim.x * 256) {
    float v = gld(a.a[0] + i);
    for (int k = 1; k < a.n; ++k) v = v + gld(a.a[k] + i);
    for (int k = 0; k < a.n; ++k) gst(a.a[k] + i, v);
  }
}

__global__ __launch_bounds__(256) void polyak_flat_kernel(float* T, const float* P, int64_t n, float tau,
                                                          float omt) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    gst(T + i, tau * gld(P + i) + omt * gld(T + i));
}

// ================================================================== weight normalization
// One wave per output row of a weight-normalised Linear (K <= 512: 8 columns per lane).
// kWnAdam: the row's dL/dW (G arena, dw_kernel in kDwGrad mode, all-reduced when data
// parallel) becomes torch's weight_norm backward
//   dg = (dW . v) / ||v||,   dv = (g / ||v||) dW - (g (dW . v) / ||v||^3) v
// then Adam on (bias, g, v) with the group's moments (adam_elem, + Polyak of the targets) and
// the row of W = v * (g / ||v||) is derived again from the updated parameters (and targets).
__device__ __forceinline__ float wn_norm(const float (&v)[8], int K, int lane) {
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (rcol(lane, j) < K) q += v[j] * v[j];
  return sqrtf(wsum(q));
}

__device__ __forceinline__ void wn_store_w(float* arena, const WnLinear& L, int i, int lane, float (&v)[8],
                                           float g) {
  const float sc = g / wn_norm(v, L.K, lane);
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = v[j] * sc;
  rv_store(arena + L.offW + (size_t)i * L.ld, L.K, lane, v);
}

__device__ __forceinline__ float lane0(float x) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 0));
}

__global__ __launch_bounds__(256) void wn_kernel(WnArgs a) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= a.rows) return;
  int l = 0;
  while (l + 1 < a.nlin && r >= a.lin[l + 1].row0) ++l;
  const WnLinear& L = a.lin[l];
  const int i = r - L.row0;
  float v[8];
  if (a.mode == kWnDerive) {
    for (float* arena : {a.arena, a.arena2}) {
      if (!arena) continue;
      rv_load(v, arena + L.offv + (size_t)i * L.ld, L.K, lane);
      wn_store_w(arena, L, i, lane, v, gld(arena + L.offg + i));
    }
    return;
  }
  const AdamArgs& A = a.adam;
  float* T = a.polyak ? A.T : nullptr;
  // every operand of the row requested up front: v, dW, the moments (and targets) of v, and on
  // lane 0 g, the bias and their optimizer state
  const size_t ov = L.offv + (size_t)i * L.ld;
  float gw[8], m[8], w2[8], vt[8];
  rv_load(v, A.P + ov, L.K, lane);
  rv_load(gw, A.G + L.offW + (size_t)i * L.ld, L.K, lane);
  rv_load(m, A.M + ov, L.K, lane);
  rv_load(w2, A.V + ov, L.K, lane);
  if (T) rv_load(vt, T + ov, L.K, lane);
  const size_t og = L.offg + i, ob = L.offb + i;
  float sg[4] = {0.f, 0.f, 0.f, 0.f}, sb[4] = {0.f, 0.f, 0.f, 0.f}, gb = 0.f;
  if (lane == 0) {
    sg[0] = gld(A.P + og); sg[1] = gld(A.M + og); sg[2] = gld(A.V + og);
    sb[0] = gld(A.P + ob); sb[1] = gld(A.M + ob); sb[2] = gld(A.V + ob);
    gb = gld(A.G + ob);
    if (T) { sg[3] = gld(T + og); sb[3] = gld(T + ob); }
  }
  const AdamK k = make_adam(A);
  const float g = lane0(sg[0]);
#pragma unroll
  for (int j = 0; j < 8; ++j) gw[j] *= k.gscale;
  const float n = wn_norm(v, L.K, lane);
  const float sdot = wsum(rv_pdot(gw, v, L.K, lane));
  const float ca = g / n;
  const float cb = ca * sdot / (n * n);
  const float dg = sdot / n;
  // v: element-wise Adam in registers (pads stay 0: zero grads and moments)
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float d = ca * gw[j] - cb * v[j];
    if (rcol(lane, j) < L.K) {
      adam_regs(v[j], m[j], w2[j], d, k);
      if (T) vt[j] = k.tau * v[j] + k.omt * vt[j];        // TD3_featured.py:167-171
    }
  }
  rv_store(A.P + ov, L.K, lane, v);
  rv_store(A.M + ov, L.K, lane, m);
  rv_store(A.V + ov, L.K, lane, w2);
  if (T) rv_store(T + ov, L.K, lane, vt);
  if (lane == 0) {
    adam_regs(sg[0], sg[1], sg[2], dg, k);
    adam_regs(sb[0], sb[1], sb[2], gb * k.gscale, k);
    pst(A.P + og, sg[0]); sst(A.M + og, sg[1]); sst(A.V + og, sg[2]);
    pst(A.P + ob, sb[0]); sst(A.M + ob, sb[1]); sst(A.V + ob, sb[2]);
    if (T) {
      sg[3] = k.tau * sg[0] + k.omt * sg[3];
      sb[3] = k.tau * sb[0] + k.omt * sb[3];
      gst(T + og, sg[3]);
      gst(T + ob, sb[3]);
    }
  }
  const float gn = lane0(sg[0]), gt = lane0(sg[3]);
  wn_store_w(A.P, L, i, lane, v, gn);
  if (T) wn_store_w(T, L, i, lane, vt, gt);
}

// ================================================================== launchers
template <int MODE, int WN, int PRO>
static void gl(const GemmTable& t, int nblocks, int Bp, int lds, Counters* bump, int ba, hipStream_t s) {
  const int padded = (nblocks + 7) & ~7;
  const int tb1 = t.nprob > 1 ? t.p[1].tile_begin : nblocks, tb2 = t.nprob > 2 ? t.p[2].tile_begin : nblocks;
  const int tb3 = t.nprob > 3 ? t.p[3].tile_begin : nblocks;
  constexpr int nw = gemm_nw(MODE, WN, PRO);
  const int l = std::max(lds, nw * 32 * 33 * 4);   // the K-split reduction tile of nw waves
  hipLaunchKernelGGL((gemm_kernel<MODE, WN, PRO>), dim3(padded), dim3(64 * nw), l, s, nblocks, t.nprob, tb1,
                     tb2, tb3, Bp, t, bump, ba);
}

using GemmFn = void (*)(const GemmTable&, int, int, int, Counters*, int, hipStream_t);

// Forward stages use Copy / LN / the two policy heads; input-grad stages use LN-bwd and the
// three loss heads.  Only those combinations are instantiated.
template <int WN>
static GemmFn pick_fwd(int pro) {
  switch (pro) {
    case kProCopy: return gl<0, WN, kProCopy>;
    case kProLN: return gl<0, WN, kProLN>;
    case kProGather: return gl<0, WN, kProGather>;
    case kProL0: return gl<0, WN, kProL0>;
    case kProL0G: return gl<0, WN, kProL0G>;
  }
  return nullptr;
}

template <int WN>
static GemmFn pick_bwd(int pro) {
  switch (pro) {
    case kProCopy: return gl<1, WN, kProCopy>;
    case kProLNBwd: return gl<1, WN, kProLNBwd>;
    case kProHeadBwd: return gl<1, WN, kProHeadBwd>;
  }
  return nullptr;
}

static GemmFn pick_4x2(int mode, int pro) {      // kWn4x2: the plain prologues only
  if (mode == 0 && pro == kProCopy) return gl<0, kWn4x2, kProCopy>;
  if (mode == 0 && pro == kProLN) return gl<0, kWn4x2, kProLN>;
  if (mode == 1 && pro == kProCopy) return gl<1, kWn4x2, kProCopy>;
  if (mode == 1 && pro == kProLNBwd) return gl<1, kWn4x2, kProLNBwd>;
  if (mode == 1 && pro == kProHeadBwd) return gl<1, kWn4x2, kProHeadBwd>;
  return nullptr;
}

static GemmFn pick_gemm(int mode, int wn, int pro) {
  if (wn == kWn4x2) return pick_4x2(mode, pro);
  if (mode == 0 && wn == 0) return pick_fwd<0>(pro);
  if (mode == 1 && wn == 0) return pick_bwd<0>(pro);
  if (mode == 0 && wn == 1) return pick_fwd<1>(pro);
  if (mode == 0 && wn == 2) return pick_fwd<2>(pro);
  if (mode == 0 && wn == 4) return pick_fwd<4>(pro);
  if (mode == 1 && wn == 1) return pick_bwd<1>(pro);
  if (mode == 1 && wn == 2) return pick_bwd<2>(pro);
  if (mode == 1 && wn == 4) return pick_bwd<4>(pro);
  return nullptr;
}

// The stage pairs the planner merges (stages.hip merge_gemm_pair): {forward layer of the target twin} x {input-grad
// stage of the unit critic backward} at the widths gemm_wn picks for B = 64..1024.
#define TD3_GEMM2_PAIRS(X)                                            \
  X(0, 1, kProL0, 1, 1, kProCopy) X(0, 0, kProLN, 1, 1, kProLNBwd)     \
  X(0, 0, kProL0, 1, 0, kProCopy) X(0, 0, kProLN, 1, 0, kProLNBwd)     \
  X(0, 4, kProL0, 1, 4, kProCopy) X(0, 1, kProLN, 1, 4, kProLNBwd)     \
  X(0, 4, kProCopy, 1, 4, kProCopy) X(0, 4, kProLN, 1, 4, kProLNBwd)   \
  X(0, 0, kProCopy, 1, 0, kProCopy) X(0, 1, kProL0, 1, 0, kProCopy)    \
  X(0, 0, kProL0, 1, 1, kProCopy) X(0, 1, kProLN, 1, 1, kProLNBwd)     \
  X(0, kWn4x2, kProCopy, 1, kWn4x2, kProCopy) X(0, kWn4x2, kProLN, 1, kWn4x2, kProLNBwd)

int gemm2_supported(int m1, int w1, int p1, int m2, int w2, int p2) {
#define TD3_G2_Q(A, B, C, D, E, F) \
  if (m1 == A && w1 == B && p1 == C && m2 == D && w2 == E && p2 == F) return 1;
  TD3_GEMM2_PAIRS(TD3_G2_Q)
#undef TD3_G2_Q
  return 0;
}

int launch_gemm2(int m1, int w1, int p1, const GemmTable& t1, int nb1, int m2, int w2, int p2, const GemmTable& t2,
                 int nb2, int Bp, int lds, hipStream_t s) {
  const dim3 grid(8 * (((nb1 + 7) >> 3) + ((nb2 + 7) >> 3)));
  auto dir = [](const GemmTable& t, int n, int i) { return t.nprob > i ? t.p[i].tile_begin : n; };
  bool done = false;
#define TD3_G2_L(A, B, C, D, E, F)                                                                           \
  if (!done && m1 == A && w1 == B && p1 == C && m2 == D && w2 == E && p2 == F) {                              \
    hipLaunchKernelGGL((gemm2_kernel<A, B, C, D, E, F>), grid, dim3(64 * kNW), lds, s, nb1, nb2, Bp, t1.nprob, \
                       dir(t1, nb1, 1), dir(t1, nb1, 2), dir(t1, nb1, 3), t2.nprob, dir(t2, nb2, 1),           \
                       dir(t2, nb2, 2), dir(t2, nb2, 3), t1, t2);                                            \
    done = true;                                                                                              \
  }
  TD3_GEMM2_PAIRS(TD3_G2_L)
#undef TD3_G2_L
  if (!done) {
    set_error("launch_gemm2: stage pair (%d,%d,%d)+(%d,%d,%d) not instantiated", m1, w1, p1, m2, w2, p2);
    return -1;
  }
  TD3_HIP(hipGetLastError());
  return 0;
}

// the 16-row fused layer-0 stages: NCT x WK = (5, 2) (80 columns, 10 waves) or (2, 4) (32 columns, 8)
int l0r16_lds_bytes(int Kp, int nct, int wk) {
  return 4 * (2 * 16 * lds_stride(Kp) + 16 * kR16XS + nct * wk * 16 * 17);
}
int launch_l0r16(int nct, int wk, int gather, const GemmTable& t, int nblocks, int Bp, Counters* bump, int bump_actor,
                 hipStream_t s) {
  if (nblocks <= 0) return 0;
  if (Bp % 16 != 0) {
    set_error("launch_l0r16: Bp %d is not a multiple of 16", Bp);
    return -1;
  }
  for (int k = 0; k < t.nprob; ++k) {
    const int K0 = t.p[k].exi[ring_l0::kK0], N0p = t.p[k].exi[ring_l0::kN0p], Kp = t.p[k].Kp;
    if (Kp > 512 || K0 < 1 || K0 > 32 || N0p > 512 || N0p != Kp) {
      set_error("launch_l0r16: unsupported layer-0/1 shape (K0 %d, N0p %d, Kp %d)", K0, N0p, Kp);
      return -1;
    }
  }
  const int padded = (nblocks + 7) & ~7;
  const int tb1 = t.nprob > 1 ? t.p[1].tile_begin : nblocks, tb2 = t.nprob > 2 ? t.p[2].tile_begin : nblocks;
  const int tb3 = t.nprob > 3 ? t.p[3].tile_begin : nblocks;
  const int lds = l0r16_lds_bytes(512, nct, wk);
  const dim3 grid(padded), block(64 * nct * wk);
  if (nct == 5 && wk == 2) {
    if (gather) hipLaunchKernelGGL((l0r16_kernel<5, 2, true>), grid, block, lds, s, nblocks, t.nprob, tb1, tb2, tb3, Bp, t, bump, bump_actor);
    else hipLaunchKernelGGL((l0r16_kernel<5, 2, false>), grid, block, lds, s, nblocks, t.nprob, tb1, tb2, tb3, Bp, t, bump, bump_actor);
  } else if (nct == 6 && wk == 2) {
    if (gather) hipLaunchKernelGGL((l0r16_kernel<6, 2, true>), grid, block, lds, s, nblocks, t.nprob, tb1, tb2, tb3, Bp, t, bump, bump_actor);
    else hipLaunchKernelGGL((l0r16_kernel<6, 2, false>), grid, block, lds, s, nblocks, t.nprob, tb1, tb2, tb3, Bp, t, bump, bump_actor);
  } else if (nct == 2 && wk == 4) {
    if (gather) hipLaunchKernelGGL((l0r16_kernel<2, 4, true>), grid, block, lds, s, nblocks, t.nprob, tb1, tb2, tb3, Bp, t, bump, bump_actor);
    else hipLaunchKernelGGL((l0r16_kernel<2, 4, false>), grid, block, lds, s, nblocks, t.nprob, tb1, tb2, tb3, Bp, t, bump, bump_actor);
  } else {
    set_error("launch_l0r16: no (%d, %d) instantiation", nct, wk);
    return -1;
  }
  TD3_HIP(hipGetLastError());
  return 0;
}

int launch_gemm(int mode, int wn, int pro, const GemmTable& t, int nblocks, int Bp, int lds,
                Counters* bump, int bump_actor, hipStream_t s) {
  if (nblocks <= 0) return 0;
  GemmFn f = pick_gemm(mode, wn, pro);
  if (!f) {
    set_error("launch_gemm: unsupported mode %d wn %d pro %d", mode, wn, pro);
    return -1;
  }
  f(t, nblocks, Bp, lds, bump, bump_actor, s);
  TD3_HIP(hipGetLastError());
  return 0;
}

// The wide-head LDS stage (wide_stage) of row problem p of kind `kind`: its bytes, or 0 when the
// head is narrow (<= kHeadRegs outputs) or its rows cannot be staged (alignment, > 64 KB, no
// transposed W1 copy) and the kernel requests them block by block.
static int wide_head_bytes(int kind, const GemmProb& p) {
  const auto al16 = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
  size_t n = 0;
  if (kind == kRowPolicyHead) {
    const int ad = p.exi[policy_head::kAd], ldw4 = p.exi[policy_head::kLdw4];
    if (ad <= kHeadRegs || ldw4 % 4 || !al16(p.ex[policy_head::kW4])) return 0;
    n = (size_t)ad * ldw4;
  } else if (kind == kRowActorHeadBwd || kind == kRowActorHeadBwdBc) {   // (the BC kind keeps the plain kind's slots)
    namespace ab = actor_head_bwd;
    const int ad = p.exi[ab::kAd], ldw4 = p.exi[ab::kLdw4], ld1 = p.exi[ab::kLdW1T];
    if (ad <= kHeadRegs || !p.ex[ab::kW1T] || ld1 % 4 || ldw4 % 4 || !al16(p.ex[ab::kW1T]) || !al16(p.ex[ab::kW4]))
      return 0;
    n = (size_t)ad * (ld1 + ldw4);
  }
  return n * 4 <= (size_t)kWideStage * 64 * kWideRows * 16 ? (int)(n * 4) : 0;
}

// Marks the wide problems (GemmProb::tile_begin, read by the row kernels as the wide flag) of a
// row table whose problems [0, n1) are of kind k1 and the rest of kind k2; returns the LDS bytes.
// TD3_WIDE_HEADS=0 keeps the block-by-block requests (read per launch: the bit-identity test flips it)
static thread_local int g_last_row_lds = -1;   // td3_debug_row_lds
static int mark_wide(GemmTable& d, int k1, int k2, int n1) {
  const char* e = getenv("TD3_WIDE_HEADS");
  const bool on = !e || atoi(e) != 0;
  int lds = 0;
  for (int i = 0; i < d.nprob; ++i) {
    const int b = on ? wide_head_bytes(i < n1 ? k1 : k2, d.p[i]) : 0;
    d.p[i].tile_begin = b > 0;
    lds = std::max(lds, b);
  }
  g_last_row_lds = lds;
  return lds;
}
int last_row_lds() { return g_last_row_lds; }

template <bool NORM>
static int launch_rows_t(int kind, const GemmTable& d0, int Bp, hipStream_t s) {
  const dim3 grid(Bp / kRowWaves, d0.nprob);
  GemmTable d = d0;
  const int lds = mark_wide(d, kind, kind, d.nprob);
  const dim3 wgrid(Bp / kWideRows, d0.nprob), wblock(64 * kWideRows);
  switch (kind) {
    case kRowPolicyHead:
      if (lds) hipLaunchKernelGGL((row_kernel<kRowPolicyHead, NORM, kWideRows>), wgrid, wblock, lds, s, Bp, d);
      else hipLaunchKernelGGL((row_kernel<kRowPolicyHead, NORM>), grid, dim3(64 * kRowWaves), 0, s, Bp, d);
      break;
    case kRowActorHeadBwd:
      if (lds) hipLaunchKernelGGL((row_kernel<kRowActorHeadBwd, NORM, kWideRows>), wgrid, wblock, lds, s, Bp, d);
      else hipLaunchKernelGGL((row_kernel<kRowActorHeadBwd, NORM>), grid, dim3(64 * kRowWaves), 0, s, Bp, d);
      break;
    case kRowActorHeadBwdBc:   // its kernels live in bc.hip, a code object of their own
      return launch_rows_bc(d, lds, Bp, s);
    case kRowCriticLossP:
      hipLaunchKernelGGL((row_kernel<kRowCriticLossP, NORM>), grid, dim3(64 * kRowWaves), 0, s, Bp, d);
      break;
    case kRowActorLossP: hipLaunchKernelGGL((row_kernel<kRowActorLossP, NORM>), grid, dim3(64 * kRowWaves), 0, s, Bp, d); break;
    case kRowActorHeadBwdP:
      hipLaunchKernelGGL((row_kernel<kRowActorHeadBwdP, NORM>), grid, dim3(64 * kRowWaves), 0, s, Bp, d);
      break;
    default:   // the kinds of launch_rows2 only, and the retired values 1 and 2
      set_error("internal: unknown row kernel %d", kind);
      return -1;
  }
  return 0;
}

// norm is a template parameter of the row kernels: with it a runtime flag, every LayerNorm operand
// load sat in its own basic block and the scheduler issued the row's loads in ~6 dependent rounds.
int launch_rows(int kind, const GemmTable& d, int Bp, hipStream_t s) {
  const int rc = d.p[0].norm ? launch_rows_t<true>(kind, d, Bp, s) : launch_rows_t<false>(kind, d, Bp, s);
  if (rc) return rc;
  TD3_HIP(hipGetLastError());
  return 0;
}

template <bool NORM>
static int launch_rows2_t(int k1, int k2, int n1, const GemmTable& d0, int Bp, hipStream_t s) {
  const dim3 grid(Bp / kRowWaves, d0.nprob);
  GemmTable d = d0;
  const int lds = mark_wide(d, k1, k2, n1);
  if (k1 == kRowPolicyHead && k2 == kRowUnitLoss && lds)
    hipLaunchKernelGGL((row_kernel2<kRowPolicyHead, kRowUnitLoss, NORM, kWideRows>), dim3(Bp / kWideRows, d0.nprob),
                       dim3(64 * kWideRows), lds, s, Bp, n1, d);
  else if (k1 == kRowPolicyHead && k2 == kRowUnitLoss)
    hipLaunchKernelGGL((row_kernel2<kRowPolicyHead, kRowUnitLoss, NORM>), grid, dim3(64 * kRowWaves), 0, s, Bp, n1, d);
  else if (k1 == kRowTargetLoss && k2 == kRowLnBwd)
    hipLaunchKernelGGL((row_kernel2<kRowTargetLoss, kRowLnBwd, NORM>), grid, dim3(64 * kRowWaves), 0, s, Bp, n1, d);
  else {
    set_error("internal: row kinds %d + %d are not instantiated together", k1, k2);
    return -1;
  }
  return 0;
}

int launch_rows2(int kind1, int kind2, int n1, const GemmTable& d, int Bp, hipStream_t s) {
  if (n1 < 1 || n1 >= d.nprob) {
    set_error("internal: launch_rows2 split %d of %d problems", n1, d.nprob);
    return -1;
  }
  const int rc = d.p[0].norm ? launch_rows2_t<true>(kind1, kind2, n1, d, Bp, s)
                             : launch_rows2_t<false>(kind1, kind2, n1, d, Bp, s);
  if (rc) return rc;
  TD3_HIP(hipGetLastError());
  return 0;
}

int launch_heads(const HeadArgs& a, int nprob, hipStream_t s) {
  hipLaunchKernelGGL(head_kernel, dim3(a.Bp / 4, nprob), dim3(256), 0, s, a);
  TD3_HIP(hipGetLastError());
  return 0;
}

int launch_gemv(const GemvArgs& a, int nprob, hipStream_t s) {
  int N = 0;
  for (int k = 0; k < nprob; ++k) N = std::max(N, a.p[k].N);
  if (nprob < 1 || nprob > 2 || a.B < 1 || a.B > kGemvRows) {
    set_error("launch_gemv: %d problems (max 2), %d rows (max %d)", nprob, a.B, kGemvRows);
    return -1;
  }
  for (int k = 0; k < nprob; ++k)
    if (a.p[k].K > 512 || a.p[k].K < 1) {
      set_error("launch_gemv: input width %d (max 512)", a.p[k].K);
      return -1;
    }
  const dim3 grid((N + 15) / 16, nprob);
  if (a.B == 1) hipLaunchKernelGGL(gemv_kernel<1>, grid, dim3(256), 0, s, a);
  else if (a.B == 2) hipLaunchKernelGGL(gemv_kernel<2>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(gemv_kernel<4>, grid, dim3(256), 0, s, a);
  TD3_HIP(hipGetLastError());
  return 0;
}

int launch_act(const ActArgs& a, int nprob, hipStream_t s) {
  const int B = a.g.l1.B;
  int N1 = 0;
  bool ok = nprob >= 1 && nprob <= 2 && B >= 1 && B <= kGemvRows && a.g.K0 >= 1 && a.g.K0 <= kGemv0K &&
            a.g.N0 >= 1 && a.g.N0 <= 512 && a.ctr;
  for (int k = 0; ok && k < nprob; ++k) {
    const GemvProb &p1 = a.g.l1.p[k], &p2 = a.l2[k];
    const HeadProb& hd = a.head[k];
    N1 = std::max(N1, p1.N);
    ok = p1.K == a.g.N0 && p1.N >= 1 && p1.N <= 512 && p2.K == p1.N && p2.X == p1.Y && p2.N >= 1 && p2.N <= p1.N &&
         hd.H3 == p2.Y && hd.K3 == p2.N && hd.nout >= 1 && hd.nout <= 64 && hd.ldw <= 512;
  }
  if (!ok) {
    set_error("launch_act: unsupported query shape (%d problems, %d rows, layer 0 %d -> %d)", nprob, B, a.g.K0, a.g.N0);
    return -1;
  }
  for (int k = 1; k < nprob; ++k)
    if (a.g.l1.p[k].N != N1) {
      set_error("launch_act: networks of one launch need the same layer-1 width");
      return -1;
    }
  const dim3 grid((N1 + 15) / 16, nprob);
  if (a.g.ldw0 < (a.g.K0 <= 32 ? 32 : 64)) {
    set_error("launch_act: layer-0 rows of %d floats (K0 %d)", a.g.ldw0, a.g.K0);
    return -1;
  }
  if (a.g.K0 <= 32) {
    if (B == 1) hipLaunchKernelGGL((act_kernel<1, 8>), grid, dim3(256), 0, s, a);
    else if (B == 2) hipLaunchKernelGGL((act_kernel<2, 8>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((act_kernel<4, 8>), grid, dim3(256), 0, s, a);
  } else {
    if (B == 1) hipLaunchKernelGGL((act_kernel<1, 16>), grid, dim3(256), 0, s, a);
    else if (B == 2) hipLaunchKernelGGL((act_kernel<2, 16>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((act_kernel<4, 16>), grid, dim3(256), 0, s, a);
  }
  TD3_HIP(hipGetLastError());
  return 0;
}

int launch_gemv01(const Gemv01Args& a, int nprob, hipStream_t s) {
  int N = 0;
  for (int k = 0; k < nprob; ++k) N = std::max(N, a.l1.p[k].N);
  if (nprob < 1 || nprob > 2 || a.l1.B < 1 || a.l1.B > kGemvRows || a.K0 < 1 || a.K0 > kGemv0K ||
      a.N0 > 512 || a.N0 < 1) {
    set_error("launch_gemv01: %d problems, %d rows, layer 0 %d -> %d (max 2, %d, %d -> 512)", nprob, a.l1.B, a.K0,
              a.N0, kGemvRows, kGemv0K);
    return -1;
  }
  for (int k = 0; k < nprob; ++k)
    if (a.l1.p[k].K != a.N0 || a.l1.p[k].K > 512) {
      set_error("launch_gemv01: layer-1 input width %d != layer-0 width %d", a.l1.p[k].K, a.N0);
      return -1;
    }
  const dim3 grid((N + 15) / 16, nprob);
  if (a.l1.B == 1) hipLaunchKernelGGL(gemv01_kernel<1>, grid, dim3(256), 0, s, a);
  else if (a.l1.B == 2) hipLaunchKernelGGL(gemv01_kernel<2>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(gemv01_kernel<4>, grid, dim3(256), 0, s, a);
  TD3_HIP(hipGetLastError());
  return 0;
}

int launch_lnbwd_rows(const LnBwdTable& tab, int nprob, int Bp, int norm, hipStream_t s) {
  if (nprob < 1 || nprob > kMaxLnBwd || Bp % (kRowWaves * kLnBwdRB) != 0) {
    set_error("launch_lnbwd_rows: %d problems (max %d), Bp %d (multiple of %d)", nprob, kMaxLnBwd, Bp, kRowWaves * kLnBwdRB);
    return -1;
  }
  if (norm) hipLaunchKernelGGL(lnbwd_rows_kernel<true>, dim3(Bp / (kRowWaves * kLnBwdRB), nprob), dim3(64 * kRowWaves), 0, s, Bp, tab);
  else hipLaunchKernelGGL(lnbwd_rows_kernel<false>, dim3(Bp / (kRowWaves * kLnBwdRB), nprob), dim3(64 * kRowWaves), 0, s, Bp, tab);
  TD3_HIP(hipGetLastError());
  return 0;
}

#ifndef TD3_DW64G
#define TD3_DW64G 1
#endif
int launch_dw(const DwArgs& a, int nblocks, hipStream_t s) {
  if (nblocks <= 0) return 0;
  const dim3 grid((nblocks + 7) & ~7);
  if (a.tile64 && (a.Bp & 63) == 0 && TD3_DW64G) {
    if (a.scaled) hipLaunchKernelGGL(dw64g_kernel<true>, grid, dim3(512), 0, s, a, nblocks);
    else hipLaunchKernelGGL(dw64g_kernel<false>, grid, dim3(512), 0, s, a, nblocks);
  } else if (a.tile64) {
    if (a.scaled) hipLaunchKernelGGL(dw64_kernel<true>, grid, dim3(512), 0, s, a, nblocks);
    else hipLaunchKernelGGL(dw64_kernel<false>, grid, dim3(512), 0, s, a, nblocks);
  } else {
    if (a.scaled) hipLaunchKernelGGL(dw_kernel<true>, grid, dim3(256), 0, s, a, nblocks);
    else hipLaunchKernelGGL(dw_kernel<false>, grid, dim3(256), 0, s, a, nblocks);
  }
  TD3_HIP(hipGetLastError());
  return 0;
}

int launch_dw_split(const DwArgs& a, const DwSplit& k, hipStream_t s) {
  if (k.ntile <= 0) return 0;
  if (k.G <= 0 || (k.G & 7) || k.S <= 0 || (a.Bp & 63) || a.Bp != 64 * k.S || (k.tm != 64 && k.tm != 128) ||
      k.slot < k.tm * k.tm || k.J <= 0) {
    set_error("launch_dw_split: bad split (G %d, S %d, tm %d, slot %d, J %d, Bp %d)", k.G, k.S, k.tm, k.slot,
              k.J, a.Bp);
    return -1;
  }
  if (k.tm == 128) {
    if (a.scaled) hipLaunchKernelGGL((dwsk_kernel<true, true>), dim3(k.G), dim3(512), 0, s, a, k);
    else hipLaunchKernelGGL((dwsk_kernel<false, true>), dim3(k.G), dim3(512), 0, s, a, k);
  } else {
    if (a.scaled) hipLaunchKernelGGL((dwsk_kernel<true, false>), dim3(k.G), dim3(512), 0, s, a, k);
    else hipLaunchKernelGGL((dwsk_kernel<false, false>), dim3(k.G), dim3(512), 0, s, a, k);
  }
  hipLaunchKernelGGL(dwsk_combine_kernel, dim3(4 * k.ntile), dim3(256), 0, s, a, k);
  TD3_HIP(hipGetLastError());
  return 0;
}

int launch_adam_flat(const AdamArgs& a, int64_t n, int polyak, hipStream_t s, const W4Map* w4) {
  auto al16 = [](const float* p) { return ((uintptr_t)p & 15) == 0; };
  if ((n & 3) || !al16(a.P) || !al16(a.G) || !al16(a.M) || !al16(a.V) || (polyak && !al16(a.T))) {
    set_error("launch_adam_flat: the range must be float4-aligned (n %% 4 == 0, 16-B aligned arenas)");
    return -1;
  }
  W4Map w{};
  if (w4 && w4->P4) {
    w = *w4;
    bool ok = w.nmat >= 1 && w.nmat <= 8 && (w.base & 3) == 0 && (!polyak || w.T4);
    for (int m = 0; ok && m < w.nmat; ++m) ok = (w.off[m] & 3) == 0 && w.Kp[m] % 4 == 0;
    if (!ok) {
      set_error("launch_adam_flat: bad k-quad image map");
      return -1;
    }
  }
  const int blocks = (int)std::min<int64_t>((n / 4 + 255) / 256, 2048);
  hipLaunchKernelGGL(adam_flat_kernel, dim3(blocks), dim3(256), 0, s, a, n, polyak, w);
  TD3_HIP(hipGetLastError());
  return 0;
}

int launch_wn(const WnArgs& a, hipStream_t s) {
  if (a.nlin < 1 || a.nlin > kMaxWnLinears || a.rows < 1) {
    set_error("launch_wn: %d linears (max %d), %d rows", a.nlin, kMaxWnLinears, a.rows);
    return -1;
  }
  for (int l = 0; l < a.nlin; ++l)
    if (a.lin[l].K < 1 || a.lin[l].K > 512) {
      set_error("launch_wn: input width %d (max 512)", a.lin[l].K);
      return -1;
    }
  hipLaunchKernelGGL(wn_kernel, dim3((a.rows + 3) / 4), dim3(256), 0, s, a);
  TD3_HIP(hipGetLastError());
  return 0;
}

int launch_local_sum(const LocalSumArgs& a, hipStream_t s) {
  if (a.n < 1 || a.n > kMaxLocalReplicas || a.size < 0) {
    set_error("launch_local_sum: %d replicas (max %d)", a.n, kMaxLocalReplicas);
    return -1;
  }
  const int blocks = (int)std::min<int64_t>((a.size + 255) / 256, 2048);
  if (blocks > 0) hipLaunchKernelGGL(local_sum_kernel, dim3(blocks), dim3(256), 0, s, a);
  TD3_HIP(hipGetLastError());
  return 0;
}

// One thread per 16-B piece (n, k-quad j) of a matrix: a coalesced float4 read along k, a float4
// store into the image (consecutive threads: consecutive j of one row; the stores scatter by Np * 16 B)
__global__ __launch_bounds__(256) void w4_pack_kernel(W4PackArgs a) {
  const int64_t total = a.first[a.nmat];
  for (int64_t e = blockIdx.x * 256 + threadIdx.x; e < (int64_t)a.npair * total; e += (int64_t)gridDim.x * 256) {
    const int pr = (int)(e / total);
    const int64_t q = e - (int64_t)pr * total;
    int m = 0;
    while (m + 1 < a.nmat && q >= a.first[m + 1]) ++m;
    const int64_t pc = q - a.first[m];
    const int kq = a.Kp[m] >> 2;
    const int n = (int)(pc / kq), j = (int)(pc - (int64_t)n * kq);
    const float4 v = gld4(a.src[pr] + a.off[m] + (int64_t)n * a.Kp[m] + 4 * j);
    gst4(a.dst[pr] + a.off[m] + ((int64_t)j * a.Np[m] + n) * 4, v);
  }
}

int launch_w4_pack(const W4PackArgs& a, hipStream_t s) {
  if (a.nmat < 1 || a.nmat > kMaxW4Mats || a.npair < 1 || a.npair > 2) {
    set_error("launch_w4_pack: %d matrices, %d arena pairs", a.nmat, a.npair);
    return -1;
  }
  for (int m = 0; m < a.nmat; ++m)
    if (a.Kp[m] % 4 || a.first[m + 1] - a.first[m] != (int64_t)a.Np[m] * (a.Kp[m] / 4)) {
      set_error("launch_w4_pack: matrix %d ranges", m);
      return -1;
    }
  const int64_t n = (int64_t)a.npair * a.first[a.nmat];
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 2048);
  hipLaunchKernelGGL(w4_pack_kernel, dim3(blocks), dim3(256), 0, s, a);
  TD3_HIP(hipGetLastError());
  return 0;
}

__global__ void pack_kernel(const float* __restrict__ src, int cols, int B, int Bp, float* d1, int ld1,
                            int c1, float* d2, int ld2, int c2, float* d3, int ld3, int c3) {
  const int row = blockIdx.x;
  for (int c = threadIdx.x; c < cols; c += blockDim.x) {
    const float v = row < B ? src[(size_t)row * cols + c] : 0.f;
    if (d1) d1[(size_t)row * ld1 + c1 + c] = v;
    if (d2) d2[(size_t)row * ld2 + c2 + c] = v;
    if (d3) d3[(size_t)row * ld3 + c3 + c] = v;
  }
  (void)Bp;
}

int launch_pack(const float* src, int cols, int B, int Bp, std::initializer_list<PackDst> dst, hipStream_t s) {
  if (dst.size() < 1 || dst.size() > 3) {
    set_error("launch_pack: %zu destinations", dst.size());
    return -1;
  }
  PackDst d[3] = {};
  for (size_t k = 0; k < dst.size(); ++k) d[k] = dst.begin()[k];
  hipLaunchKernelGGL(pack_kernel, dim3(Bp), dim3(64), 0, s, src, cols, B, Bp, d[0].p, d[0].ld, d[0].col, d[1].p,
                     d[1].ld, d[1].col, d[2].p, d[2].ld, d[2].col);
  TD3_HIP(hipGetLastError());
  return 0;
}

// One thread per (row, 4 action columns): the Philox counter of the quad is drawn once, the OU state
// and the action are read and written in place (utils/noise.py:15-19 order: drift, + diffusion, + X).
__global__ __launch_bounds__(256) void explore_kernel(ExploreArgs a) {
  const int ad4 = (a.ad + 3) >> 2;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)a.n * ad4) return;
  const int row = (int)(t / ad4), q = (int)(t - (int64_t)row * ad4);
  const float* pi = a.pi + (size_t)row * a.ldp;
  const size_t o = (size_t)row * a.ad;
  if (a.plain) {
    for (int c = 4 * q; c < min(4 * q + 4, a.ad); ++c) a.action_out[o + c] = pi[c];
    return;
  }
  float z[4];
  if (!a.inject_z) philox_normal4(a.seed, a.step, kStreamExplore, (uint32_t)t, z);
  const bool rst = a.reset && a.reset[row] != 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = 4 * q + j;
    if (c >= a.ad) break;
    const float zz = a.inject_z ? a.inject_z[o + c] : z[j];
    float e;
    if (a.x) {
      const float X = rst ? a.mu : a.x[o + c];
      e = X + (a.theta * (a.mu - X) + a.sigma * zz);
      a.x[o + c] = e;
    } else {
      e = a.sigma * zz;
    }
    if (a.z_out) a.z_out[o + c] = zz;
    a.action_out[o + c] = fminf(fmaxf(pi[c] + e, -a.max_action), a.max_action);
  }
}

int launch_explore(const ExploreArgs& a, hipStream_t s) {
  if (a.n < 1 || a.ad < 1 || !a.pi || !a.action_out) {
    set_error("launch_explore: %d rows x %d columns", a.n, a.ad);
    return -1;
  }
  const int64_t threads = (int64_t)a.n * ((a.ad + 3) >> 2);
  hipLaunchKernelGGL(explore_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, a);
  TD3_HIP(hipGetLastError());
  return 0;
}

// Polyak over a whole arena (the sharded data-parallel step, behind its all-gather) that also
// refreshes the k-quad images of the weight matrices from the gathered P and the new T (w.base = 0)
__global__ __launch_bounds__(256) void polyak_w4_kernel(float* T, const float* P, int64_t n, float tau, float omt,
                                                        W4Map w) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (n >> 2); i += (int64_t)gridDim.x * 256) {
    const int64_t e = 4 * i;
    const float4 p4 = gld4(P + e), t4 = gld4(T + e);
    const float4 o = make_float4(tau * p4.x + omt * t4.x, tau * p4.y + omt * t4.y, tau * p4.z + omt * t4.z,
                                 tau * p4.w + omt * t4.w);
    gst4(T + e, o);
    for (int m = 0; m < w.nmat; ++m) {
      const int64_t r = e - w.off[m];
      if (r < 0 || r >= (int64_t)w.Np[m] * w.Kp[m]) continue;
      const int nn = (int)(r / w.Kp[m]), kq = (int)(r - (int64_t)nn * w.Kp[m]) >> 2;
      const int64_t iq = w.off[m] + ((int64_t)kq * w.Np[m] + nn) * 4;
      pst4(w.P4 + iq, p4);
      pst4(w.T4 + iq, o);
      break;
    }
  }
}

int launch_polyak_w4(float* T, const float* P, int64_t n, float tau, const W4Map& w, hipStream_t s) {
  if ((n & 3) || ((uintptr_t)T & 15) || ((uintptr_t)P & 15) || !w.P4 || !w.T4 || w.base != 0 || w.nmat < 1 ||
      w.nmat > 8) {
    set_error("launch_polyak_w4: float4-aligned whole arena and an image map required");
    return -1;
  }
  const int blocks = (int)std::min<int64_t>((n / 4 + 255) / 256, 2048);
  const float omt = (float)(1.0 - (double)tau);
  hipLaunchKernelGGL(polyak_w4_kernel, dim3(blocks), dim3(256), 0, s, T, P, n, tau, omt, w);
  TD3_HIP(hipGetLastError());
  return 0;
}

int launch_polyak_flat(float* T, const float* P, int64_t n, float tau, hipStream_t s) {
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 2048);
  const float omt = (float)(1.0 - (double)tau);
  hipLaunchKernelGGL(polyak_flat_kernel, dim3(blocks), dim3(256), 0, s, T, P, n, tau, omt);
  TD3_HIP(hipGetLastError());
  return 0;
}

template <int WN>
static int set_attr_all() {
  const int max_lds = 160 * 1024;
#define TD3_ATTR(MODE, PRO)                                                                   \
  TD3_HIP(hipFuncSetAttribute((const void*)gemm_kernel<MODE, WN, PRO>,                        \
                              hipFuncAttributeMaxDynamicSharedMemorySize, max_lds))
  TD3_ATTR(0, kProCopy);
  TD3_ATTR(0, kProLN);
  TD3_ATTR(0, kProGather);
  TD3_ATTR(0, kProL0);
  TD3_ATTR(0, kProL0G);
  TD3_ATTR(1, kProCopy);
  TD3_ATTR(1, kProLNBwd);
  TD3_ATTR(1, kProHeadBwd);
#undef TD3_ATTR
  return 0;
}

int kernels_init() {
#define TD3_G2_A(A, B, C, D, E, F)                                                               \
  TD3_HIP(hipFuncSetAttribute((const void*)gemm2_kernel<A, B, C, D, E, F>,                        \
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  TD3_GEMM2_PAIRS(TD3_G2_A)
#undef TD3_G2_A
  int rc = set_attr_all<0>();
  if (!rc) rc = set_attr_all<1>();
  if (!rc) rc = set_attr_all<2>();
  if (!rc) rc = set_attr_all<4>();
  if (rc) return rc;
  for (const void* f : {(const void*)gemm_kernel<0, kWn4x2, kProCopy>, (const void*)gemm_kernel<0, kWn4x2, kProLN>,
                        (const void*)gemm_kernel<1, kWn4x2, kProCopy>, (const void*)gemm_kernel<1, kWn4x2, kProLNBwd>,
                        (const void*)gemm_kernel<1, kWn4x2, kProHeadBwd>,
                        (const void*)l0r16_kernel<5, 2, true>, (const void*)l0r16_kernel<5, 2, false>,
                        (const void*)l0r16_kernel<2, 4, true>, (const void*)l0r16_kernel<2, 4, false>,
                        (const void*)l0r16_kernel<6, 2, true>, (const void*)l0r16_kernel<6, 2, false>})
    TD3_HIP(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  return 0;
}

}  // namespace td3

#ifdef TD3_TL
// Experiment builds only: copy the gemm-stage timeline of the last launch (n workgroups).
extern "C" int td3_tl_read(unsigned long long* out, int n) {
  if (n > 8192) n = 8192;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(td3::td3_tl), (size_t)n * 8 * 8, 0, hipMemcpyDeviceToHost) != hipSuccess)
    return -1;
  return 0;
}
extern "C" int td3_clk_read(unsigned long long* out, int n) {
  if (n > 8192) n = 8192;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(td3::td3_clk), (size_t)n * 2 * 8, 0, hipMemcpyDeviceToHost) != hipSuccess)
    return -1;
  return 0;
}
extern "C" int td3_clk_sum_read(unsigned long long* out, int clear) {
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(td3::td3_clk_sum), 16, 0, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  static const unsigned long long z[2] = {0, 0};
  if (clear && hipMemcpyToSymbol(HIP_SYMBOL(td3::td3_clk_sum), z, 16, 0, hipMemcpyHostToDevice) != hipSuccess) return -1;
  return 0;
}
extern "C" int td3_tl_clear() {
  static unsigned long long z[8192][8];
  return hipMemcpyToSymbol(HIP_SYMBOL(td3::td3_tl), z, sizeof(z), 0, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}
#endif
