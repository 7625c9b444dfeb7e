// Part of kernels.hip: the batch-row GEMM stage: load_chunk*, gemm_body, gemm_kernel and the dual launch
// gemm2_kernel that runs two stages' tiles in one grid.
// Needs the prologues and Ctx of kernels_prologues.h, which form each tile's input rows.
#pragma once
#include "dev.h"
#include "kernels.h"
#include "row_actor.h"
#include "kernels_prologues.h"

namespace td3 {

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

}  // namespace td3
