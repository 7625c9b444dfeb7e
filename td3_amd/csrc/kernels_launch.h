// Part of kernels.hip: the host launchers of every kernel of the other parts, the four small kernels defined
// among them (w4_pack, pack, explore, polyak_w4) and kernels_init.  Needs all the parts before it.
//
// The launchers stay together and in this order on purpose.  The compiler emits template kernels in the order
// the host code first references them, and where a kernel lands in the code object is worth a few tenths of
// a percent of the step ("A code object of its own").  Moving a launcher next to its kernels, or
// reordering the references inside one, moves kernels: compare the device assembly before and after.
#pragma once
#include <stdlib.h>

#include "dev.h"
#include "kernels.h"
#include "row_actor.h"
#include "kernels_timeline.h"
#include "kernels_prologues.h"
#include "kernels_rows.h"
#include "kernels_gemm.h"
#include "kernels_l0r16.h"
#include "kernels_query.h"
#include "kernels_dw.h"
#include "kernels_dwsk.h"
#include "kernels_optim.h"

namespace td3 {

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

// Every kernel launched with dynamic LDS may ask for the whole 160 KB of a CU; above 64 KB a launch fails
// unless kernels_init raised the kernel's limit.  So each family of such instantiations is ONE list, expanded
// by the code that launches it and by the code that raises its limit: a kernel cannot be in one and not the other.
constexpr int kMaxDynLds = 160 * 1024;
static hipError_t allow_max_lds(const void* kernel) {
  return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynLds);
}

// Forward stages use Copy / LN / the two policy heads; input-grad stages use LN-bwd and the
// three loss heads.  Only those combinations are instantiated (wn 0, 1, 2, 4: pick_gemm, kernels_init).
#define TD3_FWD_PROS(X) X(kProCopy) X(kProLN) X(kProGather) X(kProL0) X(kProL0G)
#define TD3_BWD_PROS(X) X(kProCopy) X(kProLNBwd) X(kProHeadBwd)
// kWn4x2: (mode, prologue), the plain prologues only
#define TD3_4X2_KERNELS(X) X(0, kProCopy) X(0, kProLN) X(1, kProCopy) X(1, kProLNBwd) X(1, kProHeadBwd)

template <int WN>
static GemmFn pick_fwd(int pro) {
  switch (pro) {
#define TD3_PICK(PRO) case PRO: return gl<0, WN, PRO>;
    TD3_FWD_PROS(TD3_PICK)
#undef TD3_PICK
  }
  return nullptr;
}

template <int WN>
static GemmFn pick_bwd(int pro) {
  switch (pro) {
#define TD3_PICK(PRO) case PRO: return gl<1, WN, PRO>;
    TD3_BWD_PROS(TD3_PICK)
#undef TD3_PICK
  }
  return nullptr;
}

static GemmFn pick_4x2(int mode, int pro) {
#define TD3_PICK(MODE, PRO) if (mode == MODE && pro == PRO) return gl<MODE, kWn4x2, PRO>;
  TD3_4X2_KERNELS(TD3_PICK)
#undef TD3_PICK
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

// the 16-row fused layer-0 stages: NCT x WK = (5, 2) (80 columns, 10 waves), (6, 2) or (2, 4) (32 columns, 8),
// each with and without the ring gather
#define TD3_L0R16_SHAPES(X) X(5, 2) X(6, 2) X(2, 4)
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
  bool done = false;
#define TD3_L0R16_L(NCT, WK)                                                                                        \
  if (!done && nct == NCT && wk == WK) {                                                                            \
    if (gather) hipLaunchKernelGGL((l0r16_kernel<NCT, WK, true>), grid, block, lds, s, nblocks, t.nprob, tb1, tb2,  \
                                   tb3, Bp, t, bump, bump_actor);                                                   \
    else hipLaunchKernelGGL((l0r16_kernel<NCT, WK, false>), grid, block, lds, s, nblocks, t.nprob, tb1, tb2, tb3,   \
                            Bp, t, bump, bump_actor);                                                               \
    done = true;                                                                                                    \
  }
  TD3_L0R16_SHAPES(TD3_L0R16_L)
#undef TD3_L0R16_L
  if (!done) {
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
  } else if (kind == kRowActorHeadBwd || kind == kRowActorHeadBwdBc ||
             kind == kRowActorHeadBwdBcF) {   // (the BC kinds keep the plain kind's slots)
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
    case kRowActorHeadBwdBcF:  // and these in bcf.hip
      return launch_rows_bcf(d, lds, Bp, s);
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
  const int R = gemv_rows(a.B);
  if (R == 1) hipLaunchKernelGGL(gemv_kernel<1>, grid, dim3(256), 0, s, a);
  else if (R == 2) hipLaunchKernelGGL(gemv_kernel<2>, grid, dim3(256), 0, s, a);
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
  const int R = gemv_rows(B), KQ = act_kq(a.g.K0);
  if (a.g.ldw0 < 4 * KQ) {
    set_error("launch_act: layer-0 rows of %d floats (K0 %d)", a.g.ldw0, a.g.K0);
    return -1;
  }
  if (KQ == 8) {
    if (R == 1) hipLaunchKernelGGL((act_kernel<1, 8>), grid, dim3(256), 0, s, a);
    else if (R == 2) hipLaunchKernelGGL((act_kernel<2, 8>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((act_kernel<4, 8>), grid, dim3(256), 0, s, a);
  } else {
    if (R == 1) hipLaunchKernelGGL((act_kernel<1, 16>), grid, dim3(256), 0, s, a);
    else if (R == 2) hipLaunchKernelGGL((act_kernel<2, 16>), grid, dim3(256), 0, s, a);
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
  const int R = gemv_rows(a.l1.B);
  if (R == 1) hipLaunchKernelGGL(gemv01_kernel<1>, grid, dim3(256), 0, s, a);
  else if (R == 2) hipLaunchKernelGGL(gemv01_kernel<2>, grid, dim3(256), 0, s, a);
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

// The flat optimizer launches' argument check (launch_adam_flat here, launch_adam_flat_clip in clip.hip): the
// range float4-aligned, the image map (w4 nullable, or without P4: no images) sound; out: the map to pass, the grid
int adam_flat_args(const char* who, const AdamArgs& a, int64_t n, int polyak, const W4Map* w4, W4Map* out,
                   int* blocks) {
  auto al16 = [](const float* p) { return ((uintptr_t)p & 15) == 0; };
  if ((n & 3) || !al16(a.P) || !al16(a.G) || !al16(a.M) || !al16(a.V) || (polyak && !al16(a.T))) {
    set_error("%s: the range must be float4-aligned (n %% 4 == 0, 16-B aligned arenas)", who);
    return -1;
  }
  W4Map w{};
  if (w4 && w4->P4) {
    w = *w4;
    bool ok = w.nmat >= 1 && w.nmat <= 8 && (w.base & 3) == 0 && (!polyak || w.T4);
    for (int m = 0; ok && m < w.nmat; ++m) ok = (w.off[m] & 3) == 0 && w.Kp[m] % 4 == 0;
    if (!ok) {
      set_error("%s: bad k-quad image map", who);
      return -1;
    }
  }
  *out = w;
  *blocks = (int)std::min<int64_t>((n / 4 + 255) / 256, 2048);
  return 0;
}

int launch_adam_flat(const AdamArgs& a, int64_t n, int polyak, hipStream_t s, const W4Map* w4) {
  W4Map w;
  int blocks;
  TD3_RC(adam_flat_args("launch_adam_flat", a, n, polyak, w4, &w, &blocks));
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
#define TD3_ATTR_FWD(PRO) TD3_HIP(allow_max_lds((const void*)gemm_kernel<0, WN, PRO>));
#define TD3_ATTR_BWD(PRO) TD3_HIP(allow_max_lds((const void*)gemm_kernel<1, WN, PRO>));
  TD3_FWD_PROS(TD3_ATTR_FWD)
  TD3_BWD_PROS(TD3_ATTR_BWD)
#undef TD3_ATTR_FWD
#undef TD3_ATTR_BWD
  return 0;
}

int kernels_init() {
#define TD3_G2_A(A, B, C, D, E, F) TD3_HIP(allow_max_lds((const void*)gemm2_kernel<A, B, C, D, E, F>));
  TD3_GEMM2_PAIRS(TD3_G2_A)
#undef TD3_G2_A
  int rc = set_attr_all<0>();
  if (!rc) rc = set_attr_all<1>();
  if (!rc) rc = set_attr_all<2>();
  if (!rc) rc = set_attr_all<4>();
  if (rc) return rc;
#define TD3_4X2_A(MODE, PRO) TD3_HIP(allow_max_lds((const void*)gemm_kernel<MODE, kWn4x2, PRO>));
  TD3_4X2_KERNELS(TD3_4X2_A)
#undef TD3_4X2_A
#define TD3_L0R16_A(NCT, WK)                                        \
  TD3_HIP(allow_max_lds((const void*)l0r16_kernel<NCT, WK, true>)); \
  TD3_HIP(allow_max_lds((const void*)l0r16_kernel<NCT, WK, false>));
  TD3_L0R16_SHAPES(TD3_L0R16_A)
#undef TD3_L0R16_A
  return 0;
}

}  // namespace td3
