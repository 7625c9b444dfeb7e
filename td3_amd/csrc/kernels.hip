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
//
// This file is the one translation unit of the step's kernels; the code is in the parts below,
// one concern each.  The split is textual on purpose: the kernels share one code object, and the
// order of the parts (and of the launchers inside kernels_launch.h) fixes where each kernel lands
// in it, which is worth a few tenths of a percent of the step ("A code object of its
// own").  Add a part here, in place; do not compile a part on its own or reorder the list.
#include <math.h>
#include <stdlib.h>

#include "dev.h"
#include "kernels.h"
#include "row_actor.h"          // lds_barrier, RowCtx, the wide-head stage, row_actor_head_bwd (shared with bc.hip)

#include "kernels_timeline.h"   // TD3_TL marks and clocks (experiment builds), their host readers
#include "kernels_prologues.h"  // lds_put_row, Ctx, pro_copy / ln / lnbwd / headbwd / gather, the l0_* helpers
#include "kernels_rows.h"       // row heads and losses, row_lnbwd, row_dispatch, row_kernel, row_kernel2
#include "kernels_gemm.h"       // load_chunk*, gemm_body, gemm_kernel, the dual launch gemm2_kernel
#include "kernels_l0r16.h"      // l0r16_kernel: fused layers 0-1 on 16-row tiles
#include "kernels_query.h"      // head_kernel, gemv_kernel, gemv01_kernel, act_kernel (select_action / eval_q)
#include "kernels_dw.h"         // lnbwd_rows_kernel, Adam / Polyak state helpers, dw / dw64 / dw64g_kernel
#include "kernels_dwsk.h"       // split-K dW: dwsk_kernel, dwsk_combine_kernel
#include "kernels_optim.h"      // adam_flat / local_sum / polyak_flat kernels, wn_kernel
#include "kernels_launch.h"     // every launcher, w4_pack / pack / explore / polyak_w4 kernels, kernels_init
