// Problem descriptors of the TD3 step kernels (kernel-argument tables, read with scalar
// loads by every workgroup; pointers are fixed for the handle's life so the launches can
// be captured once into a hipGraph and replayed).
#pragma once
#include <initializer_list>

#include "common.h"

#ifndef TD3_GEMM_WAVES
#define TD3_GEMM_WAVES 8
#endif

namespace td3 {

// Waves per GEMM-stage workgroup (K of a 32-row x 32*WN tile is split over kGemmWaves / WN waves).
constexpr int kGemmWaves = TD3_GEMM_WAVES;

// ------------------------------------------------------------------ batch-row GEMM stage
// C[Bp x Nout] = epi( pro(A)[Bp x Kp] * B[Kp x Nout] )
//   MODE 0 (forward layer):  B[k][j] = W[n0+j][k]   (W row-major [Nout][Kp], torch Linear layout)
//   MODE 1 (input grad):     B[k][j] = W[k][n0+j]   (W row-major [Kp][Nout]; dX = dZ * W)
// The prologue builds the workgroup's 32 A rows (full Kp) in LDS; its kind is a
// template parameter of the kernel (one kind per launch):
enum Pro : int {
  kProCopy = 0,        // A rows as stored (network inputs, dZ rows from a row kernel)
  kProLN = 1,          // LayerNorm of the previous hidden layer (ReLU -> LN order)
  kProLNBwd = 2,       // dZ = relu'(LN_bwd(dU)) of the following layer
  kProGather = 3,      // replay-ring rows of this step: Philox index draw + record read (the
                       // sample() of my_replay_buffer.py:119-128 fused into the first layer)
  kProL0 = 4,          // layer 0 (input width <= 32) recomputed for the workgroup's 32 rows on
                       // MFMA, ReLU, LayerNorm: the A rows of layer 1 (one launch for two layers)
  kProL0G = 5,         // kProL0 with the input rows sampled from the replay ring (as kProGather)
  kProHeadBwd = 6,     // the actor loss's Q1 head backward (dU3 = -1/B w4 on every row): dZ3 =
                       // relu'(LN3_bwd(dU3)) with LN3's statistics from the H3 rows themselves
                       // (operands: head_bwd_pro)
};
constexpr int kL0XS = 36;        // LDS row stride of the staged layer-0 input rows

// Row kernels (one batch row per wave) between the GEMM stages; they reuse GemmProb's
// ex / exi / exf operand slots (one slot namespace per kind below).
enum RowKind : int {
  kRowPolicyHead = 0,    // a' = clamp(ma*tanh(head(LN3(H3))) + clip(eps)) or pi = ma*tanh(...)
  // 1 and 2 stay unused (retired kinds): the values are template arguments, i.e. part of the
  // kernel names in profiles/ and of the Stage names
  kRowActorHeadBwd = 3,  // dQ1/da (Q1 LN1 bwd, W1 action cols), tanh bwd, actor head + LN3 bwd
  kRowCriticLossP = 4,   // TD3_particles: the same over A Q outputs, optional CDQ
  kRowActorLossP = 5,    // TD3_particles: -mean over B*A
  kRowActorHeadBwdP = 6, // TD3_particles: dQ1/da through lnorm1, tanh bwd, actor head + LN3 bwd
  // The twin critic's backward runs on UNIT loss gradients (dL/dQ_r = 1): every per-row
  // gradient vector of the MLP backward is linear in the row's dL/dQ_r, so the dX chain does not
  // wait for the clipped double-Q target; the dW stage scales row r by g_r = 2/B (Q_r - y_r).
  kRowUnitLoss = 7,      // Q_j head, LN3 of Q_j, unit dU3 / dZ3 rows of Q_j
  kRowTargetLoss = 8,    // target heads -> y (:140-142), g_j = 2/B (Q_j - y) (:148), squared errors
  kRowLnBwd = 9,         // dZ = relu'(LN_bwd(dU)) of full rows (layer 0, no GEMM follows)
  kRowActorHeadBwdBc = 10,   // kRowActorHeadBwd of the TD3+BC actor loss: dL/dpi = lambda dQ1/da + 2/(B A) (pi - a)
  kRowActorHeadBwdBcF = 11,  // the same with the BC term on the kept rows only (td3_set_bc_filter): rows r < n_d,
                             // and with the Q-filter those with Q1(s, a) > Q1(s, pi); 2/(n_d A) in place of 2/(B A)
};

// ------------------------------------------------------------------ operand slots
// GemmProb::ex (pointers) / exi (ints) / exf (floats) by kind: every kind names its slots here, once
// for the kernels (kernels.hip) and the host planner (stages.hip, step.hip).  Per kind: pointer slots, integer
// slots, float slots, each enum closed by its slot count.  "x3" / "x2" slots are consecutive, one
// per network, indexed kName + n.
constexpr int kMaxEx = 24;
constexpr int kMaxExi = 12, kMaxExf = 4;
#define TD3_SLOTS_FIT(kind)                                                                        \
  static_assert(kind::kNumPtr <= kMaxEx && kind::kNumInt <= kMaxExi && kind::kNumFlt <= kMaxExf, \
                #kind ": operand slots past GemmProb's arrays")

// LayerNorm 3 + head: the leading slots of kRowPolicyHead, kRowActorLossP and kRowUnitLoss
namespace ln3_head {
enum : int {
  kH3 = 0,       // last hidden rows (post-ReLU) [Bp][ld3]
  kGamma3 = 1,   // LN3 affine
  kBeta3 = 2,
  kW4 = 3,       // head weight rows [nout][ldw4]
  kB4 = 4,       // head bias
  kNumPtr
};
enum : int {
  kK3 = 0,       // real width of H3
  kLd3 = 1,      // its row stride
  kNumInt
};
}  // namespace ln3_head

// kRowPolicyHead (row_policy_head)
namespace policy_head {
using namespace ln3_head;
enum : int {
  kNoise = ln3_head::kNumPtr,   // smoothing noise [Bp][ldn]: read (kGenNoise = 0) or written (drawn here)
  kOut,          // out: critic input rows, the action at columns kActCol.. (ld kLdOut)
  kTanh,         // out: tanh of the head [Bp][32]
  kU3,           // out: LN3 output rows
  kStats3,       // out: LN3 (mean, rstd) [2][Bp]
  kOut2,         // out, nullable: second critic-input buffer for the action (ld kLdOut)
  kNumPtr
};
enum : int {
  kLdw4 = ln3_head::kNumInt,
  kLdOut,
  kGenNoise,     // 1: draw the noise (Philox), 0: read kNoise
  kAd,           // action width
  kActCol,       // first action column of the out rows
  kLdNoise,
  kTarget,       // 1: target smoothing; 0: policy
  kClamp,        // clamp a' to +-max_action (TD3_featured :135-137; TD3_particles :179-181 has none)
  kNumInt
};
enum : int {
  kMaxAction = 0,   // 1 for TD3_particles: tanh output (:68)
  kPolicyNoise,
  kNoiseClip,
  kNumFlt
};
}  // namespace policy_head
TD3_SLOTS_FIT(policy_head);

// kRowUnitLoss (row_unit_loss); Aout = unit dZ3_j
namespace unit_loss {
using namespace ln3_head;
enum : int {
  kQ = ln3_head::kNumPtr,   // out: Q_j [Bp]
  kU3,           // out: LN3 output rows of Q_j
  kStats3,       // out: LN3 (mean, rstd) [2][Bp]
  kDU3,          // out: unit dU3_j rows (w4)
  kNumPtr
};
enum : int { kNumInt = ln3_head::kNumInt, kNumFlt = 0 };
}  // namespace unit_loss
TD3_SLOTS_FIT(unit_loss);

// kRowActorLossP (row_actor_loss_p); Aout = dZ3
namespace actor_loss_p {
using namespace ln3_head;
enum : int {
  kQ = ln3_head::kNumPtr,   // out: Q [Bp][32]
  kNumPtr
};
enum : int {
  kNq = ln3_head::kNumInt,   // Q outputs per row
  kLdw4,
  kNumInt
};
enum : int {
  kGradScale = 0,   // -1/(B*nq)
  kNumFlt
};
}  // namespace actor_loss_p
TD3_SLOTS_FIT(actor_loss_p);

// kProHeadBwd (pro_headbwd): H3, the LN3 affine and the widths are the GEMM's own A / lng / lnb /
// Kreal / Kp; the head comes in the slots it has in ln3_head
namespace head_bwd_pro {
using ln3_head::kW4;
using ln3_head::kB4;
enum : int {
  kQ = ln3_head::kNumPtr,   // out: Q1 [Bp] (n-tile 0)
  kNumPtr
};
enum : int { kNumInt = 0 };
enum : int {
  kGradScale = 0,   // dL/dQ of a live row: -1/B
  kNumFlt
};
}  // namespace head_bwd_pro
TD3_SLOTS_FIT(head_bwd_pro);

// Shared by kRowActorHeadBwd and kRowActorHeadBwdP: the actor's head / LN3 operands and outputs
// (Aout = dZ3 of the actor); slots 0..4 / 0..2 are the kind's own
namespace actor_bwd {
enum : int {
  kTanh = 5,     // tanh of the actor head [Bp][32]
  kW4,           // actor head weight rows
  kH3,           // actor H3 rows
  kStats3,       // actor LN3 (mean, rstd)
  kGamma3,       // actor LN3 gamma
  kDZ4,          // out: dZ4 of the actor (ld 32)
  kDU3,          // out: dU3 of the actor
  kNumPtr
};
enum : int {
  kActCol = 3,   // first action column of the Q1 input rows
  kAd,           // action width
  kK3,
  kLd3,
  kLdw4,
  kNumInt
};
enum : int {
  kMaxAction = 0,   // scale of the policy output
  kNumFlt
};
}  // namespace actor_bwd

// kRowActorHeadBwd (row_actor_head_bwd): dQ1/da through Q1's layer 0
namespace actor_head_bwd {
using namespace actor_bwd;
enum : int {
  kDU0 = 0,      // dU0 of Q1(s, pi)
  kH0,           // H0 of Q1(s, pi)
  kStats0,       // LN0 (mean, rstd) of Q1
  kGamma0,       // LN0 gamma of Q1
  kW1,           // layer-0 weight of Q1 [N0][ldw1]: the action columns are read
  kW1T = actor_bwd::kNumPtr,   // nullable: those columns transposed [ad][kLdW1T] (ring_l0::kTCopy wrote them)
  kNumPtr
};
enum : int {
  kK0 = 0,       // real width of H0
  kLd0,
  kLdw1,
  kLdW1T = actor_bwd::kNumInt,
  kNumInt
};
}  // namespace actor_head_bwd
TD3_SLOTS_FIT(actor_head_bwd);

// kRowActorHeadBwdBc (row_actor_head_bwd<.., BC = true>): kRowActorHeadBwd's operands, then those of the
// behaviour-cloning term (td3_set_bc, include/td3.h)
namespace actor_head_bwd_bc {
using namespace actor_head_bwd;
enum : int {
  kQv = actor_head_bwd::kNumPtr,   // Q1(s, pi(s)) of the rows [Bp] (pro_headbwd wrote them): lambda = alpha / mean |Q|
  kAct,          // the batch's [s | a] rows (ld kLdAct): the stored action at columns kActCol..
  kRowSe,        // out: sum over o of (pi_o - a_o)^2 of a live row, 0 for a pad row [Bp]
  kLam,          // out (row 0, lane 0): (lambda, mean |Q|), 2 floats
  kNumPtr
};
enum : int {
  kLdAct = actor_head_bwd::kNumInt,
  kNumInt
};
enum : int {
  kAlpha = actor_bwd::kNumFlt,
  kBcScale,      // 2/(B A)
  kNumFlt
};
}  // namespace actor_head_bwd_bc
TD3_SLOTS_FIT(actor_head_bwd_bc);

// kRowActorHeadBwdBcF (row_actor_head_bwd<.., BC = kBcFiltered>): kRowActorHeadBwdBc's operands (kBcScale is
// not read: the wave forms 2/(n_d A) from the kNDemo word), then those of the row mask (td3_set_bc_filter)
namespace actor_head_bwd_bcf {
using namespace actor_head_bwd_bc;
enum : int {
  kQ1sa = actor_head_bwd_bc::kNumPtr,   // Q1(s, a) of the rows [Bp] (the critic phase's kRowUnitLoss wrote them)
  kNDemo,        // one int32 word the plan owns: n_d, the candidate rows [0, n_d) of this step
  kKeep,         // out: 1.0f for a row whose BC term is kept, 0.0f for every other row (pad rows too) [Bp]
  kNumPtr
};
enum : int {
  kQFilter = actor_head_bwd_bc::kNumInt,   // 1: keep a candidate row only while Q1(s, a) > Q1(s, pi)
  kNumInt
};
enum : int { kNumFlt = actor_head_bwd_bc::kNumFlt };
}  // namespace actor_head_bwd_bcf
TD3_SLOTS_FIT(actor_head_bwd_bcf);

// kRowActorHeadBwdP (row_actor_head_bwd_p): dQ1/da through lnorm1 of the Q1 input
namespace actor_head_bwd_p {
using namespace actor_bwd;
enum : int {
  kDUin = 0,     // grad of the lnorm1 output of Q1(s, pi)
  kXin,          // lnorm1 input rows
  kStatsIn,      // lnorm1 (mean, rstd)
  kGammaIn,      // lnorm1 gamma
};
enum : int {
  kKin = 0,      // real input width
  kLdIn,
};
}  // namespace actor_head_bwd_p
TD3_SLOTS_FIT(actor_head_bwd_p);

// kRowCriticLossP (row_critic_loss_p); x3 = (target q1, target q2 (= target q1 without CDQ), online q_j);
// Aout = dZ3_j
namespace critic_loss_p {
enum : int {
  kH3 = 0,       // x3
  kGamma3 = 3,   // x3
  kBeta3 = 6,    // x3
  kW4 = 9,       // x3: [nq][ldw4]; the head's bias sits in the same arena, kB4Off floats behind it
  kReward = 12,
  kNotDone,
  kDZ4,          // out: dZ4_j (ld 32)
  kDU3,          // out: dU3_j
  kU3,           // out: LN3 output rows of Q_j
  kStats3,       // out: LN3 (mean, rstd) of Q_j
  kY,            // out: target [Bp][32] (written by j = 0)
  kSqErr,        // out: weighted squared errors of Q_j, summed over the outputs [Bp]
  kQ,            // out: Q_j [Bp][32]
  kW,            // importance weight of the row [Bp] (ones unless the step is prioritized)
  kTd,           // out: sum over the outputs of |Q_j - y| of a live row, 0 for a pad row [Bp]
  kNumPtr
};
enum : int {
  kK3 = 0,
  kLd3,
  kJ,            // which online critic
  kNq,           // Q outputs per row
  kLdw4,
  kCdq,          // clipped double-Q on
  kB4Off,        // x3: head bias = kW4 + n's pointer + this many floats
  kNumInt = kB4Off + 3
};
enum : int {
  kDiscount = 0,
  kGradScale,    // 2/(B*nq)
  kNumFlt
};
}  // namespace critic_loss_p
TD3_SLOTS_FIT(critic_loss_p);

// kRowTargetLoss (row_target_loss); x2 = (q1, q2)
namespace target_loss {
enum : int {
  kH3 = 0,       // x2: H3 of the target critics
  kGamma3 = 2,   // x2
  kBeta3 = 4,    // x2
  kW4 = 6,       // x2
  kB4 = 8,       // x2
  kReward = 10,
  kNotDone,
  kQ,            // x2: online Q_j [Bp] (kRowUnitLoss wrote them)
  kY = 14,       // out: target y [Bp]
  kDZ4,          // x2, out: dZ4 of Q_j (ld 32)
  kSqErr = 17,   // out: squared errors [2][Bp]
  kG,            // x2, out: g_j = 2/B w (Q_j - y) [Bp]
  kW = 20,       // importance weight of the row [Bp] (ones unless the step is prioritized)
  kTd,           // out: 0.5 (|Q1 - y| + |Q2 - y|) of a live row, 0 for a pad row [Bp]
  kNumPtr
};
enum : int {
  kK3 = 0,
  kLd3,
  kNumInt
};
enum : int {
  kDiscount = 0,
  kGradScale,    // 2/B
  kNumFlt
};
}  // namespace target_loss
TD3_SLOTS_FIT(target_loss);

// kRowLnBwd (row_lnbwd)
namespace ln_bwd {
enum : int {
  kDU = 0,       // dU rows
  kH,            // post-ReLU activations
  kStats,        // LN (mean, rstd) [2][Bp]
  kGamma,
  kDZ,           // out: dZ rows
  kNumPtr
};
enum : int {
  kLd = 0,       // row stride
  kK,            // real width
  kNumInt
};
enum : int { kNumFlt = 0 };
}  // namespace ln_bwd
TD3_SLOTS_FIT(ln_bwd);

// The ring / layer-0 family: kProGather, kProL0, kProL0G (and the plain layer 0 that keeps a
// transposed weight copy)
namespace ring_l0 {
enum : int {
  // ring outputs, written by a problem's first column tile (each nullable)
  kRowCopy2 = 0,  // second copy of the sampled input row (ld kLdRowCopy2)
  kReward,        // reward / not_done of the sampled records [Bp]
  kNotDone,
  kRowCopy,       // kProL0G: first copy of the row (ld kLdRowCopy); kProGather stores it to Aout (ld ldao)
  // layer 0 inside the layer-1 launch (kProL0 / kProL0G)
  kW0 = 8,        // [N0p][32] (or its k-quad image, GemmProb::w0sk)
  kB0,
  kH0,            // out, nullable: H0 rows (ld kN0p)
  // a stand-alone layer 0: row tile 0 also writes its weight rows' columns [kTCol, kTCol + kTN)
  kTCopy = 12,    // nullable: transposed [kTN][Nout]
  kNumPtr
};
enum : int {
  kRecOff = 0,    // offset of the input row inside the record
  kRecOffRw,      // offset of reward (not_done follows it)
  kLdRowCopy2 = 3,
  kN0p = 5,       // padded layer-0 width (<= 512, the layer-1 Kp)
  kK0,            // input width (<= 32)
  kLdRowCopy = 8,
  kTCol = 10,
  kTN,
  kNumInt
};
enum : int { kNumFlt = 0 };
}  // namespace ring_l0
TD3_SLOTS_FIT(ring_l0);
#undef TD3_SLOTS_FIT

// Waves of a single-stage GEMM launch (gemm_kernel): input-grad stages (MODE 1) and 16-column
// stages (WN = 0) run 16 waves — half the prologue rows per wave (their LN-backward / head
// prologues are VALU-bound) and twice the K split; the forward LN / fused layer-0 stages and the
// dual launches (gemm2_kernel) keep kGemmWaves (A/B in DESIGN.md).
#ifndef TD3_GEMM_NW16
#define TD3_GEMM_NW16 1
#endif
// WN = kWn4x2 (B >= 512): the WN = 4 workgroup over TWO 32-row tiles, 64 x 128 outputs, each
// wave's 32 weight columns reused for both (half the weight stream per MAC of WN = 4); prologue
// kinds Copy / LN / LN-bwd / head-bwd only; 8 waves, one workgroup per CU (A rows 2 x 32 x Kp).
constexpr int kWn4x2 = 12;
constexpr int wn_cols(int wn) { return wn == kWn4x2 ? 4 : wn; }   // 32-column waves of a K group
constexpr int wn_rt(int wn) { return wn == kWn4x2 ? 2 : 1; }      // 32-row tiles per workgroup
constexpr int gemm_nw(int mode, int wn, int pro) {
  return (TD3_GEMM_NW16 && wn != kWn4x2 && pro != kProL0 && pro != kProL0G && (mode == 1 || wn == 0)) ? 16
                                                                                                   : kGemmWaves;
}

struct GemmProb {
  // The first 136 bytes (pointers, then ints, no implicit padding) are everything a GEMM
  // workgroup reads before its operand loads: gemm_kernel requests all of them in one scalar batch.
  const float* A;                 // batch rows of the A side (kProCopy / kProLN / kProLNBwd)
  const float* lng; const float* lnb;   // LayerNorm affine of the A-side features
  const float* H;                 // kProLNBwd: post-ReLU activations of the A side
  float* stats;                   // [2][Bp] (mean, rstd): written by kProLN (n-tile 0), read by kProLNBwd
  float* Aout;                    // nullable: n-tile 0 stores pro(A) rows (U_{l-1} or dZ_l)
  const float* W;
  const float* bias;              // MODE 0, nullable
  float* C;
  int lda;
  int Kreal, Kp;                  // reduction length (real / padded to 32), Kp <= 512
  int ldh;
  int ldao;
  int ldw;
  int Nout;                       // padded output width (multiple of 32)
  int ldc;
  int relu;
  int ntiles;                     // output column tiles of 32*WN
  int tile_begin;                 // first flat workgroup id of this problem (row kernels: unused)
  int norm;                       // LayerNorm present (norm="layer")
  int B;                          // real batch rows (rows >= B are padding)
  // MODE 0 weight image: the 16-B piece W[n][4j .. 4j+3] is at W + n * ldw + j * wsk.  Row-major
  // [n][Kp] (the parameter arena): ldw = Kp, wsk = 4 (0 reads as 4).  The k-quad image [Kp/4][Np][4]
  // (learner.h Group::P4 / T4): ldw = 4, wsk = 4 * Np -- the 16 lanes of an MFMA fragment load (16 or 32
  // consecutive n, one k-quad) read 256 contiguous bytes instead of 16 rows' pieces.
  int wsk;
  int w0sk;                       // kProL0*: the same for W0 (ring_l0::kW0): 0 = row-major [N0p][32]
  int wpad_;
  // operands of the row kinds and of the prologues with extra operands (slot names per kind above)
  float* ex[kMaxEx];
  int exi[kMaxExi];
  float exf[kMaxExf];
  uint64_t seed;
  const Counters* ctr;
};

// kProGather: the step's replay-ring sample.  Every workgroup draws the indices of its 32 rows
// (Philox step = total_it + 1, exactly as gather_kernel) and reads its A rows from the records
// (ring_l0::kRecOff = offset of the row inside the record, Kreal = its width).
struct RingSide {
  const float* data; int rec;
  const int64_t* d_size;          // sample range [0, *d_size)
  int64_t* idx_out;               // drawn rows (td3_step_stats.idx)
  uint64_t seed;
  const Counters* ctr;
};

// Problems of one GEMM / row launch, passed BY VALUE in the kernel arguments (one scalar
// load level fewer than a device table at the head of every workgroup's dependency chain).
constexpr int kMaxProbs = 4;
struct GemmTable {
  GemmProb p[kMaxProbs];
  int nprob;
  RingSide rs;                    // kProGather only
};

// ------------------------------------------------------------------ row-wise heads (act / eval_q)
enum HeadMode : int { kHeadTargetAction = 0, kHeadPolicy = 1, kHeadQ = 2 };

struct HeadProb {
  const float* H3; int ldh; int K3;          // last hidden (post-ReLU), real width K3
  const float* lng; const float* lnb;        // LN3 (nullable: norm=None)
  float* U3; int ldu;                        // nullable: store LN3 output
  float* stats;                              // nullable: store LN3 (mean, rstd) [2][Bp]
  const float* W4; int ldw; const float* b4; int nout;
  int mode;
  float* out; int ldo; int out_col;   // policy: out[row*ldo + out_col + o]; Q: out[row*ldo + o]
  float* tanh_out;
  float* noise; int ldn;
};

struct HeadArgs {
  const HeadProb* probs;
  int B, Bp;
  float max_action, policy_noise, noise_clip;
  const Counters* ctr;
  uint64_t seed;
  int gen_noise;
};

// ------------------------------------------------------------------ small-query hidden layers
// select_action / eval_q of up to kGemvRows query rows: each hidden Linear as wave dot products
// (a 32-row MFMA tile would compute 31 pad rows, each workgroup walking K serially).
constexpr int kGemvRows = 4;
// The rows a wave of gemv_kernel / gemv01_kernel / act_kernel holds for a query of B live rows: the
// template argument R their launchers dispatch on (3 rows run R = 4 with one dead row).
constexpr int gemv_rows(int B) { return B <= 1 ? 1 : B == 2 ? 2 : 4; }
struct GemvProb {
  const float* X; int ldx; int K;       // input rows: the query, or the previous layer's ReLU output
  const float* lng; const float* lnb;   // LayerNorm of the input (nullable: layer 0 / norm=None)
  const float* W; int ldw; const float* b; int N;
  float* Y; int ldy;                    // Y[r][o] = relu(LN(X[r]) . W[o] + b[o]), o < N
};
struct GemvArgs {
  GemvProb p[2];                        // one per network (eval_q: the twin's two)
  int B;                                // live rows, 1..kGemvRows
};
int launch_gemv(const GemvArgs& a, int nprob, hipStream_t s);

// Layers 0 and 1 in one launch, for a layer 0 of at most kGemv0K inputs (the featured state /
// state-action row): every workgroup computes all of H0 = relu(W0 x + b0) into LDS (W0 is small),
// then its layer-1 columns as gemv_kernel.  The query rows travel in the kernel arguments.
constexpr int kGemv0K = 64;
constexpr int kGemvQ = kGemvRows * kGemv0K + 4;
struct Gemv01Args {
  GemvArgs l1;                          // layer 1 (its X is unused) and the live rows B
  const float* W0[2]; const float* b0[2];
  int ldw0, K0, N0;                     // the same shapes for both networks (twin critics)
  float xq[kGemvQ];                     // query rows [B][K0], zero past B*K0
};
int launch_gemv01(const Gemv01Args& a, int nprob, hipStream_t s);

// The whole query in ONE launch (act_kernel): layers 0-1 as gemv01, layer 2 after an in-launch
// hand-off of H1 (per-network counters), the head in the last-arriving workgroup.  Layer-2 columns
// ride on the layer-1 column groups (N2 <= N1); X of l2 is l1's Y, H3 of the head is l2's Y.
struct ActArgs {
  Gemv01Args g;                         // layer 0 + layer 1 (g.l1.B = live rows)
  GemvProb l2[2];                       // layer 2 per network
  HeadProb head[2];                     // LN2 + head per network
  int* ctr;                             // [network][2] hand-off counters, zero between launches
  float max_action;
  unsigned* flag;                       // nullable: [network] = seq once its outputs are written
  unsigned seq;                         //   (mapped host memory: the host polls it, no stream sync);
                                        //   seq | kActFailed when a workgroup's H1 poll gave up
  int fail_test;                        // test seam: workgroup 0 reports a timed-out poll
};
constexpr unsigned kActFailed = 0x80000000u;   // flag bit: the query's outputs are not valid
constexpr int kActFailInc = 1 << 16;           // a timed-out workgroup's arrival on the layer-2 counter
// act_kernel's template argument KQ (float4 steps of a layer-0 row) for a layer 0 of K0 inputs
constexpr int act_kq(int K0) { return K0 <= 32 ? 8 : 16; }
int launch_act(const ActArgs& a, int nprob, hipStream_t s);

// dZ = relu'(LN_bwd(dU)) on full rows (layer 0, where no GEMM follows).
struct LnBwdProb {
  const float* GU; const float* H; const float* stats; const float* lng; int ld, K;
  float* GZ;
};
constexpr int kMaxLnBwd = 3;
struct LnBwdTable {            // by value in the kernel arguments (one scalar-load batch)
  LnBwdProb p[kMaxLnBwd];
};

// ------------------------------------------------------------------ parameter-grad + Adam
struct DwProb {
  const float* G; int ldg;        // dZ_l   [Bp][ldg]  (columns n)
  const float* U; int ldu;        // U_{l-1}[Bp][ldu]  (columns k)
  int Np, Kp;
  int64_t offW, offb;             // offsets inside the group arenas
  int64_t offg, offbeta;          // LayerNorm_l affine, -1 when absent
  const float* GU; int ldgu;      // dU_l  (LN grads)
  const float* H; int ldh; const float* stats;
  int ntk;                        // k tiles of the weight
  int tile_begin;                 // matrix tiles: (Np/T)*ntk (T = 32, or 64 with tile64), then
                                  // vector tiles: Np/32
  const float* rs; int ldrs;      // row scale of dZ / dU (unit-gradient backward): rs[r * ldrs];
                                  // ldrs = 0 with rs -> 1.0f when the rows are the gradients
  int kvalid;                     // weight columns >= kvalid get a zero gradient: their U columns
                                  // may hold another field (the actor reads [s | a] rows, ld pad32(sd+ad))
};

enum DwMode : int { kDwGrad = 0, kDwAdam = 1, kDwAdamPolyak = 2 };

struct AdamArgs {
  float* P; float* G; float* M; float* V; float* T;   // group arenas
  // nullable: the k-quad images of P / T (GemmProb::wsk) that the forward GEMM stages read; dw_kernel
  // writes every updated weight element to them too (learner.h Group::P4 / T4)
  float* P4; float* T4;
  const Counters* ctr; int which;                     // 0: critic_step, 1: actor_step
  double lr, beta1, beta2, eps;
  float tau;
  float grad_scale;                                   // 1/world for the all-reduced path
};

constexpr int kMaxDwProbs = 10;    // (4 layers + input LayerNorm) x 2 networks (twin critic)
struct DwArgs {
  DwProb probs[kMaxDwProbs]; int nprob; int Bp;
  AdamArgs adam;
  int mode;
  int tile64;                     // 1: dw64_kernel (64x64 tiles, ntk counts k tiles of 64)
  int scaled;                     // 1: rows scaled by DwProb::rs (dw_kernel<true> / dw64_kernel<true>)
};

// Large batches (Bp a multiple of 64, Bp >= 512): the dW reduction over the batch rows split evenly
// over a persistent grid of one workgroup per CU (dwsk_kernel), partial sums combined with the
// optimizer update by a second launch (dwsk_combine_kernel).  A work unit is one 64-row step of one
// tile: a tm x tm weight tile (dW = dZ^T U) or a 32-column vector tile (db, dgamma, dbeta); unit u is
// step u % S of tile u / S (S = Bp / 64).  Units carry a cost weight (a matrix step costs several
// vector steps) and the host cuts the weighted list into G contiguous ranges: virtual workgroup v
// (XCD-major: the G/8 workgroups of an XCD hold consecutive v, so an XCD streams one contiguous part
// of the tile list) takes units [wg_unit[v], wg_unit[v+1]) and writes one partial per tile it
// touched to slab[v][j] (j-th tile of its range); tile t's partials come from workgroups
// tile_wg[2t] .. tile_wg[2t+1] (empty ranges skipped).
struct DwTile {
  int prob;                       // DwArgs::probs index
  int kind;                       // 0: tm x tm matrix tile (a = n tile, b = k tile), 1: vector tile (a = j)
  int a, b;
};
struct DwSplit {
  const DwTile* tiles; int ntile;
  int S;                          // steps per tile (Bp / 64)
  int G;                          // workgroups (multiple of 8)
  int J;                          // partial slots per workgroup
  int tm;                         // matrix tile edge: 64 or 128
  int slot;                       // floats per partial slot (tm * tm)
  const int* wg_unit;             // [G + 1]
  const int* tile_wg;             // [ntile][2]
  float* slab;                    // [G][J][slot]
};
int launch_dw_split(const DwArgs& a, const DwSplit& k, hipStream_t s);

// ------------------------------------------------------------------ launchers (kernels_launch.h)
// launch_gemm's bump_actor: 0 bumps total_it / critic_step, 1 also actor_step, kBumpActorOnly only
// actor_step (TD3_particles._actor_learn outside a train step: the actor's Adam step, no total_it)
constexpr int kBumpActorOnly = 2;
int launch_gemm(int mode, int wn, int pro, const GemmTable& t, int nblocks, int Bp, int lds_bytes,
                Counters* bump, int bump_actor, hipStream_t s);
// The fused layer-0 stages (kProL0 / kProL0G, same GemmProb contract) on 16-row tiles: 16 x 16*nct
// layer-1 outputs per workgroup of nct * wk waves; instantiated (nct, wk) = (5, 2), (2, 4).
int launch_l0r16(int nct, int wk, int gather, const GemmTable& t, int nblocks, int Bp, Counters* bump,
                 int bump_actor, hipStream_t s);
int l0r16_lds_bytes(int Kp, int nct, int wk);
// Two independent GEMM stages in one launch (stage 2's tile ids follow stage 1's); only the pairs
// gemm2_supported() reports are instantiated.
int gemm2_supported(int m1, int w1, int p1, int m2, int w2, int p2);
int launch_gemm2(int m1, int w1, int p1, const GemmTable& t1, int nb1, int m2, int w2, int p2, const GemmTable& t2,
                 int nb2, int Bp, int lds, hipStream_t s);
int launch_rows(int kind, const GemmTable& t, int Bp, hipStream_t s);
// Two row kinds in one launch: problems [0, n1) run kind1, [n1, nprob) kind2.
int launch_rows2(int kind1, int kind2, int n1, const GemmTable& t, int Bp, hipStream_t s);
int launch_heads(const HeadArgs& a, int nprob, hipStream_t s);
// kRowActorHeadBwdBc (bc.hip), called by launch_rows with the table's wide problems marked and the stage's bytes
int launch_rows_bc(const GemmTable& d, int lds, int Bp, hipStream_t s);
// kRowActorHeadBwdBcF (bcf.hip), called the same way
int launch_rows_bcf(const GemmTable& d, int lds, int Bp, hipStream_t s);
// Dynamic LDS bytes of the calling thread's last launch_rows / launch_rows2 (the wide-head stage;
// 0: every head was requested block by block; -1: no row launch yet): td3_debug_row_lds
int last_row_lds();
int launch_lnbwd_rows(const LnBwdTable& tab, int nprob, int Bp, int norm, hipStream_t s);
int launch_dw(const DwArgs& a, int nblocks, hipStream_t s);
// The flat optimizer's view of the images: the range it updates starts at arena offset `base`; a
// float4 inside matrix m ([off, off + Np * Kp), off % 4 == 0) is also stored at its image piece
struct W4Map {
  float* P4; float* T4;         // image bases (arena offset 0); P4 null: no images
  int64_t base;
  int nmat;
  int64_t off[8]; int Np[8], Kp[8];
};
int launch_adam_flat(const AdamArgs& a, int64_t n, int polyak, hipStream_t s, const W4Map* w4 = nullptr);
int adam_flat_args(const char* who, const AdamArgs& a, int64_t n, int polyak, const W4Map* w4, W4Map* out,
                   int* blocks);
int launch_polyak_w4(float* T, const float* P, int64_t n, float tau, const W4Map& w, hipStream_t s);
// Data-parallel replicas in one process (td3_comm_init_local): arena k <- sum over j of arena j,
// summed in replica order (the same value lands in every replica, like a ring all-reduce).
constexpr int kMaxLocalReplicas = 8;
struct LocalSumArgs {
  float* a[kMaxLocalReplicas];
  int n;
  int64_t size;
};
int launch_local_sum(const LocalSumArgs& a, hipStream_t s);

// ------------------------------------------------------------------ weight normalization
// norm = "weight_normalization" (TD3_featured.py:33-35, 68-70: torch weight_norm, dim 0, on
// every Linear): the parameters of a Linear are bias, weight_g [N,1] and weight_v [N,K]; the
// GEMM stages read the derived W = v * (g / ||v||) kept at the Linear's weight offset.
struct WnLinear {
  int64_t offW, offb, offg, offv;    // offsets in a group arena (W and v: [Np][Kp] rows)
  int N, K, ld;                      // real rows / columns, row stride Kp
  int row0;                          // first row of this Linear in the launch's row numbering
};
constexpr int kMaxWnLinears = 8;     // 4 Linears x 2 networks (twin critic)
struct WnArgs {
  WnLinear lin[kMaxWnLinears];
  int nlin, rows;                    // rows = sum of N: one wave per output row
  AdamArgs adam;                     // P, T, M, V, G arenas, counters, hyper-parameters
  int mode;                          // kWnDerive: W of `arena` (and `arena2`); kWnAdam: optimizer step
  int polyak;                        // kWnAdam: Polyak the targets (T) too and re-derive their W
  float* arena; float* arena2;       // kWnDerive
};
enum WnMode : int { kWnDerive = 0, kWnAdam = 1 };
int launch_wn(const WnArgs& a, hipStream_t s);
int launch_polyak_flat(float* T, const float* P, int64_t n, float tau, hipStream_t s);
// k-quad weight images (GemmProb::wsk): dst[off + ((k/4) * Np + n) * 4 + k % 4] = src[off + n * Kp + k]
// for every listed matrix (off, Np, Kp), over up to two (src, dst) arena pairs (P -> P4, T -> T4)
constexpr int kMaxW4Mats = 16;
struct W4PackArgs {
  const float* src[2]; float* dst[2]; int npair;
  int64_t off[kMaxW4Mats]; int Np[kMaxW4Mats], Kp[kMaxW4Mats]; int64_t first[kMaxW4Mats + 1];   // piece ranges
  int nmat;
};
int launch_w4_pack(const W4PackArgs& a, hipStream_t s);
// pack_kernel: the [B][cols] rows of src into columns [col, col + cols) of up to three ld-strided
// destinations (a null p is skipped), zeros for rows B .. Bp - 1; one workgroup per row of Bp
struct PackDst { float* p; int ld, col; };
int launch_pack(const float* src, int cols, int B, int Bp, std::initializer_list<PackDst> dst, hipStream_t s);
// Epilogue of td3_select_action_device: the policy head's rows pi (max_action * tanh, row stride ldp)
// -> action_out [n][ad].  plain: a copy.  Otherwise z ~ N(0,1) (Philox kStreamExplore, or inject_z),
// x != null: the Ornstein-Uhlenbeck state X <- X + (theta (mu - X) + sigma z) (X = mu first where
// reset[row] != 0) and a = clamp(pi + X); x == null: a = clamp(pi + sigma z).
struct ExploreArgs {
  const float* pi; int ldp;
  float* action_out;
  int n, ad;
  int plain;
  float max_action;
  float* x;
  float mu, theta, sigma;
  const uint8_t* reset;
  uint64_t seed, step;
  const float* inject_z;
  float* z_out;
};
int launch_explore(const ExploreArgs& a, hipStream_t s);
int kernels_init();

}  // namespace td3
