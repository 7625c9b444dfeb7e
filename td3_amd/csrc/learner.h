// Internal header of the learner's translation units (td3.hip, stages.hip, step.hip, act.hip, dp.hip,
// debug.hip, trainlog.hip, clip.hip): the types they share and the functions that cross a file boundary.  Functions used in
// one file are static there.
#pragma once
#include <rccl/rccl.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "encoder.h"
#include "kernels.h"
#include "replay.h"
#include "../../include/td3.h"

namespace td3 {

// ------------------------------------------------------------------ layouts
// offW: the weight the GEMM stages read; with weight normalization it is derived from
// (offg, offv) = (weight_g [Np], weight_v [Np][Kp]) by wn_kernel, else offg = offv = -1.
struct LinearL { int N, K, Np, Kp; int64_t offW, offb, offg = -1, offv = -1; };
struct LNormL { int N, Np; int64_t offg, offb; };
struct NetL {
  LinearL lin[4];
  LNormL ln[3];
  // TD3_particles networks: the particle encoder block (EncOff layout) and lnorm1, the
  // LayerNorm of the concatenated MLP input (TD3_particles.py:43-46 / :95-98)
  int D = 0;                 // particle feature width (0: featured network)
  int64_t enc_off = -1;
  bool lnin = false;
  LNormL ln_in{};
};
struct TensorRef { std::string name; int64_t rows, cols; int64_t off; int ld; };

struct Group {
  int64_t size = 0;          // floats per arena copy
  int64_t cap = 0;           // allocated floats per copy (>= size + 256: the sharded optimizer's
                             // rank slices of 4-float multiples may run past `size` into zero pads)
  float *P = nullptr, *T = nullptr, *M = nullptr, *V = nullptr, *G = nullptr;
  // k-quad images of P and T (kernels.h GemmProb::wsk: W[n][4j .. 4j+3] at ((j * Np + n) * 4) inside a
  // matrix's [offW, offW + Np * Kp) range), read by the forward GEMM stages of a plan with Plan::w4.
  // Such a plan's dW stages (dw_kernel) write every updated weight to them as well; anything else
  // that writes P / T (td3_set_params, another plan's optimizer) clears w4_valid and the next w4
  // step repacks them first (ensure_w4).
  float *P4 = nullptr, *T4 = nullptr;
  bool w4_valid = false;
  std::vector<NetL> nets;
  std::vector<TensorRef> tensors;
  WnArgs wn{};               // weight normalization: the group's Linears (wn.nlin = 0 otherwise)
};

// ------------------------------------------------------------------ per-batch buffers
struct EvalB {
  float* X = nullptr; int ldx = 0;
  float* H[3] = {};
  float* U[3] = {};
  float* stats[3] = {};
  float* GU[3] = {};
  float* GZ[4] = {};
  float* T = nullptr;   // policy head tanh output [Bp][32]
  float* Qv = nullptr;  // [Bp] (featured) / [Bp][32] (particles: one Q per action dim)
  // particles: lnorm1 output / stats / grad, conv2 ReLU bits, encoder grad partial slabs
  float* Uin = nullptr;
  float* statsIn = nullptr;
  float* GUin = nullptr;
  uint64_t* mask = nullptr;
  float* partial = nullptr;
  float* gpool = nullptr;   // [Bp][128] pooled-feature grad rows of the encoder backward
};

// A guard of zeros behind a scratch's last buffer, for the kernels' clamped / whole-tile vector loads
// that run past the rows they use.  Not space anyone may carve.
constexpr size_t kScratchTail = 16384;   // floats

// base == nullptr: a measuring pass (take advances `used` and returns null), see carve_scratch
struct Scratch {
  float* base = nullptr;
  size_t used = 0;
  float* take(size_t floats) {
    size_t n = (floats + 63) & ~(size_t)63;
    float* p = base ? base + used : nullptr;
    used += n;
    return p;
  }
};

// A GEMM stage's launch, kept so the planner can merge two independent stages into one launch.
struct GemmLaunch {
  int mode, wn, pro;
  GemmTable t;
  int blocks, Bp, lds;
  bool plain;           // no ring binding, no counter bump: mergeable
};

struct Stage {
  std::string name;
  std::function<int(hipStream_t)> run;
  double flops = 0;
  std::string kernel;   // HIP kernel function the stage launches (rocprof name)
  // algorithmic HBM bytes of one launch (t_roof = max(flops / peak, bytes / 8 TB/s)):
  // the operands and results a launch must move once; 0 where not accounted (row kernels)
  double bytes = 0;
  std::shared_ptr<GemmLaunch> gemm;   // GEMM stages only
  int collective = -1;  // data parallel: the gradient all-reduce of group 0 (actor) / 1 (critic)
  // the all-reduced range of the group's G arena (floats; coll_n < 0: the whole arena) and, for a
  // bucket of the overlapped schedule, the optimizer step of that range the in-process seam runs
  // on its own stream after the fixed-order sum (RCCL mode: both queued on the comm stream)
  int64_t coll_off = 0, coll_n = -1;
  std::function<int(hipStream_t)> after;
  // the sharded optimizer step (reduce-scatter -> Adam on the rank's slice -> all-gather of the
  // parameters): the slice length; the seam copies each owner's parameter slice to the others
  int64_t coll_slice = 0;
};

// Replicas of one process sharing a device (td3_comm_init_local): the test seam of the data-parallel
// path.  Their steps run stage by stage on one stream (td3_train_step_local), and each all-reduce
// is a fixed-order device sum over the replicas' G arenas in place of ncclAllReduce.
struct LocalGroup {
  std::vector<td3_handle*> hs;
};

// The split-K dW stages' partial slab: one per plan, sized to its largest stage.  A plan's stages run
// one after another on one stream (and a stage's combine consumes the slab right behind it), so every
// split-K stage of the plan can share it (launch_dw_split reads the pointer at launch).
struct SlabRef {
  float* p = nullptr;
  size_t bytes = 0;
};

struct Plan {
  int B = 0, Bp = 0;
  SlabRef dwslab;
  bool dp_overlap = false;              // stages queue work on the comm stream: launched directly
  float* scratch = nullptr;
  size_t scratch_bytes = 0;
  // inputs
  float *X_SA = nullptr, *X_S2A = nullptr, *X_SP = nullptr;
  int ld_sa = 0;
  float *R = nullptr, *ND = nullptr, *noise = nullptr, *Y = nullptr, *sqerr = nullptr;
  float* gscale[2] = {};                // [Bp] g_r = 2/B (Q_j,r - y_r): row scale of Q_j's unit backward
  // Q1's layer-0 action columns transposed, [ad][Np0] (W1[:, sd + o] as row o), written by the actor
  // phase's separate layer-0 stage (AF_fwd0) for actor_head_bwd's coalesced reads; null when layer 0
  // is fused into the layer-1 launch (those rows are 32 floats: the strided reads cost nothing)
  float* W1aT = nullptr;
  int64_t* d_idx = nullptr;
  int64_t* d_inject_idx = nullptr;
  // the rows' importance weights in the critic loss (target_loss::kW / critic_loss_p::kW), ones unless
  // the last step was prioritized (per_w_dirty: the next other step refills them, ensure_unit_weights),
  // the rows' |TD error| and the injected mass fractions of a prioritized draw
  float *per_w = nullptr, *per_td = nullptr, *per_u = nullptr;
  bool per_w_dirty = false;
  // TD3+BC (td3_set_bc; null / false in a plan built with it off): the live rows' sum over the action
  // of (pi - a)^2 [Bp], and (lambda, mean |Q1(s, pi)|) of the last actor step, written by its
  // actor_head_bwd stage
  float *bc_se = nullptr, *bc_lam = nullptr;
  bool bc = false;
  // The filtered BC term (td3_set_bc_filter; null / false unless bc and a switch is on): the rows' 0/1 mask
  // [Bp] of the last actor step, and the int32 word its actor_head_bwd stage reads n_d from -- B from the
  // plan's build on, rewritten ahead of every actor step's body while demo_rows is on (queue_bc_rows)
  float* bcf_keep = nullptr;
  int* bcf_nd = nullptr;
  bool bcf = false;
  // particles: each critic's rows' sum over the Q outputs of |Q_j - y| (critic_loss_p::kTd), [J][Bp];
  // the prioritized step combines them into per_td (per_td_combine_kernel)
  float* per_tdj = nullptr;
  uint64_t per_ring_gen = 0;            // Ring::gen of the last prioritized step's ring (d_inject_idx holds its rows)
  // the last mixed step (td3_train_step_mixed): Ring::gen of its online and demo rings, its n_demo and
  // total_it after it (any later step moves total_it on); d_idx holds its rows
  uint64_t mixed_gen[2] = {0, 0};
  int mixed_n_demo = 0;
  int64_t mixed_it = 0;
  EvalB TA, Q[2], A, TQ[2], AQ;
  // device problem tables (owned)
  std::vector<void*> tables;
  // stage lists (excluding the input stage): [actor_phase][inject_noise]
  std::vector<Stage> body[2][2];
  // featured replay-ring bodies: the sample fused into F_fwd0 (kProGather), ring bound in rside
  std::vector<Stage> body_ring[2][2];
  RingSide rside{};
  // the sample runs inside F_fwd0 only for short records: each F_fwd0 workgroup re-reads its
  // rows' records, a loss once they are KBs (Humanoid: gather 4.8 + F_fwd0 23 us separate vs
  // 34 us fused)
  bool fuse_gather = false;
  bool w4 = false;                      // forward weights read from the k-quad images (Group::P4 / T4)
  hipGraphExec_t graph[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
  // the same bodies with the replay-ring gather captured in front (Philox draw path)
  hipGraphExec_t graph_g[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
  uint64_t graph_ring_gen = 0;          // Ring::gen the graph_g variants were captured with
  // ---- TD3_particles
  int particles = 0;
  int nq = 1, ldq = 1;                  // Q outputs per row and the row stride of Y / Qv
  int ld_a = 0, ld_q = 0;               // MLP input widths (pad32(128+F), pad32(128+F+A))
  float *XA = nullptr, *XTA = nullptr, *XAQ = nullptr, *XQ[2] = {}, *XTQ[2] = {};
  float* pbatch = nullptr;              // foreign-buffer path: [Bp][2*N*D] particles of (s, s')
  int64_t* d_iota = nullptr;
  const float* src_data = nullptr;      // where the encoders read particles: ring or pbatch
  int src_rec = 0, src_op = 0, src_op2 = 0;
  const int64_t* src_idx = nullptr;
  uint64_t src_key = 0;                 // Ring::gen of the source ring, kBatchSource for pbatch
  int nwg = 0;                          // encoder-backward workgroups per role per critic network
  int nwg_a = 0;                        // ... for the actor's encoder (one network per launch)
  // TD3_particles._actor_learn(state_features, state_particles) on its own (TD3_particles.py:209-224)
  std::vector<Stage> actor_learn;
};

// Query batches up to this many (padded) rows keep their inputs and outputs in mapped pinned host
// memory that the stages read and write in place: an idle select_action is then the launch chain
// and one stream sync, without the two copy commands (~10 + ~25 us on the host for pageable
// copies, tools/api_cost.hip).  Larger batches use device buffers and DMA copies.
constexpr int kMappedRows = 256;

struct ActPlan {       // select_action / eval_q at small batch
  int Bp = 0;
  float* scratch = nullptr;
  float* hio = nullptr;  // mapped pinned block (Bp <= kMappedRows), else nullptr
  bool dev = false;      // a plan of the device-resident queries (td3_handle::act_dev)
  // device addresses the stages use; the h* twins are their host views when mapped
  float *X_S = nullptr, *X_SA = nullptr, *out = nullptr, *q[2] = {nullptr, nullptr};
  float *XQ2 = nullptr, *pbatch = nullptr;   // particles
  float *hX_S = nullptr, *hX_SA = nullptr, *hout = nullptr, *hq[2] = {nullptr, nullptr};
  float *hXQ2 = nullptr, *hpbatch = nullptr;
  int ldo = 0;           // row stride of `out`
  // featured queries of n <= kGemvRows rows: hidden layers as gemv_kernel launches, then the head
  bool gemv = false, gemv01 = false;
  GemvArgs gv_act[3], gv_q[3];
  Gemv01Args g01_act{}, g01_q{};
  HeadArgs head_act{}, head_q{};
  // the same query as ONE launch (act_kernel): select_action / eval_q (separate counters: they run
  // on different streams)
  bool act1 = false;
  ActArgs a1_act{}, a1_q{};
  unsigned* hflag[2] = {nullptr, nullptr};    // host views of a1_act.flag / a1_q.flag (mapped)
  unsigned seq[2] = {0, 0};
  int fail_test = 0;                          // td3_debug_act_fail: queries left whose poll "times out"
  int64_t* d_iota = nullptr;
  // device-resident particle queries: the caller's [dev_n][N*D] rows the encoder stage reads in place,
  // set by the query before it runs the stages (launch arguments are copied at launch)
  const float* dev_part = nullptr;
  int dev_n = 0;
  EvalB A, Q[2];
  std::vector<void*> tables;
  std::vector<Stage> act, evalq;
};

// How a featured query of n rows runs on plan A (act.hip: td3_select_action, td3_eval_q, run_gemv and
// td3_debug_query_route all ask query_route): the launches, and where the query's rows travel.
enum QueryKind {
  kQueryAct1,     // one act_kernel launch, completion flags polled on the host
  kQueryGemv01,   // gemv01_kernel (layers 0 + 1) -> gemv_kernel (layer 2) -> head_kernel
  kQueryGemv,     // gemv_kernel per hidden layer -> head_kernel
  kQueryStages,   // the plan's stage list (A->act / A->evalq)
};
enum QueryRows { kRowsArgs, kRowsMapped, kRowsDevice };   // kernel arguments / mapped host block / device scratch
struct QueryRoute {
  QueryKind kind;
  QueryRows rows;
  std::vector<Stage>* stages;   // kQueryStages: the list to run (q: evalq, else act)
};
QueryRoute query_route(ActPlan* A, int n, bool q);

// Carves an ActPlan's query inputs / outputs from the mapped block, or from the device scratch.
struct IoCarve {
  Scratch* S;
  bool mapped = false;  // the plan has a mapped block (h, d null: measuring it)
  float* h = nullptr;   // host view of the mapped block
  float* d = nullptr;   // its device address
  size_t used = 0;
  float* take(size_t floats, float** host) {
    if (!mapped) {
      *host = nullptr;
      return S->take(floats);
    }
    const size_t n = (floats + 63) & ~(size_t)63;
    *host = h ? h + used : nullptr;
    float* p = d ? d + used : nullptr;
    used += n;
    return p;
  }
};

// store_u: keep the LN outputs U (input of the dW of the next layer);
// stats: keep the LN row statistics (needed by any backward through this network).
// Batch buffers the ring-sampled first layer fills (first column tile of a problem).
struct RingOut {
  float* a; int lda;      // the A row
  float* b; int ldb;      // a second copy of it
  float* r; float* nd;    // reward, not_done
};

struct FwdItem {
  const NetL* net; const float* P; EvalB* e; bool store_u; bool stats;
  int ring_src = -1;      // layer 0 read from the replay ring (kProGather): record offset of the input
  // separate layer-0 stage only: columns [tcol, tcol + tn) of the layer-0 weight, transposed into
  // tcopy [tn][Np0] by the stage's first row tile
  float* tcopy = nullptr;
  int tcol = 0, tn = 0;
};
struct BwdItem { const NetL* net; const float* P; EvalB* e; bool store_dz; };

// Where a policy head puts its action, and how: columns [acol, acol + ad) of the ld-strided rows of
// out (and out2, nullable); clamp: a' to +-max_action
struct PolicyDst {
  float* out; float* out2; int ld, acol;
  int clamp; float max_action;
};

// The training log of a handle (include/td3.h, "training log"; trainlog.hip): a ring of `cap` entries in
// device memory.  `count` steps were logged so far; ev is recorded behind every log launch on the
// step's stream, so a read waits for the last one without holding a caller's stream.
struct TrainLog {
  int cap = 0, every = 1;
  int64_t count = 0;
  int64_t floor = 0;       // the oldest sequence number td3_log_set restored (0: none lost that way)
  td3_log_entry* d = nullptr;
  hipEvent_t ev = nullptr;
  bool ev_recorded = false;
  // the last logged step, for td3_debug_log_launch: its flags, its total_it and the plan whose buffers it read
  bool last_actor = false, last_prioritized = false;
  int64_t last_step = 0;
  const Plan* last_plan = nullptr;
};

// Global-norm gradient clipping (include/td3.h, "gradient clipping"; clip.hip): one group's device state.
// The setter writes max_norm; the group's gnorm stage writes the partials; its Adam stage writes
// (total, coef) of the step for td3_clip_info.
constexpr int kClipMaxWg = 128;
struct ClipDev {
  double max_norm;
  double total;
  double partial[kClipMaxWg];
  float coef;
  float pad_;
};

struct EncItem {
  const NetL* net;
  const float* P;         // group arena (encoder at P + net->enc_off)
  float* X; int ldx;      // pooled features -> X[:, 0:128]
  int next;               // 1: the next-state particles
  uint64_t* mask;         // nullable (networks that are back-propagated)
};

}  // namespace td3

struct td3_handle {
  td3_config cfg;
  int sd, ad;                 // featured: state / action dims; particles: feature / action dims
  int particles = 0, N = 0, D = 0, cdq = 1;
  td3::Group actor, critic;
  float* arena = nullptr;
  td3::Counters* d_ctr = nullptr;
  float* ones = nullptr;      // 64 x 1.0f: the row scale of dW problems whose rows are the gradients
  int64_t total_it = 0, critic_step = 0, actor_step = 0;   // host mirror
  // Adam hyper-parameters per optimizer, [0] critic, [1] actor (AdamArgs::which).  Both start
  // from the config; torch's Adam.load_state_dict adopts a checkpoint's param_groups, and so
  // does td3_set_adam.
  struct AdamHp { double lr, beta1, beta2, eps; } adam[2];
  hipStream_t stream = nullptr;
  // Acting path: a query runs behind a queued actor update in that update's own
  // stream (actor_stream: stream order is the dependency -- an event record and a cross-queue wait
  // each left a ~6 us hole in the GPU timeline) and otherwise on its own stream, where it overlaps
  // critic-only steps (total_it % policy_freq != 0) instead of queueing behind them.
  hipStream_t act_stream = nullptr;
  hipStream_t actor_stream = nullptr;         // a queued step there may still update the online actor
  // the same for an update queued on a caller's stream (td3_train_step's `stream`, a replica of a
  // local group): an event recorded there, which the acting stream waits for once
  hipEvent_t actor_ev = nullptr;
  bool actor_ev_pending = false;
  bool act_used = false;                      // a query ran (use_graph auto: replay idle critic steps)
  hipStream_t last_step_stream = nullptr;     // the stream of the last train step
  std::unique_ptr<td3::Plan> plan;
  std::map<int, std::unique_ptr<td3::ActPlan>> act;
  // Device-resident queries (td3_select_action_device / td3_eval_q_device) run asynchronously on the
  // step stream or a caller's: plans of their own (device I/O only), so a query still in flight never
  // shares scratch with a synchronous host query on the acting stream.  dev_stream: the stream of the
  // last one; a query on another stream waits for dev_ev recorded there (same scratch).
  std::map<int, std::unique_ptr<td3::ActPlan>> act_dev;
  hipStream_t dev_stream = nullptr;
  hipEvent_t dev_ev = nullptr;
  ncclComm_t comm = nullptr;
  // the overlapped data-parallel schedule (dp.hip add_dp_overlapped): the all-reduces and the per-bucket
  // optimizer steps run on comm_stream, ordered after the bucket's dW by comm_ev (recorded on the step
  // stream) and joined back by comm_done before the next stage that reads the parameters
  hipStream_t comm_stream = nullptr;
  hipEvent_t comm_ev = nullptr, comm_ev1 = nullptr, comm_done = nullptr;
  std::shared_ptr<td3::LocalGroup> local;          // td3_comm_init_local (comm stays null)
  int nranks = 1, rank = 0;
  bool dp_sharded = false;                    // the plan's optimizer steps are sharded (add_dp_sharded)
  bool w4_build = false;                      // the plan being built reads / maintains the k-quad images
  int64_t opt_gathered_it = -1;               // total_it of the last td3_dp_gather_optimizer_state
  std::vector<td3::Stage>* last_body = nullptr;
  td3::Ring* last_ring = nullptr;                  // the ring of the last td3_profile_stages (stage 0: its gather)
  uint64_t last_ring_gen = 0;                 // its Ring::gen (td3_time_stage refuses a destroyed ring)
  // td3_probe_kernel: while set, steps launch directly and every stage launching `probe_kernel` is
  // bracketed by a pair of HIP events on the step's stream (probe_ev[2k], probe_ev[2k + 1])
  bool probing = false;
  bool per_step = false;                      // inside a prioritized step: the body keeps its weights
  std::string probe_kernel;
  std::vector<hipEvent_t> probe_ev;
  int probe_used = 0;
  std::vector<std::string> stage_names;
  std::vector<std::string> stage_kernels;
  std::unique_ptr<td3::TrainLog> log;         // td3_log_enable; null: steps queue nothing for it
  // TD3+BC (td3_set_bc): the weight alpha (0: off) and total_it of the last actor step taken with it in
  // the current plan (0: none; the plan holds that step's lambda and row errors)
  double bc_alpha = 0.0;
  int64_t bc_step = 0;
  // The BC term's row mask (td3_set_bc_filter): the two switches, and n_d of the last actor step queued with
  // the filtered form in the current plan (td3_bc_filter_info's n_demo; bc_step is that step's total_it)
  int bc_demo_rows = 0, bc_q_filter = 0;
  int bcf_n_demo = 0;
  // Gradient clipping (td3_set_grad_clip), index = group (0 actor, 1 critic): the threshold (0: off), its
  // device state (allocated by the first call that turns a group on), and total_it of the group's last
  // optimizer step taken with clipping in the current plan (clip_has: there is one to report)
  double clip_max[2] = {0.0, 0.0};
  td3::ClipDev* d_clip = nullptr;
  int64_t clip_step[2] = {0, 0};
  bool clip_has[2] = {false, false};
};

namespace td3 {

// What travels together on every call of the stage builders: the handle, the owner of the plan's
// device tables, the padded and the live batch rows.
struct StageCtx {
  td3_handle* h;
  std::vector<void*>& owned;
  int Bp, B;
};
// add_fwd_stages: bump / bump_actor: the step counters the launch behind the sample bumps; ring / ro /
// o_r: layer 0 sampled from the replay ring (RingSide bound at launch, the batch buffers its first
// column tiles fill, the record offset of the reward); fuse_l0 / r16: see can_fuse_l0 / l0r16_config.
struct FwdOpts {
  Counters* bump = nullptr;
  int bump_actor = 0;
  const RingSide* ring = nullptr;
  const RingOut* ro = nullptr;
  int o_r = 0;
  bool fuse_l0 = false, r16 = false;
};
struct BwdOpts {
  bool need_dz0 = false, need_in = false;
  std::vector<GemmProb>* lnbwd_rows = nullptr;
  float head_bwd_scale = 0.f;
};
struct DwOpts {
  int which = 0;            // AdamArgs::which: 0 critic, 1 actor
  bool polyak = false;
  int enc_nwg = 0;
  const std::vector<const float*>* unit_scale = nullptr;
  SlabRef* slab = nullptr;
};
// A dW stage's work (stages.hip make_dw_work): the launch arguments (every problem of the group's
// networks, the optimizer's view of its arenas), the tile count of the one-tile-per-workgroup kernels,
// whether the split-K kernels take it, and the roofline's flops and algorithmic bytes.
struct DwWork {
  DwArgs a;
  int blocks;
  bool split;
  double flops, bytes;
};
// A plan's carving, written once and run twice by carve_scratch (measuring, then on the allocation)
using CarveFn = std::function<void(Scratch&, IoCarve&)>;

// ---- stages.hip
int upload(td3_handle* h, std::vector<void*>& owned, const void* host, size_t bytes, void** out);
void alloc_eval(Scratch& S, const NetL& n, int Bp, float* X, int ldx, bool bwd, bool norm, bool policy_or_q,
                EvalB& e);
int carve_scratch(const CarveFn& carve, ActPlan* mapped, float** scratch, size_t* scratch_bytes);
bool merge_gemm_pair(std::vector<Stage>& st, size_t i, size_t j);
int stage_index(const std::vector<Stage>& st, const std::string& name);
int push_row_stage(std::vector<Stage>& st, std::vector<GemmProb>& probs, int kind, int Bp, const std::string& name);
int push_row2_stage(std::vector<Stage>& st, std::vector<GemmProb>& probs, int kind1, int kind2, int n1, int Bp,
                    const std::string& name);
int env_int(const char* name, int dflt);
bool can_fuse_l0(const std::vector<FwdItem>& items);
bool w4_eligible(const td3_handle* h, int Bp);
int ensure_w4(td3_handle* h, hipStream_t s);
int w4_pack_args(const Group& g, bool with_t, W4PackArgs* out);
int add_fwd_stages(const StageCtx& c, std::vector<Stage>& st, const std::vector<FwdItem>& items, const char* tag,
                   const FwdOpts& o);
int add_bwd_stages(const StageCtx& c, std::vector<Stage>& st, const std::vector<BwdItem>& items, const char* tag,
                   const BwdOpts& o);
int add_dw_stage(const StageCtx& c, std::vector<Stage>& st, Group& g, const std::vector<BwdItem>& items,
                 const char* tag, const DwOpts& o);
DwWork dw_bucket(const DwWork& w, const std::vector<BwdItem>& items, size_t b);
int push_dw_stage(const StageCtx& c, std::vector<Stage>& st, const DwWork& w, SlabRef* slab, const std::string& name);
int push_wn_stage(std::vector<Stage>& st, const Group& g, const AdamArgs& adam, bool polyak, const char* tag);
int alloc_dw_slab(Plan* P);
void free_plan_tables(std::vector<void*>& t);
// ---- step.hip
void destroy_plan(Plan* p);
int run_stages(std::vector<Stage>& st, hipStream_t s);
int input_from_ring(td3_handle* h, Ring* r, Plan* P, bool inject_idx, hipStream_t s);
int ensure_unit_weights(td3_handle* h, hipStream_t s);
int build_plan(td3_handle* h, int B);
int ensure_plan(td3_handle* h, int B);
int bind_ring(td3_handle* h, Ring* r);
int finish_step(td3_handle* h, int actor_phase, hipStream_t s, td3_step_stats* stats, bool prioritized = false);
enum RingUser : int { kLearnerStep = 0, kReplicaStep = 1 };
int check_ring(const td3_handle* h, const Ring* r, RingUser what);
// the host's note of a step just queued with the BC actor phase (td3_bc_info's `step`); total_it is the step's
inline void note_bc_step(td3_handle* h, int actor_phase) {
  if (actor_phase && h->plan && h->plan->bc) h->bc_step = h->total_it;
}
// The candidate rows [0, n_d) of a step about to be queued on s (td3_set_bc_filter): with demo_rows on, an
// actor step writes n_d to the plan's word ahead of its body -- a direct operation on the step's stream,
// outside every captured graph, so n_d may change from step to step.  With demo_rows off the word keeps the
// B the plan's build wrote and nothing is queued.  n_d: the mixed step's n_demo; B for every other step.
int queue_bc_rows(td3_handle* h, int actor_phase, int n_d, hipStream_t s);
// ---- clip.hip
// whether the group `which` steps (AdamArgs::which: 0 critic, 1 actor) clips its gradient
inline bool clip_on(const td3_handle* h, int which) { return h->clip_max[which == 1 ? 0 : 1] > 0.0; }
// the host's note of a step just queued (td3_clip_info's `step`): the critic group steps every time
inline void note_clip_step(td3_handle* h, int actor_phase) {
  for (int g = 0; g < 2; ++g)
    if (h->clip_max[g] > 0.0 && (g == 1 || actor_phase)) {
      h->clip_step[g] = h->total_it;
      h->clip_has[g] = true;
    }
}
int add_clip_optimizer(td3_handle* h, std::vector<Stage>& st, Group& g, const AdamArgs& adam, bool polyak,
                       const char* tag);
// ---- trainlog.hip
int log_step(td3_handle* h, int actor_phase, bool prioritized, hipStream_t s);
void destroy_train_log(td3_handle* h);
// ---- act.hip
int map_io(ActPlan* A, size_t floats, IoCarve* io);
// ---- dp.hip
bool dp_overlap(const td3_handle* h);
bool dp_buckets(const td3_handle* h, const Group& g, const std::vector<BwdItem>& items, const DwOpts& o,
                const DwWork& w);
int add_dp_overlapped(const StageCtx& c, std::vector<Stage>& st, Group& g, const std::vector<BwdItem>& items,
                      const char* tag, const DwOpts& o, const DwWork& w);
int add_dp_optimizer(td3_handle* h, std::vector<Stage>& st, Group& g, AdamArgs adam, bool polyak, const char* tag);
int w4_map(const td3_handle* h, const Group& g, int64_t base, W4Map* out);
int gather_moments_for_rebuild(td3_handle* h);
int consolidate_moments(td3_handle* h, int which);

}  // namespace td3
