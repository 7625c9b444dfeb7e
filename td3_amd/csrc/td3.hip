// Learner state, step planning, hipGraph replay and the td3_* C-ABI (include/td3.h).
//
// Reference mapping (/root/reference):
//   TD3_featured.TD3.__init__   :100-110  -> td3_create (param arenas, targets = copies)
//   TD3_featured.TD3.train      :123-171  -> td3_train_step (the stage list built by build_step)
//   TD3_featured.TD3.select_action :113-115 -> td3_select_action
//   TD3_featured.TD3.eval_q     :117-121  -> td3_eval_q
//   main.py:249-252 (select_action + OU noise + clip) on device rows -> td3_select_action_device;
//   eval_q on device rows -> td3_eval_q_device (asynchronous, nothing crosses the host)
//   TD3_particles.TD3.select_action / eval_q (TD3_particles.py:153-164) on device rows ->
//   td3_select_action_particles_device / td3_eval_q_particles_device (particles read in place)
//   TD3_base save/load         TD3_base.py:26-50 -> td3_get_params / td3_set_params
//
// HBM layout
//   * one fp32 arena per parameter group (actor: 1 MLP; critic: q1 then q2), five
//     parallel copies: params P, targets T, Adam exp_avg M, exp_avg_sq V, grads G.
//     Every Linear weight is stored [pad32(out)][pad32(in)] (zero pads, which stay
//     exactly zero through Adam and Polyak), biases / LayerNorm affines [pad32(out)].
//   * one scratch arena for the batch: padded inputs, per-network activations
//     H (post-ReLU), U (post-LN), LN row stats, and the backward dU / dZ rows.
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

static thread_local char g_err[1024] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

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

// Parameter layout of one network in reference state_dict order.  Featured (TD3_featured.py:
// 15-37 / 50-71): linears.{0..3}, lnorms.{0..2}; with weight normalization (:33-35, 68-70)
// linears.{i}.{bias, weight_g, weight_v} (torch weight_norm's registration order) and no
// lnorms.  Particles (TD3_particles.py:19-50 / 71-101): conv1, conv2, linears.{0..3}, lnorm1,
// lnorms.{0..2}.  norm_kind: 0 None, 1 "layer", 2 "weight_normalization".
static NetL layout_mlp(int in, const int hid[3], int out, int norm_kind, const std::string& prefix,
                       int64_t& off, std::vector<TensorRef>& tensors, int enc_D = 0) {
  NetL n{};
  const bool norm = norm_kind == 1, wn = norm_kind == 2;
  if (enc_D > 0) {
    off = (off + 3) & ~(int64_t)3;           // float4 loads of the conv2 weight
    n.D = enc_D;
    n.enc_off = off;
    tensors.push_back({prefix + "conv1.weight", kEncC1, enc_D, off + EncOff::w1(enc_D), enc_D});
    tensors.push_back({prefix + "conv1.bias", kEncC1, 0, off + EncOff::b1(enc_D), 0});
    tensors.push_back({prefix + "conv2.weight", kEncC2, kEncC1, off + EncOff::w2(enc_D), kEncC1});
    tensors.push_back({prefix + "conv2.bias", kEncC2, 0, off + EncOff::b2(enc_D), 0});
    off += EncOff::size(enc_D);
    off = (off + 31) & ~(int64_t)31;
  }
  int dims[5] = {in, hid[0], hid[1], hid[2], out};
  for (int l = 0; l < 4; ++l) {
    LinearL& L = n.lin[l];
    L.K = dims[l];
    L.N = dims[l + 1];
    L.Kp = pad32(L.K);
    L.Np = pad32(L.N);
    L.offW = off;
    off += (int64_t)L.Np * L.Kp;
    L.offb = off;
    off += L.Np;
    const std::string name = prefix + "linears." + std::to_string(l);
    if (wn) {
      L.offg = off;
      off += L.Np;
      L.offv = off;
      off += (int64_t)L.Np * L.Kp;
      tensors.push_back({name + ".bias", L.N, 0, L.offb, 0});
      tensors.push_back({name + ".weight_g", L.N, 1, L.offg, 1});
      tensors.push_back({name + ".weight_v", L.N, L.K, L.offv, L.Kp});
      continue;
    }
    tensors.push_back({name + ".weight", L.N, L.K, L.offW, L.Kp});
    tensors.push_back({name + ".bias", L.N, 0, L.offb, 0});
  }
  if (enc_D > 0) {
    n.lnin = norm;
    n.ln_in.N = in;
    n.ln_in.Np = pad32(in);
    n.ln_in.offg = off;
    off += n.ln_in.Np;
    n.ln_in.offb = off;
    off += n.ln_in.Np;
    if (norm) {
      tensors.push_back({prefix + "lnorm1.weight", in, 0, n.ln_in.offg, 0});
      tensors.push_back({prefix + "lnorm1.bias", in, 0, n.ln_in.offb, 0});
    }
  }
  for (int l = 0; l < 3; ++l) {
    LNormL& Ln = n.ln[l];
    Ln.N = dims[l + 1];
    Ln.Np = pad32(Ln.N);
    Ln.offg = off;
    off += Ln.Np;
    Ln.offb = off;
    off += Ln.Np;
    if (norm) {
      tensors.push_back({prefix + "lnorms." + std::to_string(l) + ".weight", Ln.N, 0, Ln.offg, 0});
      tensors.push_back({prefix + "lnorms." + std::to_string(l) + ".bias", Ln.N, 0, Ln.offb, 0});
    }
  }
  return n;
}

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

struct Scratch {
  float* base = nullptr;
  size_t cap = 0, used = 0;
  float* take(size_t floats) {
    size_t n = (floats + 63) & ~(size_t)63;
    float* p = base + used;
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
  // featured: the rows' importance weights in the critic loss (target_loss::kW), ones unless the last
  // step was prioritized (per_w_dirty: the next other step refills them, ensure_unit_weights), the
  // rows' |TD error| (kTd) and the injected mass fractions of a prioritized draw
  float *per_w = nullptr, *per_td = nullptr, *per_u = nullptr;
  bool per_w_dirty = false;
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

// Carves an ActPlan's query inputs / outputs from the mapped block, or from the device scratch.
struct IoCarve {
  Scratch* S;
  float* h = nullptr;   // host view of the mapped block
  float* d = nullptr;   // its device address
  size_t used = 0;
  float* take(size_t floats, float** host) {
    if (!h) {
      *host = nullptr;
      return S->take(floats);
    }
    const size_t n = (floats + 63) & ~(size_t)63;
    *host = h + used;
    float* p = d + used;
    used += n;
    return p;
  }
};

static int map_io(ActPlan* A, size_t floats, IoCarve* io) {
  if (A->Bp > kMappedRows) return 0;
  TD3_HIP(hipHostMalloc(&A->hio, floats * 4, hipHostMallocMapped));
  memset(A->hio, 0, floats * 4);
  void* d = nullptr;
  TD3_HIP(hipHostGetDevicePointer(&d, A->hio, 0));
  io->h = A->hio;
  io->d = static_cast<float*>(d);
  return 0;
}

}  // namespace td3

using namespace td3;

struct td3_handle {
  td3_config cfg;
  int sd, ad;                 // featured: state / action dims; particles: feature / action dims
  int particles = 0, N = 0, D = 0, cdq = 1;
  Group actor, critic;
  float* arena = nullptr;
  Counters* d_ctr = nullptr;
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
  std::unique_ptr<Plan> plan;
  std::map<int, std::unique_ptr<ActPlan>> act;
  // Device-resident queries (td3_select_action_device / td3_eval_q_device) run asynchronously on the
  // step stream or a caller's: plans of their own (device I/O only), so a query still in flight never
  // shares scratch with a synchronous host query on the acting stream.  dev_stream: the stream of the
  // last one; a query on another stream waits for dev_ev recorded there (same scratch).
  std::map<int, std::unique_ptr<ActPlan>> act_dev;
  hipStream_t dev_stream = nullptr;
  hipEvent_t dev_ev = nullptr;
  ncclComm_t comm = nullptr;
  // the overlapped data-parallel schedule (add_dw_stage buckets): the all-reduces and the per-bucket
  // optimizer steps run on comm_stream, ordered after the bucket's dW by comm_ev (recorded on the step
  // stream) and joined back by comm_done before the next stage that reads the parameters
  hipStream_t comm_stream = nullptr;
  hipEvent_t comm_ev = nullptr, comm_ev1 = nullptr, comm_done = nullptr;
  std::shared_ptr<LocalGroup> local;          // td3_comm_init_local (comm stays null)
  int nranks = 1, rank = 0;
  bool dp_sharded = false;                    // the plan's optimizer steps are sharded (add_dw_stage)
  bool w4_build = false;                      // the plan being built reads / maintains the k-quad images
  int64_t opt_gathered_it = -1;               // total_it of the last td3_dp_gather_optimizer_state
  std::vector<Stage>* last_body = nullptr;
  Ring* last_ring = nullptr;                  // the ring of the last td3_profile_stages (stage 0: its gather)
  uint64_t last_ring_gen = 0;                 // its Ring::gen (td3_time_stage refuses a destroyed ring)
  // td3_probe_kernel: while set, steps launch directly and every stage launching `probe_kernel` is
  // bracketed by a pair of HIP events on the step's stream (probe_ev[2k], probe_ev[2k + 1])
  bool probing = false;
  bool per_step = false;                      // inside td3_train_step_prioritized: the body keeps its weights
  std::string probe_kernel;
  std::vector<hipEvent_t> probe_ev;
  int probe_used = 0;
  std::vector<std::string> stage_names;
  std::vector<std::string> stage_kernels;
};

namespace td3 {

static int upload(td3_handle* h, std::vector<void*>& owned, const void* host, size_t bytes, void** out) {
  void* d = nullptr;
  TD3_HIP(hipMalloc(&d, bytes));
  TD3_HIP(hipMemcpy(d, host, bytes, hipMemcpyHostToDevice));
  owned.push_back(d);
  *out = d;
  (void)h;
  return 0;
}

static void alloc_eval(Scratch& S, const NetL& n, int Bp, float* X, int ldx, bool bwd, bool norm,
                       bool policy_or_q, EvalB& e) {
  e.X = X;
  e.ldx = ldx;
  for (int l = 0; l < 3; ++l) {
    const int Np = n.lin[l].Np;
    e.H[l] = S.take((size_t)Bp * Np);
    e.U[l] = norm ? S.take((size_t)Bp * Np) : e.H[l];
    e.stats[l] = S.take((size_t)2 * Bp);
    if (bwd) {
      e.GU[l] = S.take((size_t)Bp * Np);
      e.GZ[l] = S.take((size_t)Bp * Np);
    }
  }
  if (bwd) e.GZ[3] = S.take((size_t)Bp * 32);
  if (policy_or_q) {
    e.T = S.take((size_t)Bp * 32);
    e.Qv = S.take((size_t)Bp * 32);
  }
  if (n.D > 0) {
    const int Kp0 = n.lin[0].Kp;
    e.Uin = norm ? S.take((size_t)Bp * Kp0) : X;
    e.statsIn = S.take((size_t)2 * Bp);
    if (bwd) e.GUin = S.take((size_t)Bp * Kp0);
  }
}

static int gemm_lds_bytes(int Kp, int rt = 1) {
  int f = std::max(32 * rt * lds_stride(Kp), kGemmWaves * 32 * 33);
  return f * 4;
}

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

// Algorithmic bytes of a GEMM stage's problems: each weight once (and layer 0's for the fused
// layer-0 stages), the batch rows of A once, the output rows once (real widths, B real rows).
static double gemm_bytes(const GemmProb* p, int n, int pro) {
  const bool l0 = pro == kProL0 || pro == kProL0G;
  double b = 0;
  for (int i = 0; i < n; ++i) {
    const GemmProb& q = p[i];
    b += 4.0 * ((double)q.Nout * q.Kreal + (double)q.B * q.Kreal + (double)q.B * q.Nout);
    if (l0) {
      const int N0p = q.exi[ring_l0::kN0p], K0 = q.exi[ring_l0::kK0];
      b += 4.0 * ((double)N0p * K0 + (double)q.B * K0);
    }
  }
  return b;
}

static int push_gemm_stage(td3_handle* h, std::vector<void*>& owned, std::vector<Stage>& st,
                           std::vector<GemmProb>& probs, int mode, int wn, int pro, int Bp, int lds,
                           int blocks, double flops, const std::string& name, Counters* bump,
                           int bump_actor, const RingSide* rs = nullptr) {
  (void)h;
  (void)owned;
  TD3_ARG(!probs.empty() && probs.size() <= (size_t)kMaxProbs, "too many problems in one gemm stage");
  GemmTable t{};
  for (size_t i = 0; i < probs.size(); ++i) t.p[i] = probs[i];
  t.nprob = (int)probs.size();
  char kname[64];
  snprintf(kname, sizeof(kname), "td3::gemm_kernel<%d, %d, %d>", mode, wn, pro);
  if (rs) {      // the ring bound at launch (capture) time: Plan::rside, filled by bind_ring
    st.push_back({name,
                  [=](hipStream_t s) {
                    GemmTable tt = t;
                    tt.rs = *rs;
                    if (!tt.rs.data) {
                      set_error("internal: ring-sampled stage launched without a bound ring");
                      return -1;
                    }
                    return launch_gemm(mode, wn, pro, tt, blocks, Bp, lds, bump, bump_actor, s);
                  },
                  flops, kname});
    st.back().bytes = gemm_bytes(t.p, t.nprob, pro);
    return 0;
  }
  st.push_back({name,
                [=](hipStream_t s) { return launch_gemm(mode, wn, pro, t, blocks, Bp, lds, bump, bump_actor, s); },
                flops, kname});
  st.back().gemm = std::make_shared<GemmLaunch>(GemmLaunch{mode, wn, pro, t, blocks, Bp, lds, bump == nullptr});
  st.back().bytes = gemm_bytes(t.p, t.nprob, pro);
  return 0;
}

// Run GEMM stage j inside stage i's launch (i < j; stage j must depend on nothing in (i, j) and
// nothing in (i, j) on it).  Forward stage first in the pair.  Left as two launches when the pair
// is not instantiated (gemm2_supported) or either stage binds the ring / bumps the counters.
#ifndef TD3_MERGE_GEMM_PAIRS
#define TD3_MERGE_GEMM_PAIRS 1
#endif
static bool merge_gemm_pair(std::vector<Stage>& st, size_t i, size_t j) {
  if (!TD3_MERGE_GEMM_PAIRS || i >= j || j >= st.size()) return false;
  const std::shared_ptr<GemmLaunch> a0 = st[i].gemm, b0 = st[j].gemm;
  if (!a0 || !b0 || !a0->plain || !b0->plain || a0->Bp != b0->Bp) return false;
  const bool a_first = a0->mode == 0;
  const GemmLaunch f = a_first ? *a0 : *b0, g = a_first ? *b0 : *a0;
  if (!gemm2_supported(f.mode, f.wn, f.pro, g.mode, g.wn, g.pro)) return false;
  Stage m;
  m.name = st[i].name + "+" + st[j].name;
  m.flops = st[i].flops + st[j].flops;
  m.bytes = st[i].bytes + st[j].bytes;
  char kname[96];
  snprintf(kname, sizeof(kname), "td3::gemm2_kernel<%d, %d, %d, %d, %d, %d>", f.mode, f.wn, f.pro, g.mode, g.wn,
           g.pro);
  m.kernel = kname;
  const int lds = std::max(f.lds, g.lds);
  m.run = [=](hipStream_t s) {
    return launch_gemm2(f.mode, f.wn, f.pro, f.t, f.blocks, g.mode, g.wn, g.pro, g.t, g.blocks, f.Bp, lds, s);
  };
  st[i] = m;
  st.erase(st.begin() + (long)j);
  return true;
}

static int stage_index(const std::vector<Stage>& st, const std::string& name) {
  for (size_t k = 0; k < st.size(); ++k)
    if (st[k].name == name) return (int)k;
  return -1;
}

static int push_row_stage(td3_handle* h, std::vector<void*>& owned, std::vector<Stage>& st,
                          std::vector<GemmProb>& probs, int kind, int Bp, const std::string& name) {
  (void)h;
  (void)owned;
  TD3_ARG(!probs.empty() && probs.size() <= (size_t)kMaxProbs, "too many problems in one row stage");
  GemmTable t{};
  for (size_t i = 0; i < probs.size(); ++i) t.p[i] = probs[i];
  t.nprob = (int)probs.size();
  char kname[64];
  snprintf(kname, sizeof(kname), "td3::row_kernel<%d>", kind);
  st.push_back({name, [=](hipStream_t s) { return launch_rows(kind, t, Bp, s); }, 0, kname});
  return 0;
}

// Two independent row stages in one launch: problems [0, n1) of kind1, the rest of kind2.
static int push_row2_stage(std::vector<Stage>& st, std::vector<GemmProb>& probs, int kind1, int kind2, int n1,
                           int Bp, const std::string& name) {
  TD3_ARG(!probs.empty() && probs.size() <= (size_t)kMaxProbs, "too many problems in one row stage");
  TD3_ARG(n1 >= 1 && n1 < (int)probs.size(), "internal: row stage split");
  GemmTable t{};
  for (size_t i = 0; i < probs.size(); ++i) t.p[i] = probs[i];
  t.nprob = (int)probs.size();
  char kname[64];
  snprintf(kname, sizeof(kname), "td3::row_kernel2<%d, %d>", kind1, kind2);
  st.push_back({name, [=](hipStream_t s) { return launch_rows2(kind1, kind2, n1, t, Bp, s); }, 0, kname});
  return 0;
}

// Planner tuning knobs read from the environment when a plan is built (A/B runs; defaults are the
// measured best)
static int env_int(const char* name, int dflt) {
  const char* e = std::getenv(name);
  return e && *e ? std::atoi(e) : dflt;
}

// Output columns per GEMM workgroup.  32 (WN=1, K split 8 ways) gives the shortest MFMA chain,
// right for most latency-bound B=256 stages.  A stage of >= 256 such workgroups is bound by the
// A rows and weights that every 32-column tile re-reads instead:
//   * B >= 512: 128 columns (WN=4, K split 2 ways, wide K streamed chunk by chunk): Humanoid
//     B=1024 2.70k -> 2.92k steps/s, particles B=4096 MLP stages -20 %;
//   * B = 256 forward stages (3-4 networks): 64 columns (WN=2): HalfCheetah F_fwd1 15.0 ->
//     13.8 us, F_fwd2 13.9 -> 12.4 us; WN=4 there is slower (18.3 us), and the input-grad
//     stages (strided weight reads) lose with WN=2 (CB_bwd1 9.0 -> 10.8 us).
// Narrow K (<= 128) always uses WN=4.  A stage of <= 128 32-column workgroups (one- and
// two-network B=256 layers) leaves half the CUs idle: 16 columns per workgroup (WN=0,
// v_mfma_f32_16x16x4_f32) doubles the workgroups and halves each one's MFMA chain.
#ifndef TD3_WN2_MIN
#define TD3_WN2_MIN 256
#endif
#ifndef TD3_WN0_MAX
#define TD3_WN0_MAX 128
#endif
// B >= 512 stages whose 128-column split leaves the chip under-filled (fewer than TD3_WN4_MIN
// workgroups, e.g. a one- or two-network layer: 128 of 256 CUs) take 64-column workgroups when
// those fit about one round (<= TD3_WN2_MAXB): the prologue repeats per column tile but the MFMA
// chain halves (the timeline: MFMA phase ~7.5 us of a 12.6 us TF_fwd2 span on 128 CUs).
// Input-grad stages too (TD3_WN2_BWD; those paired with a forward stage in a dual launch have
// >= 256 WN = 4 workgroups and stay at WN = 4). Humanoid 3.78 k -> 3.94 k steps/s: TF_fwd2 13.7 -> 10.8,
// AF_fwd0 12.6 -> 9.3, AF_fwd1 15.4 -> 11.9, AQB_bwd1 14.6 -> 11.0, AB_bwd1 15.4 -> 12.5 us.
static int gemm_wn(int maxK, int Bp, int wn1_blocks, bool fwd, int wn4_blocks = 0, int wn2_blocks = 0) {
  if (maxK <= 128) return 4;
  if (Bp >= 512 && wn1_blocks >= 256) {
    static const int wn4_min = env_int("TD3_WN4_MIN", 224), wn2_maxb = env_int("TD3_WN2_MAXB", 288);
    static const bool wn2_bwd = env_int("TD3_WN2_BWD", 1) != 0;
    if ((fwd || wn2_bwd) && wn4_blocks > 0 && wn4_blocks < wn4_min && wn2_blocks <= wn2_maxb) return 2;
    return 4;
  }
  if (wn1_blocks <= TD3_WN0_MAX) return 0;
  return (fwd && wn1_blocks >= TD3_WN2_MIN) ? 2 : 1;
}
static int gemm_outw(int wn) { return wn == 0 ? 16 : 32 * wn_cols(wn); }   // output columns per workgroup
// Two 32-row tiles per 128-column workgroup (kWn4x2, one workgroup per CU) against WN = 4 (two
// workgroups per CU): a win only for stages of >= 384 WN = 4 workgroups at B <= 2048 (Humanoid
// F_fwd0 23.9 -> 21.2 us, F_fwd1 30.0 -> 28.8); every smaller stage, and the B = 4096 particle
// MLP stages, lost 10-60 % (fewer waves per SIMD to hide the weight stream).  Plain prologues only.
#ifndef TD3_WN4X2
#define TD3_WN4X2 1
#endif
#ifndef TD3_WN4X2_MIN_BLOCKS
#define TD3_WN4X2_MIN_BLOCKS 384
#endif
static int gemm_wn_rows(int wn, int pro, int Bp, int wn4_blocks) {
  const bool plain = pro == kProCopy || pro == kProLN || pro == kProLNBwd || pro == kProHeadBwd;
  return (TD3_WN4X2 && wn == 4 && plain && Bp >= 512 && Bp <= 2048 && Bp % 64 == 0 &&
          wn4_blocks >= TD3_WN4X2_MIN_BLOCKS) ? kWn4x2 : wn;
}

// Forward layers 0..2 of several networks (one launch per layer); layer 0 copies the
// network input rows, layers 1 and 2 apply the previous layer's LayerNorm in the prologue.
// fuse_l0: layer 0 is recomputed inside the layer-1 launch (kProL0 / kProL0G) when every network's
// input is <= 32 wide (HalfCheetah, Pendulum): one dependent launch fewer per forward chain.
static bool can_fuse_l0(const std::vector<FwdItem>& items) {
  for (auto& it : items) {
    const NetL& n = *it.net;
    if (n.lnin || n.D > 0 || n.lin[0].Kp != 32 || n.lin[0].Np > 512 || n.lin[1].Kp != n.lin[0].Np) return false;
    if (it.ring_src < 0 && (it.e->ldx < 32)) return false;
  }
  return true;
}

// The fused layer-0 stage on 16-row tiles (l0r16_kernel) where it fills the chip in one round:
// 32-column workgroups (8 waves) when those fit 256 (one network: AF_fwd01), else 96-column ones
// (12 waves) or 80-column ones (10 waves) when 16-row tiles of every network fit 256 workgroups,
// else none (the 32-row gemm_body stage).  B < 512 only; TD3_L0R16=0 turns it off.
static bool l0r16_config(const std::vector<FwdItem>& items, int Bp, int* nct, int* wk) {
  static const bool on = env_int("TD3_L0R16", 1) != 0;
  if (!on || Bp >= 512 || Bp % 16) return false;
  int b80 = 0, b32 = 0, b96 = 0;
  for (auto& it : items) {
    const LinearL& L = it.net->lin[1];
    if (L.Kp > 512 || it.net->lin[0].Np != L.Kp) return false;
    b80 += (Bp / 16) * ((L.N + 79) / 80);
    b32 += (Bp / 16) * ((L.N + 31) / 32);
    b96 += (Bp / 16) * ((L.N + 95) / 96);
  }
  static const int maxwg = env_int("TD3_L0R16_MAXWG", 256);
  if (b32 <= 256) {
    *nct = 2;
    *wk = 4;
    return true;
  }
  // 96-column workgroups of 12 waves before 80-column ones of 10: three waves on every SIMD (10
  // waves put three on two SIMDs and two on the others, whose layer-1 MFMA issue then waits for the
  // first two) and the layer-0 tiles over 12 waves (C2 10.77 / 10.78 k -> 10.79 / 10.81 k, C1
  // 10.95 / 10.97 k -> 10.98 / 10.99 k)
  static const bool n96 = env_int("TD3_L0R16_N96", 1) != 0;
  if (n96 && b96 <= 256) {
    *nct = 6;
    *wk = 2;
    return true;
  }
  if (b80 <= maxwg) {
    *nct = 5;
    *wk = 2;
    return true;
  }
  return false;
}

// The k-quad image of an arena copy (nullptr: none, or the plan being built does not use them)
static const float* w4_of(const td3_handle* h, const float* base) {
  if (!h->w4_build) return nullptr;
  for (const Group* g : {&h->actor, &h->critic}) {
    if (base == g->P) return g->P4;
    if (base == g->T) return g->T4;
  }
  return nullptr;
}

// Forward GEMM weight loads from k-quad images (GemmProb::wsk).  An MFMA fragment load puts 16 (or
// 32) consecutive output columns n in the 16 lanes of an access group, each reading 16 B of its own
// weight row: 16 rows' lines per group instruction from the row-major [n][k] arena, 256 contiguous
// bytes from the [k/4][n][4] image.  Measured on C2 with the image addressing of the arena itself
// (TD3_W4FAKE, timing only): 10.08 k -> 10.95 k steps/s; CB_bwd2+TF_fwd01 14.5 -> 11.9 us, odd
// F_fwd01 15.5 -> 12.1, even F_fwd01 18.3 -> 15.9, AF_fwd01 9.7 -> 8.1.  The images are maintained by
// the dW kernels' optimizer epilogues (dw_kernel, dw64 / dw64g, the split-K combine) and, in
// data-parallel plans (flat Adam after the exchange), by a pack stage behind it (push_w4_pack).
// Weight normalization (wn_kernel derives W) and the particle learner read the row-major arena.
// TD3_W4=0 turns them off.
static bool w4_eligible(const td3_handle* h, int Bp) {
  (void)Bp;
  const bool on = env_int("TD3_W4", 1) != 0;     // read at every plan build (tests switch it)
  return on && !h->particles && h->cfg.norm != 2;
}

// The pack of a group's forward weights (layers 0-2: the heads are read by the row kernels) from P
// (and T) into their images
static int w4_pack_args(const Group& g, bool with_t, W4PackArgs* out) {
  W4PackArgs a{};
  a.src[0] = g.P;
  a.dst[0] = g.P4;
  a.src[1] = g.T;
  a.dst[1] = g.T4;
  a.npair = with_t ? 2 : 1;
  for (const NetL& n : g.nets)
    for (int l = 0; l < 3; ++l) {
      const LinearL& L = n.lin[l];
      TD3_ARG(a.nmat < kMaxW4Mats, "internal: too many matrices for the k-quad pack");
      a.off[a.nmat] = L.offW;
      a.Np[a.nmat] = L.Np;
      a.Kp[a.nmat] = L.Kp;
      a.first[a.nmat + 1] = a.first[a.nmat] + (int64_t)L.Np * (L.Kp / 4);
      ++a.nmat;
    }
  *out = a;
  return 0;
}

// Before a w4 plan runs: the images of both groups rebuilt from P / T if anything else wrote those
static int ensure_w4(td3_handle* h, hipStream_t s) {
  if (!h->plan || !h->plan->w4) return 0;
  for (Group* g : {&h->actor, &h->critic}) {
    if (g->w4_valid) continue;
    W4PackArgs a;
    TD3_RC(w4_pack_args(*g, true, &a));
    TD3_RC(launch_w4_pack(a, s));
    g->w4_valid = true;
  }
  return 0;
}

// The flat optimizer's image map of a group's forward weights (P4 null when the plan being built does
// not use the images); `base`: the arena offset of the range it updates
static int w4_map(const td3_handle* h, const Group& g, int64_t base, W4Map* out) {
  W4Map w{};
  if (h->w4_build) {
    w.P4 = g.P4;
    w.T4 = g.T4;
    w.base = base;
    for (const NetL& n : g.nets)
      for (int l = 0; l < 3; ++l) {
        TD3_ARG(w.nmat < 8, "internal: too many matrices for the flat optimizer's image map");
        w.off[w.nmat] = n.lin[l].offW;
        w.Np[w.nmat] = n.lin[l].Np;
        w.Kp[w.nmat] = n.lin[l].Kp;
        ++w.nmat;
      }
  }
  *out = w;
  return 0;
}

// The sharded data-parallel step updates 1/N of P per rank and all-gathers P: the images are
// repacked by a stage of their own behind it (the dW kernels run gradient-only in data-parallel
// plans; the replicated flat optimizer of the all-reduce schedules writes the images itself)
static int push_w4_pack(td3_handle* h, std::vector<Stage>& st, const Group& g, bool polyak, const char* tag) {
  if (!h->w4_build) return 0;
  W4PackArgs a;
  TD3_RC(w4_pack_args(g, polyak, &a));
  st.push_back({std::string(tag) + "_w4", [=](hipStream_t s) { return launch_w4_pack(a, s); }, 0,
                "td3::w4_pack_kernel"});
  return 0;
}

static int add_fwd_stages(td3_handle* h, std::vector<void*>& owned, std::vector<Stage>& st,
                          const std::vector<FwdItem>& items, int Bp, int B, const char* tag,
                          Counters* bump, int bump_actor, const RingSide* ring = nullptr,
                          const RingOut* ro = nullptr, int o_r = 0, bool fuse_l0 = false, bool r16 = false) {
  const bool norm = h->cfg.norm == 1;
  fuse_l0 = fuse_l0 && can_fuse_l0(items);
  for (int l = fuse_l0 ? 1 : 0; l < 3; ++l) {
    std::vector<GemmProb> probs;
    int maxKp = 0;
    int wn1_blocks = 0;
    int wn4_blocks = 0, wn2_blocks = 0;
    for (auto& it : items) {
      maxKp = std::max(maxKp, it.net->lin[l].Kp);
      wn1_blocks += (Bp / 32) * ((it.net->lin[l].Np + 31) / 32);
      wn2_blocks += (Bp / 32) * ((it.net->lin[l].Np + 63) / 64);
      wn4_blocks += (Bp / 32) * ((it.net->lin[l].Np + 127) / 128);
    }
    int wn = gemm_wn(maxKp, Bp, wn1_blocks, true, wn4_blocks, wn2_blocks);
    const bool lnin = items[0].net->lnin;          // TD3_particles lnorm1 on the MLP input
    const bool l0 = fuse_l0 && l == 1;             // this launch also computes layer 0
    const bool gather = ring && (l == 0 || l0);
    int pro = gather ? kProGather : l == 0 ? (lnin ? kProLN : kProCopy) : (norm ? kProLN : kProCopy);
    if (l0) pro = gather ? kProL0G : kProL0;
    wn = gemm_wn_rows(wn, pro, Bp, wn4_blocks);
    const int rt = wn_rt(wn);
    int blocks = 0, lds = 0;
    double flops = 0;
    for (size_t k = 0; k < items.size(); ++k) {
      const FwdItem& it = items[k];
      const LinearL& L = it.net->lin[l];
      GemmProb p{};
      p.norm = norm ? 1 : 0;
      p.B = B;
      if (l == 0) {
        p.A = it.e->X;
        p.lda = it.e->ldx;
        if (lnin) {
          p.lng = it.P + it.net->ln_in.offg;
          p.lnb = it.P + it.net->ln_in.offb;
          p.stats = it.stats ? it.e->statsIn : nullptr;
          if (it.store_u) {
            p.Aout = it.e->Uin;
            p.ldao = L.Kp;
          }
        }
      } else {
        p.A = it.e->H[l - 1];
        p.lda = it.net->lin[l - 1].Np;
        if (norm) {
          p.lng = it.P + it.net->ln[l - 1].offg;
          p.lnb = it.P + it.net->ln[l - 1].offb;
          p.stats = it.stats ? it.e->stats[l - 1] : nullptr;
          if (it.store_u) {
            p.Aout = it.e->U[l - 1];
            p.ldao = L.Kp;
          }
        }
      }
      if (l == 0 && !l0 && !gather && !lnin && it.tcopy) {
        p.ex[ring_l0::kTCopy] = it.tcopy;
        p.exi[ring_l0::kTCol] = it.tcol;
        p.exi[ring_l0::kTN] = it.tn;
      }
      if (gather) {                               // ring outputs (kProGather / kProL0G)
        TD3_ARG(it.ring_src >= 0 && !lnin && ro, "internal: ring-sampled layer without a record field");
        p.exi[ring_l0::kRecOff] = it.ring_src;
        if (l0) {                                 // the first copy of the row: kProGather stores it to Aout
          p.ex[ring_l0::kRowCopy] = ro[k].a;
          p.exi[ring_l0::kLdRowCopy] = ro[k].lda;
        } else {
          p.Aout = ro[k].a;
          p.ldao = ro[k].lda;
        }
        p.ex[ring_l0::kRowCopy2] = ro[k].b;
        p.exi[ring_l0::kLdRowCopy2] = ro[k].ldb;
        p.ex[ring_l0::kReward] = ro[k].r;
        p.ex[ring_l0::kNotDone] = ro[k].nd;
        p.exi[ring_l0::kRecOffRw] = o_r;
      }
      if (l0) {                                   // layer-0 operands
        const LinearL& L0 = it.net->lin[0];
        if (!gather) {
          p.A = it.e->X;
          p.lda = it.e->ldx;
        }
        p.ex[ring_l0::kW0] = const_cast<float*>(it.P + L0.offW);
        p.ex[ring_l0::kB0] = const_cast<float*>(it.P + L0.offb);
        p.ex[ring_l0::kH0] = (it.stats || (!norm && it.store_u)) ? it.e->H[0] : nullptr;
        p.exi[ring_l0::kN0p] = L0.Np;
        p.exi[ring_l0::kK0] = L0.K;
      }
      p.Kreal = L.K;
      p.Kp = L.Kp;
      p.W = it.P + L.offW;
      p.ldw = L.Kp;
      if (const float* q = w4_of(h, it.P)) {     // the k-quad image of the same weights
        p.W = q + L.offW;
        p.ldw = 4;
        p.wsk = 4 * L.Np;
        if (l0) {
          p.ex[ring_l0::kW0] = const_cast<float*>(q + it.net->lin[0].offW);
          p.w0sk = 4 * it.net->lin[0].Np;
        }
      }
      p.bias = it.P + L.offb;
      p.Nout = L.Np;
      p.C = it.e->H[l];
      p.ldc = L.Np;
      p.relu = 1;
      p.ntiles = (L.Np + gemm_outw(wn) - 1) / gemm_outw(wn);
      p.tile_begin = blocks;
      blocks += (Bp / (32 * rt)) * p.ntiles;
      flops += 2.0 * Bp * L.N * L.K;
      // fused layer 0: + the staged input rows and (networks with a backward, norm on: l0_mfma's
      // `keep`) the H0 rows kept for the sliced store
      const bool keep_h0 = l0 && norm && it.stats;
      lds = std::max(lds, gemm_lds_bytes(L.Kp, rt) + (l0 ? 32 * kL0XS * 4 : 0) +
                              (keep_h0 ? 32 * lds_stride(L.Kp) * 4 : 0));
      if (l0) flops += 2.0 * Bp * it.net->lin[0].N * it.net->lin[0].K;
      probs.push_back(p);
    }
    // the step counters are bumped by the launch after the one that draws the sample
    const int bump_l = fuse_l0 ? 2 : 1;
    int nct = 0, wk = 0;
    if (l0 && r16 && l0r16_config(items, Bp, &nct, &wk)) {
      // the same problems on 16-row tiles of 16*nct real layer-1 columns (the pad columns of H1 are
      // zero from the scratch's creation and no stage writes them)
      int nb16 = 0;
      for (auto& p : probs) {
        const int nreal = items[&p - probs.data()].net->lin[1].N;
        p.ntiles = (nreal + 16 * nct - 1) / (16 * nct);
        p.tile_begin = nb16;
        p.Nout = std::min(p.Nout, p.ntiles * 16 * nct);
        nb16 += (Bp / 16) * p.ntiles;
      }
      GemmTable t{};
      for (size_t i = 0; i < probs.size(); ++i) t.p[i] = probs[i];
      t.nprob = (int)probs.size();
      char kname[64];
      snprintf(kname, sizeof(kname), "td3::l0r16_kernel<%d, %d, %s>", nct, wk, gather ? "true" : "false");
      Counters* bmp = l == bump_l ? bump : nullptr;
      const std::string name = std::string(tag) + "_fwd01";
      if (gather) {
        const RingSide* rs = ring;
        st.push_back({name,
                      [=](hipStream_t s) {
                        GemmTable tt = t;
                        tt.rs = *rs;
                        if (!tt.rs.data) {
                          set_error("internal: ring-sampled stage launched without a bound ring");
                          return -1;
                        }
                        return launch_l0r16(nct, wk, 1, tt, nb16, Bp, bmp, bump_actor, s);
                      },
                      flops, kname});
      } else {
        st.push_back({name, [=](hipStream_t s) { return launch_l0r16(nct, wk, 0, t, nb16, Bp, bmp, bump_actor, s); },
                      flops, kname});
      }
      st.back().bytes = gemm_bytes(t.p, t.nprob, pro);
      continue;
    }
    TD3_RC(push_gemm_stage(h, owned, st, probs, 0, wn, pro, Bp, lds, blocks, flops,
                           std::string(tag) + (l0 ? "_fwd01" : "_fwd" + std::to_string(l)),
                           l == bump_l ? bump : nullptr, bump_actor, gather ? ring : nullptr));
  }
  return 0;
}

// dU_1 = dZ_2 * W_2 (dZ_2 built by the fused head prologue `pro2`), dU_0 = dZ_1 * W_1
// (dZ_1 = relu'(LN_bwd(dU_1)) in the prologue), then dZ_0 rows when needed.
// need_in (TD3_particles): dU_in = dZ_0 * W_0 as well (dZ_0 formed in its prologue and kept),
// the input grad that feeds lnorm1's backward, the encoder and dQ1/da; replaces the dZ_0 rows.
static int add_bwd_stages(td3_handle* h, std::vector<void*>& owned, std::vector<Stage>& st,
                          const std::vector<BwdItem>& items, int Bp, int B, const char* tag,
                          bool need_dz0, bool need_in = false,
                          std::vector<GemmProb>* lnbwd_rows = nullptr, float head_bwd_scale = 0.f) {
  const bool norm = h->cfg.norm == 1;
  for (int l = 2; l >= (need_in ? 0 : 1); --l) {
    std::vector<GemmProb> probs;
    int blocks = 0, lds = 0;
    double flops = 0;
    int maxKp = 0;
    int wn1_blocks = 0;
    int wn4_blocks = 0, wn2_blocks = 0;
    for (auto& it : items) {
      maxKp = std::max(maxKp, it.net->lin[l].Np);
      wn1_blocks += (Bp / 32) * ((it.net->lin[l].Kp + 31) / 32);
      wn2_blocks += (Bp / 32) * ((it.net->lin[l].Kp + 63) / 64);
      wn4_blocks += (Bp / 32) * ((it.net->lin[l].Kp + 127) / 128);
    }
    const int pro = l < 2 ? kProLNBwd : head_bwd_scale != 0.f ? kProHeadBwd : kProCopy;
    const int wn = gemm_wn_rows(gemm_wn(maxKp, Bp, wn1_blocks, false, wn4_blocks, wn2_blocks), pro, Bp, wn4_blocks);
    const int rt = wn_rt(wn);
    for (size_t k = 0; k < items.size(); ++k) {
      const BwdItem& it = items[k];
      const LinearL& L = it.net->lin[l];
      GemmProb p{};
      p.norm = norm ? 1 : 0;
      p.B = B;
      if (l == 2 && head_bwd_scale != 0.f) {   // dZ2 formed from H2 by the prologue (kProHeadBwd)
        const NetL& n = *it.net;
        p.A = it.e->H[2];
        p.lda = L.Np;
        p.lng = it.P + n.ln[2].offg;
        p.lnb = it.P + n.ln[2].offb;
        p.ex[head_bwd_pro::kW4] = const_cast<float*>(it.P + n.lin[3].offW);
        p.ex[head_bwd_pro::kB4] = const_cast<float*>(it.P + n.lin[3].offb);
        p.ex[head_bwd_pro::kQ] = it.e->Qv;
        p.exf[head_bwd_pro::kGradScale] = head_bwd_scale;
      } else if (l == 2) {                // dZ2 rows come from the loss / head row kernel
        p.A = it.e->GZ[2];
        p.lda = L.Np;
      } else {
        p.A = it.e->GU[l];
        p.lda = L.Np;
        p.H = it.e->H[l];
        p.ldh = L.Np;
        p.lng = it.P + it.net->ln[l].offg;
        p.stats = it.e->stats[l];
        if (it.store_dz) {
          p.Aout = it.e->GZ[l];
          p.ldao = L.Np;
        }
      }
      p.Kreal = L.N;
      p.Kp = L.Np;
      p.W = it.P + L.offW;
      p.ldw = L.Kp;
      p.Nout = L.Kp;
      p.C = l > 0 ? it.e->GU[l - 1] : it.e->GUin;
      p.ldc = L.Kp;
      p.relu = 0;
      p.ntiles = (L.Kp + gemm_outw(wn) - 1) / gemm_outw(wn);
      p.tile_begin = blocks;
      blocks += (Bp / (32 * rt)) * p.ntiles;
      flops += 2.0 * Bp * L.N * L.K;
      lds = std::max(lds, gemm_lds_bytes(L.Np, rt));
      probs.push_back(p);
    }
    TD3_RC(push_gemm_stage(h, owned, st, probs, 1, wn, pro, Bp, lds, blocks,
                           flops, std::string(tag) + "_bwd" + std::to_string(l), nullptr, 0));
  }
  if (need_dz0 && !need_in && lnbwd_rows) {     // as row problems for a shared row launch (kRowLnBwd)
    for (auto& it : items) {
      const LinearL& L = it.net->lin[0];
      GemmProb p{};
      p.norm = norm ? 1 : 0;
      p.B = B;
      p.ex[ln_bwd::kDU] = it.e->GU[0];
      p.ex[ln_bwd::kH] = it.e->H[0];
      p.ex[ln_bwd::kStats] = it.e->stats[0];
      p.ex[ln_bwd::kGamma] = const_cast<float*>(it.P + it.net->ln[0].offg);
      p.ex[ln_bwd::kDZ] = it.e->GZ[0];
      p.exi[ln_bwd::kLd] = L.Np;
      p.exi[ln_bwd::kK] = L.N;
      lnbwd_rows->push_back(p);
    }
    return 0;
  }
  if (need_dz0 && !need_in) {
    LnBwdTable tab{};
    int np = 0;
    for (auto& it : items) {
      const LinearL& L = it.net->lin[0];
      LnBwdProb p{};
      p.GU = it.e->GU[0];
      p.H = it.e->H[0];
      p.stats = it.e->stats[0];
      p.lng = it.P + it.net->ln[0].offg;
      p.ld = L.Np;
      p.K = L.N;
      p.GZ = it.e->GZ[0];
      if (np == kMaxLnBwd) {
        set_error("%s_lnbwd0: more than %d networks", tag, kMaxLnBwd);
        return -1;
      }
      tab.p[np++] = p;
    }
    const int nrm = norm ? 1 : 0;
    st.push_back({std::string(tag) + "_lnbwd0",
                  [=](hipStream_t s) { return launch_lnbwd_rows(tab, np, Bp, nrm, s); }, 0,
                  "td3::lnbwd_rows_kernel"});
  }
  return 0;
}

// B >= 512 with Bp a multiple of 64: the split-K persistent dW (dwsk_kernel + dwsk_combine_kernel)
// instead of one 64x64 tile per workgroup (dw64g_kernel)
#ifndef TD3_DWSK
#define TD3_DWSK 1
#endif
#ifndef TD3_DWSK_G
#define TD3_DWSK_G 256
#endif
constexpr int kDwSplitWorkgroups = TD3_DWSK_G;   // one per CU of the MI355X
// Matrix tile edge (64; TD3_DWSK_T=128 selects 128 x 128 tiles: slower on Humanoid, 54 vs 45 us) and the cost of a full matrix
// step relative to a vector step (TD3_DWSK_WM, default 6: Humanoid A_dw 28.0 -> 26.2 us, particles C_dw 105 -> 97 us against 8): read when a plan is built, for A/B runs
static int dwsk_tile_edge() { return env_int("TD3_DWSK_T", 64) == 128 ? 128 : 64; }
static int dwsk_matrix_weight() { return std::max(1, env_int("TD3_DWSK_WM", 6)); }

// The overlapped (bucketed) data-parallel dW schedule: TD3_DP_BUCKETS = 0 (default) off; 1 for real
// peers (RCCL, nranks > 1) and the in-process seam; 2 also on a one-rank communicator (bench.py
// --dp-self: the schedule's price without peers).  Off by default: splitting the critic's dW into
// two half-size launches costs ~12 us of GPU time at Humanoid B = 1024, about what
// bucket 0's exchange can hide behind dW_1.  Read when a plan is built.
static bool dp_overlap(const td3_handle* h) {
  const int m = env_int("TD3_DP_BUCKETS", 0);
  if (m <= 0) return false;
  if (h->local) return true;
  return h->comm && (h->nranks > 1 || m >= 2);
}

// The data-parallel optimizer step: sharded (reduce-scatter -> Adam on the rank's 1/N slice ->
// all-gather of the parameters) or all-reduce -> replicated flat Adam.  TD3_DP_SHARD = 0 (default):
// all-reduce -- the form that wins bench.py --dp-self on C2 and C3 while no run with
// RCCL peers has priced the sharded form's second collective call; 1: sharded for more than one
// rank; 2: sharded always (tests, pricing).  Weight normalization and the bucketed schedule keep
// the all-reduce.  Read at plan build.
static bool dp_shard(const td3_handle* h) {
  const int m = env_int("TD3_DP_SHARD", 0);
  return m == 2 || (m == 1 && h->nranks > 1);
}
static int64_t shard_slice(const Group& g, int nranks) { return ((g.size + 4 * nranks - 1) / (4 * nranks)) * 4; }

// The split-K partition of a dW stage's problems (kernels.h DwSplit): every tile's 64-row steps in
// one weighted list, cut evenly over one workgroup per CU; per problem its tm x tm matrix tiles (n tile
// major, so an XCD's consecutive tiles share dZ column blocks), then its 32-column vector tiles.  The
// tile list and the partition are uploaded into `owned`; the partial slab is the plan's (`slab`).
static int make_dw_split(td3_handle* h, std::vector<void*>& owned, const DwArgs& a, SlabRef* slab, DwSplit& out) {
  const int tm = dwsk_tile_edge();
  const int wm = dwsk_matrix_weight();
  std::vector<DwTile> tiles;
  std::vector<int> wt;                          // cost of one 64-row step of the tile
  for (int pi = 0; pi < a.nprob; ++pi) {
    const DwProb& p = a.probs[pi];
    if (p.ntk > 0) {
      for (int nt = 0; nt < (p.Np + tm - 1) / tm; ++nt)
        for (int kt = 0; kt < (p.Kp + tm - 1) / tm; ++kt) {
          tiles.push_back(DwTile{pi, 0, nt, kt});
          // MFMA work of the busiest SIMD (dwsk_matrix128's quadrant map), out of 4 quadrants
          const int an = std::min(tm, p.Np - nt * tm) / 32, ak = std::min(tm, p.Kp - kt * tm) / 32;
          const int q = tm == 128 ? (an > 2 ? 2 : 1) * (ak > 2 ? 2 : 1) : 1;
          wt.push_back(2 + wm * q / 4);
        }
    }
    for (int j = 0; j < p.Np / 32; ++j) {
      tiles.push_back(DwTile{pi, 1, j, 0});
      wt.push_back(1);
    }
  }
  DwSplit k{};
  k.ntile = (int)tiles.size();
  k.S = a.Bp / 64;
  k.G = kDwSplitWorkgroups;
  k.tm = tm;
  k.slot = tm * tm;
  const int units = k.ntile * k.S;
  int64_t wtot = 0;
  for (int w : wt) wtot += (int64_t)w * k.S;
  const int64_t cw = (wtot + k.G - 1) / k.G;
  // unit -> workgroup by the unit's weighted midpoint: nondecreasing, every workgroup ~cw of cost
  std::vector<int> idx(k.G + 1 + 2 * k.ntile, units);   // [wg_unit (G + 1)][tile_wg (2 ntile)]
  std::vector<int> vu(units);
  int64_t pos = 0;
  int vcur = 0;
  idx[0] = 0;
  for (int u = 0; u < units; ++u) {
    const int w = wt[u / k.S];
    const int v = (int)std::min<int64_t>(k.G - 1, (2 * pos + w) / (2 * cw));
    while (vcur < v) idx[++vcur] = u;
    vu[u] = v;
    pos += w;
  }
  for (int t = 0; t < k.ntile; ++t) {
    idx[k.G + 1 + 2 * t] = vu[t * k.S];
    idx[k.G + 1 + 2 * t + 1] = vu[t * k.S + k.S - 1];
  }
  for (int v = 0; v < k.G; ++v)                 // partial slots: the tiles one workgroup's units touch
    if (idx[v] < idx[v + 1]) k.J = std::max(k.J, (idx[v + 1] - 1) / k.S - idx[v] / k.S + 1);
  void* d = nullptr;
  TD3_RC(upload(h, owned, tiles.data(), tiles.size() * sizeof(DwTile), &d));
  k.tiles = static_cast<const DwTile*>(d);
  TD3_RC(upload(h, owned, idx.data(), idx.size() * sizeof(int), &d));
  k.wg_unit = static_cast<const int*>(d);
  k.tile_wg = k.wg_unit + k.G + 1;
  TD3_ARG(slab != nullptr, "internal: split-K dW stage without a plan slab");
  slab->bytes = std::max(slab->bytes, (size_t)k.G * k.J * k.slot * sizeof(float));
  out = k;
  return 0;
}

// Weight / bias / LN grads of every layer of `items`, fused with the optimizer.
// enc (TD3_particles): the encoder partial slabs of `items` (reduced + optimizer in one launch).
// unit_scale (featured critic): per item, the dense [Bp] row scale g_r of its unit-gradient
// backward rows (layers 0..2 and their LayerNorms; the head's dZ is the true gradient already).
static int add_dw_stage(td3_handle* h, std::vector<void*>& owned, std::vector<Stage>& st,
                        Group& g, int which, const std::vector<BwdItem>& items, int Bp,
                        const char* tag, bool polyak, int enc_nwg = 0,
                        const std::vector<const float*>* unit_scale = nullptr, SlabRef* slab = nullptr) {
  const bool norm = h->cfg.norm == 1;
  // B >= 512: 64x64 weight tiles with LDS-staged operands (dw64_kernel: half the operand
  // traffic, Humanoid C_dw 73 -> 63 us), else 32x32 register tiles (dw_kernel: more, shorter
  // workgroups for the latency-bound small batches)
  const bool tile64 = Bp >= 512;
  std::vector<DwProb> probs;
  int blocks = 0;
  double flops = 0;
  double dw_operand_bytes = 0, dw_params = 0, dw_weights = 0;
  TD3_ARG(!unit_scale || unit_scale->size() == items.size(), "internal: one row scale per dW item");
  for (size_t k = 0; k < items.size(); ++k) {
    const BwdItem& it = items[k];
    const NetL& n = *it.net;
    const float* usc = unit_scale ? (*unit_scale)[k] : nullptr;
    for (int l = 0; l < 4; ++l) {
      const LinearL& L = n.lin[l];
      DwProb p{};
      p.rs = (usc && l < 3) ? usc : h->ones;
      p.ldrs = (usc && l < 3) ? 1 : 0;
      p.G = it.e->GZ[l];
      p.ldg = (l == 3) ? 32 : L.Np;
      p.U = (l == 0) ? (n.D > 0 ? it.e->Uin : it.e->X) : it.e->U[l - 1];
      p.ldu = (l == 0) ? ((n.D > 0 && norm) ? L.Kp : it.e->ldx) : n.lin[l - 1].Np;
      p.Np = L.Np;
      p.Kp = L.Kp;
      p.offW = L.offW;
      p.offb = L.offb;
      if (norm && l < 3) {
        p.offg = n.ln[l].offg;
        p.offbeta = n.ln[l].offb;
        p.GU = it.e->GU[l];
        p.ldgu = L.Np;
        p.H = it.e->H[l];
        p.ldh = L.Np;
        p.stats = it.e->stats[l];
      } else {
        p.offg = -1;
        p.offbeta = -1;
      }
      p.kvalid = L.K;                  // layer 0 may read a wider row (the actor's [s | a] input)
      p.ntk = tile64 ? (L.Kp + 63) / 64 : L.Kp / 32;
      p.tile_begin = blocks;
      blocks += (tile64 ? (L.Np + 63) / 64 : L.Np / 32) * p.ntk + L.Np / 32;   // matrix, then vector tiles
      flops += 2.0 * Bp * L.N * L.K;
      // operands once (dZ and U rows; the LayerNorm vector tiles also dU, H and the statistics),
      // then the optimizer's state per parameter (weight, bias, LN affine)
      dw_operand_bytes += 4.0 * Bp * ((double)L.N + L.K) + ((norm && l < 3) ? 4.0 * Bp * (2.0 * L.N + 2.0) : 0.0);
      dw_params += (double)L.N * L.K + L.N + ((norm && l < 3) ? 2.0 * L.N : 0.0);
      dw_weights += (double)L.N * L.K;
      probs.push_back(p);
    }
    if (n.lnin) {                                   // lnorm1 affine grads (vector tiles only)
      DwProb p{};
      p.rs = usc ? usc : h->ones;
      p.ldrs = usc ? 1 : 0;
      p.Np = n.ln_in.Np;
      p.offb = -1;
      p.offg = n.ln_in.offg;
      p.offbeta = n.ln_in.offb;
      p.GU = it.e->GUin;
      p.ldgu = n.lin[0].Kp;
      p.H = it.e->X;
      p.ldh = it.e->ldx;
      p.stats = it.e->statsIn;
      p.ntk = 0;
      p.kvalid = 0;
      p.tile_begin = blocks;
      blocks += p.Np / 32;
      probs.push_back(p);
    }
  }
  TD3_ARG(probs.size() <= (size_t)kMaxDwProbs, "too many problems in one dw stage");
  DwArgs a{};
  for (size_t i = 0; i < probs.size(); ++i) a.probs[i] = probs[i];
  a.nprob = (int)probs.size();
  a.Bp = Bp;
  a.adam.P = g.P;
  a.adam.G = g.G;
  a.adam.M = g.M;
  a.adam.V = g.V;
  a.adam.T = g.T;
  a.adam.ctr = h->d_ctr;
  a.adam.which = which;
  a.adam.lr = h->adam[which].lr;
  a.adam.beta1 = h->adam[which].beta1;
  a.adam.beta2 = h->adam[which].beta2;
  a.adam.eps = h->adam[which].eps;
  a.adam.tau = (float)h->cfg.tau;
  a.adam.grad_scale = 1.0f;
  if (h->w4_build) {                       // the dW kernels keep the k-quad images current
    TD3_ARG(g.P4 && g.T4, "internal: k-quad images not allocated");
    a.adam.P4 = g.P4;
    a.adam.T4 = g.T4;
  }
  const bool dp = h->comm != nullptr || h->local != nullptr;
  const bool wn = g.wn.nlin > 0;            // weight normalization: dW -> (dg, dv) in wn_kernel
  a.mode = (dp || wn) ? kDwGrad : (polyak ? kDwAdamPolyak : kDwAdam);
  // a launch's algorithmic bytes: gradient-only dW writes 4 B per parameter; the fused Adam reads and
  // writes P, M, V (24 B; the gradient never leaves registers), Polyak reads and writes T (+8 B), and
  // the k-quad images take every updated weight once more (+4 B, +4 B more for T4 on Polyak steps)
  const double dw_bytes =
      dw_operand_bytes +
      (a.mode == kDwGrad ? 4.0 * dw_params
                         : dw_params * (a.mode == kDwAdamPolyak ? 32.0 : 24.0) +
                               (h->w4_build ? dw_weights * (a.mode == kDwAdamPolyak ? 8.0 : 4.0) : 0.0));
  a.tile64 = tile64 ? 1 : 0;
  a.scaled = unit_scale ? 1 : 0;
  const int tm = dwsk_tile_edge();
  const bool split = tile64 && Bp % 64 == 0 && TD3_DWSK;
  if (dp && split && !wn && enc_nwg == 0 && items.size() == 2 && dp_overlap(h)) {
    // The overlapped data-parallel schedule for a twin critic: one bucket per network
    // in arena order.  Stages: dW_0 (split-K, gradient only; then an event on the step stream),
    // dW_1 (then a second event), bucket 0's all-reduce + Adam (+ Polyak) on the comm stream behind
    // the first event, bucket 1's on the comm stream behind the second (one RCCL stream per
    // communicator: ADVICE r04), then the join (the step stream waits for bucket 1's Adam).
    // Bucket 0's exchange runs under dW_1; dW_1 is enqueued before the host makes bucket 0's RCCL
    // call.  The in-process seam runs the same buckets: a fixed-order sum of the range, then the
    // bucket's optimizer step (Stage::after), on its one stream.
    const bool local = h->local != nullptr;
    ncclComm_t comm = h->comm;
    hipStream_t cs = h->comm_stream;
    hipEvent_t ev = h->comm_ev, ev1 = h->comm_ev1, done = h->comm_done;
    TD3_ARG(local || (cs && ev && ev1 && done), "internal: data-parallel handle without a comm stream");
    const int pol = polyak ? 1 : 0;
    const std::string kname = std::string("td3::dwsk_kernel<") + (unit_scale ? "true, " : "false, ") +
                              (tm == 128 ? "true>" : "false>");
    int p0 = 0;
    std::vector<Stage> exch;                        // bucket b's exchange stage
    for (size_t b = 0; b < items.size(); ++b) {
      const NetL& n = *items[b].net;
      const int cnt = 4 + (n.lnin ? 1 : 0);
      DwArgs ab = a;
      ab.nprob = cnt;
      double fb = 0;
      for (int i = 0; i < cnt; ++i) {
        ab.probs[i] = a.probs[p0 + i];
        if (i < 4) fb += 2.0 * Bp * n.lin[i].N * n.lin[i].K;
      }
      p0 += cnt;
      DwSplit kb{};
      TD3_RC(make_dw_split(h, owned, ab, slab, kb));
      const bool first = b == 0;
      const std::string bn = std::string(tag) + "_dw_" + std::to_string(b);
      st.push_back({bn,
                    [=](hipStream_t s) {
                      DwSplit kk = kb;
                      kk.slab = slab->p;
                      TD3_RC(launch_dw_split(ab, kk, s));
                      if (!local) TD3_HIP(hipEventRecord(first ? ev : ev1, s));
                      return 0;
                    },
                    fb, kname});
      const int64_t off = n.enc_off >= 0 ? n.enc_off : n.lin[0].offW;
      const int64_t end = b + 1 < items.size()
                              ? (items[b + 1].net->enc_off >= 0 ? items[b + 1].net->enc_off : items[b + 1].net->lin[0].offW)
                              : g.size;
      TD3_ARG(off >= 0 && end > off && end <= g.size, "internal: bucket range");
      const int64_t nb = end - off;
      AdamArgs ar = a.adam;
      ar.P += off; ar.G += off; ar.M += off; ar.V += off; ar.T += off;
      W4Map wm;
      TD3_RC(w4_map(h, g, off, &wm));
      ar.grad_scale = 1.0f / (float)h->nranks;
      float* Gb = g.G + off;
      Stage x{std::string(tag) + "_" + std::to_string(b) + "_allreduce",
              [=](hipStream_t s) {
                if (local) {
                  set_error("a td3_comm_init_local replica steps through td3_train_step_local only");
                  return -1;
                }
                // both buckets on the comm stream (one RCCL stream per communicator),
                // each behind its own dW; the join waits for the last bucket's Adam
                TD3_HIP(hipStreamWaitEvent(cs, first ? ev : ev1, 0));
                ncclResult_t r = ncclAllReduce(Gb, Gb, (size_t)nb, ncclFloat, ncclSum, comm, cs);
                if (r != ncclSuccess) {
                  set_error("ncclAllReduce: %s", ncclGetErrorString(r));
                  return -2;
                }
                TD3_RC(launch_adam_flat(ar, nb, pol, cs, &wm));
                if (!first) TD3_HIP(hipEventRecord(done, cs));
                return 0;
              },
              0, "rccl"};
      x.collective = which == 1 ? 0 : 1;
      x.coll_off = off;
      x.coll_n = nb;
      x.after = [=](hipStream_t s) { return launch_adam_flat(ar, nb, pol, s, &wm); };
      exch.push_back(x);
    }
    for (auto& x : exch) st.push_back(x);          // dW_0, dW_1, exchange 0 (comm), exchange 1 (step)
    st.push_back({std::string(tag) + "_join",
                  [=](hipStream_t s) {
                    if (local) return 0;            // the seam ran the buckets on its stream
                    TD3_HIP(hipStreamWaitEvent(s, done, 0));
                    return 0;
                  },
                  0, "(stream join)"});
    return 0;
  }
  if (split) {
    DwSplit k{};
    TD3_RC(make_dw_split(h, owned, a, slab, k));
    st.push_back({std::string(tag) + "_dw",
                  [=](hipStream_t s) {
                    DwSplit kk = k;
                    kk.slab = slab->p;
                    return launch_dw_split(a, kk, s);
                  },
                  flops,
                  std::string("td3::dwsk_kernel<") + (unit_scale ? "true, " : "false, ") +
                      (tm == 128 ? "true>" : "false>")});
    st.back().bytes = dw_bytes;
  } else {
    st.push_back({std::string(tag) + "_dw", [=](hipStream_t s) { return launch_dw(a, blocks, s); }, flops,
                  std::string(tile64 ? "td3::dw64_kernel<" : "td3::dw_kernel<") + (unit_scale ? "true>" : "false>")});
    st.back().bytes = dw_bytes;
  }
  if (enc_nwg > 0) {
    EncAdamArgs ea{};
    for (auto& it : items) {
      if (it.net->D <= 0) continue;
      TD3_ARG(ea.nprob < 3, "too many encoders in one dw stage");
      ea.p[ea.nprob].partial = it.e->partial;
      ea.p[ea.nprob].off = it.net->enc_off;
      ea.nprob++;
    }
    ea.nwg = enc_nwg;
    ea.size = EncOff::size(items[0].net->D);
    ea.adam = a.adam;
    ea.mode = a.mode;
    st.push_back({std::string(tag) + "_enc_adam", [=](hipStream_t s) { return launch_enc_adam(ea, s); }, 0,
                  "td3::enc_adam_kernel"});
  }
  AdamArgs aa = a.adam;
  if (dp) aa.grad_scale = 1.0f / (float)h->nranks;
  const int pol = polyak ? 1 : 0;
  if (dp && !wn && dp_shard(h)) {
    // Sharded optimizer step (ZeRO-1 form): the summed gradient reaches only this
    // rank's slice (ncclReduceScatter, in place), Adam runs on that slice alone (the moments of the
    // other slices live on their owners), ncclAllGather brings every rank the updated parameters,
    // then Polyak runs replicated over the whole arena (the same inputs on every rank: the replicas
    // stay bit-identical, each element computed once).  Same bytes on the links as the all-reduce,
    // one extra collective launch, 1/N of the Adam pass.
    const int N = h->nranks, R = h->rank;
    const int64_t slice = shard_slice(g, N);
    TD3_ARG(N * slice <= g.cap, "internal: shard slices past the arena");
    h->dp_sharded = true;
    ncclComm_t comm = h->comm;
    float* G = g.G;
    float* Pp = g.P;
    const bool local = h->local != nullptr;
    AdamArgs as = aa;
    as.P += R * slice; as.G += R * slice; as.M += R * slice; as.V += R * slice; as.T += R * slice;
    Stage x{std::string(tag) + "_rs_adam_ag",
            [=](hipStream_t s) {
              if (local) {
                set_error("a td3_comm_init_local replica steps through td3_train_step_local only");
                return -1;
              }
              ncclResult_t r = ncclReduceScatter(G, G + R * slice, (size_t)slice, ncclFloat, ncclSum, comm, s);
              if (r != ncclSuccess) {
                set_error("ncclReduceScatter: %s", ncclGetErrorString(r));
                return -2;
              }
              TD3_RC(launch_adam_flat(as, slice, 0, s));
              r = ncclAllGather(Pp + R * slice, Pp, (size_t)slice, ncclFloat, comm, s);
              if (r != ncclSuccess) {
                set_error("ncclAllGather: %s", ncclGetErrorString(r));
                return -2;
              }
              return 0;
            },
            0, "rccl"};
    x.collective = which == 1 ? 0 : 1;
    x.coll_slice = slice;
    x.after = [=](hipStream_t s) { return launch_adam_flat(as, slice, 0, s); };
    st.push_back(x);
    if (polyak && h->w4_build) {        // Polyak and both images in one pass over the gathered arena
      float* Tp = g.T;
      const int64_t n = g.size;
      const float tau = (float)h->cfg.tau;
      W4Map wm;
      TD3_RC(w4_map(h, g, 0, &wm));
      st.push_back({std::string(tag) + "_polyak", [=](hipStream_t s) { return launch_polyak_w4(Tp, Pp, n, tau, wm, s); },
                    0, "td3::polyak_w4_kernel"});
      return 0;
    }
    if (polyak) {
      float* Tp = g.T;
      const int64_t n = g.size;
      const float tau = (float)h->cfg.tau;
      st.push_back({std::string(tag) + "_polyak", [=](hipStream_t s) { return launch_polyak_flat(Tp, Pp, n, tau, s); },
                    0, "td3::polyak_flat_kernel"});
    }
    TD3_RC(push_w4_pack(h, st, g, false, tag));
    return 0;
  }
  if (dp) {
    ncclComm_t comm = h->comm;
    float* G = g.G;
    const int64_t n = g.size;
    const bool local = h->local != nullptr;
    st.push_back({std::string(tag) + "_allreduce",
                  [=](hipStream_t s) {
                    if (local) {
                      set_error("a td3_comm_init_local replica steps through td3_train_step_local only");
                      return -1;
                    }
                    ncclResult_t r = ncclAllReduce(G, G, (size_t)n, ncclFloat, ncclSum, comm, s);
                    if (r != ncclSuccess) {
                      set_error("ncclAllReduce: %s", ncclGetErrorString(r));
                      return -2;
                    }
                    return 0;
                  },
                  0, "rccl"});
    st.back().collective = which == 1 ? 0 : 1;     // AdamArgs::which 1 = actor -> group 0
  }
  if (wn) {
    WnArgs w = g.wn;
    w.adam = aa;
    w.mode = kWnAdam;
    w.polyak = pol;
    st.push_back({std::string(tag) + "_wn", [=](hipStream_t s) { return launch_wn(w, s); }, 0, "td3::wn_kernel"});
  } else if (dp) {
    const int64_t n = g.size;
    W4Map wm;
    TD3_RC(w4_map(h, g, 0, &wm));
    st.push_back({std::string(tag) + "_adam",
                  [=](hipStream_t s) { return launch_adam_flat(aa, n, pol, s, &wm); }, 0,
                  "td3::adam_flat_kernel"});
  }
  return 0;
}

static int alloc_dw_slab(Plan* P) {
  if (!P->dwslab.bytes) return 0;
  void* d = nullptr;
  TD3_HIP(hipMalloc(&d, P->dwslab.bytes));
  P->tables.push_back(d);
  P->dwslab.p = static_cast<float*>(d);
  return 0;
}

static void free_plan_tables(std::vector<void*>& t) {
  for (void* p : t) (void)hipFree(p);
  t.clear();
}

static void destroy_plan(Plan* p) {
  if (!p) return;
  for (int a = 0; a < 2; ++a) {
    for (int b = 0; b < 2; ++b) {
      if (p->graph[a][b]) (void)hipGraphExecDestroy(p->graph[a][b]);
      if (p->graph_g[a][b]) (void)hipGraphExecDestroy(p->graph_g[a][b]);
    }
  }
  free_plan_tables(p->tables);
  if (p->scratch) (void)hipFree(p->scratch);
}

static size_t eval_floats(const NetL& n, int Bp, bool bwd, bool norm) {
  size_t f = 0;
  if (n.D > 0) f += (size_t)Bp * n.lin[0].Kp * 2 + 2 * (size_t)Bp + 256;
  for (int l = 0; l < 3; ++l) {
    size_t np = (size_t)Bp * n.lin[l].Np;
    f += np + 64;
    if (norm) f += np + 64;
    f += 2 * (size_t)Bp + 64;
    if (bwd) f += 2 * (np + 64);
  }
  f += (size_t)Bp * 32 * 3 + 256;
  return f;
}

// The LN3 + head operands (ln3_head slots) of network n (arena Pp) evaluated into e
static void set_ln3_head(GemmProb& p, const float* Pp, const NetL& n, const EvalB& e) {
  p.ex[ln3_head::kH3] = e.H[2];
  p.ex[ln3_head::kGamma3] = const_cast<float*>(Pp + n.ln[2].offg);
  p.ex[ln3_head::kBeta3] = const_cast<float*>(Pp + n.ln[2].offb);
  p.ex[ln3_head::kW4] = const_cast<float*>(Pp + n.lin[3].offW);
  p.ex[ln3_head::kB4] = const_cast<float*>(Pp + n.lin[3].offb);
  p.exi[ln3_head::kK3] = n.lin[2].N;
  p.exi[ln3_head::kLd3] = n.lin[2].Np;
}

// The actor's head / LN3 operands and outputs shared by kRowActorHeadBwd and kRowActorHeadBwdP
// (actor_bwd slots): the actor (arena Pa) evaluated into e, its action at column acol of the Q1 input
static void set_actor_bwd(GemmProb& p, const float* Pa, const NetL& an, const EvalB& e, int acol, int ad,
                          float max_action) {
  p.ex[actor_bwd::kTanh] = e.T;
  p.ex[actor_bwd::kW4] = const_cast<float*>(Pa + an.lin[3].offW);
  p.ex[actor_bwd::kH3] = e.H[2];
  p.ex[actor_bwd::kStats3] = e.stats[2];
  p.ex[actor_bwd::kGamma3] = const_cast<float*>(Pa + an.ln[2].offg);
  p.ex[actor_bwd::kDZ4] = e.GZ[3];
  p.ex[actor_bwd::kDU3] = e.GU[2];
  p.Aout = e.GZ[2];
  p.ldao = an.lin[2].Np;
  p.exi[actor_bwd::kActCol] = acol;
  p.exi[actor_bwd::kAd] = ad;
  p.exi[actor_bwd::kK3] = an.lin[2].N;
  p.exi[actor_bwd::kLd3] = an.lin[2].Np;
  p.exi[actor_bwd::kLdw4] = an.lin[3].Kp;
  p.exf[actor_bwd::kMaxAction] = max_action;
}

// Where a policy head puts its action, and how: columns [acol, acol + ad) of the ld-strided rows of
// out (and out2, nullable); clamp: a' to +-max_action
struct PolicyDst {
  float* out; float* out2; int ld, acol;
  int clamp; float max_action;
};
// kRowPolicyHead problem: the actor (arena Pp) evaluated into e; target: smoothing noise (drawn
// here when gen_noise, else read from the plan's noise rows)
static GemmProb policy_head_prob(const td3_handle* h, const Plan& pl, const float* Pp, const EvalB& e,
                                 const PolicyDst& d, int target, int gen_noise) {
  namespace ph = policy_head;
  const NetL& an = h->actor.nets[0];
  GemmProb p{};
  p.norm = h->cfg.norm == 1 ? 1 : 0;
  p.B = pl.B;
  set_ln3_head(p, Pp, an, e);
  p.ex[ph::kNoise] = pl.noise;
  p.ex[ph::kOut] = d.out;
  p.ex[ph::kTanh] = e.T;
  p.ex[ph::kU3] = e.U[2];
  p.ex[ph::kStats3] = e.stats[2];
  p.ex[ph::kOut2] = d.out2;
  p.exi[ph::kLdw4] = an.lin[3].Kp;
  p.exi[ph::kLdOut] = d.ld;
  p.exi[ph::kGenNoise] = gen_noise;
  p.exi[ph::kAd] = h->ad;
  p.exi[ph::kActCol] = d.acol;
  p.exi[ph::kLdNoise] = h->ad;
  p.exi[ph::kTarget] = target;
  p.exi[ph::kClamp] = d.clamp;
  p.exf[ph::kMaxAction] = d.max_action;
  p.exf[ph::kPolicyNoise] = (float)h->cfg.policy_noise;
  p.exf[ph::kNoiseClip] = (float)h->cfg.noise_clip;
  p.seed = h->cfg.seed;
  p.ctr = h->d_ctr;
  return p;
}

static int build_step(td3_handle* h, int B) {
  std::unique_ptr<Plan> P(new Plan());
  const int Bp = pad32(B);
  P->B = B;
  P->Bp = Bp;
  h->w4_build = w4_eligible(h, Bp);
  P->w4 = h->w4_build;
  const bool norm = h->cfg.norm == 1;
  const int sd = h->sd, ad = h->ad;
  P->ld_sa = pad32(sd + ad);
  P->fuse_gather = 2 * sd + ad + 2 <= 128;
  const NetL& an = h->actor.nets[0];
  const NetL& q1 = h->critic.nets[0];
  const NetL& q2 = h->critic.nets[1];
  size_t floats = (size_t)Bp * 3 * P->ld_sa + 13 * (size_t)Bp + (size_t)Bp * ad + 4096 + 192 + (size_t)ad * q1.lin[0].Np;
  floats += eval_floats(an, Bp, false, norm) + 2 * eval_floats(q1, Bp, true, norm) +
            eval_floats(an, Bp, true, norm) + 2 * eval_floats(q1, Bp, false, norm) +
            eval_floats(q1, Bp, true, norm) + 1024;
  P->scratch_bytes = floats * sizeof(float);
  TD3_HIP(hipMalloc(&P->scratch, P->scratch_bytes));
  TD3_HIP(hipMemset(P->scratch, 0, P->scratch_bytes));
  TD3_HIP(hipDeviceSynchronize());   // null-stream memset vs the non-blocking step stream
  Scratch S{P->scratch, floats, 0};
  // network inputs: [s | a] (twin, and the actor reads its first sd columns: the dW of its layer 0
  // masks columns >= sd, DwProb::kvalid), [s' | a'] (target twin; the target actor reads s' there),
  // [s | pi(s)] (Q1 of the actor loss).  Columns past a row's fields are zero.
  P->X_SA = S.take((size_t)Bp * P->ld_sa);
  P->X_S2A = S.take((size_t)Bp * P->ld_sa);
  P->X_SP = S.take((size_t)Bp * P->ld_sa);
  P->R = S.take(Bp);
  P->ND = S.take(Bp);
  P->noise = S.take((size_t)Bp * ad);
  P->Y = S.take(Bp);
  P->sqerr = S.take(2 * (size_t)Bp);
  P->d_idx = (int64_t*)S.take(2 * (size_t)Bp);
  P->d_inject_idx = (int64_t*)S.take(2 * (size_t)Bp);
  P->gscale[0] = S.take(Bp);
  P->gscale[1] = S.take(Bp);
  P->per_w = S.take(Bp);
  P->per_td = S.take(Bp);
  P->per_u = S.take(Bp);
  {
    const std::vector<float> ones((size_t)Bp, 1.0f);
    TD3_HIP(hipMemcpy(P->per_w, ones.data(), (size_t)Bp * sizeof(float), hipMemcpyHostToDevice));
  }
  P->W1aT = S.take((size_t)ad * q1.lin[0].Np);
  alloc_eval(S, an, Bp, P->X_S2A, P->ld_sa, false, norm, false, P->TA);
  alloc_eval(S, q1, Bp, P->X_SA, P->ld_sa, true, norm, true, P->Q[0]);
  alloc_eval(S, q2, Bp, P->X_SA, P->ld_sa, true, norm, true, P->Q[1]);
  alloc_eval(S, an, Bp, P->X_SA, P->ld_sa, true, norm, true, P->A);
  alloc_eval(S, q1, Bp, P->X_S2A, P->ld_sa, false, norm, true, P->TQ[0]);
  alloc_eval(S, q2, Bp, P->X_S2A, P->ld_sa, false, norm, true, P->TQ[1]);
  alloc_eval(S, q1, Bp, P->X_SP, P->ld_sa, true, norm, true, P->AQ);
  if (S.used > S.cap) {
    set_error("internal: scratch overflow (%zu > %zu)", S.used, S.cap);
    return -2;
  }

  // Layout offsets are absolute inside each group arena, so every network of a group
  // uses the group's base pointer (q1 and q2 simply have different offsets).
  const float* Pa = h->actor.P;
  const float* Pta = h->actor.T;
  const float* Pq1 = h->critic.P;
  const float* Pq2 = h->critic.P;
  const float* Ptq1 = h->critic.T;
  const float* Ptq2 = h->critic.T;

  const float ma = h->cfg.max_action;
  // a' = clamp(ma tanh + noise) (TD3_featured.py:131-137) / pi(s) into the action columns of a critic input
  auto policy_head = [&](const float* Pp, EvalB& e, float* out, int target, int gen_noise) {
    return policy_head_prob(h, *P, Pp, e, {out, nullptr, P->ld_sa, sd, 1, ma}, target, gen_noise);
  };

  for (int actor_phase = 0; actor_phase < 2; ++actor_phase) {
    for (int inj = 0; inj < 2; ++inj) {
      std::vector<Stage>& st = P->body[actor_phase][inj];
      // ---- forward of target actor (s'), online twin (s, a), online actor (s) on policy steps
      std::vector<FwdItem> f1 = {{&an, Pta, &P->TA, false, false}, {&q1, Pq1, &P->Q[0], true, true},
                                 {&q2, Pq2, &P->Q[1], true, true}};
      if (actor_phase) f1.push_back({&an, Pa, &P->A, true, true});
      TD3_RC(add_fwd_stages(h, P->tables, st, f1, Bp, B, "F", h->d_ctr, actor_phase, nullptr, nullptr, 0, true,
                            true));
      {  // the ring-sampled first layer (record layout [s | a | s' | r | not_done], replay.hip)
        // the first column tile of each problem keeps what the later stages read: the target-twin
        // input s' (X_S2A), the twin (and actor) dW input [s | a] (X_SA), reward / not_done, and on
        // policy steps the policy-Q input s (X_SP)
        std::vector<FwdItem> f1r = f1;
        f1r[0].ring_src = sd + ad;                   // target actor on s'
        f1r[1].ring_src = 0;                         // twin on [s | a]
        f1r[2].ring_src = 0;
        if (actor_phase) f1r[3].ring_src = 0;        // actor on s
        std::vector<Stage> fr;
        RingOut ro[4] = {{P->X_S2A, P->ld_sa, nullptr, 0, nullptr, nullptr},
                         {P->X_SA, P->ld_sa, nullptr, 0, nullptr, nullptr},
                         {nullptr, 0, nullptr, 0, P->R, P->ND},
                         {P->X_SP, P->ld_sa, nullptr, 0, nullptr, nullptr}};
        TD3_RC(add_fwd_stages(h, P->tables, fr, f1r, Bp, B, "F", h->d_ctr, actor_phase, &P->rside, ro,
                              2 * sd + ad, true, true));
        P->body_ring[actor_phase][inj].push_back(fr[0]);
      }
      // Critic phase on unit loss gradients (kRowUnitLoss): the twin's input-grad chain runs
      // between the heads and the target twin, independent of y; the target-loss row stage
      // (y, g_j = 2/B (Q_j - y)) shares its launch with the layer-0 LN backward rows, and the
      // dW stage scales the unit rows by g_j.  One launch fewer than the sequential order
      // (heads -> target twin -> critic loss -> input grads -> dW).
      {
        std::vector<GemmProb> hp = {policy_head(Pta, P->TA, P->X_S2A, 1, inj ? 0 : 1)};
        if (actor_phase) hp.push_back(policy_head(Pa, P->A, P->X_SP, 0, 0));
        const int n1 = (int)hp.size();
        for (int j = 0; j < 2; ++j) {
          const NetL& qj = j ? q2 : q1;
          GemmProb p{};
          p.norm = norm ? 1 : 0;
          p.B = B;
          set_ln3_head(p, Pq1, qj, P->Q[j]);
          p.ex[unit_loss::kQ] = P->Q[j].Qv;
          p.ex[unit_loss::kU3] = P->Q[j].U[2];
          p.ex[unit_loss::kStats3] = P->Q[j].stats[2];
          p.ex[unit_loss::kDU3] = P->Q[j].GU[2];
          p.Aout = P->Q[j].GZ[2];
          p.ldao = qj.lin[2].Np;
          hp.push_back(p);
        }
        TD3_RC(push_row2_stage(st, hp, kRowPolicyHead, kRowUnitLoss, n1, Bp, "heads"));
      }
      std::vector<BwdItem> cb = {{&q1, Pq1, &P->Q[0], true}, {&q2, Pq2, &P->Q[1], true}};
      std::vector<GemmProb> rows;
      {   // the target loss row problem first (kRowTargetLoss), the LN0 backward rows after it
        GemmProb p{};
        p.norm = norm ? 1 : 0;
        p.B = B;
        namespace tl = target_loss;
        for (int j = 0; j < 2; ++j) {
          const NetL& qj = j ? q2 : q1;
          const float* Ptq = j ? Ptq2 : Ptq1;
          p.ex[tl::kH3 + j] = P->TQ[j].H[2];
          p.ex[tl::kGamma3 + j] = const_cast<float*>(Ptq + qj.ln[2].offg);
          p.ex[tl::kBeta3 + j] = const_cast<float*>(Ptq + qj.ln[2].offb);
          p.ex[tl::kW4 + j] = const_cast<float*>(Ptq + qj.lin[3].offW);
          p.ex[tl::kB4 + j] = const_cast<float*>(Ptq + qj.lin[3].offb);
          p.ex[tl::kQ + j] = P->Q[j].Qv;
          p.ex[tl::kDZ4 + j] = P->Q[j].GZ[3];
          p.ex[tl::kG + j] = P->gscale[j];
        }
        p.ex[tl::kReward] = P->R;
        p.ex[tl::kNotDone] = P->ND;
        p.ex[tl::kY] = P->Y;
        p.ex[tl::kSqErr] = P->sqerr;
        p.ex[tl::kW] = P->per_w;
        p.ex[tl::kTd] = P->per_td;
        p.exi[tl::kK3] = q1.lin[2].N;
        p.exi[tl::kLd3] = q1.lin[2].Np;
        p.exf[tl::kDiscount] = (float)h->cfg.discount;
        p.exf[tl::kGradScale] = (float)(2.0 / (double)B);
        rows.push_back(p);
      }
      TD3_RC(add_bwd_stages(h, P->tables, st, cb, Bp, B, "CB", true, false, &rows));
      std::vector<FwdItem> f2 = {{&q1, Ptq1, &P->TQ[0], false, false}, {&q2, Ptq2, &P->TQ[1], false, false}};
      TD3_RC(add_fwd_stages(h, P->tables, st, f2, Bp, B, "TF", nullptr, 0, nullptr, nullptr, 0, true));
      {   // the unit backward's input-grad stages share launches with the target twin's layers, in
          // order: TF layer k moves up to CB stage k only while every earlier TF layer moved too
        const char* cbn[2] = {"CB_bwd2", "CB_bwd1"};
        std::vector<std::string> tfn;
        for (const char* n : {"TF_fwd0", "TF_fwd01", "TF_fwd1", "TF_fwd2"})
          if (stage_index(st, n) >= 0) tfn.push_back(n);
        for (size_t k = 0; k < 2 && k < tfn.size(); ++k) {
          const int i = stage_index(st, cbn[k]), j = stage_index(st, tfn[k]);
          if (i < 0 || j <= i || !merge_gemm_pair(st, (size_t)i, (size_t)j)) break;
        }
      }
      TD3_RC(push_row2_stage(st, rows, kRowTargetLoss, kRowLnBwd, 1, Bp, "critic_loss"));
      const std::vector<const float*> usc = {P->gscale[0], P->gscale[1]};
      TD3_RC(add_dw_stage(h, P->tables, st, h->critic, 0, cb, Bp, "C", actor_phase != 0, 0, &usc, &P->dwslab));
      if (!actor_phase) continue;
      // ---------------- delayed policy update (TD3_featured.py:156-171)
      std::vector<FwdItem> f3 = {{&q1, Pq1, &P->AQ, false, true}};
      const bool w1at = !can_fuse_l0(f3);        // layer 0 is its own stage: it writes W1aT
      if (w1at) {
        f3[0].tcopy = P->W1aT;
        f3[0].tcol = sd;
        f3[0].tn = ad;
      }
      TD3_RC(add_fwd_stages(h, P->tables, st, f3, Bp, B, "AF", nullptr, 0, nullptr, nullptr, 0, true, true));
      // the actor loss -mean Q1(s, pi(s)) (:159): Q1's head and its backward are the prologue of
      // AQB_bwd2 (kProHeadBwd; the particle path has the row launch kRowActorLossP instead)
      std::vector<BwdItem> aqb = {{&q1, Pq1, &P->AQ, false}};
      TD3_RC(add_bwd_stages(h, P->tables, st, aqb, Bp, B, "AQB", false, false, nullptr, (float)(-1.0) / (float)B));
      {
        GemmProb p{};
        p.norm = norm ? 1 : 0;
        p.B = B;
        namespace ab = actor_head_bwd;
        p.ex[ab::kDU0] = P->AQ.GU[0];
        p.ex[ab::kH0] = P->AQ.H[0];
        p.ex[ab::kStats0] = P->AQ.stats[0];
        p.ex[ab::kGamma0] = const_cast<float*>(Pq1 + q1.ln[0].offg);
        p.ex[ab::kW1] = const_cast<float*>(Pq1 + q1.lin[0].offW);
        p.ex[ab::kW1T] = w1at ? P->W1aT : nullptr;      // the action columns as rows (AF_fwd0 wrote them)
        p.exi[ab::kLdW1T] = q1.lin[0].Np;
        p.exi[ab::kK0] = q1.lin[0].N;
        p.exi[ab::kLd0] = q1.lin[0].Np;
        p.exi[ab::kLdw1] = q1.lin[0].Kp;
        set_actor_bwd(p, Pa, an, P->A, sd, ad, ma);
        std::vector<GemmProb> v = {p};
        TD3_RC(push_row_stage(h, P->tables, st, v, kRowActorHeadBwd, Bp, "actor_head_bwd"));
      }
      std::vector<BwdItem> ab = {{&an, Pa, &P->A, true}};
      TD3_RC(add_bwd_stages(h, P->tables, st, ab, Bp, B, "AB", true));
      TD3_RC(add_dw_stage(h, P->tables, st, h->actor, 1, ab, Bp, "A", true, 0, nullptr, &P->dwslab));
    }
  }
  for (int a = 0; a < 2; ++a)          // ring bodies: F_fwd0 sampled from the ring, the rest shared
    for (int i = 0; i < 2; ++i) {
      std::vector<Stage>& br = P->body_ring[a][i];
      br.insert(br.end(), P->body[a][i].begin() + 1, P->body[a][i].end());
    }
  TD3_RC(alloc_dw_slab(P.get()));
  P->dp_overlap = (h->comm || h->local) && dp_overlap(h);
  if (h->plan) destroy_plan(h->plan.get());
  h->plan = std::move(P);
  return 0;
}

// ================================================================== TD3_particles step
// TD3_particles.TD3.train (TD3_particles.py:167-224): the featured schedule plus the particle
// encoder of every network (enc_fwd / enc_bwd / enc_adam), lnorm1 on the MLP input, Q heads with
// one output per action dimension, no clamp on a', tanh policy output, optional CDQ.
struct EncItem {
  const NetL* net;
  const float* P;         // group arena (encoder at P + net->enc_off)
  float* X; int ldx;      // pooled features -> X[:, 0:128]
  int next;               // 1: the next-state particles
  uint64_t* mask;         // nullable (networks that are back-propagated)
};

static void push_enc_fwd(td3_handle* h, Plan* P, std::vector<Stage>& st, const std::vector<EncItem>& items,
                         const std::string& name) {
  const int N = h->N, D = h->D;
  const double flops = 2.0 * P->B * N * ((double)kEncC1 * D + (double)kEncC2 * kEncC1) * items.size();
  st.push_back({name,
                [=](hipStream_t s) {
                  EncFwdArgs a{};
                  for (size_t k = 0; k < items.size(); ++k) {
                    const EncItem& it = items[k];
                    a.p[k] = EncFwdProb{it.P + it.net->enc_off, it.next ? P->src_op2 : P->src_op, it.X, it.ldx,
                                        it.mask};
                  }
                  a.nprob = (int)items.size();
                  a.data = P->src_data;
                  a.rec = P->src_rec;
                  a.idx = P->src_idx;
                  a.B = P->B;
                  a.Bp = P->Bp;
                  a.N = N;
                  a.D = D;
                  a.ntile = (N + 31) / 32;
                  return launch_enc_fwd(a, s);
                },
                flops, "td3::enc_fwd_kernel<" + std::to_string(((D + 3) / 4) * 4) + ">"});
}

// One launch covers every network of a stage; its workgroups split the batch rows, 256 in all
// (role A holds W2^T in LDS: one workgroup per CU).
static int enc_bwd_nwg(int B, int nnets) { return std::max(1, std::min(B, 256 / std::max(1, nnets))); }

static void push_enc_bwd(td3_handle* h, Plan* P, std::vector<Stage>& st, const std::vector<BwdItem>& items,
                         const std::vector<float*>& X, const std::string& name) {
  const int N = h->N, D = h->D;
  const bool norm = h->cfg.norm == 1;
  const double flops = 2.0 * P->B * N * (2.0 * kEncC2 * kEncC1 + (double)kEncC1 * D) * items.size();
  st.push_back({name,
                [=](hipStream_t s) {
                  EncBwdArgs a{};
                  for (size_t k = 0; k < items.size(); ++k) {
                    const BwdItem& it = items[k];
                    EncBwdProb& q = a.p[k];
                    q.enc = it.P + it.net->enc_off;
                    q.part_off = P->src_op;
                    q.mask = it.e->mask;
                    q.X = X[k];
                    q.ldx = it.net->lin[0].Kp;
                    q.GU = it.e->GUin;
                    q.ldgu = it.net->lin[0].Kp;
                    q.stats = norm ? it.e->statsIn : nullptr;
                    q.gamma = it.P + it.net->ln_in.offg;
                    q.Kin = it.net->lin[0].K;
                    q.partial = it.e->partial;
                    q.gpool = it.e->gpool;
                  }
                  a.nprob = (int)items.size();
                  a.data = P->src_data;
                  a.rec = P->src_rec;
                  a.idx = P->src_idx;
                  a.B = P->B;
                  a.Bp = P->Bp;
                  a.N = N;
                  a.D = D;
                  a.ntile = (N + 31) / 32;
                  a.nwg = enc_bwd_nwg(P->B, (int)items.size());
                  return launch_enc_bwd(a, s);
                },
                flops, "td3::enc_bwd_kernel<" + std::to_string(((D + 3) / 4) * 4) + (TD3_ENC_FUSED ? ", 2>" : ", 0>")});
}

static void destroy_graphs(Plan* P) {
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b) {
      if (P->graph[a][b]) (void)hipGraphExecDestroy(P->graph[a][b]);
      if (P->graph_g[a][b]) (void)hipGraphExecDestroy(P->graph_g[a][b]);
      P->graph[a][b] = P->graph_g[a][b] = nullptr;
    }
  P->graph_ring_gen = 0;
}

// The encoders read particles in place; graphs bake the source, so a new source re-captures.
constexpr uint64_t kBatchSource = ~0ull;

static void set_particle_source(Plan* P, uint64_t key, const float* data, int rec, int op, int op2,
                                const int64_t* idx) {
  if (P->src_key == key && P->src_data == data) return;
  destroy_graphs(P);
  P->src_key = key;
  P->src_data = data;
  P->src_rec = rec;
  P->src_op = op;
  P->src_op2 = op2;
  P->src_idx = idx;
}

static int build_step_particles(td3_handle* h, int B) {
  std::unique_ptr<Plan> P(new Plan());
  const int Bp = pad32(B);
  P->B = B;
  P->Bp = Bp;
  P->particles = 1;
  const bool norm = h->cfg.norm == 1;
  const bool cdq = h->cdq != 0;
  const int F = h->sd, ad = h->ad, N = h->N, D = h->D;
  const int nqn = cdq ? 2 : 1;
  const NetL& an = h->actor.nets[0];
  const NetL& q1 = h->critic.nets[0];
  const NetL& q2 = h->critic.nets[cdq ? 1 : 0];
  P->nq = ad;
  P->ldq = 32;
  P->ld_a = an.lin[0].Kp;
  P->ld_q = q1.lin[0].Kp;
  P->nwg = enc_bwd_nwg(B, nqn);
  P->nwg_a = enc_bwd_nwg(B, 1);
  const int ntile = (N + 31) / 32;
  const size_t encsz = (size_t)EncOff::size(D);
  const size_t mask_f = (size_t)Bp * ntile * 64 * 2;
  size_t floats = (size_t)Bp * (2 * P->ld_a + 5 * P->ld_q) + 16 * (size_t)Bp + (size_t)Bp * ad +
                  (size_t)Bp * 32 + (size_t)Bp * 2 * N * D + 3 * (3 * mask_f + (size_t)Bp * kEncC2) +
                  (2 * P->nwg + P->nwg_a) * encsz +
                  3 * (size_t)Bp * kEncC2 + 16384;
  floats += 2 * eval_floats(an, Bp, true, norm) + 6 * eval_floats(q1, Bp, true, norm);
  P->scratch_bytes = floats * sizeof(float);
  TD3_HIP(hipMalloc(&P->scratch, P->scratch_bytes));
  TD3_HIP(hipMemset(P->scratch, 0, P->scratch_bytes));
  TD3_HIP(hipDeviceSynchronize());   // null-stream memset vs the non-blocking step stream
  Scratch S{P->scratch, floats, 0};
  P->XA = S.take((size_t)Bp * P->ld_a);
  P->XTA = S.take((size_t)Bp * P->ld_a);
  P->XAQ = S.take((size_t)Bp * P->ld_q);
  for (int j = 0; j < nqn; ++j) {
    P->XQ[j] = S.take((size_t)Bp * P->ld_q);
    P->XTQ[j] = S.take((size_t)Bp * P->ld_q);
  }
  P->R = S.take(Bp);
  P->ND = S.take(Bp);
  P->noise = S.take((size_t)Bp * ad);
  P->Y = S.take((size_t)Bp * 32);
  P->sqerr = S.take(2 * (size_t)Bp);
  P->d_idx = (int64_t*)S.take(2 * (size_t)Bp);
  P->d_inject_idx = (int64_t*)S.take(2 * (size_t)Bp);
  P->d_iota = (int64_t*)S.take(2 * (size_t)Bp);
  P->pbatch = S.take((size_t)Bp * 2 * N * D);
  alloc_eval(S, an, Bp, P->XTA, P->ld_a, false, norm, true, P->TA);
  alloc_eval(S, an, Bp, P->XA, P->ld_a, true, norm, true, P->A);
  for (int j = 0; j < nqn; ++j) {
    alloc_eval(S, j ? q2 : q1, Bp, P->XQ[j], P->ld_q, true, norm, true, P->Q[j]);
    alloc_eval(S, j ? q2 : q1, Bp, P->XTQ[j], P->ld_q, false, norm, true, P->TQ[j]);
  }
  alloc_eval(S, q1, Bp, P->XAQ, P->ld_q, true, norm, true, P->AQ);
  for (EvalB* e : {&P->Q[0], &P->Q[1], &P->A}) {
    if (e == &P->Q[1] && !cdq) continue;
    // conv2 words, conv1 words, positive-row counts [Bp][128] (EncFwdProb::mask)
    e->mask = reinterpret_cast<uint64_t*>(S.take(3 * mask_f + (size_t)Bp * kEncC2));
    e->partial = S.take((size_t)(e == &P->A ? P->nwg_a : P->nwg) * encsz);
    e->gpool = S.take((size_t)Bp * kEncC2);
  }
  if (S.used > S.cap) {
    set_error("internal: scratch overflow (%zu > %zu)", S.used, S.cap);
    return -2;
  }
  {
    std::vector<int64_t> iota(Bp);
    for (int i = 0; i < Bp; ++i) iota[i] = i;
    TD3_HIP(hipMemcpy(P->d_iota, iota.data(), Bp * 8, hipMemcpyHostToDevice));
  }

  const float* Pa = h->actor.P;
  const float* Pta = h->actor.T;
  const float* Pq = h->critic.P;
  const float* Ptq = h->critic.T;
  const int acol = kEncC2 + F;        // first action column of the Q input rows (TD3_particles.py:110)

  // no clamp of a' (TD3_particles.py:179-181), tanh output (:68)
  auto policy_head = [&](const float* Pp, EvalB& e, float* out, float* out2, int target, int gen_noise) {
    return policy_head_prob(h, *P, Pp, e, {out, out2, P->ld_q, acol, 0, 1.0f}, target, gen_noise);
  };

  // ---------------- delayed policy update (TD3_particles.py:206-224): _actor_learn on (s features, s
  // particles) with the post-step critic; A_dw also runs the actor's Polyak (the critic's is in C_dw)
  auto actor_phase_stages = [&](std::vector<Stage>& st) -> int {
    Plan* Pp = P.get();
    push_enc_fwd(h, Pp, st, {{&q1, Pq, P->XAQ, P->ld_q, 0, nullptr}}, "AF_enc");
    std::vector<FwdItem> f3 = {{&q1, Pq, &P->AQ, false, true}};
    TD3_RC(add_fwd_stages(h, P->tables, st, f3, Bp, B, "AF", nullptr, 0));
    {
      GemmProb p{};
      p.norm = norm ? 1 : 0;
      p.B = B;
      set_ln3_head(p, Pq, q1, P->AQ);
      p.ex[actor_loss_p::kQ] = P->AQ.Qv;
      p.Aout = P->AQ.GZ[2];
      p.ldao = q1.lin[2].Np;
      p.exi[actor_loss_p::kNq] = ad;
      p.exi[actor_loss_p::kLdw4] = q1.lin[3].Kp;
      p.exf[actor_loss_p::kGradScale] = (float)(-1.0 / ((double)B * ad));
      std::vector<GemmProb> v = {p};
      TD3_RC(push_row_stage(h, P->tables, st, v, kRowActorLossP, Bp, "actor_loss"));
    }
    std::vector<BwdItem> aqb = {{&q1, Pq, &P->AQ, false}};
    TD3_RC(add_bwd_stages(h, P->tables, st, aqb, Bp, B, "AQB", false, true));
    {
      GemmProb p{};
      p.norm = norm ? 1 : 0;
      p.B = B;
      namespace ab = actor_head_bwd_p;
      p.ex[ab::kDUin] = P->AQ.GUin;
      p.ex[ab::kXin] = P->XAQ;
      p.ex[ab::kStatsIn] = P->AQ.statsIn;
      p.ex[ab::kGammaIn] = const_cast<float*>(Pq + q1.ln_in.offg);
      p.exi[ab::kKin] = q1.lin[0].K;
      p.exi[ab::kLdIn] = q1.lin[0].Kp;
      set_actor_bwd(p, Pa, an, P->A, acol, ad, 1.0f);
      std::vector<GemmProb> v = {p};
      TD3_RC(push_row_stage(h, P->tables, st, v, kRowActorHeadBwdP, Bp, "actor_head_bwd"));
    }
    std::vector<BwdItem> ab = {{&an, Pa, &P->A, true}};
    TD3_RC(add_bwd_stages(h, P->tables, st, ab, Bp, B, "AB", true, true));
    push_enc_bwd(h, Pp, st, ab, {P->XA}, "AB_enc");
    TD3_RC(add_dw_stage(h, P->tables, st, h->actor, 1, ab, Bp, "A", true, P->nwg_a, nullptr, &P->dwslab));
    return 0;
  };

  for (int actor_phase = 0; actor_phase < 2; ++actor_phase) {
    for (int inj = 0; inj < 2; ++inj) {
      std::vector<Stage>& st = P->body[actor_phase][inj];
      Plan* Pp = P.get();
      // ---- encoders of the critic phase (+ the actor's on policy steps)
      {
        std::vector<EncItem> e = {{&an, Pta, P->XTA, P->ld_a, 1, nullptr},
                                  {&q1, Ptq, P->XTQ[0], P->ld_q, 1, nullptr},
                                  {&q1, Pq, P->XQ[0], P->ld_q, 0, P->Q[0].mask}};
        if (cdq) {
          e.push_back({&q2, Ptq, P->XTQ[1], P->ld_q, 1, nullptr});
          e.push_back({&q2, Pq, P->XQ[1], P->ld_q, 0, P->Q[1].mask});
        }
        if (actor_phase) e.push_back({&an, Pa, P->XA, P->ld_a, 0, P->A.mask});
        push_enc_fwd(h, Pp, st, e, "ENC_fwd");
      }
      std::vector<FwdItem> f1 = {{&an, Pta, &P->TA, false, false}, {&q1, Pq, &P->Q[0], true, true}};
      if (cdq) f1.push_back({&q2, Pq, &P->Q[1], true, true});
      if (actor_phase) f1.push_back({&an, Pa, &P->A, true, true});
      TD3_RC(add_fwd_stages(h, P->tables, st, f1, Bp, B, "F", h->d_ctr, actor_phase));
      {
        std::vector<GemmProb> hp = {policy_head(Pta, P->TA, P->XTQ[0], cdq ? P->XTQ[1] : nullptr, 1, inj ? 0 : 1)};
        if (actor_phase) hp.push_back(policy_head(Pa, P->A, P->XAQ, nullptr, 0, 0));
        TD3_RC(push_row_stage(h, P->tables, st, hp, kRowPolicyHead, Bp, "heads"));
      }
      std::vector<FwdItem> f2 = {{&q1, Ptq, &P->TQ[0], false, false}};
      if (cdq) f2.push_back({&q2, Ptq, &P->TQ[1], false, false});
      TD3_RC(add_fwd_stages(h, P->tables, st, f2, Bp, B, "TF", nullptr, 0));
      {
        std::vector<GemmProb> cl;
        for (int j = 0; j < nqn; ++j) {
          const NetL& qj = j ? q2 : q1;
          const NetL& t1 = cdq ? q2 : q1;
          EvalB& T1 = P->TQ[cdq ? 1 : 0];
          GemmProb p{};
          p.norm = norm ? 1 : 0;
          p.B = B;
          namespace cp = critic_loss_p;
          // the three heads: target q1, target q2 (= target q1 without CDQ), online q_j
          const NetL* hn[3] = {&q1, &t1, &qj};
          const float* hp[3] = {Ptq, Ptq, Pq};
          const EvalB* he[3] = {&P->TQ[0], &T1, &P->Q[j]};
          for (int n = 0; n < 3; ++n) {
            p.ex[cp::kH3 + n] = he[n]->H[2];
            p.ex[cp::kGamma3 + n] = const_cast<float*>(hp[n] + hn[n]->ln[2].offg);
            p.ex[cp::kBeta3 + n] = const_cast<float*>(hp[n] + hn[n]->ln[2].offb);
            p.ex[cp::kW4 + n] = const_cast<float*>(hp[n] + hn[n]->lin[3].offW);
            p.ex[cp::kB4 + n] = const_cast<float*>(hp[n] + hn[n]->lin[3].offb);
          }
          p.ex[cp::kReward] = P->R;
          p.ex[cp::kNotDone] = P->ND;
          p.ex[cp::kDZ4] = P->Q[j].GZ[3];
          p.ex[cp::kDU3] = P->Q[j].GU[2];
          p.ex[cp::kU3] = P->Q[j].U[2];
          p.ex[cp::kStats3] = P->Q[j].stats[2];
          p.ex[cp::kY] = P->Y;
          p.ex[cp::kSqErr] = P->sqerr + (size_t)j * Bp;
          p.ex[cp::kQ] = P->Q[j].Qv;
          p.Aout = P->Q[j].GZ[2];
          p.ldao = qj.lin[2].Np;
          p.exi[cp::kK3] = qj.lin[2].N;
          p.exi[cp::kLd3] = qj.lin[2].Np;
          p.exi[cp::kJ] = j;
          p.exi[cp::kNq] = ad;
          p.exi[cp::kLdw4] = qj.lin[3].Kp;
          p.exi[cp::kCdq] = cdq ? 1 : 0;
          p.exf[cp::kDiscount] = (float)h->cfg.discount;
          p.exf[cp::kGradScale] = (float)(2.0 / ((double)B * ad));
          cl.push_back(p);
        }
        TD3_RC(push_row_stage(h, P->tables, st, cl, kRowCriticLossP, Bp, "critic_loss"));
      }
      std::vector<BwdItem> cb = {{&q1, Pq, &P->Q[0], true}};
      std::vector<float*> cbx = {P->XQ[0]};
      if (cdq) {
        cb.push_back({&q2, Pq, &P->Q[1], true});
        cbx.push_back(P->XQ[1]);
      }
      TD3_RC(add_bwd_stages(h, P->tables, st, cb, Bp, B, "CB", true, true));
      push_enc_bwd(h, Pp, st, cb, cbx, "CB_enc");
      TD3_RC(add_dw_stage(h, P->tables, st, h->critic, 0, cb, Bp, "C", actor_phase != 0, P->nwg, nullptr, &P->dwslab));
      if (!actor_phase) continue;
      TD3_RC(actor_phase_stages(st));
    }
  }
  {   // _actor_learn called on its own (evaluate_model.py:39-49): the actor's forward on s, pi(s),
      // then the policy-step stages; the step counter of the actor's Adam only (no total_it), and
      // the critic's Polyak as a flat pass (TD3_particles.py:219-221; inside a train step C_dw does it)
    std::vector<Stage>& st = P->actor_learn;
    push_enc_fwd(h, P.get(), st, {{&an, Pa, P->XA, P->ld_a, 0, P->A.mask}}, "L_enc");
    std::vector<FwdItem> f1 = {{&an, Pa, &P->A, true, true}};
    TD3_RC(add_fwd_stages(h, P->tables, st, f1, Bp, B, "L", h->d_ctr, kBumpActorOnly));
    std::vector<GemmProb> hp = {policy_head(Pa, P->A, P->XAQ, nullptr, 0, 0)};
    TD3_RC(push_row_stage(h, P->tables, st, hp, kRowPolicyHead, Bp, "L_head"));
    TD3_RC(actor_phase_stages(st));
    float* Tc = h->critic.T;
    const float* Pc = h->critic.P;
    const int64_t nc = h->critic.size;
    const float tau = (float)h->cfg.tau;
    st.push_back({"L_polyak_critic", [=](hipStream_t s) { return launch_polyak_flat(Tc, Pc, nc, tau, s); }, 0,
                  "td3::polyak_flat_kernel"});
  }
  TD3_RC(alloc_dw_slab(P.get()));
  P->dp_overlap = (h->comm || h->local) && dp_overlap(h);
  if (h->plan) destroy_plan(h->plan.get());
  h->plan = std::move(P);
  return 0;
}

static int run_stages(std::vector<Stage>& st, hipStream_t s) {
  for (auto& x : st) TD3_RC(x.run(s));
  return 0;
}

// run_stages with the probed kernel's launches between two events each (td3_probe_kernel)
static int run_stages_probed(td3_handle* h, std::vector<Stage>& st, hipStream_t s) {
  for (auto& x : st) {
    const bool hit = x.kernel == h->probe_kernel;
    if (hit) {
      while ((int)h->probe_ev.size() < h->probe_used + 2) {
        hipEvent_t e;
        TD3_HIP(hipEventCreate(&e));
        h->probe_ev.push_back(e);
      }
      TD3_HIP(hipEventRecord(h->probe_ev[h->probe_used], s));
    }
    TD3_RC(x.run(s));
    if (hit) {
      TD3_HIP(hipEventRecord(h->probe_ev[h->probe_used + 1], s));
      h->probe_used += 2;
    }
  }
  return 0;
}

// Input stage: Philox index draw + gather from the ring into the padded batch buffers.
static int input_from_ring_particles(td3_handle* h, Ring* r, Plan* P, bool inject_idx, hipStream_t s);

// A step's gather without its segments: the plan's batch, the rows drawn by the step counter.
static GatherArgs step_gather(const td3_handle* h, const Ring* r, const Plan* P, bool inject_idx) {
  GatherArgs a = gather_base(r);
  a.B = P->B;
  a.Bp = P->Bp;
  a.inject_idx = inject_idx ? P->d_inject_idx : nullptr;
  a.idx_out = P->d_idx;
  a.ctr = h->d_ctr;
  return a;
}

static int input_from_ring(td3_handle* h, Ring* r, Plan* P, bool inject_idx, hipStream_t s) {
  if (P->particles) return input_from_ring_particles(h, r, P, inject_idx, s);
  GatherArgs a = step_gather(h, r, P, inject_idx);
  const int sd = h->sd, ad = h->ad;
  int k = 0;
  // s once per network input that holds it ([s | a] and [s | pi(s)]), s' once ([s' | a']): the
  // actors read the state columns of those rows (build_step)
  a.seg[k++] = GatherSeg{P->X_SA, P->ld_sa, 0, r->o_s, sd};
  a.seg[k++] = GatherSeg{P->X_SA, P->ld_sa, sd, r->o_a, ad};
  a.seg[k++] = GatherSeg{P->X_SP, P->ld_sa, 0, r->o_s, sd};
  a.seg[k++] = GatherSeg{P->X_S2A, P->ld_sa, 0, r->o_s2, sd};
  a.seg[k++] = GatherSeg{P->R, 1, 0, r->o_r, 1};
  a.seg[k++] = GatherSeg{P->ND, 1, 0, r->o_nd, 1};
  a.nseg = k;
  return launch_gather(a, s);
}

// Particle rings: the small fields go to every network's MLP input rows; the particle blocks
// stay in the ring and are read there by the encoders (rows P->d_idx).
static int input_from_ring_particles(td3_handle* h, Ring* r, Plan* P, bool inject_idx, hipStream_t s) {
  GatherArgs a = step_gather(h, r, P, inject_idx);
  const int F = h->sd, ad = h->ad, c0 = kEncC2;
  const bool cdq = h->cdq != 0;
  int k = 0;
  a.seg[k++] = GatherSeg{P->XA, P->ld_a, c0, r->o_s, F};
  a.seg[k++] = GatherSeg{P->XAQ, P->ld_q, c0, r->o_s, F};
  a.seg[k++] = GatherSeg{P->XTA, P->ld_a, c0, r->o_s2, F};
  for (int j = 0; j < (cdq ? 2 : 1); ++j) {
    a.seg[k++] = GatherSeg{P->XQ[j], P->ld_q, c0, r->o_s, F};
    a.seg[k++] = GatherSeg{P->XQ[j], P->ld_q, c0 + F, r->o_a, ad};
    a.seg[k++] = GatherSeg{P->XTQ[j], P->ld_q, c0, r->o_s2, F};
  }
  a.seg[k++] = GatherSeg{P->R, 1, 0, r->o_r, 1};
  a.seg[k++] = GatherSeg{P->ND, 1, 0, r->o_nd, 1};
  a.nseg = k;
  return launch_gather(a, s);
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

static int input_from_batch(td3_handle* h, Plan* P, const float* s, const float* a, const float* s2,
                            const float* r, const float* nd, hipStream_t st) {
  const int sd = h->sd, ad = h->ad, Bp = P->Bp, B = P->B;
  hipLaunchKernelGGL(pack_kernel, dim3(Bp), dim3(64), 0, st, s, sd, B, Bp, P->X_SA, P->ld_sa, 0,
                     P->X_SP, P->ld_sa, 0, (float*)nullptr, 0, 0);
  hipLaunchKernelGGL(pack_kernel, dim3(Bp), dim3(64), 0, st, a, ad, B, Bp, P->X_SA, P->ld_sa, sd,
                     (float*)nullptr, 0, 0, (float*)nullptr, 0, 0);
  hipLaunchKernelGGL(pack_kernel, dim3(Bp), dim3(64), 0, st, s2, sd, B, Bp, P->X_S2A, P->ld_sa, 0,
                     (float*)nullptr, 0, 0, (float*)nullptr, 0, 0);
  hipLaunchKernelGGL(pack_kernel, dim3(Bp), dim3(64), 0, st, r, 1, B, Bp, P->R, 1, 0,
                     (float*)nullptr, 0, 0, (float*)nullptr, 0, 0);
  hipLaunchKernelGGL(pack_kernel, dim3(Bp), dim3(64), 0, st, nd, 1, B, Bp, P->ND, 1, 0,
                     (float*)nullptr, 0, 0, (float*)nullptr, 0, 0);
  TD3_HIP(hipGetLastError());
  return 0;
}

// Unit importance weights for a step that is not prioritized: refilled on its stream, ahead of its
// body, only when a prioritized step overwrote them (a host flag: the common path queues nothing).
__global__ void fill_f32_kernel(float* p, int n, float v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}
static int ensure_unit_weights(td3_handle* h, hipStream_t s) {
  Plan* P = h->plan.get();
  if (!P->per_w_dirty || h->per_step) return 0;
  hipLaunchKernelGGL(fill_f32_kernel, dim3((P->Bp + 255) / 256), dim3(256), 0, s, P->per_w, P->Bp, 1.0f);
  TD3_HIP(hipGetLastError());
  P->per_w_dirty = false;
  return 0;
}

// One step body on stream s.  With `ring` set, the replay-ring gather (Philox draw) is
// launched first and, in graph mode, captured into the same hipGraph (one replay per step).
static int run_body(td3_handle* h, int actor_phase, int inj, hipStream_t s, Ring* ring) {
  if (h->local) {
    set_error("a td3_comm_init_local replica steps through td3_train_step_local only");
    return -1;
  }
  TD3_RC(ensure_w4(h, s));
  TD3_RC(ensure_unit_weights(h, s));
  Plan* P = h->plan.get();
  const bool fused = ring && P->fuse_gather;     // featured: the sample runs inside F_fwd0
  std::vector<Stage>& st = fused ? P->body_ring[actor_phase][inj] : P->body[actor_phase][inj];
  h->last_body = &st;
  // use_graph 2 (auto): a hipGraph replay costs ~8 us of GPU time on top of its kernels
  // (tools/launch_floor.hip) but little host time; direct launches cost the host ~3 us each and
  // the GPU nothing extra.  While the last policy step is still queued the host is ahead of the
  // GPU, so its launch time is hidden: launch directly.  Otherwise (host-bound acting loops: the
  // last policy step has finished: a query waited for it) replay.  Without queries (act_used;
  // asking the stream queues a marker, a per-step drain) training launches directly.
  // Data parallel (RCCL comm attached): auto launches directly, so every rank issues its
  // all-reduces the same way whatever its local progress (no captured / uncaptured mix).
  const bool graph = !h->probing && !P->dp_overlap && (h->cfg.use_graph == 1 ||
                                      (h->cfg.use_graph == 2 && !h->comm && !actor_phase && h->act_used &&
                                       !h->actor_stream));
  if (!graph) {
    if (ring && !fused) TD3_RC(input_from_ring(h, ring, P, false, s));
    return h->probing ? run_stages_probed(h, st, s) : run_stages(st, s);
  }
  // graphs bake the ring in (records, d_size, seed, record width): a ring allocated since —
  // even at the same address, e.g. after ReplayBuffer.load() — is captured again
  if (ring && P->graph_ring_gen != ring->gen) {
    for (int a = 0; a < 2; ++a)
      for (int b = 0; b < 2; ++b)
        if (P->graph_g[a][b]) {
          TD3_HIP(hipGraphExecDestroy(P->graph_g[a][b]));
          P->graph_g[a][b] = nullptr;
        }
    P->graph_ring_gen = ring->gen;
  }
  hipGraphExec_t& ge = ring ? P->graph_g[actor_phase][inj] : P->graph[actor_phase][inj];
  if (!ge) {
    hipStream_t cs;
    TD3_HIP(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    TD3_HIP(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
    int rc = ring && !fused ? input_from_ring(h, ring, P, false, cs) : 0;
    if (!rc) rc = run_stages(st, cs);
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(cs, &g);
    if (rc) {
      if (g) (void)hipGraphDestroy(g);
      (void)hipStreamDestroy(cs);
      return rc;
    }
    TD3_HIP(e);
    TD3_HIP(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
    TD3_HIP(hipGraphDestroy(g));
    TD3_HIP(hipStreamDestroy(cs));
  }
  TD3_HIP(hipGraphLaunch(ge, s));
  return 0;
}

static int build_step_particles(td3_handle* h, int B);

// The Adam moments of a sharded schedule live on their slice owners: a plan that stops sharding
// (TD3_DP_SHARD changed between builds) first brings every rank the whole M / V arenas, or each
// rank would carry on with stale moments for the slices it did not own.  Every rank
// rebuilds at the same call (same batch, same environment), so the all-gather is collective; the
// in-process seam copies the owners' slices.
static int gather_moments_for_rebuild(td3_handle* h) {
  if (h->local) {
    TD3_HIP(hipDeviceSynchronize());          // the replicas stepped on non-blocking streams
    for (int which : {TD3_ACTOR_ADAM_M, TD3_ACTOR_ADAM_V, TD3_CRITIC_ADAM_M, TD3_CRITIC_ADAM_V}) {
      const bool actor = which == TD3_ACTOR_ADAM_M || which == TD3_ACTOR_ADAM_V;
      const bool m = which == TD3_ACTOR_ADAM_M || which == TD3_CRITIC_ADAM_M;
      const int64_t sl = shard_slice(actor ? h->actor : h->critic, h->nranks);
      for (int k = 0; k < (int)h->local->hs.size(); ++k) {
        td3_handle* o = h->local->hs[k];
        if (o == h || !o) continue;
        const Group& src = actor ? o->actor : o->critic;
        const Group& dst = actor ? h->actor : h->critic;
        TD3_HIP(hipMemcpy((m ? dst.M : dst.V) + k * sl, (m ? src.M : src.V) + k * sl, (size_t)sl * 4,
                          hipMemcpyDeviceToDevice));
      }
    }
    return 0;
  }
  if (!h->comm || h->nranks <= 1) return 0;
  if (h->last_step_stream && h->last_step_stream != h->stream) TD3_HIP(hipStreamSynchronize(h->last_step_stream));
  for (Group* g : {&h->actor, &h->critic}) {
    const int64_t sl = shard_slice(*g, h->nranks);
    for (float* a : {g->M, g->V}) {
      ncclResult_t r = ncclAllGather(a + h->rank * sl, a, (size_t)sl, ncclFloat, h->comm, h->stream);
      if (r != ncclSuccess) {
        set_error("ncclAllGather: %s", ncclGetErrorString(r));
        return -2;
      }
    }
  }
  TD3_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

static int build_plan(td3_handle* h, int B) {
  const bool was_sharded = h->dp_sharded && h->nranks > 1;
  h->dp_sharded = false;                      // set again by add_dw_stage when it shards
  // the profiled stage list lives in the plan being replaced
  h->last_body = nullptr;
  h->last_ring = nullptr;
  // the images are not maintained by every plan: the first step of a new one repacks them
  h->actor.w4_valid = h->critic.w4_valid = false;
  h->w4_build = false;
  const int rc = h->particles ? build_step_particles(h, B) : build_step(h, B);
  h->w4_build = false;
  if (!rc && was_sharded && !h->dp_sharded) return gather_moments_for_rebuild(h);
  return rc;
}

static int ensure_plan(td3_handle* h, int B) {
  if (h->plan && h->plan->B == B) return 0;
  TD3_HIP(hipStreamSynchronize(h->stream));
  return build_plan(h, B);
}

// A particle learner's encoders read the ring the step samples from.
// A featured learner's first layer samples the ring (kProGather; record layout checked at plan
// build against replay.hip's [s | a | s' | r | not_done]).
static int bind_ring(td3_handle* h, Ring* r) {
  Plan* P = h->plan.get();
  if (P->particles) {
    set_particle_source(P, r->gen, r->data, r->rec, r->o_p, r->o_p2, P->d_idx);
    return 0;
  }
  const int sd = h->sd, ad = h->ad;
  TD3_ARG(r->o_s == 0 && r->o_a == sd && r->o_s2 == sd + ad && r->o_r == 2 * sd + ad && r->o_nd == r->o_r + 1,
          "replay record layout is not [s | a | s' | r | not_done]");
  RingSide& g = P->rside;
  g = RingSide{};
  g.data = r->data;
  g.rec = r->rec;
  g.d_size = r->d_size;
  g.idx_out = P->d_idx;
  g.seed = r->seed;
  g.ctr = h->d_ctr;
  return 0;
}

// A queued step on s updates the online actor: queries run behind it (query_stream) -- in s itself
// when it is the handle's own stream, else behind an event recorded on s (a caller's stream may be
// gone by the next query).
static int note_actor_update(td3_handle* h, hipStream_t s) {
  if (s == h->stream) {
    h->actor_stream = s;
    return 0;
  }
  if (!h->actor_ev) TD3_HIP(hipEventCreateWithFlags(&h->actor_ev, TD3_EV_FLAGS));
  TD3_HIP(hipEventRecord(h->actor_ev, s));
  h->actor_ev_pending = true;
  return 0;
}

static int finish_step(td3_handle* h, int actor_phase, hipStream_t s, td3_step_stats* stats) {
  h->total_it += 1;
  h->critic_step += 1;
  h->last_step_stream = s;
  if (actor_phase) {
    h->actor_step += 1;
    TD3_RC(note_actor_update(h, s));
  }
  if (!stats) return 0;
  Plan* P = h->plan.get();
  TD3_HIP(hipStreamSynchronize(s));
  const int B = P->B, Bp = P->Bp, nq = P->nq, ldq = P->ldq;
  const bool twin = !P->particles || h->cdq;
  std::vector<float> sq(2 * (size_t)Bp);
  TD3_HIP(hipMemcpy(sq.data(), P->sqerr, sq.size() * 4, hipMemcpyDeviceToHost));
  double l1 = 0, l2 = 0;
  for (int i = 0; i < B; ++i) {
    l1 += sq[i];
    l2 += sq[Bp + i];
  }
  const double n = (double)B * nq;                // F.mse_loss mean over all elements
  stats->critic_loss = l1 / n + (twin ? l2 / n : 0.0);
  stats->actor_step = actor_phase;
  stats->actor_loss = NAN;
  auto rows = [&](float* dst, const float* src) -> int {     // [Bp][ldq] -> [B][nq]
    TD3_HIP(hipMemcpy2D(dst, (size_t)nq * 4, src, (size_t)ldq * 4, (size_t)nq * 4, B, hipMemcpyDeviceToHost));
    return 0;
  };
  if (actor_phase) {
    std::vector<float> q((size_t)B * nq);
    TD3_RC(rows(q.data(), P->AQ.Qv));
    double m = 0;
    for (float v : q) m += v;
    stats->actor_loss = -m / n;
  }
  if (stats->y) TD3_RC(rows(stats->y, P->Y));
  if (stats->q1) TD3_RC(rows(stats->q1, P->Q[0].Qv));
  if (stats->q2) TD3_RC(rows(stats->q2, P->Q[twin ? 1 : 0].Qv));
  if (stats->idx) TD3_HIP(hipMemcpy(stats->idx, P->d_idx, B * 8, hipMemcpyDeviceToHost));
  if (stats->noise) TD3_HIP(hipMemcpy(stats->noise, P->noise, (size_t)B * h->ad * 4, hipMemcpyDeviceToHost));
  return 0;
}

// ------------------------------------------------------------------ act / eval_q plans
// select_action / eval_q of <= kGemvRows rows as one act_kernel launch (TD3_ACT1=1, the default) or
// the gemv01 -> gemv -> head chain of three launches (0: the A/B reference; read when a plan is built)
// dev: a plan of the device-resident queries (td3_handle::act_dev): inputs and outputs in device
// scratch at every size (no mapped block, so no one-launch query either: the stage lists run).
static int build_act(td3_handle* h, int Bp, ActPlan** out, bool dev = false) {
  auto& plans = dev ? h->act_dev : h->act;
  auto it = plans.find(Bp);
  if (it != plans.end()) {
    *out = it->second.get();
    return 0;
  }
  std::unique_ptr<ActPlan> A(new ActPlan());
  A->Bp = Bp;
  const bool norm = h->cfg.norm == 1;
  const NetL& an = h->actor.nets[0];
  const NetL& q1 = h->critic.nets[0];
  const NetL& q2 = h->critic.nets[1];
  const int lds_s = pad32(h->sd), lds_sa = pad32(h->sd + h->ad);
  const size_t io_floats = (size_t)Bp * (lds_s + lds_sa + h->ad + 2) + 8 * 64;   // + the one-launch query flags
  size_t floats = io_floats + eval_floats(an, Bp, false, norm) + 2 * eval_floats(q1, Bp, false, norm) + 4096;
  TD3_HIP(hipMalloc(&A->scratch, floats * 4));
  TD3_HIP(hipMemset(A->scratch, 0, floats * 4));
  TD3_HIP(hipDeviceSynchronize());
  Scratch S{A->scratch, floats, 0};
  IoCarve io{&S};
  if (!dev) TD3_RC(map_io(A.get(), io_floats, &io));
  A->X_S = io.take((size_t)Bp * lds_s, &A->hX_S);
  A->X_SA = io.take((size_t)Bp * lds_sa, &A->hX_SA);
  A->out = io.take((size_t)Bp * h->ad, &A->hout);
  A->ldo = h->ad;
  for (int j = 0; j < 2; ++j) A->q[j] = io.take(Bp, &A->hq[j]);
  alloc_eval(S, an, Bp, A->X_S, lds_s, false, norm, true, A->A);
  alloc_eval(S, q1, Bp, A->X_SA, lds_sa, false, norm, true, A->Q[0]);
  alloc_eval(S, q2, Bp, A->X_SA, lds_sa, false, norm, true, A->Q[1]);
  auto gemv_layer = [&](const NetL& n, const float* Pp, const EvalB& e, int l) {
    GemvProb g{};
    g.X = l ? e.H[l - 1] : e.X;
    g.ldx = l ? n.lin[l - 1].Np : e.ldx;
    g.K = n.lin[l].K;
    g.lng = (l && norm) ? Pp + n.ln[l - 1].offg : nullptr;
    g.lnb = (l && norm) ? Pp + n.ln[l - 1].offb : nullptr;
    g.W = Pp + n.lin[l].offW;
    g.ldw = n.lin[l].Kp;
    g.b = Pp + n.lin[l].offb;
    g.N = n.lin[l].N;
    g.Y = e.H[l];
    g.ldy = n.lin[l].Np;
    return g;
  };
  A->gemv = true;
  for (int l = 0; l < 3; ++l) {
    A->gv_act[l].p[0] = gemv_layer(an, h->actor.P, A->A, l);
    A->gv_q[l].p[0] = gemv_layer(q1, h->critic.P, A->Q[0], l);
    A->gv_q[l].p[1] = gemv_layer(q2, h->critic.P, A->Q[1], l);
    for (const NetL* n : {&an, &q1, &q2}) A->gemv = A->gemv && n->lin[l].K <= 512;
  }
  A->gemv01 = A->gemv && an.lin[0].K <= kGemv0K && q1.lin[0].K <= kGemv0K;
  auto g01 = [&](Gemv01Args& g, const GemvArgs& l1, std::initializer_list<const NetL*> nets, const float* Pp) {
    g = Gemv01Args{};
    g.l1 = l1;
    int k = 0;
    for (const NetL* n : nets) {
      g.W0[k] = Pp + n->lin[0].offW;
      g.b0[k] = Pp + n->lin[0].offb;
      g.ldw0 = n->lin[0].Kp;
      g.K0 = n->lin[0].K;
      g.N0 = n->lin[0].N;
      ++k;
    }
  };
  g01(A->g01_act, A->gv_act[1], {&an}, h->actor.P);
  g01(A->g01_q, A->gv_q[1], {&q1, &q2}, h->critic.P);
  auto head = [&](const NetL& n, const float* Pp, EvalB& e, int mode) {
    HeadProb q{};
    q.H3 = e.H[2];
    q.ldh = n.lin[2].Np;
    q.K3 = n.lin[2].N;
    q.lng = norm ? Pp + n.ln[2].offg : nullptr;
    q.lnb = norm ? Pp + n.ln[2].offb : nullptr;
    q.W4 = Pp + n.lin[3].offW;
    q.ldw = n.lin[3].Kp;
    q.b4 = Pp + n.lin[3].offb;
    q.nout = n.lin[3].N;
    q.mode = mode;
    return q;
  };
  {
    std::vector<FwdItem> f = {{&an, h->actor.P, &A->A, false, false}};
    TD3_RC(add_fwd_stages(h, A->tables, A->act, f, Bp, Bp, "act", nullptr, 0));
    HeadProb p = head(an, h->actor.P, A->A, kHeadPolicy);
    p.out = A->out;
    p.ldo = A->ldo;
    p.out_col = 0;
    p.tanh_out = A->A.T;
    void* d = nullptr;
    TD3_RC(upload(h, A->tables, &p, sizeof(p), &d));
    HeadArgs a{};
    a.probs = (const HeadProb*)d;
    a.B = Bp;
    a.Bp = Bp;
    a.max_action = h->cfg.max_action;
    A->head_act = a;
    A->act.push_back({"act_head", [=](hipStream_t s) { return launch_heads(a, 1, s); }, 0});
  }
  {
    std::vector<FwdItem> f = {{&q1, h->critic.P, &A->Q[0], false, false},
                              {&q2, h->critic.P, &A->Q[1], false, false}};
    TD3_RC(add_fwd_stages(h, A->tables, A->evalq, f, Bp, Bp, "evq", nullptr, 0));
    std::vector<HeadProb> hp;
    for (int j = 0; j < 2; ++j) {
      HeadProb p = head(j ? q2 : q1, h->critic.P, A->Q[j], kHeadQ);
      p.out = A->q[j];
      p.ldo = 1;
      hp.push_back(p);
    }
    void* d = nullptr;
    TD3_RC(upload(h, A->tables, hp.data(), hp.size() * sizeof(HeadProb), &d));
    HeadArgs a{};
    a.probs = (const HeadProb*)d;
    a.B = Bp;
    a.Bp = Bp;
    a.max_action = h->cfg.max_action;
    A->head_q = a;
    A->evalq.push_back({"evq_head", [=](hipStream_t s) { return launch_heads(a, 2, s); }, 0});
  }
  // one-launch queries: layer 2 rides on the layer-1 column groups (N2 <= N1, same N1 for the twins)
  if (A->gemv01 && env_int("TD3_ACT1", 1) != 0) {
    int* ctr = reinterpret_cast<int*>(S.take(64));      // zeroed with the scratch
    auto mk = [&](ActArgs& a, const Gemv01Args& g, const GemvArgs& l2, std::initializer_list<const NetL*> nets,
                  const float* Pp, EvalB* const* ev, float* const* outs, int ldo, int mode, int* c) {
      a = ActArgs{};
      a.g = g;
      a.ctr = c;
      a.max_action = h->cfg.max_action;
      int k = 0;
      bool ok = true;
      for (const NetL* n : nets) {
        a.l2[k] = l2.p[k];
        HeadProb q = head(*n, Pp, *ev[k], mode);
        q.out = outs[k];
        q.ldo = ldo;
        q.out_col = 0;
        a.head[k] = q;
        ok = ok && n->lin[2].N <= n->lin[1].N && n->lin[1].N == nets.begin()[0]->lin[1].N && n->lin[3].N <= 64;
        ++k;
      }
      return ok;
    };
    EvalB* ea[1] = {&A->A};
    float* oa[1] = {A->out};
    EvalB* eq[2] = {&A->Q[0], &A->Q[1]};
    float* oq[2] = {A->q[0], A->q[1]};
    A->act1 = A->hio && mk(A->a1_act, A->g01_act, A->gv_act[2], {&an}, h->actor.P, ea, oa, A->ldo, kHeadPolicy, ctr) &&
              mk(A->a1_q, A->g01_q, A->gv_q[2], {&q1, &q2}, h->critic.P, eq, oq, 1, kHeadQ, ctr + 8);
    if (A->act1) {       // completion flags in the mapped block (io_floats reserves 4 * 64 floats of slack)
      float* hf = nullptr;
      A->a1_act.flag = reinterpret_cast<unsigned*>(io.take(64, &hf));
      A->hflag[0] = reinterpret_cast<unsigned*>(hf);
      A->a1_q.flag = reinterpret_cast<unsigned*>(io.take(64, &hf));
      A->hflag[1] = reinterpret_cast<unsigned*>(hf);
    }
  }
  *out = A.get();
  plans[Bp] = std::move(A);
  return 0;
}

// select_action / eval_q of TD3_particles (TD3_particles.py:153-164): the particles of the n
// query states are uploaded packed ([n][N*D], rows 0..n-1), the encoders read them in place.
// dev: a plan of the device-resident queries (td3_handle::act_dev, as build_act's): device scratch at
// every size, and the encoder stage reads the CALLER's particle rows where they are -- the query sets
// ActPlan::dev_part / dev_n before it runs the stages (data = part, rec = N*D, identity idx, B = n;
// enc_fwd_kernel writes zeros for rows >= B without touching data).  Such a plan has no pbatch.
static int build_act_particles(td3_handle* h, int Bp, ActPlan** out, bool dev = false) {
  auto& plans = dev ? h->act_dev : h->act;
  auto it = plans.find(Bp);
  if (it != plans.end()) {
    *out = it->second.get();
    return 0;
  }
  std::unique_ptr<ActPlan> A(new ActPlan());
  A->Bp = Bp;
  const bool norm = h->cfg.norm == 1;
  const bool cdq = h->cdq != 0;
  const int N = h->N, D = h->D, ad = h->ad;
  const NetL& an = h->actor.nets[0];
  const NetL& q1 = h->critic.nets[0];
  const NetL& q2 = h->critic.nets[cdq ? 1 : 0];
  const int lda = an.lin[0].Kp, ldq = q1.lin[0].Kp;
  const size_t io_floats = (size_t)Bp * (lda + 2 * ldq + (dev ? 0 : (size_t)N * D) + 32 + 2 * 32) + 8 * 64;
  size_t floats = io_floats + 2 * (size_t)Bp + eval_floats(an, Bp, false, norm) +
                  2 * eval_floats(q1, Bp, false, norm) + 8192;
  TD3_HIP(hipMalloc(&A->scratch, floats * 4));
  TD3_HIP(hipMemset(A->scratch, 0, floats * 4));
  TD3_HIP(hipDeviceSynchronize());
  Scratch S{A->scratch, floats, 0};
  IoCarve io{&S};
  if (!dev) TD3_RC(map_io(A.get(), io_floats, &io));
  A->X_S = io.take((size_t)Bp * lda, &A->hX_S);
  A->X_SA = io.take((size_t)Bp * ldq, &A->hX_SA);
  A->XQ2 = io.take((size_t)Bp * ldq, &A->hXQ2);
  if (!dev) A->pbatch = io.take((size_t)Bp * N * D, &A->hpbatch);
  A->out = io.take((size_t)Bp * 32, &A->hout);
  A->ldo = 32;
  for (int j = 0; j < 2; ++j) A->q[j] = io.take((size_t)Bp * 32, &A->hq[j]);
  A->d_iota = (int64_t*)S.take(2 * (size_t)Bp);
  alloc_eval(S, an, Bp, A->X_S, lda, false, norm, true, A->A);
  alloc_eval(S, q1, Bp, A->X_SA, ldq, false, norm, true, A->Q[0]);
  alloc_eval(S, q2, Bp, A->XQ2, ldq, false, norm, true, A->Q[1]);
  {
    std::vector<int64_t> iota(Bp);
    for (int i = 0; i < Bp; ++i) iota[i] = i;
    TD3_HIP(hipMemcpy(A->d_iota, iota.data(), Bp * 8, hipMemcpyHostToDevice));
  }
  auto enc_stage = [&](std::vector<Stage>& st, std::vector<EncFwdProb> probs, const char* name) {
    EncFwdArgs a{};
    for (size_t k = 0; k < probs.size(); ++k) a.p[k] = probs[k];
    a.nprob = (int)probs.size();
    a.data = A->pbatch;
    a.rec = N * D;
    a.idx = A->d_iota;
    a.B = Bp;
    a.Bp = Bp;
    a.N = N;
    a.D = D;
    a.ntile = (N + 31) / 32;
    if (dev) {
      const ActPlan* Ap = A.get();                    // owned by the plan map: outlives its stages
      st.push_back({name,
                    [=](hipStream_t s) {
                      EncFwdArgs b = a;
                      b.data = Ap->dev_part;
                      b.B = Ap->dev_n;
                      return launch_enc_fwd(b, s);
                    },
                    0, "td3::enc_fwd_kernel"});
      return;
    }
    st.push_back({name, [=](hipStream_t s) { return launch_enc_fwd(a, s); }, 0, "td3::enc_fwd_kernel"});
  };
  auto head = [&](const NetL& n, const float* Pp, EvalB& e, int mode) {
    HeadProb q{};
    q.H3 = e.H[2];
    q.ldh = n.lin[2].Np;
    q.K3 = n.lin[2].N;
    q.lng = norm ? Pp + n.ln[2].offg : nullptr;
    q.lnb = norm ? Pp + n.ln[2].offb : nullptr;
    q.W4 = Pp + n.lin[3].offW;
    q.ldw = n.lin[3].Kp;
    q.b4 = Pp + n.lin[3].offb;
    q.nout = n.lin[3].N;
    q.mode = mode;
    return q;
  };
  const float* Pa = h->actor.P;
  const float* Pq = h->critic.P;
  {
    enc_stage(A->act, {EncFwdProb{Pa + an.enc_off, 0, A->X_S, lda, nullptr}}, "act_enc");
    std::vector<FwdItem> f = {{&an, Pa, &A->A, false, false}};
    TD3_RC(add_fwd_stages(h, A->tables, A->act, f, Bp, Bp, "act", nullptr, 0));
    HeadProb p = head(an, Pa, A->A, kHeadPolicy);
    p.out = A->out;
    p.ldo = 32;
    p.out_col = 0;
    void* d = nullptr;
    TD3_RC(upload(h, A->tables, &p, sizeof(p), &d));
    HeadArgs a{};
    a.probs = (const HeadProb*)d;
    a.B = Bp;
    a.Bp = Bp;
    a.max_action = 1.0f;                              // tanh policy (TD3_particles.py:68)
    A->act.push_back({"act_head", [=](hipStream_t s) { return launch_heads(a, 1, s); }, 0});
  }
  {
    std::vector<EncFwdProb> ep = {EncFwdProb{Pq + q1.enc_off, 0, A->X_SA, ldq, nullptr}};
    if (cdq) ep.push_back(EncFwdProb{Pq + q2.enc_off, 0, A->XQ2, ldq, nullptr});
    enc_stage(A->evalq, ep, "evq_enc");
    std::vector<FwdItem> f = {{&q1, Pq, &A->Q[0], false, false}};
    if (cdq) f.push_back({&q2, Pq, &A->Q[1], false, false});
    TD3_RC(add_fwd_stages(h, A->tables, A->evalq, f, Bp, Bp, "evq", nullptr, 0));
    std::vector<HeadProb> hp;
    for (int j = 0; j < (cdq ? 2 : 1); ++j) {
      HeadProb p = head(j ? q2 : q1, Pq, A->Q[j], kHeadQ);
      p.out = A->q[j];
      p.ldo = 32;
      hp.push_back(p);
    }
    void* d = nullptr;
    TD3_RC(upload(h, A->tables, hp.data(), hp.size() * sizeof(HeadProb), &d));
    HeadArgs a{};
    a.probs = (const HeadProb*)d;
    a.B = Bp;
    a.Bp = Bp;
    a.max_action = 1.0f;
    const int nh = (int)hp.size();
    A->evalq.push_back({"evq_head", [=](hipStream_t s) { return launch_heads(a, nh, s); }, 0});
  }
  (void)ad;
  *out = A.get();
  plans[Bp] = std::move(A);
  return 0;
}

static int copy_rows_h2d(float* dst, int ld, int col, const float* src, int n, int cols, hipStream_t s) {
  TD3_HIP(hipMemcpy2DAsync(dst + col, (size_t)ld * 4, src, (size_t)cols * 4, (size_t)cols * 4, n,
                           hipMemcpyHostToDevice, s));
  return 0;
}

}  // namespace td3

// ================================================================== C-ABI
extern "C" {

const char* td3_last_error(void) { return g_err; }

size_t td3_config_size(void) { return sizeof(td3_config); }

int td3_default_config(td3_config* c, size_t cfg_size) {
  TD3_ARG(c != nullptr, "null config");
  if (cfg_size != sizeof(td3_config)) {
    set_error("td3_default_config: caller's td3_config is %zu bytes, the library's %zu (binding out of date "
              "with include/td3.h)", cfg_size, sizeof(td3_config));
    return -1;
  }
  memset(c, 0, sizeof(*c));
  c->struct_size = (int)sizeof(td3_config);
  c->actor_hidden[0] = 500; c->actor_hidden[1] = 400; c->actor_hidden[2] = 300;    // TD3_featured.py:19
  c->critic_hidden[0] = 500; c->critic_hidden[1] = 400; c->critic_hidden[2] = 200; // TD3_featured.py:54
  c->norm = 1;
  c->max_action = 1.0f;
  c->discount = 0.99;       // TD3_base.py:9 / main.py:112
  c->tau = 0.005;
  c->policy_noise = 0.2;
  c->noise_clip = 0.5;
  c->policy_freq = 2;
  c->lr = 1e-4;             // TD3_featured.py:100 / main.py:116
  c->beta1 = 0.9;
  c->beta2 = 0.999;
  c->eps = 1e-8;
  c->seed = 0;
  c->device = 0;
  c->use_graph = 2;
  c->particles = 0;
  c->cdq = 1;
  return 0;
}

// Device counters with the Adam bias-correction powers at these steps (Python's beta ** step).
static Counters make_counters(const td3_handle* h, int64_t total_it, int64_t critic_step, int64_t actor_step) {
  Counters c{};
  c.total_it = total_it;
  c.critic_step = critic_step;
  c.actor_step = actor_step;
  c.beta[0] = h->adam[0].beta1;
  c.beta[1] = h->adam[0].beta2;
  c.beta[2] = h->adam[1].beta1;
  c.beta[3] = h->adam[1].beta2;
  c.pw[0] = std::pow(c.beta[0], (double)critic_step);
  c.pw[1] = std::pow(c.beta[1], (double)critic_step);
  c.pw[2] = std::pow(c.beta[2], (double)actor_step);
  c.pw[3] = std::pow(c.beta[3], (double)actor_step);
  return c;
}

int td3_create(const td3_config* cfg, td3_handle** out) {
  TD3_ARG(cfg && out, "null argument");
  if (cfg->struct_size != (int)sizeof(td3_config)) {
    set_error("td3_create: td3_config.struct_size is %d, the library's td3_config is %zu bytes (fill it with "
              "td3_default_config; binding out of date with include/td3.h?)", cfg->struct_size, sizeof(td3_config));
    return -1;
  }
  TD3_ARG(cfg->state_dim > 0 && cfg->action_dim > 0, "dims must be positive");
  TD3_ARG(cfg->action_dim <= 32, "action_dim > 32 not supported by the head kernels");
  TD3_ARG(cfg->policy_freq > 0, "policy_freq must be positive");
  TD3_ARG(cfg->norm >= 0 && cfg->norm <= 2, "norm must be 0 (None), 1 (layer) or 2 (weight_normalization)");
  TD3_ARG(!(cfg->particles && cfg->norm == 2), "weight_normalization is a TD3_featured option");
  const int in_extra = cfg->particles ? kEncC2 : 0;
  TD3_ARG(pad32(in_extra + cfg->state_dim + cfg->action_dim) <= 512, "network input width must be <= 512");
  if (cfg->particles) {
    TD3_ARG(cfg->n_particles > 0 && cfg->particle_dim > 0, "particle shape must be positive");
    TD3_ARG(cfg->particle_dim <= kEncMaxD, "particle_dim > 16 not supported by the encoder kernels");
  }
  for (int i = 0; i < 3; ++i) {
    TD3_ARG(cfg->actor_hidden[i] > 0 && cfg->actor_hidden[i] <= 512, "actor hidden in (0, 512]");
    TD3_ARG(cfg->critic_hidden[i] > 0 && cfg->critic_hidden[i] <= 512, "critic hidden in (0, 512]");
  }
  TD3_HIP(hipSetDevice(cfg->device));
  TD3_RC(kernels_init());
  TD3_RC(encoder_init());
  td3_handle* h = new td3_handle();
  h->cfg = *cfg;
  h->adam[0] = h->adam[1] = td3_handle::AdamHp{cfg->lr, cfg->beta1, cfg->beta2, cfg->eps};
  h->sd = cfg->state_dim;
  h->ad = cfg->action_dim;
  const int norm = cfg->norm;
  int64_t off = 0;
  if (cfg->particles) {                     // TD3_particles.py:19-50 (Actor), :71-128 (Critic)
    h->particles = 1;
    h->N = cfg->n_particles;
    h->D = cfg->particle_dim;
    h->cdq = cfg->cdq ? 1 : 0;
    const int F = h->sd, A = h->ad, D = h->D;
    h->actor.nets.push_back(layout_mlp(kEncC2 + F, cfg->actor_hidden, A, norm, "", off, h->actor.tensors, D));
    h->actor.size = (off + 63) & ~(int64_t)63;
    off = 0;
    h->critic.nets.push_back(
        layout_mlp(kEncC2 + F + A, cfg->critic_hidden, A, norm, "q1.", off, h->critic.tensors, D));
    if (h->cdq)
      h->critic.nets.push_back(
          layout_mlp(kEncC2 + F + A, cfg->critic_hidden, A, norm, "q2.", off, h->critic.tensors, D));
    h->critic.size = (off + 63) & ~(int64_t)63;
  } else {
    h->actor.nets.push_back(layout_mlp(h->sd, cfg->actor_hidden, h->ad, norm, "", off, h->actor.tensors));
    h->actor.size = off;
    off = 0;
    h->critic.nets.push_back(layout_mlp(h->sd + h->ad, cfg->critic_hidden, 1, norm, "q1.", off, h->critic.tensors));
    h->critic.nets.push_back(layout_mlp(h->sd + h->ad, cfg->critic_hidden, 1, norm, "q2.", off, h->critic.tensors));
    h->critic.size = off;
  }
  h->actor.cap = ((h->actor.size + 255) & ~(int64_t)255) + 256;
  h->critic.cap = ((h->critic.size + 255) & ~(int64_t)255) + 256;
  const size_t total = 7 * (size_t)(h->actor.cap + h->critic.cap);
  hipError_t e = hipMalloc(&h->arena, total * sizeof(float));
  if (e != hipSuccess) {
    set_error("td3_create: hipMalloc failed: %s", hipGetErrorString(e));
    delete h;
    return -2;
  }
  TD3_HIP(hipMemset(h->arena, 0, total * sizeof(float)));
  float* p = h->arena;
  for (Group* g : {&h->actor, &h->critic}) {
    g->P = p; p += g->cap;
    g->T = p; p += g->cap;
    g->M = p; p += g->cap;
    g->V = p; p += g->cap;
    g->G = p; p += g->cap;
    g->P4 = p; p += g->cap;
    g->T4 = p; p += g->cap;
  }
  TD3_HIP(hipMalloc(&h->d_ctr, sizeof(Counters)));
  {
    float one[64];
    for (float& v : one) v = 1.0f;
    TD3_HIP(hipMalloc(&h->ones, sizeof(one)));
    TD3_HIP(hipMemcpy(h->ones, one, sizeof(one), hipMemcpyHostToDevice));
  }
  {
    const Counters c0 = make_counters(h, 0, 0, 0);
    TD3_HIP(hipMemcpy(h->d_ctr, &c0, sizeof(c0), hipMemcpyHostToDevice));
  }
  if (norm == 2) {
    for (Group* g : {&h->actor, &h->critic}) {
      WnArgs& w = g->wn;
      for (const NetL& n : g->nets)
        for (const LinearL& L : n.lin) {
          TD3_ARG(w.nlin < kMaxWnLinears, "too many weight-normalised Linears");
          w.lin[w.nlin++] = WnLinear{L.offW, L.offb, L.offg, L.offv, L.N, L.K, L.Kp, w.rows};
          w.rows += L.N;
        }
    }
  }
  TD3_HIP(hipDeviceSynchronize());          // null-stream memsets vs the handle's non-blocking streams
  TD3_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  TD3_HIP(hipStreamCreateWithFlags(&h->act_stream, hipStreamNonBlocking));
  *out = h;
  return 0;
}

int td3_destroy(td3_handle* h) {
  if (!h) return 0;
  (void)hipSetDevice(h->cfg.device);
  (void)hipStreamSynchronize(h->stream);
  (void)hipStreamSynchronize(h->act_stream);
  ring_forget_stream(h->stream);        // rings that noted it as their reader / writer
  if (h->plan) destroy_plan(h->plan.get());
  // a device-resident query on a caller's stream may still read its plan and the parameters
  if (h->dev_stream && h->dev_stream != h->stream) (void)hipStreamSynchronize(h->dev_stream);
  if (h->dev_ev) (void)hipEventDestroy(h->dev_ev);
  for (auto* plans : {&h->act, &h->act_dev})
    for (auto& kv : *plans) {
      free_plan_tables(kv.second->tables);
      (void)hipFree(kv.second->scratch);
      if (kv.second->hio) (void)hipHostFree(kv.second->hio);
    }
  if (h->comm_stream) {
    (void)hipStreamSynchronize(h->comm_stream);
    (void)hipStreamDestroy(h->comm_stream);
    (void)hipEventDestroy(h->comm_ev);
    (void)hipEventDestroy(h->comm_ev1);
    (void)hipEventDestroy(h->comm_done);
  }
  if (h->comm) ncclCommDestroy(h->comm);
  if (h->local)       // the group loses a member: the rest refuse td3_train_step_local from now on
    for (auto& m : h->local->hs)
      if (m == h) m = nullptr;
  (void)hipFree(h->arena);
  (void)hipFree(h->d_ctr);
  (void)hipFree(h->ones);
  (void)hipStreamSynchronize(h->act_stream);
  (void)hipStreamDestroy(h->act_stream);
  if (h->actor_ev) (void)hipEventDestroy(h->actor_ev);
  (void)hipStreamDestroy(h->stream);
  delete h;
  return 0;
}

int td3_tensor_count(const td3_handle* h, int g) {
  if (!h) return -1;
  return (int)(g ? h->critic.tensors.size() : h->actor.tensors.size());
}

int td3_tensor_info(const td3_handle* h, int g, int i, char* name, int name_len, int64_t* rows,
                    int64_t* cols) {
  TD3_ARG(h != nullptr, "null handle");
  const Group& G = g ? h->critic : h->actor;
  TD3_ARG(i >= 0 && i < (int)G.tensors.size(), "tensor index out of range");
  const TensorRef& t = G.tensors[i];
  if (name && name_len > 0) snprintf(name, name_len, "%s", t.name.c_str());
  if (rows) *rows = t.rows;
  if (cols) *cols = t.cols;
  return 0;
}

int64_t td3_num_params(const td3_handle* h, int g) {
  if (!h) return -1;
  const Group& G = g ? h->critic : h->actor;
  int64_t n = 0;
  for (auto& t : G.tensors) n += t.rows * (t.cols ? t.cols : 1);
  return n;
}

static int which_ptr(td3_handle* h, int which, Group** g, float** base) {
  switch (which) {
    case TD3_ACTOR: *g = &h->actor; *base = h->actor.P; return 0;
    case TD3_ACTOR_TARGET: *g = &h->actor; *base = h->actor.T; return 0;
    case TD3_CRITIC: *g = &h->critic; *base = h->critic.P; return 0;
    case TD3_CRITIC_TARGET: *g = &h->critic; *base = h->critic.T; return 0;
    case TD3_ACTOR_ADAM_M: *g = &h->actor; *base = h->actor.M; return 0;
    case TD3_ACTOR_ADAM_V: *g = &h->actor; *base = h->actor.V; return 0;
    case TD3_CRITIC_ADAM_M: *g = &h->critic; *base = h->critic.M; return 0;
    case TD3_CRITIC_ADAM_V: *g = &h->critic; *base = h->critic.V; return 0;
    case TD3_ACTOR_GRAD: *g = &h->actor; *base = h->actor.G; return 0;
    case TD3_CRITIC_GRAD: *g = &h->critic; *base = h->critic.G; return 0;
  }
  set_error("unknown tensor group %d", which);
  return -1;
}

// Sharded optimizer state (the Adam moments of slice k live on rank k): the in-process seam copies
// the other replicas' slices in before a moment is read; RCCL ranks gather them with the collective
// td3_dp_gather_optimizer_state, which a read of the moments then requires.
static int consolidate_moments(td3_handle* h, int which) {
  if (!h->dp_sharded || h->nranks <= 1) return 0;
  const bool m = which == TD3_ACTOR_ADAM_M || which == TD3_CRITIC_ADAM_M;
  const bool v = which == TD3_ACTOR_ADAM_V || which == TD3_CRITIC_ADAM_V;
  if (!m && !v) return 0;
  const bool actor = which == TD3_ACTOR_ADAM_M || which == TD3_ACTOR_ADAM_V;
  if (h->local) {
    const int64_t sl = shard_slice(actor ? h->actor : h->critic, h->nranks);
    for (int k = 0; k < (int)h->local->hs.size(); ++k) {
      td3_handle* o = h->local->hs[k];
      if (o == h || !o) continue;
      const Group& src = actor ? o->actor : o->critic;
      const Group& dst = actor ? h->actor : h->critic;
      TD3_HIP(hipMemcpy((m ? dst.M : dst.V) + k * sl, (m ? src.M : src.V) + k * sl, (size_t)sl * 4,
                        hipMemcpyDeviceToDevice));
    }
    return 0;
  }
  TD3_ARG(h->opt_gathered_it == h->total_it,
          "sharded optimizer state: call td3_dp_gather_optimizer_state on every rank before reading the "
          "Adam moments (a collective)");
  return 0;
}

int td3_dp_gather_optimizer_state(td3_handle* h) {
  TD3_ARG(h != nullptr, "null handle");
  TD3_HIP(hipSetDevice(h->cfg.device));
  if (h->dp_sharded && h->comm && h->nranks > 1) {
    // a C-API caller may have stepped on its own stream: the moments are final only once it drained
    if (h->last_step_stream && h->last_step_stream != h->stream) TD3_HIP(hipStreamSynchronize(h->last_step_stream));
    for (Group* g : {&h->actor, &h->critic}) {
      const int64_t sl = shard_slice(*g, h->nranks);
      for (float* a : {g->M, g->V}) {
        ncclResult_t r = ncclAllGather(a + h->rank * sl, a, (size_t)sl, ncclFloat, h->comm, h->stream);
        if (r != ncclSuccess) {
          set_error("ncclAllGather: %s", ncclGetErrorString(r));
          return -2;
        }
      }
    }
    TD3_HIP(hipStreamSynchronize(h->stream));
  }
  h->opt_gathered_it = h->total_it;
  return 0;
}

int td3_get_params(td3_handle* h, int which, float* out, int64_t n) {
  TD3_ARG(h && out, "null argument");
  Group* g;
  float* base;
  TD3_RC(which_ptr(h, which, &g, &base));
  TD3_ARG(n == td3_num_params(h, g == &h->critic), "size mismatch");
  TD3_HIP(hipSetDevice(h->cfg.device));
  TD3_HIP(hipStreamSynchronize(h->stream));
  TD3_HIP(hipDeviceSynchronize());
  TD3_RC(consolidate_moments(h, which));
  std::vector<float> host(g->size);
  TD3_HIP(hipMemcpy(host.data(), base, g->size * 4, hipMemcpyDeviceToHost));
  int64_t o = 0;
  for (auto& t : g->tensors) {
    if (t.cols) {
      for (int64_t r = 0; r < t.rows; ++r)
        memcpy(out + o + r * t.cols, host.data() + t.off + r * t.ld, t.cols * 4);
      o += t.rows * t.cols;
    } else {
      memcpy(out + o, host.data() + t.off, t.rows * 4);
      o += t.rows;
    }
  }
  return 0;
}

int td3_set_params(td3_handle* h, int which, const float* in, int64_t n) {
  TD3_ARG(h && in, "null argument");
  TD3_ARG(which != TD3_ACTOR_GRAD && which != TD3_CRITIC_GRAD, "the gradient arenas are read only");
  Group* g;
  float* base;
  TD3_RC(which_ptr(h, which, &g, &base));
  TD3_ARG(n == td3_num_params(h, g == &h->critic), "size mismatch");
  TD3_HIP(hipSetDevice(h->cfg.device));
  TD3_HIP(hipStreamSynchronize(h->stream));
  TD3_HIP(hipDeviceSynchronize());
  std::vector<float> host(g->size, 0.f);
  int64_t o = 0;
  for (auto& t : g->tensors) {
    if (t.cols) {
      for (int64_t r = 0; r < t.rows; ++r)
        memcpy(host.data() + t.off + r * t.ld, in + o + r * t.cols, t.cols * 4);
      o += t.rows * t.cols;
    } else {
      memcpy(host.data() + t.off, in + o, t.rows * 4);
      o += t.rows;
    }
  }
  TD3_HIP(hipMemcpy(base, host.data(), g->size * 4, hipMemcpyHostToDevice));
  if (base == g->P || base == g->T) g->w4_valid = false;   // repacked by the next w4 step
  if (g->wn.nlin > 0 && (base == g->P || base == g->T)) {   // W = v * (g / ||v||) of the new (g, v)
    WnArgs w = g->wn;
    w.mode = kWnDerive;
    w.arena = base;
    w.arena2 = nullptr;
    TD3_RC(launch_wn(w, h->stream));
    TD3_HIP(hipStreamSynchronize(h->stream));
  }
  return 0;
}

int td3_get_counters(const td3_handle* h, int64_t* total_it, int64_t* critic_step, int64_t* actor_step) {
  TD3_ARG(h != nullptr, "null handle");
  if (total_it) *total_it = h->total_it;
  if (critic_step) *critic_step = h->critic_step;
  if (actor_step) *actor_step = h->actor_step;
  return 0;
}

int td3_set_counters(td3_handle* h, int64_t total_it, int64_t critic_step, int64_t actor_step) {
  TD3_ARG(h != nullptr, "null handle");
  TD3_ARG(total_it >= 0 && critic_step >= 0 && actor_step >= 0, "negative counter");
  TD3_HIP(hipSetDevice(h->cfg.device));
  TD3_HIP(hipStreamSynchronize(h->stream));
  const Counters c = make_counters(h, total_it, critic_step, actor_step);
  TD3_HIP(hipMemcpy(h->d_ctr, &c, sizeof(c), hipMemcpyHostToDevice));
  h->total_it = total_it;
  h->critic_step = critic_step;
  h->actor_step = actor_step;
  return 0;
}

int td3_set_adam(td3_handle* h, int group, double lr, double beta1, double beta2, double eps) {
  TD3_ARG(h != nullptr, "null handle");
  TD3_ARG(group == 0 || group == 1, "group must be 0 (actor) or 1 (critic)");
  TD3_ARG(lr >= 0 && eps >= 0 && beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1,
          "Adam hyper-parameters out of range (torch adam.py: 0 <= lr, eps; 0 <= betas < 1)");
  TD3_HIP(hipSetDevice(h->cfg.device));
  TD3_HIP(hipStreamSynchronize(h->stream));
  td3_handle::AdamHp& hp = h->adam[group == 0 ? 1 : 0];
  if (hp.lr == lr && hp.beta1 == beta1 && hp.beta2 == beta2 && hp.eps == eps) return 0;
  hp = td3_handle::AdamHp{lr, beta1, beta2, eps};
  const Counters c = make_counters(h, h->total_it, h->critic_step, h->actor_step);
  TD3_HIP(hipMemcpy(h->d_ctr, &c, sizeof(c), hipMemcpyHostToDevice));
  if (h->plan) TD3_RC(build_plan(h, h->plan->B));   // the dW stages carry lr / betas / eps
  return 0;
}

int td3_get_adam(const td3_handle* h, int group, double out[4]) {
  TD3_ARG(h && out, "null argument");
  TD3_ARG(group == 0 || group == 1, "group must be 0 (actor) or 1 (critic)");
  const td3_handle::AdamHp& hp = h->adam[group == 0 ? 1 : 0];
  out[0] = hp.lr;
  out[1] = hp.beta1;
  out[2] = hp.beta2;
  out[3] = hp.eps;
  return 0;
}

int td3_train_step(td3_handle* h, rb_handle* rbh, int batch, void* stream, const int64_t* inject_idx,
                   const float* inject_noise, td3_step_stats* stats) {
  TD3_ARG(h && rbh, "null handle");
  TD3_ARG(batch > 0, "batch must be positive");
  Ring* r = reinterpret_cast<Ring*>(rbh);
  TD3_ARG(r->sd == h->sd && r->ad == h->ad, "replay buffer dims do not match the learner");
  TD3_ARG(r->size > 0 || inject_idx, "train on an empty replay buffer");
  TD3_ARG(r->device == h->cfg.device, "replay buffer lives on another device");
  TD3_HIP(hipSetDevice(h->cfg.device));
  TD3_ARG(r->particles == h->particles, "replay buffer kind does not match the learner");
  TD3_ARG(!r->particles || (r->N == h->N && r->D == h->D), "particle shape does not match the learner");
  TD3_RC(ensure_plan(h, batch));
  Plan* P = h->plan.get();
  TD3_RC(bind_ring(h, r));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  TD3_RC(ring_begin_read(r, s));                 // the adds queued before this step, not after
  if (inject_idx) {
    for (int i = 0; i < batch; ++i)
      TD3_ARG(inject_idx[i] >= 0 && inject_idx[i] < r->cap, "injected index out of range");
    TD3_HIP(hipMemcpyAsync(P->d_inject_idx, inject_idx, (size_t)batch * 8, hipMemcpyHostToDevice, s));
  }
  if (inject_noise)
    TD3_HIP(hipMemcpyAsync(P->noise, inject_noise, (size_t)batch * h->ad * 4, hipMemcpyHostToDevice, s));
  const int actor_phase = ((h->total_it + 1) % h->cfg.policy_freq) == 0;
  if (inject_idx) {
    TD3_RC(input_from_ring(h, r, P, true, s));
    TD3_RC(run_body(h, actor_phase, inject_noise ? 1 : 0, s, nullptr));
  } else {
    TD3_RC(run_body(h, actor_phase, inject_noise ? 1 : 0, s, r));
  }
  TD3_RC(ring_end_read(r, s));                   // later adds wait for this step's reads
  if (inject_idx || inject_noise) TD3_HIP(hipStreamSynchronize(s));   // host sources are pageable
  return finish_step(h, actor_phase, s, stats);
}

int td3_train_step_prioritized(td3_handle* h, rb_handle* rbh, int batch, double beta, void* stream,
                               const float* inject_u, const float* inject_noise, td3_step_stats* stats,
                               td3_per_stats* per) {
  TD3_ARG(h && rbh, "null handle");
  TD3_ARG(batch > 0, "batch must be positive");
  TD3_ARG(beta >= 0.0 && beta <= 1.0, "beta must be in [0, 1]");
  TD3_ARG(!h->particles, "td3_train_step_prioritized on a particle learner (its loss takes no importance weights)");
  TD3_ARG(!h->comm && !h->local, "td3_train_step_prioritized on a data-parallel handle (comm group attached)");
  Ring* r = reinterpret_cast<Ring*>(rbh);
  TD3_ARG(r->particles == h->particles, "replay buffer kind does not match the learner");
  TD3_ARG(r->sd == h->sd && r->ad == h->ad, "replay buffer dims do not match the learner");
  TD3_ARG(r->device == h->cfg.device, "replay buffer lives on another device");
  TD3_ARG(r->pri.on, "priorities are not enabled on this ring (rb_enable_priorities)");
  TD3_ARG(r->size > 0, "train on an empty replay buffer");
  TD3_HIP(hipSetDevice(h->cfg.device));
  TD3_RC(ensure_plan(h, batch));
  Plan* P = h->plan.get();
  TD3_RC(bind_ring(h, r));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  TD3_RC(ring_begin_read(r, s));                 // one section: draw, gather, body, priority write-back
  if (inject_u) TD3_HIP(hipMemcpyAsync(P->per_u, inject_u, (size_t)batch * 4, hipMemcpyHostToDevice, s));
  if (inject_noise)
    TD3_HIP(hipMemcpyAsync(P->noise, inject_noise, (size_t)batch * h->ad * 4, hipMemcpyHostToDevice, s));
  const int actor_phase = ((h->total_it + 1) % h->cfg.policy_freq) == 0;
  P->per_w_dirty = true;
  TD3_RC(ring_draw_prioritized(r, batch, beta, inject_u ? P->per_u : nullptr, P->d_inject_idx, P->d_idx, P->per_w, s));
  TD3_RC(input_from_ring(h, r, P, true, s));
  h->per_step = true;
  const int rc = run_body(h, actor_phase, inject_noise ? 1 : 0, s, nullptr);
  h->per_step = false;
  TD3_RC(rc);
  TD3_RC(ring_store_priorities(r, P->d_inject_idx, P->per_td, batch, true, s));
  TD3_RC(ring_end_read(r, s));                   // later adds wait for the step and its write-back
  if (inject_u || inject_noise) TD3_HIP(hipStreamSynchronize(s));   // host sources are pageable
  TD3_RC(finish_step(h, actor_phase, s, stats));
  if (per && (per->weight || per->td_abs)) {
    TD3_HIP(hipStreamSynchronize(s));
    if (per->weight) TD3_HIP(hipMemcpy(per->weight, P->per_w, (size_t)batch * 4, hipMemcpyDeviceToHost));
    if (per->td_abs) TD3_HIP(hipMemcpy(per->td_abs, P->per_td, (size_t)batch * 4, hipMemcpyDeviceToHost));
  }
  return 0;
}

int td3_train_step_batch(td3_handle* h, const float* state, const float* action, const float* next_state,
                         const float* reward, const float* not_done, int batch, void* stream,
                         const float* inject_noise, td3_step_stats* stats) {
  TD3_ARG(h != nullptr, "null handle");
  TD3_ARG(state && action && next_state && reward && not_done, "null input");
  TD3_ARG(batch > 0, "batch must be positive");
  TD3_ARG(!h->particles, "td3_train_step_batch on a particle learner (use td3_train_step_batch_particles)");
  TD3_HIP(hipSetDevice(h->cfg.device));
  TD3_RC(ensure_plan(h, batch));
  Plan* P = h->plan.get();
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  if (inject_noise)
    TD3_HIP(hipMemcpyAsync(P->noise, inject_noise, (size_t)batch * h->ad * 4, hipMemcpyHostToDevice, s));
  const int actor_phase = ((h->total_it + 1) % h->cfg.policy_freq) == 0;
  TD3_RC(input_from_batch(h, P, state, action, next_state, reward, not_done, s));
  TD3_RC(run_body(h, actor_phase, inject_noise ? 1 : 0, s, nullptr));
  if (inject_noise) TD3_HIP(hipStreamSynchronize(s));
  return finish_step(h, actor_phase, s, stats);
}

// Host-side query I/O of an ActPlan: rows into the plan's inputs / outputs out to the caller.
// Mapped plans (Bp <= kMappedRows) are written and read in place by the host; the stream is idle
// when they are touched (every query ends in a sync, and one starts with it in case an earlier
// query failed before its own).
static int put_rows(const ActPlan* A, float* dev, float* host, int ld, int col, const float* src, int n, int cols,
                    hipStream_t s) {
  if (!host) return copy_rows_h2d(dev, ld, col, src, n, cols, s);
  for (int i = 0; i < n; ++i) memcpy(host + (size_t)i * ld + col, src + (size_t)i * cols, (size_t)cols * 4);
  (void)A;
  return 0;
}

static int get_rows(float* dst, int cols, const float* dev, const float* host, int ld, int n, hipStream_t s) {
  if (host) {
    for (int i = 0; i < n; ++i) memcpy(dst + (size_t)i * cols, host + (size_t)i * ld, (size_t)cols * 4);
    return 0;
  }
  TD3_HIP(hipMemcpy2DAsync(dst, (size_t)cols * 4, dev, (size_t)ld * 4, (size_t)cols * 4, n, hipMemcpyDeviceToHost, s));
  TD3_HIP(hipStreamSynchronize(s));
  return 0;
}

// The one-launch query publishes its outputs with a flag in mapped host memory (act_kernel): the host
// polls that flag instead of synchronising the stream (a stream sync's wake-up is most of the ~10 us
// launch + sync round trip, DESIGN "Acting path").  A flag that does not arrive within 2 s falls back
// to a stream synchronize, then reports an error if it is still missing.
// A flag published with kActFailed (a workgroup's in-launch H1 poll gave up) is an error, not a result;
// after any failure the hand-off counters are re-zeroed once the launch has drained, so the next query
// does not start from a leftover count.
static int wait_flags(volatile unsigned* f, int nprob, unsigned seq, hipStream_t s, int* ctr) {
  const auto t0 = std::chrono::steady_clock::now();
  const char* err = nullptr;
  for (int k = 0; k < nprob && !err; ++k) {
    int spin = 0;
    unsigned v;
    while ((v = f[k]) != seq && v != (seq | kActFailed)) {
      __builtin_ia32_pause();
      if ((++spin & 1023) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
        TD3_HIP(hipStreamSynchronize(s));
        v = f[k];
        if (v != seq && v != (seq | kActFailed)) err = "the query kernel's completion flag did not arrive";
        break;
      }
    }
    if (!err && v == (seq | kActFailed)) err = "a query-kernel workgroup timed out waiting for layer 1 (outputs invalid)";
  }
  if (err) {
    TD3_HIP(hipStreamSynchronize(s));
    TD3_HIP(hipMemsetAsync(ctr, 0, sizeof(int) * 2 * nprob, s));
    TD3_HIP(hipStreamSynchronize(s));
    set_error("select_action / eval_q: %s", err);
    return -1;
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return 0;
}

// A featured query of n <= kGemvRows rows: layers 0 and 1 in one gemv01 launch when layer 0 is
// narrow (the query rows [x0 | x1] in its arguments), else one gemv launch per layer; then the
// head over 4 rows.
static int run_gemv(const ActPlan* A, bool q, int n, const float* x0, int c0, const float* x1, int c1,
                    hipStream_t s) {
  const GemvArgs(&gv)[3] = q ? A->gv_q : A->gv_act;
  const int nprob = q ? 2 : 1;
  if (A->act1) {                                        // the whole query in one launch
    ActArgs a = q ? A->a1_q : A->a1_act;
    a.g.l1.B = n;
    const int K0 = c0 + c1;
    for (int r = 0; r < n; ++r) {
      memcpy(a.g.xq + r * K0, x0 + (size_t)r * c0, (size_t)c0 * 4);
      if (c1) memcpy(a.g.xq + r * K0 + c0, x1 + (size_t)r * c1, (size_t)c1 * 4);
    }
    ActPlan* M = const_cast<ActPlan*>(A);
    unsigned& sq = M->seq[q ? 1 : 0];
    sq = (sq + 1) & ~kActFailed;            // the top bit marks a failed query; 0 is the flags' initial value
    if (sq == 0) sq = 1;
    a.seq = sq;
    if (M->fail_test > 0) {
      a.fail_test = 1;
      --M->fail_test;
    }
    TD3_RC(launch_act(a, nprob, s));
    return wait_flags(M->hflag[q ? 1 : 0], nprob, a.seq, s, a.ctr);
  }
  int l = 0;
  if (A->gemv01) {
    Gemv01Args g = q ? A->g01_q : A->g01_act;
    g.l1.B = n;
    const int K0 = c0 + c1;
    for (int r = 0; r < n; ++r) {
      memcpy(g.xq + r * K0, x0 + (size_t)r * c0, (size_t)c0 * 4);
      if (c1) memcpy(g.xq + r * K0 + c0, x1 + (size_t)r * c1, (size_t)c1 * 4);
    }
    TD3_RC(launch_gemv01(g, nprob, s));
    l = 2;
  }
  for (; l < 3; ++l) {
    GemvArgs a = gv[l];
    a.B = n;
    TD3_RC(launch_gemv(a, nprob, s));
  }
  HeadArgs head = q ? A->head_q : A->head_act;
  head.B = n;
  head.Bp = kGemvRows;
  return launch_heads(head, nprob, s);
}

// The stream a query runs on: behind a queued actor update in its own stream (critic-only steps
// leave the actor as it is), else the acting stream.  A query returns after its results landed, so
// the update it queued behind has finished: query_done forgets that stream.
static int query_stream(td3_handle* h, hipStream_t* out) {
  h->act_used = true;
  hipStream_t q = h->actor_stream ? h->actor_stream : h->act_stream;
  if (h->actor_ev_pending) {
    TD3_HIP(hipStreamWaitEvent(q, h->actor_ev, 0));
    h->actor_ev_pending = false;
  }
  *out = q;
  return 0;
}
static int query_done(td3_handle* h, hipStream_t s, int rc) {
  if (rc == 0 && s == h->actor_stream) h->actor_stream = nullptr;
  return rc;
}

int td3_select_action(td3_handle* h, const float* state, float* action_out, int n) {
  TD3_ARG(h && state && action_out, "null argument");
  TD3_ARG(!h->particles, "particle learner: use td3_select_action_particles");
  TD3_ARG(n > 0, "n must be positive");
  TD3_HIP(hipSetDevice(h->cfg.device));
  ActPlan* A;
  TD3_RC(build_act(h, pad32(n), &A));
  hipStream_t s;
  TD3_RC(query_stream(h, &s));
  if (A->act1 && A->gemv && n <= kGemvRows) {
    // the query travels in the kernel arguments and the outputs of the previous query were read
    // before it returned: no stream synchronize on either side (wait_flags)
    TD3_RC(run_gemv(A, false, n, state, h->sd, nullptr, 0, s));
    return query_done(h, s, get_rows(action_out, h->ad, A->out, A->hout, A->ldo, n, s));
  }
  if (A->hio) TD3_HIP(hipStreamSynchronize(s));
  if (A->gemv && n <= kGemvRows) {
    if (!A->gemv01) TD3_RC(put_rows(A, A->X_S, A->hX_S, pad32(h->sd), 0, state, n, h->sd, s));
    TD3_RC(run_gemv(A, false, n, state, h->sd, nullptr, 0, s));
  } else {
    TD3_RC(put_rows(A, A->X_S, A->hX_S, pad32(h->sd), 0, state, n, h->sd, s));
    TD3_RC(run_stages(A->act, s));
  }
  if (A->hio) TD3_HIP(hipStreamSynchronize(s));
  return query_done(h, s, get_rows(action_out, h->ad, A->out, A->hout, A->ldo, n, s));
}

int td3_eval_q(td3_handle* h, const float* state, const float* action, float* q_out, int n) {
  TD3_ARG(h && state && action && q_out, "null argument");
  TD3_ARG(!h->particles, "particle learner: use td3_eval_q_particles");
  TD3_ARG(n > 0, "n must be positive");
  TD3_HIP(hipSetDevice(h->cfg.device));
  ActPlan* A;
  TD3_RC(build_act(h, pad32(n), &A));
  hipStream_t s = h->stream;
  const int ld = pad32(h->sd + h->ad);
  const bool small = A->gemv && n <= kGemvRows;
  if (A->act1 && small) {        // one launch, completion flags polled on the host (no stream syncs)
    TD3_RC(run_gemv(A, true, n, state, h->sd, action, h->ad, s));
    TD3_RC(get_rows(q_out, 1, A->q[0], A->hq[0], 1, n, s));
    return get_rows(q_out + n, 1, A->q[1], A->hq[1], 1, n, s);
  }
  if (A->hio) TD3_HIP(hipStreamSynchronize(s));
  if (!small || !A->gemv01) {
    TD3_RC(put_rows(A, A->X_SA, A->hX_SA, ld, 0, state, n, h->sd, s));
    TD3_RC(put_rows(A, A->X_SA, A->hX_SA, ld, h->sd, action, n, h->ad, s));
  }
  if (small) TD3_RC(run_gemv(A, true, n, state, h->sd, action, h->ad, s));
  else TD3_RC(run_stages(A->evalq, s));
  if (A->hio) TD3_HIP(hipStreamSynchronize(s));
  TD3_RC(get_rows(q_out, 1, A->q[0], A->hq[0], 1, n, s));
  return get_rows(q_out + n, 1, A->q[1], A->hq[1], 1, n, s);
}

// ------------------------------------------------------------------ device-resident queries
// The stream a device query runs on, ordered by events where stream order does not already do it:
// after the last queued step (the parameters it may still update) and after a previous device query
// on another stream (the act_dev plans' scratch).  NULL is the step stream itself.
static int device_query_stream(td3_handle* h, void* stream, hipStream_t* out) {
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  if (!h->dev_ev) TD3_HIP(hipEventCreateWithFlags(&h->dev_ev, TD3_EV_FLAGS));
  for (hipStream_t prev : {h->last_step_stream, h->dev_stream}) {
    if (!prev || prev == s) continue;
    TD3_HIP(hipEventRecord(h->dev_ev, prev));
    TD3_HIP(hipStreamWaitEvent(s, h->dev_ev, 0));
  }
  h->dev_stream = s;
  *out = s;
  return 0;
}

// The epilogue of both device policy queries: the head's rows (stride A->ldo) -> action_out [n][ad],
// with the exploration noise of `ex` and the clip to cfg.max_action (ex NULL: the rows as they are).
static int explore_rows(td3_handle* h, const ActPlan* A, int n, const td3_explore* ex, float* action_out,
                        hipStream_t s) {
  ExploreArgs e{};
  e.pi = A->out;
  e.ldp = A->ldo;
  e.action_out = action_out;
  e.n = n;
  e.ad = h->ad;
  e.plain = ex ? 0 : 1;
  e.max_action = h->cfg.max_action;
  if (ex) {
    e.x = ex->x;
    e.mu = ex->mu;
    e.theta = ex->theta;
    e.sigma = ex->sigma;
    e.reset = ex->reset;
    e.seed = ex->seed;
    e.step = ex->step;
    e.inject_z = ex->inject_z;
    e.z_out = ex->z_out;
  }
  return launch_explore(e, s);
}

int td3_select_action_device(td3_handle* h, const float* state, int n, const td3_explore* ex,
                             float* action_out, void* stream) {
  TD3_ARG(n > 0, "n must be positive");
  TD3_ARG(h && state && action_out, "null argument");
  TD3_ARG(!h->particles, "particle learner: use td3_select_action_particles_device");
  TD3_HIP(hipSetDevice(h->cfg.device));
  const int Bp = pad32(n);
  ActPlan* A;
  TD3_RC(build_act(h, Bp, &A, true));
  hipStream_t s;
  TD3_RC(device_query_stream(h, stream, &s));
  hipLaunchKernelGGL(pack_kernel, dim3(Bp), dim3(64), 0, s, state, h->sd, n, Bp, A->X_S, pad32(h->sd), 0,
                     (float*)nullptr, 0, 0, (float*)nullptr, 0, 0);
  TD3_HIP(hipGetLastError());
  TD3_RC(run_stages(A->act, s));
  return explore_rows(h, A, n, ex, action_out, s);
}

int td3_eval_q_device(td3_handle* h, const float* state, const float* action, int n, float* q_out, void* stream) {
  TD3_ARG(n > 0, "n must be positive");
  TD3_ARG(h && state && action && q_out, "null argument");
  TD3_ARG(!h->particles, "particle learner: use td3_eval_q_particles_device");
  TD3_HIP(hipSetDevice(h->cfg.device));
  const int Bp = pad32(n), ld = pad32(h->sd + h->ad);
  ActPlan* A;
  TD3_RC(build_act(h, Bp, &A, true));
  hipStream_t s;
  TD3_RC(device_query_stream(h, stream, &s));
  hipLaunchKernelGGL(pack_kernel, dim3(Bp), dim3(64), 0, s, state, h->sd, n, Bp, A->X_SA, ld, 0,
                     (float*)nullptr, 0, 0, (float*)nullptr, 0, 0);
  hipLaunchKernelGGL(pack_kernel, dim3(Bp), dim3(64), 0, s, action, h->ad, n, Bp, A->X_SA, ld, h->sd,
                     (float*)nullptr, 0, 0, (float*)nullptr, 0, 0);
  TD3_HIP(hipGetLastError());
  TD3_RC(run_stages(A->evalq, s));
  for (int j = 0; j < 2; ++j)        // the live rows of Q_j -> q_out[j][0..n)
    hipLaunchKernelGGL(pack_kernel, dim3(n), dim3(64), 0, s, A->q[j], 1, n, n, q_out + (size_t)j * n, 1, 0,
                       (float*)nullptr, 0, 0, (float*)nullptr, 0, 0);
  TD3_HIP(hipGetLastError());
  return 0;
}

int td3_train_step_batch_particles(td3_handle* h, const float* feat, const float* part, const float* action,
                                   const float* next_feat, const float* next_part, const float* reward,
                                   const float* not_done, int batch, void* stream, const float* inject_noise,
                                   td3_step_stats* stats) {
  TD3_ARG(h != nullptr, "null handle");
  TD3_ARG(h->particles, "td3_train_step_batch_particles on a featured learner");
  TD3_ARG(feat && part && action && next_feat && next_part && reward && not_done, "null input");
  TD3_ARG(batch > 0, "batch must be positive");
  TD3_HIP(hipSetDevice(h->cfg.device));
  TD3_RC(ensure_plan(h, batch));
  Plan* P = h->plan.get();
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  const int F = h->sd, ad = h->ad, B = P->B, Bp = P->Bp, np = h->N * h->D, c0 = kEncC2;
  const bool cdq = h->cdq != 0;
  set_particle_source(P, kBatchSource, P->pbatch, 2 * np, 0, np, P->d_iota);
  if (inject_noise)
    TD3_HIP(hipMemcpyAsync(P->noise, inject_noise, (size_t)batch * ad * 4, hipMemcpyHostToDevice, s));
  // the sampled tensors -> MLP input rows and the packed particle rows (s | s')
  hipLaunchKernelGGL(pack_kernel, dim3(Bp), dim3(64), 0, s, feat, F, B, Bp, P->XA, P->ld_a, c0, P->XAQ, P->ld_q,
                     c0, P->XQ[0], P->ld_q, c0);
  hipLaunchKernelGGL(pack_kernel, dim3(Bp), dim3(64), 0, s, action, ad, B, Bp, P->XQ[0], P->ld_q, c0 + F,
                     cdq ? P->XQ[1] : (float*)nullptr, P->ld_q, c0 + F, (float*)nullptr, 0, 0);
  hipLaunchKernelGGL(pack_kernel, dim3(Bp), dim3(64), 0, s, next_feat, F, B, Bp, P->XTA, P->ld_a, c0,
                     P->XTQ[0], P->ld_q, c0, cdq ? P->XTQ[1] : (float*)nullptr, P->ld_q, c0);
  if (cdq)
    hipLaunchKernelGGL(pack_kernel, dim3(Bp), dim3(64), 0, s, feat, F, B, Bp, P->XQ[1], P->ld_q, c0,
                       (float*)nullptr, 0, 0, (float*)nullptr, 0, 0);
  hipLaunchKernelGGL(pack_kernel, dim3(Bp), dim3(64), 0, s, part, np, B, Bp, P->pbatch, 2 * np, 0,
                     (float*)nullptr, 0, 0, (float*)nullptr, 0, 0);
  hipLaunchKernelGGL(pack_kernel, dim3(Bp), dim3(64), 0, s, next_part, np, B, Bp, P->pbatch, 2 * np, np,
                     (float*)nullptr, 0, 0, (float*)nullptr, 0, 0);
  hipLaunchKernelGGL(pack_kernel, dim3(Bp), dim3(64), 0, s, reward, 1, B, Bp, P->R, 1, 0, (float*)nullptr, 0, 0,
                     (float*)nullptr, 0, 0);
  hipLaunchKernelGGL(pack_kernel, dim3(Bp), dim3(64), 0, s, not_done, 1, B, Bp, P->ND, 1, 0, (float*)nullptr, 0,
                     0, (float*)nullptr, 0, 0);
  TD3_HIP(hipGetLastError());
  const int actor_phase = ((h->total_it + 1) % h->cfg.policy_freq) == 0;
  TD3_RC(run_body(h, actor_phase, inject_noise ? 1 : 0, s, nullptr));
  if (inject_noise) TD3_HIP(hipStreamSynchronize(s));
  return finish_step(h, actor_phase, s, stats);
}

int td3_actor_learn_particles(td3_handle* h, const float* feat, const float* part, int batch, void* stream,
                              double* actor_loss) {
  TD3_ARG(h != nullptr, "null handle");
  TD3_ARG(h->particles, "td3_actor_learn_particles on a featured learner (TD3_featured has no _actor_learn)");
  TD3_ARG(!h->local, "a td3_comm_init_local replica steps through td3_train_step_local only");
  TD3_ARG(feat && part, "null input");
  TD3_ARG(batch > 0, "batch must be positive");
  TD3_HIP(hipSetDevice(h->cfg.device));
  TD3_RC(ensure_plan(h, batch));
  Plan* P = h->plan.get();
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  const int F = h->sd, B = P->B, Bp = P->Bp, np = h->N * h->D, c0 = kEncC2;
  set_particle_source(P, kBatchSource, P->pbatch, 2 * np, 0, np, P->d_iota);
  // (features -> the actor's and Q1(s, pi)'s MLP input rows, particles -> the packed rows the
  // encoders read; the actions of Q1(s, pi) are written by the policy head)
  hipLaunchKernelGGL(pack_kernel, dim3(Bp), dim3(64), 0, s, feat, F, B, Bp, P->XA, P->ld_a, c0, P->XAQ, P->ld_q,
                     c0, (float*)nullptr, 0, 0);
  hipLaunchKernelGGL(pack_kernel, dim3(Bp), dim3(64), 0, s, part, np, B, Bp, P->pbatch, 2 * np, 0,
                     (float*)nullptr, 0, 0, (float*)nullptr, 0, 0);
  TD3_HIP(hipGetLastError());
  TD3_RC(run_stages(P->actor_learn, s));
  h->last_step_stream = s;
  h->actor_step += 1;
  TD3_RC(note_actor_update(h, s));
  if (!actor_loss) return 0;
  TD3_HIP(hipStreamSynchronize(s));
  const int nq = P->nq, ldq = P->ldq;
  std::vector<float> q((size_t)B * nq);
  TD3_HIP(hipMemcpy2D(q.data(), (size_t)nq * 4, P->AQ.Qv, (size_t)ldq * 4, (size_t)nq * 4, B, hipMemcpyDeviceToHost));
  double m = 0;
  for (float v : q) m += v;
  *actor_loss = -m / ((double)B * nq);
  return 0;
}

int td3_select_action_particles(td3_handle* h, const float* feat, const float* part, float* action_out, int n) {
  TD3_ARG(h && feat && part && action_out, "null argument");
  TD3_ARG(h->particles, "not a particle learner");
  TD3_ARG(n > 0, "n must be positive");
  TD3_HIP(hipSetDevice(h->cfg.device));
  ActPlan* A;
  TD3_RC(build_act_particles(h, pad32(n), &A));
  hipStream_t s;
  TD3_RC(query_stream(h, &s));
  if (A->hio) TD3_HIP(hipStreamSynchronize(s));
  const int np = h->N * h->D;
  const NetL& an = h->actor.nets[0];
  TD3_RC(put_rows(A, A->X_S, A->hX_S, an.lin[0].Kp, kEncC2, feat, n, h->sd, s));
  TD3_RC(put_rows(A, A->pbatch, A->hpbatch, np, 0, part, n, np, s));
  TD3_RC(run_stages(A->act, s));
  if (A->hio) TD3_HIP(hipStreamSynchronize(s));
  return query_done(h, s, get_rows(action_out, h->ad, A->out, A->hout, A->ldo, n, s));
}

int td3_eval_q_particles(td3_handle* h, const float* feat, const float* part, const float* action, float* q_out,
                         int n) {
  TD3_ARG(h && feat && part && action && q_out, "null argument");
  TD3_ARG(h->particles, "not a particle learner");
  TD3_ARG(n > 0, "n must be positive");
  TD3_HIP(hipSetDevice(h->cfg.device));
  ActPlan* A;
  TD3_RC(build_act_particles(h, pad32(n), &A));
  hipStream_t s = h->stream;
  const int np = h->N * h->D, F = h->sd, ad = h->ad;
  const int ldq = h->critic.nets[0].lin[0].Kp;
  const bool cdq = h->cdq != 0;
  if (A->hio) TD3_HIP(hipStreamSynchronize(s));
  for (int j = 0; j < (cdq ? 2 : 1); ++j) {
    float* X = j ? A->XQ2 : A->X_SA;
    float* hX = j ? A->hXQ2 : A->hX_SA;
    TD3_RC(put_rows(A, X, hX, ldq, kEncC2, feat, n, F, s));
    TD3_RC(put_rows(A, X, hX, ldq, kEncC2 + F, action, n, ad, s));
  }
  TD3_RC(put_rows(A, A->pbatch, A->hpbatch, np, 0, part, n, np, s));
  TD3_RC(run_stages(A->evalq, s));
  if (A->hio) TD3_HIP(hipStreamSynchronize(s));
  for (int j = 0; j < 2; ++j) {
    const int k = cdq ? j : 0;
    TD3_RC(get_rows(q_out + (size_t)j * n * ad, ad, A->q[k], A->hq[k], 32, n, s));
  }
  return 0;
}

// The particle learner's device queries.  The features (and actions) are packed into the MLP input rows
// behind the kEncC2 pooled columns; the particles are NOT copied: the encoder stage reads the caller's
// [n][N*D] rows in place (build_act_particles, dev) and writes zeros for the pad rows n..Bp-1.
int td3_select_action_particles_device(td3_handle* h, const float* feat, const float* part, int n,
                                       const td3_explore* ex, float* action_out, void* stream) {
  TD3_ARG(n > 0, "n must be positive");
  TD3_ARG(h && feat && part && action_out, "null argument");
  TD3_ARG(h->particles, "featured learner: use td3_select_action_device");
  TD3_HIP(hipSetDevice(h->cfg.device));
  const int Bp = pad32(n);
  ActPlan* A;
  TD3_RC(build_act_particles(h, Bp, &A, true));
  hipStream_t s;
  TD3_RC(device_query_stream(h, stream, &s));
  hipLaunchKernelGGL(pack_kernel, dim3(Bp), dim3(64), 0, s, feat, h->sd, n, Bp, A->X_S, h->actor.nets[0].lin[0].Kp,
                     kEncC2, (float*)nullptr, 0, 0, (float*)nullptr, 0, 0);
  TD3_HIP(hipGetLastError());
  A->dev_part = part;
  A->dev_n = n;
  TD3_RC(run_stages(A->act, s));
  // the head is the tanh policy (TD3_particles.py:68); the clip is main.py:252's, to cfg.max_action
  return explore_rows(h, A, n, ex, action_out, s);
}

int td3_eval_q_particles_device(td3_handle* h, const float* feat, const float* part, const float* action, int n,
                                float* q_out, void* stream) {
  TD3_ARG(n > 0, "n must be positive");
  TD3_ARG(h && feat && part && action && q_out, "null argument");
  TD3_ARG(h->particles, "featured learner: use td3_eval_q_device");
  TD3_HIP(hipSetDevice(h->cfg.device));
  const int Bp = pad32(n), F = h->sd, ad = h->ad;
  const int ldq = h->critic.nets[0].lin[0].Kp;
  const bool cdq = h->cdq != 0;
  ActPlan* A;
  TD3_RC(build_act_particles(h, Bp, &A, true));
  hipStream_t s;
  TD3_RC(device_query_stream(h, stream, &s));
  float* X2 = cdq ? A->XQ2 : nullptr;                       // Q2's own input rows (its own encoder)
  hipLaunchKernelGGL(pack_kernel, dim3(Bp), dim3(64), 0, s, feat, F, n, Bp, A->X_SA, ldq, kEncC2, X2, ldq, kEncC2,
                     (float*)nullptr, 0, 0);
  hipLaunchKernelGGL(pack_kernel, dim3(Bp), dim3(64), 0, s, action, ad, n, Bp, A->X_SA, ldq, kEncC2 + F, X2, ldq,
                     kEncC2 + F, (float*)nullptr, 0, 0);
  TD3_HIP(hipGetLastError());
  A->dev_part = part;
  A->dev_n = n;
  TD3_RC(run_stages(A->evalq, s));
  for (int j = 0; j < 2; ++j) {      // the live rows of the stride-32 head outputs -> q_out[j][n][ad]
    ExploreArgs e{};                 // explore_kernel's plain form: a strided row copy
    e.pi = A->q[cdq ? j : 0];
    e.ldp = 32;
    e.action_out = q_out + (size_t)j * n * ad;
    e.n = n;
    e.ad = ad;
    e.plain = 1;
    TD3_RC(launch_explore(e, s));
  }
  return 0;
}

int td3_comm_unique_id(unsigned char out[128]) {
  TD3_ARG(out != nullptr, "null argument");
  ncclUniqueId id;
  ncclResult_t r = ncclGetUniqueId(&id);
  if (r != ncclSuccess) {
    set_error("ncclGetUniqueId: %s", ncclGetErrorString(r));
    return -2;
  }
  static_assert(sizeof(id) == 128, "ncclUniqueId size");
  memcpy(out, &id, 128);
  return 0;
}

int td3_comm_init(td3_handle* h, const unsigned char id[128], int nranks, int rank) {
  TD3_ARG(h && id, "null argument");
  TD3_ARG(nranks >= 1 && rank >= 0 && rank < nranks, "bad rank / nranks");
  TD3_HIP(hipSetDevice(h->cfg.device));
  ncclUniqueId uid;
  memcpy(&uid, id, 128);
  ncclComm_t c;
  ncclResult_t r = ncclCommInitRank(&c, nranks, uid, rank);
  if (r != ncclSuccess) {
    set_error("ncclCommInitRank: %s", ncclGetErrorString(r));
    return -2;
  }
  if (h->comm) ncclCommDestroy(h->comm);
  h->comm = c;
  h->nranks = nranks;
  h->rank = rank;
  if (!h->comm_stream) {
    TD3_HIP(hipStreamCreateWithFlags(&h->comm_stream, hipStreamNonBlocking));
    TD3_HIP(hipEventCreateWithFlags(&h->comm_ev, hipEventDisableTiming));
    TD3_HIP(hipEventCreateWithFlags(&h->comm_ev1, hipEventDisableTiming));
    TD3_HIP(hipEventCreateWithFlags(&h->comm_done, hipEventDisableTiming));
  }
  if (h->plan) {           // stage lists change (grad write + all-reduce + flat Adam)
    int B = h->plan->B;
    TD3_RC(build_plan(h, B));
  }
  return 0;
}

int td3_comm_init_local(td3_handle** hs, int n) {
  TD3_ARG(hs != nullptr, "null argument");
  TD3_ARG(n >= 1 && n <= kMaxLocalReplicas, "1 .. 8 local replicas");
  for (int k = 0; k < n; ++k) {
    TD3_ARG(hs[k] != nullptr, "null handle");
    TD3_ARG(!hs[k]->comm && !hs[k]->local, "handle already in a data-parallel group");
    TD3_ARG(hs[k]->cfg.device == hs[0]->cfg.device, "local replicas share one device");
    TD3_ARG(hs[k]->particles == hs[0]->particles && hs[k]->actor.size == hs[0]->actor.size &&
                hs[k]->critic.size == hs[0]->critic.size && hs[k]->cfg.norm == hs[0]->cfg.norm,
            "local replicas must have the same configuration");
    for (int j = 0; j < k; ++j) TD3_ARG(hs[j] != hs[k], "a handle appears twice");
  }
  auto g = std::make_shared<LocalGroup>();
  g->hs.assign(hs, hs + n);
  for (int k = 0; k < n; ++k) {
    td3_handle* h = hs[k];
    TD3_HIP(hipSetDevice(h->cfg.device));
    TD3_HIP(hipStreamSynchronize(h->stream));
    h->local = g;
    h->nranks = n;
    h->rank = k;
    if (h->plan) TD3_RC(build_plan(h, h->plan->B));   // grad-only dW + all-reduce + flat Adam
  }
  return 0;
}

int td3_train_step_local(td3_handle** hs, rb_handle** rbs, int n, int batch, const int64_t* inject_idx,
                         const float* inject_noise, td3_step_stats* stats) {
  TD3_ARG(hs && rbs && n >= 1 && hs[0], "null argument");
  TD3_ARG(batch > 0, "batch must be positive");
  std::shared_ptr<LocalGroup> g = hs[0]->local;
  TD3_ARG(g && (int)g->hs.size() == n, "handles are not one td3_comm_init_local group");
  for (int k = 0; k < n; ++k) {
    TD3_ARG(hs[k] == g->hs[k], "handles must be passed in the group's rank order");
    TD3_ARG(rbs[k] != nullptr, "null replay buffer");
    TD3_ARG(hs[k]->total_it == hs[0]->total_it, "replicas out of step");
  }
  td3_handle* h0 = hs[0];
  TD3_HIP(hipSetDevice(h0->cfg.device));
  hipStream_t s = h0->stream;            // every replica's stages in one stream order
  for (int k = 0; k < n; ++k) {
    td3_handle* h = hs[k];
    Ring* r = reinterpret_cast<Ring*>(rbs[k]);
    TD3_ARG(r->sd == h->sd && r->ad == h->ad && r->particles == h->particles, "replay buffer does not match");
    TD3_ARG(!r->particles || (r->N == h->N && r->D == h->D), "particle replay buffer shape does not match");
    TD3_ARG(r->size > 0 || inject_idx, "train on an empty replay buffer");
    TD3_ARG(r->device == h->cfg.device, "replay buffer lives on another device");
    if (h->stream != s) TD3_HIP(hipStreamSynchronize(h->stream));
    TD3_RC(ensure_plan(h, batch));
    TD3_RC(ensure_w4(h, s));
    TD3_RC(ensure_unit_weights(h, s));
    TD3_RC(bind_ring(h, r));
    TD3_RC(ring_begin_read(r, s));
  }
  const int actor_phase = ((h0->total_it + 1) % h0->cfg.policy_freq) == 0;
  const int inj = inject_noise ? 1 : 0;
  std::vector<std::vector<Stage>*> lists(n);
  std::vector<size_t> pos(n, 0);
  for (int k = 0; k < n; ++k) {
    td3_handle* h = hs[k];
    Plan* P = h->plan.get();
    Ring* r = reinterpret_cast<Ring*>(rbs[k]);
    if (inject_idx) {
      for (int i = 0; i < batch; ++i)
        TD3_ARG(inject_idx[(size_t)k * batch + i] >= 0 && inject_idx[(size_t)k * batch + i] < r->cap,
                "injected index out of range");
      TD3_HIP(hipMemcpyAsync(P->d_inject_idx, inject_idx + (size_t)k * batch, (size_t)batch * 8,
                             hipMemcpyHostToDevice, s));
    }
    if (inject_noise)
      TD3_HIP(hipMemcpyAsync(P->noise, inject_noise + (size_t)k * batch * h->ad, (size_t)batch * h->ad * 4,
                             hipMemcpyHostToDevice, s));
    const bool fused = !inject_idx && P->fuse_gather;
    if (!fused) TD3_RC(input_from_ring(h, r, P, inject_idx != nullptr, s));
    lists[k] = fused ? &P->body_ring[actor_phase][inj] : &P->body[actor_phase][inj];
    h->last_body = lists[k];
  }
  for (;;) {
    int coll = -2;
    for (int k = 0; k < n; ++k) {
      std::vector<Stage>& st = *lists[k];
      while (pos[k] < st.size() && st[pos[k]].collective < 0) TD3_RC(st[pos[k]++].run(s));
      const int c = pos[k] < st.size() ? st[pos[k]].collective : -1;
      TD3_ARG(k == 0 || c == coll, "internal: replicas reached different collectives");
      coll = c;
    }
    if (coll < 0) break;
    LocalSumArgs a{};
    a.n = n;
    std::vector<const Stage*> cst(n);
    for (int k = 0; k < n; ++k) {
      Group& grp = coll == 0 ? hs[k]->actor : hs[k]->critic;
      cst[k] = &(*lists[k])[pos[k]];
      a.a[k] = grp.G + cst[k]->coll_off;
      a.size = cst[k]->coll_n < 0 ? grp.size : cst[k]->coll_n;
      TD3_ARG(cst[k]->coll_off == cst[0]->coll_off && cst[k]->coll_n == cst[0]->coll_n,
              "internal: replicas reached different all-reduce buckets");
      ++pos[k];
    }
    TD3_RC(launch_local_sum(a, s));
    for (int k = 0; k < n; ++k)               // the bucket's optimizer step behind its sum
      if (cst[k]->after) TD3_RC(cst[k]->after(s));
    const int64_t sl = cst[0]->coll_slice;
    if (sl > 0) {                             // sharded step: replica k owns slice k (its all-gather)
      for (int k = 0; k < n; ++k) {
        const Group& own = coll == 0 ? hs[k]->actor : hs[k]->critic;
        for (int j = 0; j < n; ++j) {
          if (j == k) continue;
          const Group& dst = coll == 0 ? hs[j]->actor : hs[j]->critic;
          TD3_HIP(hipMemcpyAsync(dst.P + k * sl, own.P + k * sl, (size_t)sl * 4, hipMemcpyDeviceToDevice, s));
        }
      }
    }
  }
  for (int k = 0; k < n; ++k) TD3_RC(ring_end_read(reinterpret_cast<Ring*>(rbs[k]), s));
  if (inject_idx || inject_noise) TD3_HIP(hipStreamSynchronize(s));
  for (int k = 0; k < n; ++k) TD3_RC(finish_step(hs[k], actor_phase, s, stats ? &stats[k] : nullptr));
  return 0;
}

// The host waits by polling an event recorded behind the queued steps: a blocking stream sync sleeps
// on an interrupt once the wait grows long, and its wake-up added tens of us to the end of every
// burst of steps (e.g. the 20-step timed runs of the driver's bench command).  One event record (a
// marker packet) per call; the poll itself queues nothing.
// The learner stream's work done: hipStreamSynchronize.  Measured against spinning on an event
// recorded on the stream (round 4, tools/short_probe.py, 20-step C2 runs): host time past the
// GPU's own span 24-30 us per run against 35-38 us, and a following torch.cuda.synchronize()
// 5-6 us against 21 us (the stream sync also lets the runtime retire the stream's launch records).
int td3_sync(td3_handle* h) {
  TD3_ARG(h != nullptr, "null handle");
  TD3_HIP(hipSetDevice(h->cfg.device));
  TD3_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

void* td3_stream(td3_handle* h) { return h ? (void*)h->stream : nullptr; }

int td3_profile_stages(td3_handle* h, rb_handle* rbh, int batch, int actor_phase, float* ms, int max_stages,
                       int* n_stages) {
  TD3_ARG(h && rbh && ms && n_stages, "null argument");
  Ring* r = reinterpret_cast<Ring*>(rbh);
  TD3_HIP(hipSetDevice(h->cfg.device));
  TD3_RC(ensure_plan(h, batch));
  Plan* P = h->plan.get();
  TD3_RC(bind_ring(h, r));
  const bool fused = P->fuse_gather;             // stage 0 (the gather) runs inside F_fwd0
  std::vector<Stage>& st = fused ? P->body_ring[actor_phase ? 1 : 0][0] : P->body[actor_phase ? 1 : 0][0];
  const int n = (int)st.size() + 1;
  TD3_ARG(max_stages >= n, "max_stages too small");
  std::vector<hipEvent_t> ev(n + 1);
  for (auto& e : ev) TD3_HIP(hipEventCreate(&e));
  hipStream_t s = h->stream;
  TD3_RC(ensure_w4(h, s));
  TD3_RC(ensure_unit_weights(h, s));
  TD3_RC(ring_begin_read(r, s));
  TD3_HIP(hipEventRecord(ev[0], s));
  if (!fused) TD3_RC(input_from_ring(h, r, P, false, s));
  TD3_HIP(hipEventRecord(ev[1], s));
  for (int i = 0; i < (int)st.size(); ++i) {
    TD3_RC(st[i].run(s));
    TD3_HIP(hipEventRecord(ev[i + 2], s));
  }
  TD3_RC(ring_end_read(r, s));
  TD3_HIP(hipStreamSynchronize(s));
  h->stage_names.clear();
  h->stage_kernels.clear();
  h->stage_names.push_back("gather");
  h->stage_kernels.push_back(fused ? "(fused into F_fwd0)" : "td3::gather_kernel");
  for (int i = 0; i < n; ++i) {
    TD3_HIP(hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]));
    if (i) {
      h->stage_names.push_back(st[i - 1].name);
      h->stage_kernels.push_back(st[i - 1].kernel);
    }
  }
  for (auto& e : ev) (void)hipEventDestroy(e);
  *n_stages = n;
  h->last_body = &st;
  h->last_ring = r;
  h->last_ring_gen = r->gen;
  // the profiled step is a real step: keep the host mirror in sync
  h->total_it += 1;
  h->critic_step += 1;
  if (actor_phase) h->actor_step += 1;   // (stream synchronised above: no actor event needed)
  return 0;
}

const char* td3_stage_name(td3_handle* h, int i) {
  if (!h || i < 0 || i >= (int)h->stage_names.size()) return "";
  return h->stage_names[i].c_str();
}

const char* td3_stage_kernel(td3_handle* h, int i) {
  if (!h || i < 0 || i >= (int)h->stage_kernels.size()) return "";
  return h->stage_kernels[i].c_str();
}

double td3_stage_flops(td3_handle* h, int i) {
  if (!h || !h->last_body || i <= 0 || i > (int)h->last_body->size()) return 0.0;
  return (*h->last_body)[i - 1].flops;
}

double td3_stage_bytes(td3_handle* h, int i) {
  if (!h || !h->last_body || i <= 0 || i > (int)h->last_body->size()) return 0.0;
  return (*h->last_body)[i - 1].bytes;
}

int td3_probe_kernel(td3_handle* h, rb_handle* rb, int batch, const char* kernel, int steps, float* ms_total,
                     int* launches) {
  TD3_ARG(h && rb && kernel && ms_total && launches, "null argument");
  TD3_ARG(steps > 0, "steps must be positive");
  TD3_ARG(!h->local, "a td3_comm_init_local replica steps through td3_train_step_local only");
  TD3_HIP(hipSetDevice(h->cfg.device));
  h->probing = true;
  h->probe_kernel = kernel;
  h->probe_used = 0;
  int rc = 0;
  for (int i = 0; i < steps && rc == 0; ++i) rc = td3_train_step(h, rb, batch, nullptr, nullptr, nullptr, nullptr);
  h->probing = false;
  if (rc == 0) rc = td3_sync(h);
  float total = 0.f;
  for (int k = 0; rc == 0 && k + 1 < h->probe_used; k += 2) {
    float ms = 0.f;
    const hipError_t e = hipEventElapsedTime(&ms, h->probe_ev[k], h->probe_ev[k + 1]);
    if (e != hipSuccess) {
      set_error("td3_probe_kernel: hipEventElapsedTime: %s", hipGetErrorString(e));
      rc = -2;
    }
    total += ms;
  }
  for (hipEvent_t e : h->probe_ev) (void)hipEventDestroy(e);
  h->probe_ev.clear();
  *ms_total = total;
  *launches = h->probe_used / 2;
  h->probe_used = 0;
  return rc;
}

int td3_debug_plan_flags(const td3_handle* h, int* flags) {
  TD3_ARG(h && flags, "null argument");
  *flags = h->plan ? ((h->plan->w4 ? 1 : 0) | (h->dp_sharded ? 2 : 0)) : 0;
  return 0;
}

int td3_debug_act_fail(td3_handle* h, int n) {
  TD3_ARG(h && n >= 0, "bad argument");
  TD3_ARG(!h->act.empty(), "no query plan yet (run select_action / eval_q first)");
  for (auto& kv : h->act) kv.second->fail_test = n;
  return 0;
}

int td3_debug_activation(td3_handle* h, int eval, int layer, float* out, int rows, int cols) {
  TD3_ARG(h && out, "null argument");
  TD3_ARG(h->plan && !h->particles, "no featured plan (run a train step first)");
  TD3_ARG(eval >= 0 && eval <= 6 && layer >= 0 && layer <= 2, "eval 0..6, layer 0..2");
  Plan* P = h->plan.get();
  const EvalB* ev[7] = {&P->TA, &P->Q[0], &P->Q[1], &P->A, &P->TQ[0], &P->TQ[1], &P->AQ};
  const NetL& n = (eval == 0 || eval == 3) ? h->actor.nets[0] : h->critic.nets[(eval == 2 || eval == 5) ? 1 : 0];
  const LinearL& L = n.lin[layer];
  TD3_ARG(rows > 0 && rows <= P->Bp && cols > 0 && cols <= L.N, "rows / cols out of range");
  TD3_ARG(ev[eval]->H[layer] != nullptr, "that activation is not kept by the plan");
  TD3_HIP(hipSetDevice(h->cfg.device));
  TD3_HIP(hipStreamSynchronize(h->stream));
  TD3_HIP(hipMemcpy2D(out, (size_t)cols * 4, ev[eval]->H[layer], (size_t)L.Np * 4, (size_t)cols * 4, rows,
                      hipMemcpyDeviceToHost));
  return 0;
}

int td3_time_stage(td3_handle* h, int stage, int iters, float* ms_mean) {
  TD3_ARG(h && ms_mean, "null argument");
  TD3_ARG(h->last_body != nullptr, "run td3_profile_stages first");
  TD3_ARG(stage >= 0 && stage <= (int)h->last_body->size(), "stage index out of range");
  TD3_ARG(iters > 0, "iters must be positive");
  TD3_ARG(stage > 0 || ring_alive(h->last_ring, h->last_ring_gen),
          "stage 0 (the gather) needs the ring of td3_profile_stages, which was destroyed or replaced");
  TD3_HIP(hipSetDevice(h->cfg.device));
  // stage 0: the stand-alone gather (Philox draw + record reads + batch writes, gather_kernel) of
  // the profiled ring -- a separate launch when the step samples it (Plan::fuse_gather false), the
  // sample phase measured on its own otherwise
  Ring* ring = h->last_ring;
  Plan* plan = h->plan.get();
  Stage gather{"gather", [=](hipStream_t s) { return input_from_ring(h, ring, plan, false, s); }, 0,
               "td3::gather_kernel"};
  Stage& st = stage ? (*h->last_body)[stage - 1] : gather;
  hipEvent_t a, b;
  TD3_HIP(hipEventCreate(&a));
  TD3_HIP(hipEventCreate(&b));
  hipStream_t s = h->stream;
  TD3_RC(st.run(s));    // warm
  // the `iters` launches are replayed from a hipGraph, as in the step: launched one by one from
  // the host, a short stage measured the host's submit rate rather than the device time
  hipGraph_t g = nullptr;
  hipGraphExec_t ge = nullptr;
  TD3_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
  int rc = 0;
  for (int i = 0; i < iters && rc == 0; ++i) rc = st.run(s);
  const hipError_t ce = hipStreamEndCapture(s, &g);
  if (rc != 0) {
    if (g) (void)hipGraphDestroy(g);
    return rc;
  }
  TD3_HIP(ce);
  TD3_HIP(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
  TD3_HIP(hipGraphLaunch(ge, s));     // warm (graph upload)
  TD3_HIP(hipEventRecord(a, s));
  TD3_HIP(hipGraphLaunch(ge, s));
  TD3_HIP(hipEventRecord(b, s));
  TD3_HIP(hipEventSynchronize(b));
  float ms = 0;
  TD3_HIP(hipEventElapsedTime(&ms, a, b));
  *ms_mean = ms / iters;
  (void)hipGraphExecDestroy(ge);
  (void)hipGraphDestroy(g);
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  return 0;
}

}  // extern "C"
