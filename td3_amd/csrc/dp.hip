// The data-parallel seam: the schedule choices read at plan build and the three schedules they choose among,
// the sharded optimizer state, the RCCL communicator and the replica group (td3_comm_*, td3_train_step_local).
#include "learner.h"

namespace td3 {

// The overlapped (bucketed) data-parallel dW schedule: TD3_DP_BUCKETS = 0 (default) off; 1 for real
// peers (RCCL, nranks > 1) and the in-process seam; 2 also on a one-rank communicator (bench.py
// --dp-self: the schedule's price without peers).  Off by default: splitting the critic's dW into
// two half-size launches costs ~12 us of GPU time at Humanoid B = 1024, about what
// bucket 0's exchange can hide behind dW_1.  Read when a plan is built.
bool dp_overlap(const td3_handle* h) {
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

// An RCCL call's result as the library's: 0, or -2 with the error text set
static int nccl_rc(ncclResult_t r, const char* call) {
  if (r == ncclSuccess) return 0;
  set_error("%s: %s", call, ncclGetErrorString(r));
  return -2;
}

// The exchange stage of the group `adam` steps: `rccl` makes the RCCL calls.  A td3_comm_init_local
// replica refuses to launch it: the seam runs its fixed-order sum and Stage::after instead.
using Launch = std::function<int(hipStream_t)>;
static Stage collective_stage(const td3_handle* h, const std::string& name, const AdamArgs& adam, Launch rccl) {
  if (h->local)
    rccl = [](hipStream_t) {
      set_error("a td3_comm_init_local replica steps through td3_train_step_local only");
      return -1;
    };
  Stage x{name, rccl, 0, "rccl"};
  x.collective = adam.which == 1 ? 0 : 1;         // AdamArgs::which 1 = actor -> group 0, 0 = critic -> group 1
  return x;
}

// The flat optimizer's image map of a group's forward weights (P4 null when the plan being built does
// not use the images); `base`: the arena offset of the range it updates
int w4_map(const td3_handle* h, const Group& g, int64_t base, W4Map* out) {
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

// The flat optimizer step of [off, off + n) of a group's arena as a launch: the AdamArgs moved to the range
// and, with `images`, the image map based there (the sharded step leaves the images to the stage behind it)
static int flat_adam(const td3_handle* h, const Group& g, AdamArgs a, int64_t off, int64_t n, int polyak,
                     bool images, Launch* out) {
  a.P += off; a.G += off; a.M += off; a.V += off; a.T += off;
  W4Map wm{};
  if (images) TD3_RC(w4_map(h, g, off, &wm));
  *out = [=](hipStream_t s) { return launch_adam_flat(a, n, polyak, s, images ? &wm : nullptr); };
  return 0;
}

// The overlapped schedule for a twin critic whose dW is split-K: one bucket per network
// in arena order.  Stages: dW_0 (gradient only; then an event on the step stream), dW_1 (then a
// second event), bucket 0's all-reduce + Adam (+ Polyak) on the comm stream behind the first event,
// bucket 1's on the comm stream behind the second (one RCCL stream per communicator: ADVICE r04),
// then the join (the step stream waits for bucket 1's Adam).  Bucket 0's exchange runs under dW_1;
// dW_1 is enqueued before the host makes bucket 0's RCCL call.  The in-process seam runs the same
// buckets: a fixed-order sum of the range, then the bucket's optimizer step (Stage::after), on its
// one stream.  dp_buckets: whether a data-parallel group's dW stage takes this schedule.
bool dp_buckets(const td3_handle* h, const Group& g, const std::vector<BwdItem>& items, const DwOpts& o,
                const DwWork& w) {
  return w.split && g.wn.nlin == 0 && o.enc_nwg == 0 && items.size() == 2 && dp_overlap(h);
}
int add_dp_overlapped(const StageCtx& c, std::vector<Stage>& st, Group& g, const std::vector<BwdItem>& items,
                      const char* tag, const DwOpts& o, const DwWork& w) {
  td3_handle* h = c.h;
  const bool local = h->local != nullptr;
  ncclComm_t comm = h->comm;
  hipStream_t cs = h->comm_stream;
  hipEvent_t done = h->comm_done;
  TD3_ARG(local || (cs && h->comm_ev && h->comm_ev1 && done), "internal: data-parallel handle without a comm stream");
  AdamArgs adam = w.a.adam;
  adam.grad_scale = 1.0f / (float)h->nranks;      // the ranks' mean
  auto begin = [](const NetL& n) { return n.enc_off >= 0 ? n.enc_off : n.lin[0].offW; };
  std::vector<Stage> exch;                        // bucket b's exchange stage
  for (size_t b = 0; b < items.size(); ++b) {
    const bool first = b == 0;
    hipEvent_t ev = first ? h->comm_ev : h->comm_ev1;
    TD3_RC(push_dw_stage(c, st, dw_bucket(w, items, b), o.slab, std::string(tag) + "_dw_" + std::to_string(b)));
    if (!local) {
      Launch dw = st.back().run;
      st.back().run = [=](hipStream_t s) {
        TD3_RC(dw(s));
        TD3_HIP(hipEventRecord(ev, s));
        return 0;
      };
    }
    const int64_t off = begin(*items[b].net);
    const int64_t end = b + 1 < items.size() ? begin(*items[b + 1].net) : g.size;
    TD3_ARG(off >= 0 && end > off && end <= g.size, "internal: bucket range");
    const int64_t nb = end - off;
    Launch step;
    TD3_RC(flat_adam(h, g, adam, off, nb, o.polyak ? 1 : 0, true, &step));
    float* Gb = g.G + off;
    Stage x = collective_stage(h, std::string(tag) + "_" + std::to_string(b) + "_allreduce", adam, [=](hipStream_t) {
      TD3_HIP(hipStreamWaitEvent(cs, ev, 0));
      TD3_RC(nccl_rc(ncclAllReduce(Gb, Gb, (size_t)nb, ncclFloat, ncclSum, comm, cs), "ncclAllReduce"));
      TD3_RC(step(cs));
      if (!first) TD3_HIP(hipEventRecord(done, cs));
      return 0;
    });
    x.coll_off = off; x.coll_n = nb;
    x.after = step;
    exch.push_back(x);
  }
  for (auto& x : exch) st.push_back(x);          // dW_0, dW_1, exchange 0, exchange 1
  st.push_back({std::string(tag) + "_join",
                [=](hipStream_t s) {
                  if (local) return 0;            // the seam ran the buckets on its stream
                  TD3_HIP(hipStreamWaitEvent(s, done, 0));
                  return 0;
                },
                0, "(stream join)"});
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

// Sharded optimizer step (ZeRO-1 form): the summed gradient reaches only this
// rank's slice (ncclReduceScatter, in place), Adam runs on that slice alone (the moments of the
// other slices live on their owners), ncclAllGather brings every rank the updated parameters,
// then Polyak runs replicated over the whole arena (the same inputs on every rank: the replicas
// stay bit-identical, each element computed once).  Same bytes on the links as the all-reduce,
// one extra collective launch, 1/N of the Adam pass.
static int add_dp_sharded(td3_handle* h, std::vector<Stage>& st, Group& g, const AdamArgs& adam, bool polyak,
                          const char* tag) {
  const int N = h->nranks, R = h->rank;
  const int64_t slice = shard_slice(g, N);
  TD3_ARG(N * slice <= g.cap, "internal: shard slices past the arena");
  h->dp_sharded = true;
  ncclComm_t comm = h->comm;
  float *G = g.G, *Pp = g.P, *Tp = g.T;
  Launch step;
  TD3_RC(flat_adam(h, g, adam, R * slice, slice, 0, false, &step));
  Stage x = collective_stage(h, std::string(tag) + "_rs_adam_ag", adam, [=](hipStream_t s) {
    TD3_RC(nccl_rc(ncclReduceScatter(G, G + R * slice, (size_t)slice, ncclFloat, ncclSum, comm, s), "ncclReduceScatter"));
    TD3_RC(step(s));
    return nccl_rc(ncclAllGather(Pp + R * slice, Pp, (size_t)slice, ncclFloat, comm, s), "ncclAllGather");
  });
  x.coll_slice = slice; x.after = step;
  st.push_back(x);
  const int64_t n = g.size;
  const float tau = (float)h->cfg.tau;
  if (polyak && h->w4_build) {          // Polyak and both images in one pass over the gathered arena
    W4Map wm;
    TD3_RC(w4_map(h, g, 0, &wm));
    st.push_back({std::string(tag) + "_polyak", [=](hipStream_t s) { return launch_polyak_w4(Tp, Pp, n, tau, wm, s); },
                  0, "td3::polyak_w4_kernel"});
    return 0;
  }
  if (polyak)
    st.push_back({std::string(tag) + "_polyak", [=](hipStream_t s) { return launch_polyak_flat(Tp, Pp, n, tau, s); },
                  0, "td3::polyak_flat_kernel"});
  return push_w4_pack(h, st, g, false, tag);
}

// All-reduce of the group's whole gradient arena, then the replicated optimizer step: the flat Adam
// (+ Polyak, + images), or wn_kernel under weight normalization
static int add_dp_allreduce(td3_handle* h, std::vector<Stage>& st, Group& g, const AdamArgs& adam, bool polyak,
                            const char* tag) {
  ncclComm_t comm = h->comm;
  float* G = g.G;
  const int64_t n = g.size;
  st.push_back(collective_stage(h, std::string(tag) + "_allreduce", adam, [=](hipStream_t s) {
    return nccl_rc(ncclAllReduce(G, G, (size_t)n, ncclFloat, ncclSum, comm, s), "ncclAllReduce");
  }));
  if (g.wn.nlin > 0) return push_wn_stage(st, g, adam, polyak, tag);
  Launch step;
  TD3_RC(flat_adam(h, g, adam, 0, n, polyak ? 1 : 0, true, &step));
  st.push_back({std::string(tag) + "_adam", step, 0, "td3::adam_flat_kernel"});
  return 0;
}

// The optimizer tail of a data-parallel group behind its gradient-only dW stage (`adam`: what the
// fused step would have used).  Weight normalization keeps the all-reduce.
int add_dp_optimizer(td3_handle* h, std::vector<Stage>& st, Group& g, AdamArgs adam, bool polyak, const char* tag) {
  adam.grad_scale = 1.0f / (float)h->nranks;      // the ranks' mean
  if (g.wn.nlin == 0 && dp_shard(h)) return add_dp_sharded(h, st, g, adam, polyak, tag);
  return add_dp_allreduce(h, st, g, adam, polyak, tag);
}

// The in-process seam's gather of one moment arena: the slices the other replicas own, copied in
static int copy_local_moments(td3_handle* h, int which) {
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
  return 0;
}

// RCCL ranks: the all-gather of both groups' moment slices (a collective), drained
static int allgather_moments(td3_handle* h) {
  // a C-API caller may have stepped on its own stream: the moments are final only once it drained
  if (h->last_step_stream && h->last_step_stream != h->stream) TD3_HIP(hipStreamSynchronize(h->last_step_stream));
  for (Group* g : {&h->actor, &h->critic}) {
    const int64_t sl = shard_slice(*g, h->nranks);
    for (float* a : {g->M, g->V})
      TD3_RC(nccl_rc(ncclAllGather(a + h->rank * sl, a, (size_t)sl, ncclFloat, h->comm, h->stream), "ncclAllGather"));
  }
  TD3_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

// The Adam moments of a sharded schedule live on their slice owners: a plan that stops sharding
// (TD3_DP_SHARD changed between builds) first brings every rank the whole M / V arenas, or each
// rank would carry on with stale moments for the slices it did not own.  Every rank
// rebuilds at the same call (same batch, same environment), so the all-gather is collective; the
// in-process seam copies the owners' slices.
int gather_moments_for_rebuild(td3_handle* h) {
  if (h->local) {
    TD3_HIP(hipDeviceSynchronize());          // the replicas stepped on non-blocking streams
    for (int which : {TD3_ACTOR_ADAM_M, TD3_ACTOR_ADAM_V, TD3_CRITIC_ADAM_M, TD3_CRITIC_ADAM_V})
      TD3_RC(copy_local_moments(h, which));
    return 0;
  }
  if (!h->comm || h->nranks <= 1) return 0;
  return allgather_moments(h);
}

// Sharded optimizer state (the Adam moments of slice k live on rank k): the in-process seam copies
// the other replicas' slices in before a moment is read; RCCL ranks gather them with the collective
// td3_dp_gather_optimizer_state, which a read of the moments then requires.
int consolidate_moments(td3_handle* h, int which) {
  if (!h->dp_sharded || h->nranks <= 1) return 0;
  const bool m = which == TD3_ACTOR_ADAM_M || which == TD3_CRITIC_ADAM_M;
  const bool v = which == TD3_ACTOR_ADAM_V || which == TD3_CRITIC_ADAM_V;
  if (!m && !v) return 0;
  if (h->local) return copy_local_moments(h, which);
  TD3_ARG(h->opt_gathered_it == h->total_it,
          "sharded optimizer state: call td3_dp_gather_optimizer_state on every rank before reading the "
          "Adam moments (a collective)");
  return 0;
}

// Whether two learners have the same networks, tensor by tensor: every dimension that sizes one.  The arena
// sizes alone do not say so: widths pad to 32, and (state, action) = (17, 6) and (3, 1) fill the same floats.
static bool same_shape(const td3_config& a, const td3_config& b) {
  if (a.particles != b.particles || a.norm != b.norm || a.state_dim != b.state_dim || a.action_dim != b.action_dim)
    return false;
  if (a.particles && (a.n_particles != b.n_particles || a.particle_dim != b.particle_dim || !a.cdq != !b.cdq))
    return false;
  for (int i = 0; i < 3; ++i)
    if (a.actor_hidden[i] != b.actor_hidden[i] || a.critic_hidden[i] != b.critic_hidden[i]) return false;
  return true;
}

}  // namespace td3

using namespace td3;

extern "C" {

int td3_dp_gather_optimizer_state(td3_handle* h) {
  TD3_ARG(h != nullptr, "null handle");
  TD3_HIP(hipSetDevice(h->cfg.device));
  if (h->dp_sharded && h->comm && h->nranks > 1) TD3_RC(allgather_moments(h));
  h->opt_gathered_it = h->total_it;
  return 0;
}

int td3_comm_unique_id(unsigned char out[128]) {
  TD3_ARG(out != nullptr, "null argument");
  ncclUniqueId id;
  TD3_RC(nccl_rc(ncclGetUniqueId(&id), "ncclGetUniqueId"));
  static_assert(sizeof(id) == 128, "ncclUniqueId size");
  memcpy(out, &id, 128);
  return 0;
}

int td3_comm_init(td3_handle* h, const unsigned char id[128], int nranks, int rank) {
  TD3_ARG(h && id, "null argument");
  TD3_ARG(nranks >= 1 && rank >= 0 && rank < nranks, "bad rank / nranks");
  TD3_ARG(!h->log, "the training log is enabled on this handle (data-parallel logging is not supported)");
  TD3_ARG(h->bc_alpha == 0.0, "TD3+BC is on for this handle (td3_set_bc): data-parallel BC is not supported");
  TD3_ARG(h->clip_max[0] == 0.0 && h->clip_max[1] == 0.0,
          "gradient clipping is on for this handle (td3_set_grad_clip): data-parallel clipping is not supported");
  TD3_HIP(hipSetDevice(h->cfg.device));
  ncclUniqueId uid;
  memcpy(&uid, id, 128);
  ncclComm_t c;
  TD3_RC(nccl_rc(ncclCommInitRank(&c, nranks, uid, rank), "ncclCommInitRank"));
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
    TD3_ARG(!hs[k]->log, "the training log is enabled on a handle (data-parallel logging is not supported)");
    TD3_ARG(hs[k]->bc_alpha == 0.0, "TD3+BC is on for a handle (td3_set_bc): data-parallel BC is not supported");
    TD3_ARG(hs[k]->clip_max[0] == 0.0 && hs[k]->clip_max[1] == 0.0,
            "gradient clipping is on for a handle (td3_set_grad_clip): data-parallel clipping is not supported");
    TD3_ARG(hs[k]->cfg.device == hs[0]->cfg.device, "local replicas share one device");
    TD3_ARG(same_shape(hs[k]->cfg, hs[0]->cfg), "local replicas must have the same configuration");
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
    TD3_RC(check_ring(h, r, kReplicaStep));
    TD3_ARG(r->size > 0 || inject_idx, "train on an empty replay buffer");
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

}  // extern "C"
