// The data-parallel seam: the schedule choices read at plan build, the sharded optimizer state,
// the RCCL communicator and the in-process replica group (td3_comm_*, td3_train_step_local).
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
bool dp_shard(const td3_handle* h) {
  const int m = env_int("TD3_DP_SHARD", 0);
  return m == 2 || (m == 1 && h->nranks > 1);
}
int64_t shard_slice(const Group& g, int nranks) { return ((g.size + 4 * nranks - 1) / (4 * nranks)) * 4; }

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
  TD3_ARG(!h->log, "the training log is enabled on this handle (data-parallel logging is not supported)");
  TD3_ARG(h->bc_alpha == 0.0, "TD3+BC is on for this handle (td3_set_bc): data-parallel BC is not supported");
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
    TD3_ARG(!hs[k]->log, "the training log is enabled on a handle (data-parallel logging is not supported)");
    TD3_ARG(hs[k]->bc_alpha == 0.0, "TD3+BC is on for a handle (td3_set_bc): data-parallel BC is not supported");
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
