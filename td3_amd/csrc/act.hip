// The query plans (select_action / eval_q), their host-side I/O and the eight query entry points.
//
// Reference mapping (/root/reference):
//   TD3_featured.TD3.select_action :113-115 -> td3_select_action
//   TD3_featured.TD3.eval_q     :117-121  -> td3_eval_q
//   main.py:249-252 (select_action + OU noise + clip) on device rows -> td3_select_action_device;
//   eval_q on device rows -> td3_eval_q_device (asynchronous, nothing crosses the host)
//   TD3_particles.TD3.select_action / eval_q (TD3_particles.py:153-164) on device rows ->
//   td3_select_action_particles_device / td3_eval_q_particles_device (particles read in place)
#include "learner.h"

namespace td3 {

int map_io(ActPlan* A, size_t floats, IoCarve* io) {
  TD3_HIP(hipHostMalloc(&A->hio, floats * 4, hipHostMallocMapped));
  memset(A->hio, 0, floats * 4);
  void* d = nullptr;
  TD3_HIP(hipHostGetDevicePointer(&d, A->hio, 0));
  io->h = A->hio;
  io->d = static_cast<float*>(d);
  return 0;
}

// ------------------------------------------------------------------ act / eval_q plans
// The LN3 + head problem of network n (arena Pp) evaluated into e (mode: kHeadPolicy / kHeadQ)
static HeadProb head_prob(bool norm, const NetL& n, const float* Pp, const EvalB& e, int mode) {
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
}

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
  A->dev = dev;
  const bool norm = h->cfg.norm == 1;
  const NetL& an = h->actor.nets[0];
  const NetL& q1 = h->critic.nets[0];
  const NetL& q2 = h->critic.nets[1];
  const int lds_s = pad32(h->sd), lds_sa = pad32(h->sd + h->ad);
  const bool mapped = !dev && Bp <= kMappedRows;
  A->gemv = true;
  for (int l = 0; l < 3; ++l)
    for (const NetL* n : {&an, &q1, &q2}) A->gemv = A->gemv && n->lin[l].K <= 512;
  A->gemv01 = A->gemv && an.lin[0].K <= kGemv0K && q1.lin[0].K <= kGemv0K;
  // one-launch queries: layer 2 rides on the layer-1 column groups (N2 <= N1, same N1 for the twins)
  auto rides = [](std::initializer_list<const NetL*> nets) {
    bool ok = true;
    for (const NetL* n : nets)
      ok = ok && n->lin[2].N <= n->lin[1].N && n->lin[1].N == nets.begin()[0]->lin[1].N && n->lin[3].N <= 64;
    return ok;
  };
  const bool one_launch = A->gemv01 && env_int("TD3_ACT1", 1) != 0;
  A->act1 = one_launch && mapped && rides({&an}) && rides({&q1, &q2});
  int* ctr = nullptr;
  unsigned* flag[2] = {nullptr, nullptr};
  auto carve = [&](Scratch& S, IoCarve& io) {
    A->X_S = io.take((size_t)Bp * lds_s, &A->hX_S);
    A->X_SA = io.take((size_t)Bp * lds_sa, &A->hX_SA);
    A->out = io.take((size_t)Bp * h->ad, &A->hout);
    A->ldo = h->ad;
    for (int j = 0; j < 2; ++j) A->q[j] = io.take(Bp, &A->hq[j]);
    alloc_eval(S, an, Bp, A->X_S, lds_s, false, norm, true, A->A);
    alloc_eval(S, q1, Bp, A->X_SA, lds_sa, false, norm, true, A->Q[0]);
    alloc_eval(S, q2, Bp, A->X_SA, lds_sa, false, norm, true, A->Q[1]);
    if (one_launch) ctr = reinterpret_cast<int*>(S.take(64));      // zeroed with the scratch
    for (int k = 0; k < 2 && A->act1; ++k) {       // completion flags in the mapped block
      float* hf = nullptr;
      flag[k] = reinterpret_cast<unsigned*>(io.take(64, &hf));
      A->hflag[k] = reinterpret_cast<unsigned*>(hf);
    }
  };
  TD3_RC(carve_scratch(carve, mapped ? A.get() : nullptr, &A->scratch, nullptr));
  const StageCtx cx{h, A->tables, Bp, Bp};
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
  for (int l = 0; l < 3; ++l) {
    A->gv_act[l].p[0] = gemv_layer(an, h->actor.P, A->A, l);
    A->gv_q[l].p[0] = gemv_layer(q1, h->critic.P, A->Q[0], l);
    A->gv_q[l].p[1] = gemv_layer(q2, h->critic.P, A->Q[1], l);
  }
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
  {
    std::vector<FwdItem> f = {{&an, h->actor.P, &A->A, false, false}};
    TD3_RC(add_fwd_stages(cx, A->act, f, "act", FwdOpts{}));
    HeadProb p = head_prob(norm, an, h->actor.P, A->A, kHeadPolicy);
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
    A->act.push_back({"act_head", [=](hipStream_t s) { return launch_heads(a, 1, s); }, 0, "td3::head_kernel"});
  }
  {
    std::vector<FwdItem> f = {{&q1, h->critic.P, &A->Q[0], false, false},
                              {&q2, h->critic.P, &A->Q[1], false, false}};
    TD3_RC(add_fwd_stages(cx, A->evalq, f, "evq", FwdOpts{}));
    std::vector<HeadProb> hp;
    for (int j = 0; j < 2; ++j) {
      HeadProb p = head_prob(norm, j ? q2 : q1, h->critic.P, A->Q[j], kHeadQ);
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
    A->evalq.push_back({"evq_head", [=](hipStream_t s) { return launch_heads(a, 2, s); }, 0, "td3::head_kernel"});
  }
  if (A->act1) {
    auto mk = [&](ActArgs& a, const Gemv01Args& g, const GemvArgs& l2, std::initializer_list<const NetL*> nets,
                  const float* Pp, EvalB* const* ev, float* const* outs, int ldo, int mode, int* c, unsigned* f) {
      a = ActArgs{};
      a.g = g;
      a.ctr = c;
      a.flag = f;
      a.max_action = h->cfg.max_action;
      int k = 0;
      for (const NetL* n : nets) {
        a.l2[k] = l2.p[k];
        HeadProb q = head_prob(norm, *n, Pp, *ev[k], mode);
        q.out = outs[k];
        q.ldo = ldo;
        q.out_col = 0;
        a.head[k] = q;
        ++k;
      }
    };
    EvalB* ea[1] = {&A->A};
    float* oa[1] = {A->out};
    EvalB* eq[2] = {&A->Q[0], &A->Q[1]};
    float* oq[2] = {A->q[0], A->q[1]};
    mk(A->a1_act, A->g01_act, A->gv_act[2], {&an}, h->actor.P, ea, oa, A->ldo, kHeadPolicy, ctr, flag[0]);
    mk(A->a1_q, A->g01_q, A->gv_q[2], {&q1, &q2}, h->critic.P, eq, oq, 1, kHeadQ, ctr + 8, flag[1]);
  }
  *out = A.get();
  plans[Bp] = std::move(A);
  return 0;
}

// The one place that decides how a featured query of n rows runs on plan A (q: eval_q, else
// select_action).  Up to kGemvRows rows of a host query skip the 32-row stage list: one act_kernel launch
// (ActPlan::act1), else the launch chain, whose first two layers are one gemv01 launch when both
// networks' layer 0 is narrow (ActPlan::gemv01).  act_kernel and gemv01_kernel take the rows in their
// arguments; everything else reads them from the plan's inputs, mapped host memory or device scratch.
QueryRoute query_route(ActPlan* A, int n, bool q) {
  QueryRoute r{kQueryStages, A->hio ? kRowsMapped : kRowsDevice, q ? &A->evalq : &A->act};
  if (A->dev || !A->gemv || n > kGemvRows) return r;
  r.kind = A->act1 ? kQueryAct1 : A->gemv01 ? kQueryGemv01 : kQueryGemv;
  if (r.kind != kQueryGemv) r.rows = kRowsArgs;
  return r;
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
  A->dev = dev;
  const bool norm = h->cfg.norm == 1;
  const bool cdq = h->cdq != 0;
  const int N = h->N, D = h->D, ad = h->ad;
  const NetL& an = h->actor.nets[0];
  const NetL& q1 = h->critic.nets[0];
  const NetL& q2 = h->critic.nets[cdq ? 1 : 0];
  const int lda = an.lin[0].Kp, ldq = q1.lin[0].Kp;
  auto carve = [&](Scratch& S, IoCarve& io) {
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
  };
  TD3_RC(carve_scratch(carve, !dev && Bp <= kMappedRows ? A.get() : nullptr, &A->scratch, nullptr));
  const StageCtx cx{h, A->tables, Bp, Bp};
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
  const float* Pa = h->actor.P;
  const float* Pq = h->critic.P;
  {
    enc_stage(A->act, {EncFwdProb{Pa + an.enc_off, 0, A->X_S, lda, nullptr}}, "act_enc");
    std::vector<FwdItem> f = {{&an, Pa, &A->A, false, false}};
    TD3_RC(add_fwd_stages(cx, A->act, f, "act", FwdOpts{}));
    HeadProb p = head_prob(norm, an, Pa, A->A, kHeadPolicy);
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
    TD3_RC(add_fwd_stages(cx, A->evalq, f, "evq", FwdOpts{}));
    std::vector<HeadProb> hp;
    for (int j = 0; j < (cdq ? 2 : 1); ++j) {
      HeadProb p = head_prob(norm, j ? q2 : q1, Pq, A->Q[j], kHeadQ);
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

}  // namespace td3

using namespace td3;

extern "C" {

// Host-side query I/O of an ActPlan: rows into the plan's inputs / outputs out to the caller.
// Mapped plans (Bp <= kMappedRows) are written and read in place by the host; the stream is idle
// when they are touched (every query ends in a sync, and one starts with it in case an earlier
// query failed before its own).
static int put_rows(const ActPlan* A, float* dev, float* host, int ld, int col, const float* src, int n, int cols,
                    hipStream_t s) {
  if (!host) {
    TD3_HIP(hipMemcpy2DAsync(dev + col, (size_t)ld * 4, src, (size_t)cols * 4, (size_t)cols * 4, n,
                             hipMemcpyHostToDevice, s));
    return 0;
  }
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

// A featured query of n <= kGemvRows rows on the route query_route chose (kind: not kQueryStages): one
// act_kernel launch; or layers 0 and 1 in one gemv01 launch when layer 0 is narrow (the query rows
// [x0 | x1] in its arguments), else one gemv launch per layer, then the head over 4 rows.
static int run_gemv(const ActPlan* A, QueryKind kind, bool q, int n, const float* x0, int c0, const float* x1,
                    int c1, hipStream_t s) {
  const GemvArgs(&gv)[3] = q ? A->gv_q : A->gv_act;
  const int nprob = q ? 2 : 1;
  if (kind == kQueryAct1) {                             // the whole query in one launch
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
  if (kind == kQueryGemv01) {
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
  const QueryRoute r = query_route(A, n, false);
  if (r.kind == kQueryAct1) {
    // the query travels in the kernel arguments and the outputs of the previous query were read
    // before it returned: no stream synchronize on either side (wait_flags)
    TD3_RC(run_gemv(A, r.kind, false, n, state, h->sd, nullptr, 0, s));
    return query_done(h, s, get_rows(action_out, h->ad, A->out, A->hout, A->ldo, n, s));
  }
  if (A->hio) TD3_HIP(hipStreamSynchronize(s));
  if (r.rows != kRowsArgs) TD3_RC(put_rows(A, A->X_S, A->hX_S, pad32(h->sd), 0, state, n, h->sd, s));
  if (r.kind == kQueryStages) TD3_RC(run_stages(*r.stages, s));
  else TD3_RC(run_gemv(A, r.kind, false, n, state, h->sd, nullptr, 0, s));
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
  const QueryRoute r = query_route(A, n, true);
  if (r.kind == kQueryAct1) {    // one launch, completion flags polled on the host (no stream syncs)
    TD3_RC(run_gemv(A, r.kind, true, n, state, h->sd, action, h->ad, s));
    TD3_RC(get_rows(q_out, 1, A->q[0], A->hq[0], 1, n, s));
    return get_rows(q_out + n, 1, A->q[1], A->hq[1], 1, n, s);
  }
  if (A->hio) TD3_HIP(hipStreamSynchronize(s));
  if (r.rows != kRowsArgs) {
    TD3_RC(put_rows(A, A->X_SA, A->hX_SA, ld, 0, state, n, h->sd, s));
    TD3_RC(put_rows(A, A->X_SA, A->hX_SA, ld, h->sd, action, n, h->ad, s));
  }
  if (r.kind == kQueryStages) TD3_RC(run_stages(*r.stages, s));
  else TD3_RC(run_gemv(A, r.kind, true, n, state, h->sd, action, h->ad, s));
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
  TD3_RC(launch_pack(state, h->sd, n, Bp, {{A->X_S, pad32(h->sd), 0}}, s));
  TD3_RC(run_stages(*query_route(A, n, false).stages, s));
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
  TD3_RC(launch_pack(state, h->sd, n, Bp, {{A->X_SA, ld, 0}}, s));
  TD3_RC(launch_pack(action, h->ad, n, Bp, {{A->X_SA, ld, h->sd}}, s));
  TD3_RC(run_stages(*query_route(A, n, true).stages, s));
  for (int j = 0; j < 2; ++j)        // the live rows of Q_j -> q_out[j][0..n)
    TD3_RC(launch_pack(A->q[j], 1, n, n, {{q_out + (size_t)j * n, 1, 0}}, s));
  return 0;
}

int td3_debug_query_route(td3_handle* h, int n, int eval_q, int device, char* buf, int len) {
  TD3_ARG(h && buf && len > 0, "null argument");
  TD3_ARG(!h->particles, "featured learners only");
  TD3_ARG(n > 0, "n must be positive");
  TD3_HIP(hipSetDevice(h->cfg.device));
  ActPlan* A;
  TD3_RC(build_act(h, pad32(n), &A, device != 0));
  const bool q = eval_q != 0;
  const QueryRoute r = query_route(A, n, q);
  const int R = gemv_rows(n);
  std::string out = r.rows == kRowsArgs ? "args" : r.rows == kRowsMapped ? "mapped" : "device";
  char name[64];
  if (r.kind == kQueryAct1) {
    snprintf(name, sizeof(name), ",td3::act_kernel<%d, %d>", R, act_kq((q ? A->a1_q : A->a1_act).g.K0));
    out += name;
  } else if (r.kind == kQueryStages) {
    for (const Stage& st : *r.stages) out += "," + st.kernel;
  } else {
    int l = 0;
    if (r.kind == kQueryGemv01) {
      snprintf(name, sizeof(name), ",td3::gemv01_kernel<%d>", R);
      out += name;
      l = 2;
    }
    snprintf(name, sizeof(name), ",td3::gemv_kernel<%d>", R);
    for (; l < 3; ++l) out += name;
    out += ",td3::head_kernel";
  }
  TD3_ARG((int)out.size() < len, "buffer too small");
  memcpy(buf, out.c_str(), out.size() + 1);
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
  TD3_RC(launch_pack(feat, h->sd, n, Bp, {{A->X_S, h->actor.nets[0].lin[0].Kp, kEncC2}}, s));
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
  TD3_RC(launch_pack(feat, F, n, Bp, {{A->X_SA, ldq, kEncC2}, {X2, ldq, kEncC2}}, s));
  TD3_RC(launch_pack(action, ad, n, Bp, {{A->X_SA, ldq, kEncC2 + F}, {X2, ldq, kEncC2 + F}}, s));
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

}  // extern "C"
