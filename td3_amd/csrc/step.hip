// The train step: the featured and the particle step plans, their execution and hipGraph replay,
// and the td3_train_step* / td3_actor_learn_particles entry points.
//
// Reference mapping (/root/reference):
//   TD3_featured.TD3.train      :123-171  -> td3_train_step (the stage list built by build_step)
//
// HBM layout
//   * one scratch arena for the batch: padded inputs, per-network activations
//     H (post-ReLU), U (post-LN), LN row stats, and the backward dU / dZ rows.
#include "learner.h"

namespace td3 {

static void destroy_graphs(Plan* P) {
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b) {
      if (P->graph[a][b]) (void)hipGraphExecDestroy(P->graph[a][b]);
      if (P->graph_g[a][b]) (void)hipGraphExecDestroy(P->graph_g[a][b]);
      P->graph[a][b] = P->graph_g[a][b] = nullptr;
    }
  P->graph_ring_gen = 0;
}

void destroy_plan(Plan* p) {
  if (!p) return;
  destroy_graphs(p);
  free_plan_tables(p->tables);
  if (p->scratch) (void)hipFree(p->scratch);
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
  P->bc = h->bc_alpha > 0.0;                  // TD3+BC (td3_set_bc): the BC form of actor_head_bwd
  P->bcf = P->bc && (h->bc_demo_rows || h->bc_q_filter);   // its filtered form (td3_set_bc_filter)
  const NetL& an = h->actor.nets[0];
  const NetL& q1 = h->critic.nets[0];
  const NetL& q2 = h->critic.nets[1];
  auto carve = [&](Scratch& S, IoCarve&) {
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
    P->W1aT = S.take((size_t)ad * q1.lin[0].Np);
    if (P->bc) {
      P->bc_se = S.take(Bp);
      P->bc_lam = S.take(4);
    }
    if (P->bcf) {
      P->bcf_keep = S.take(Bp);
      P->bcf_nd = (int*)S.take(4);
    }
    alloc_eval(S, an, Bp, P->X_S2A, P->ld_sa, false, norm, false, P->TA);
    alloc_eval(S, q1, Bp, P->X_SA, P->ld_sa, true, norm, true, P->Q[0]);
    alloc_eval(S, q2, Bp, P->X_SA, P->ld_sa, true, norm, true, P->Q[1]);
    alloc_eval(S, an, Bp, P->X_SA, P->ld_sa, true, norm, true, P->A);
    alloc_eval(S, q1, Bp, P->X_S2A, P->ld_sa, false, norm, true, P->TQ[0]);
    alloc_eval(S, q2, Bp, P->X_S2A, P->ld_sa, false, norm, true, P->TQ[1]);
    alloc_eval(S, q1, Bp, P->X_SP, P->ld_sa, true, norm, true, P->AQ);
  };
  TD3_RC(carve_scratch(carve, nullptr, &P->scratch, &P->scratch_bytes));
  {
    const std::vector<float> ones((size_t)Bp, 1.0f);
    TD3_HIP(hipMemcpy(P->per_w, ones.data(), (size_t)Bp * sizeof(float), hipMemcpyHostToDevice));
    if (P->bcf) TD3_HIP(hipMemcpy(P->bcf_nd, &B, sizeof(int), hipMemcpyHostToDevice));   // n_d = B until a step says otherwise
  }
  const StageCtx cx{h, P->tables, Bp, B};

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
      FwdOpts fo;
      fo.bump = h->d_ctr; fo.bump_actor = actor_phase;
      fo.fuse_l0 = fo.r16 = true;
      TD3_RC(add_fwd_stages(cx, st, f1, "F", fo));
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
        FwdOpts fro = fo;
        fro.ring = &P->rside; fro.ro = ro; fro.o_r = 2 * sd + ad;
        TD3_RC(add_fwd_stages(cx, fr, f1r, "F", fro));
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
      BwdOpts cbo;
      cbo.need_dz0 = true; cbo.lnbwd_rows = &rows;
      TD3_RC(add_bwd_stages(cx, st, cb, "CB", cbo));
      std::vector<FwdItem> f2 = {{&q1, Ptq1, &P->TQ[0], false, false}, {&q2, Ptq2, &P->TQ[1], false, false}};
      FwdOpts tfo;
      tfo.fuse_l0 = true;
      TD3_RC(add_fwd_stages(cx, st, f2, "TF", tfo));
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
      DwOpts cdw;
      cdw.polyak = actor_phase != 0; cdw.unit_scale = &usc; cdw.slab = &P->dwslab;
      TD3_RC(add_dw_stage(cx, st, h->critic, cb, "C", cdw));
      if (!actor_phase) continue;
      // ---------------- delayed policy update (TD3_featured.py:156-171)
      std::vector<FwdItem> f3 = {{&q1, Pq1, &P->AQ, false, true}};
      const bool w1at = !can_fuse_l0(f3);        // layer 0 is its own stage: it writes W1aT
      if (w1at) {
        f3[0].tcopy = P->W1aT;
        f3[0].tcol = sd;
        f3[0].tn = ad;
      }
      FwdOpts afo;
      afo.fuse_l0 = afo.r16 = true;
      TD3_RC(add_fwd_stages(cx, st, f3, "AF", afo));
      // the actor loss -mean Q1(s, pi(s)) (:159): Q1's head and its backward are the prologue of
      // AQB_bwd2 (kProHeadBwd; the particle path has the row launch kRowActorLossP instead)
      std::vector<BwdItem> aqb = {{&q1, Pq1, &P->AQ, false}};
      BwdOpts aqbo;
      aqbo.head_bwd_scale = (float)(-1.0) / (float)B;
      TD3_RC(add_bwd_stages(cx, st, aqb, "AQB", aqbo));
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
        if (P->bc) {
          // the stored action: the [s | a] rows every input path leaves in X_SA (the twin's dW input;
          // the ring-fused first layer writes them as the twin problem's row copy)
          namespace bc = actor_head_bwd_bc;
          p.ex[bc::kQv] = P->AQ.Qv;
          p.ex[bc::kAct] = P->X_SA;
          p.ex[bc::kRowSe] = P->bc_se;
          p.ex[bc::kLam] = P->bc_lam;
          p.exi[bc::kLdAct] = P->ld_sa;
          p.exf[bc::kAlpha] = (float)h->bc_alpha;
          p.exf[bc::kBcScale] = (float)(2.0 / ((double)B * ad));
        }
        if (P->bcf) {
          // the row mask: Q1(s, a) as the critic phase's heads stage left it (the critic before this step's
          // update, td3_step_stats.q1) against kQv, Q1(s, pi) of the updated critic; n_d from the plan's word
          namespace bf = actor_head_bwd_bcf;
          p.ex[bf::kQ1sa] = P->Q[0].Qv;
          p.ex[bf::kNDemo] = reinterpret_cast<float*>(P->bcf_nd);
          p.ex[bf::kKeep] = P->bcf_keep;
          p.exi[bf::kQFilter] = h->bc_q_filter;
        }
        std::vector<GemmProb> v = {p};
        const int kind = P->bcf ? kRowActorHeadBwdBcF : P->bc ? kRowActorHeadBwdBc : kRowActorHeadBwd;
        TD3_RC(push_row_stage(st, v, kind, Bp, "actor_head_bwd"));
      }
      std::vector<BwdItem> ab = {{&an, Pa, &P->A, true}};
      BwdOpts abo;
      abo.need_dz0 = true;
      TD3_RC(add_bwd_stages(cx, st, ab, "AB", abo));
      DwOpts adw;
      adw.which = 1; adw.polyak = true; adw.slab = &P->dwslab;
      TD3_RC(add_dw_stage(cx, st, h->actor, ab, "A", adw));
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
  auto carve = [&](Scratch& S, IoCarve&) {
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
    P->per_w = S.take(Bp);
    P->per_td = S.take(Bp);
    P->per_u = S.take(Bp);
    P->per_tdj = S.take(2 * (size_t)Bp);
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
  };
  TD3_RC(carve_scratch(carve, nullptr, &P->scratch, &P->scratch_bytes));
  const StageCtx cx{h, P->tables, Bp, B};
  {
    std::vector<int64_t> iota(Bp);
    for (int i = 0; i < Bp; ++i) iota[i] = i;
    TD3_HIP(hipMemcpy(P->d_iota, iota.data(), Bp * 8, hipMemcpyHostToDevice));
    const std::vector<float> ones((size_t)Bp, 1.0f);
    TD3_HIP(hipMemcpy(P->per_w, ones.data(), (size_t)Bp * sizeof(float), hipMemcpyHostToDevice));
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

  // the backward chains run down to the MLP input (lnorm1's backward, the encoder, dQ1/da)
  BwdOpts bwd_in, bwd_in_dz0;
  bwd_in.need_in = bwd_in_dz0.need_in = bwd_in_dz0.need_dz0 = true;

  // ---------------- delayed policy update (TD3_particles.py:206-224): _actor_learn on (s features, s
  // particles) with the post-step critic; A_dw also runs the actor's Polyak (the critic's is in C_dw)
  auto actor_phase_stages = [&](std::vector<Stage>& st) -> int {
    Plan* Pp = P.get();
    push_enc_fwd(h, Pp, st, {{&q1, Pq, P->XAQ, P->ld_q, 0, nullptr}}, "AF_enc");
    std::vector<FwdItem> f3 = {{&q1, Pq, &P->AQ, false, true}};
    TD3_RC(add_fwd_stages(cx, st, f3, "AF", FwdOpts{}));
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
      TD3_RC(push_row_stage(st, v, kRowActorLossP, Bp, "actor_loss"));
    }
    std::vector<BwdItem> aqb = {{&q1, Pq, &P->AQ, false}};
    TD3_RC(add_bwd_stages(cx, st, aqb, "AQB", bwd_in));
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
      TD3_RC(push_row_stage(st, v, kRowActorHeadBwdP, Bp, "actor_head_bwd"));
    }
    std::vector<BwdItem> ab = {{&an, Pa, &P->A, true}};
    TD3_RC(add_bwd_stages(cx, st, ab, "AB", bwd_in_dz0));
    push_enc_bwd(h, Pp, st, ab, {P->XA}, "AB_enc");
    DwOpts adw;
    adw.which = 1; adw.polyak = true; adw.enc_nwg = P->nwg_a; adw.slab = &P->dwslab;
    TD3_RC(add_dw_stage(cx, st, h->actor, ab, "A", adw));
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
      FwdOpts fo;
      fo.bump = h->d_ctr; fo.bump_actor = actor_phase;
      TD3_RC(add_fwd_stages(cx, st, f1, "F", fo));
      {
        std::vector<GemmProb> hp = {policy_head(Pta, P->TA, P->XTQ[0], cdq ? P->XTQ[1] : nullptr, 1, inj ? 0 : 1)};
        if (actor_phase) hp.push_back(policy_head(Pa, P->A, P->XAQ, nullptr, 0, 0));
        TD3_RC(push_row_stage(st, hp, kRowPolicyHead, Bp, "heads"));
      }
      std::vector<FwdItem> f2 = {{&q1, Ptq, &P->TQ[0], false, false}};
      if (cdq) f2.push_back({&q2, Ptq, &P->TQ[1], false, false});
      TD3_RC(add_fwd_stages(cx, st, f2, "TF", FwdOpts{}));
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
            p.exi[cp::kB4Off + n] = (int)(hn[n]->lin[3].offb - hn[n]->lin[3].offW);   // one arena
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
          p.ex[cp::kW] = P->per_w;
          p.ex[cp::kTd] = P->per_tdj + (size_t)j * Bp;
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
        TD3_RC(push_row_stage(st, cl, kRowCriticLossP, Bp, "critic_loss"));
      }
      std::vector<BwdItem> cb = {{&q1, Pq, &P->Q[0], true}};
      std::vector<float*> cbx = {P->XQ[0]};
      if (cdq) {
        cb.push_back({&q2, Pq, &P->Q[1], true});
        cbx.push_back(P->XQ[1]);
      }
      TD3_RC(add_bwd_stages(cx, st, cb, "CB", bwd_in_dz0));
      push_enc_bwd(h, Pp, st, cb, cbx, "CB_enc");
      DwOpts cdw;
      cdw.polyak = actor_phase != 0; cdw.enc_nwg = P->nwg; cdw.slab = &P->dwslab;
      TD3_RC(add_dw_stage(cx, st, h->critic, cb, "C", cdw));
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
    FwdOpts lo;
    lo.bump = h->d_ctr; lo.bump_actor = kBumpActorOnly;
    TD3_RC(add_fwd_stages(cx, st, f1, "L", lo));
    std::vector<GemmProb> hp = {policy_head(Pa, P->A, P->XAQ, nullptr, 0, 0)};
    TD3_RC(push_row_stage(st, hp, kRowPolicyHead, Bp, "L_head"));
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

int run_stages(std::vector<Stage>& st, hipStream_t s) {
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

int input_from_ring(td3_handle* h, Ring* r, Plan* P, bool inject_idx, hipStream_t s) {
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

// The mixed step's input (mixed.hip): the destinations of input_from_ring / input_from_ring_particles,
// filled from two rings of one record layout in one launch; a particle learner's blocks go to pbatch.
static int input_from_rings(td3_handle* h, Ring* r, Ring* demo, Plan* P, int n_demo, const int64_t* inject_idx,
                            hipStream_t s) {
  MixedArgs a{};
  a.B = P->B;
  a.Bp = P->Bp;
  a.n_demo = n_demo;
  a.rec = r->rec;
  a.side[0] = MixedSide{demo->data, demo->d_size, demo->seed};
  a.side[1] = MixedSide{r->data, r->d_size, r->seed};
  a.inject_idx = inject_idx;
  a.idx_out = P->d_idx;
  a.ctr = h->d_ctr;
  const int sd = h->sd, ad = h->ad;
  int k = 0;
  if (P->particles) {
    const int F = sd, c0 = kEncC2;
    a.seg[k++] = GatherSeg{P->XA, P->ld_a, c0, r->o_s, F};
    a.seg[k++] = GatherSeg{P->XAQ, P->ld_q, c0, r->o_s, F};
    a.seg[k++] = GatherSeg{P->XTA, P->ld_a, c0, r->o_s2, F};
    for (int j = 0; j < (h->cdq ? 2 : 1); ++j) {
      a.seg[k++] = GatherSeg{P->XQ[j], P->ld_q, c0, r->o_s, F};
      a.seg[k++] = GatherSeg{P->XQ[j], P->ld_q, c0 + F, r->o_a, ad};
      a.seg[k++] = GatherSeg{P->XTQ[j], P->ld_q, c0, r->o_s2, F};
    }
    a.pbatch = P->pbatch;
    a.np = h->N * h->D;
    a.o_p = r->o_p;
    a.o_p2 = r->o_p2;
  } else {
    a.seg[k++] = GatherSeg{P->X_SA, P->ld_sa, 0, r->o_s, sd};
    a.seg[k++] = GatherSeg{P->X_SA, P->ld_sa, sd, r->o_a, ad};
    a.seg[k++] = GatherSeg{P->X_SP, P->ld_sa, 0, r->o_s, sd};
    a.seg[k++] = GatherSeg{P->X_S2A, P->ld_sa, 0, r->o_s2, sd};
  }
  a.seg[k++] = GatherSeg{P->R, 1, 0, r->o_r, 1};
  a.seg[k++] = GatherSeg{P->ND, 1, 0, r->o_nd, 1};
  a.nseg = k;
  return launch_mixed_gather(a, s);
}

static int input_from_batch(td3_handle* h, Plan* P, const float* s, const float* a, const float* s2,
                            const float* r, const float* nd, hipStream_t st) {
  const int sd = h->sd, ad = h->ad, Bp = P->Bp, B = P->B;
  TD3_RC(launch_pack(s, sd, B, Bp, {{P->X_SA, P->ld_sa, 0}, {P->X_SP, P->ld_sa, 0}}, st));
  TD3_RC(launch_pack(a, ad, B, Bp, {{P->X_SA, P->ld_sa, sd}}, st));
  TD3_RC(launch_pack(s2, sd, B, Bp, {{P->X_S2A, P->ld_sa, 0}}, st));
  TD3_RC(launch_pack(r, 1, B, Bp, {{P->R, 1, 0}}, st));
  return launch_pack(nd, 1, B, Bp, {{P->ND, 1, 0}}, st);
}

// Unit importance weights for a step that is not prioritized: refilled on its stream, ahead of its
// body, only when a prioritized step overwrote them (a host flag: the common path queues nothing).
__global__ void fill_f32_kernel(float* p, int n, float v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}
int ensure_unit_weights(td3_handle* h, hipStream_t s) {
  Plan* P = h->plan.get();
  if (!P->per_w_dirty || h->per_step) return 0;
  hipLaunchKernelGGL(fill_f32_kernel, dim3((P->Bp + 255) / 256), dim3(256), 0, s, P->per_w, P->Bp, 1.0f);
  TD3_HIP(hipGetLastError());
  P->per_w_dirty = false;
  return 0;
}

// The particle learner's |TD error| of a row: its J critics' sums over the A outputs of |Q_j - y|
// (critic_loss_p::kTd, one [Bp] row per critic), added in critic order and scaled by 1/(J*A).  One
// fixed-order add per row; pad rows hold 0.
__global__ void per_td_combine_kernel(const float* tdj, int nj, int Bp, float scale, float* td) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Bp) return;
  float a = tdj[i];
  for (int j = 1; j < nj; ++j) a += tdj[(size_t)j * Bp + i];
  td[i] = a * scale;
}

static int combine_td(const td3_handle* h, const Plan* P, hipStream_t s) {
  const int nj = h->cdq ? 2 : 1;
  hipLaunchKernelGGL(per_td_combine_kernel, dim3((P->Bp + 255) / 256), dim3(256), 0, s, P->per_tdj, nj, P->Bp,
                     1.0f / (float)(nj * h->ad), P->per_td);
  TD3_HIP(hipGetLastError());
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

int queue_bc_rows(td3_handle* h, int actor_phase, int n_d, hipStream_t s) {
  const Plan* P = h->plan.get();
  if (!actor_phase || !P || !P->bcf) return 0;
  if (!h->bc_demo_rows) n_d = P->B;
  else TD3_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(P->bcf_nd), n_d, 1, s));
  h->bcf_n_demo = n_d;
  return 0;
}

int build_plan(td3_handle* h, int B) {
  const bool was_sharded = h->dp_sharded && h->nranks > 1;
  h->bc_step = 0;                             // the last BC step's lambda / row errors go with the plan
  for (int g = 0; g < 2; ++g) {               // and the last clipped steps' norm / coef
    h->clip_step[g] = 0;
    h->clip_has[g] = false;
  }
  h->dp_sharded = false;                      // set again by dp.hip add_dp_sharded
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

int ensure_plan(td3_handle* h, int B) {
  if (h->plan && h->plan->B == B) return 0;
  TD3_HIP(hipStreamSynchronize(h->stream));
  return build_plan(h, B);
}

// A particle learner's encoders read the ring the step samples from.
// A featured learner's first layer samples the ring (kProGather; record layout checked at plan
// build against replay.hip's [s | a | s' | r | not_done]).
int bind_ring(td3_handle* h, Ring* r) {
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

int finish_step(td3_handle* h, int actor_phase, hipStream_t s, td3_step_stats* stats, bool prioritized) {
  h->total_it += 1;
  h->critic_step += 1;
  h->last_step_stream = s;
  if (actor_phase) {
    h->actor_step += 1;
    TD3_RC(note_actor_update(h, s));
  }
  // the training log's launch: behind the body (and a prioritized step's write-back), ahead of the sync
  if (h->log && h->total_it % h->log->every == 0) TD3_RC(log_step(h, actor_phase, prioritized, s));
  note_bc_step(h, actor_phase);
  note_clip_step(h, actor_phase);
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

// A ring against the learner that trains on it: kind, dims, particle shape, device.  what: the wording
// of the kind / dims / shape messages (the replica step of td3_train_step_local has its own).
int check_ring(const td3_handle* h, const Ring* r, RingUser what) {
  const bool rep = what == kReplicaStep;
  TD3_ARG(r->particles == h->particles,
          rep ? "replay buffer does not match" : "replay buffer kind does not match the learner");
  TD3_ARG(r->sd == h->sd && r->ad == h->ad,
          rep ? "replay buffer does not match" : "replay buffer dims do not match the learner");
  TD3_ARG(!r->particles || (r->N == h->N && r->D == h->D),
          rep ? "particle replay buffer shape does not match" : "particle shape does not match the learner");
  TD3_ARG(r->device == h->cfg.device, "replay buffer lives on another device");
  return 0;
}

}  // namespace td3

using namespace td3;

extern "C" {

int td3_train_step(td3_handle* h, rb_handle* rbh, int batch, void* stream, const int64_t* inject_idx,
                   const float* inject_noise, td3_step_stats* stats) {
  TD3_ARG(h && rbh, "null handle");
  TD3_ARG(batch > 0, "batch must be positive");
  Ring* r = reinterpret_cast<Ring*>(rbh);
  TD3_RC(check_ring(h, r, kLearnerStep));
  TD3_ARG(r->size > 0 || inject_idx, "train on an empty replay buffer");
  TD3_HIP(hipSetDevice(h->cfg.device));
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
  TD3_RC(queue_bc_rows(h, actor_phase, batch, s));
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

// The prioritized step of either learner kind, after the kind check of its entry point.
static int prioritized_step(td3_handle* h, rb_handle* rbh, int batch, double beta, void* stream,
                            const float* inject_u, const float* inject_noise, td3_step_stats* stats,
                            td3_per_stats* per, const char* dp_msg) {
  TD3_ARG(!h->comm && !h->local, dp_msg);
  Ring* r = reinterpret_cast<Ring*>(rbh);
  TD3_RC(check_ring(h, r, kLearnerStep));
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
  P->per_ring_gen = r->gen;
  TD3_RC(queue_bc_rows(h, actor_phase, batch, s));
  TD3_RC(ring_draw_prioritized(r, batch, beta, inject_u ? P->per_u : nullptr, P->d_inject_idx, P->d_idx, P->per_w, s));
  TD3_RC(input_from_ring(h, r, P, true, s));
  h->per_step = true;
  const int rc = run_body(h, actor_phase, inject_noise ? 1 : 0, s, nullptr);
  h->per_step = false;
  TD3_RC(rc);
  if (P->particles) TD3_RC(combine_td(h, P, s));   // (the featured loss row writes the row's |TD error| itself)
  TD3_RC(ring_store_priorities(r, P->d_inject_idx, P->per_td, batch, true, s));
  TD3_RC(ring_end_read(r, s));                   // later adds wait for the step and its write-back
  if (inject_u || inject_noise) TD3_HIP(hipStreamSynchronize(s));   // host sources are pageable
  TD3_RC(finish_step(h, actor_phase, s, stats, true));
  if (per && (per->weight || per->td_abs)) {
    TD3_HIP(hipStreamSynchronize(s));
    if (per->weight) TD3_HIP(hipMemcpy(per->weight, P->per_w, (size_t)batch * 4, hipMemcpyDeviceToHost));
    if (per->td_abs) TD3_HIP(hipMemcpy(per->td_abs, P->per_td, (size_t)batch * 4, hipMemcpyDeviceToHost));
  }
  return 0;
}

int td3_debug_per_stage(td3_handle* h, rb_handle* rbh, int stage, void* stream) {
  TD3_ARG(h && rbh, "null handle");
  TD3_ARG(stage == 0 || stage == 1, "stage 0 (gather) or 1 (combine)");
  Ring* r = reinterpret_cast<Ring*>(rbh);
  Plan* P = h->plan.get();
  TD3_ARG(P && P->per_ring_gen != 0 && ring_alive(r, P->per_ring_gen),
          "run a prioritized step on this ring first (the plan's buffers hold its rows)");
  TD3_ARG(stage == 0 || P->particles, "the featured step has no combine (its loss row writes the |TD error|)");
  TD3_HIP(hipSetDevice(h->cfg.device));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  if (stage == 1) return combine_td(h, P, s);
  TD3_RC(ring_begin_read(r, s));
  TD3_RC(input_from_ring(h, r, P, true, s));
  return ring_end_read(r, s);
}

// Demonstration replay: batch rows [0, n_demo) from `demo`, the rest from `rb`, drawn uniformly on
// each ring; one input launch (mixed.hip), then the non-ring body of the injected-index steps.
int td3_train_step_mixed(td3_handle* h, rb_handle* rbh, rb_handle* demoh, int batch, int n_demo, void* stream,
                         const int64_t* inject_idx, const float* inject_noise, td3_step_stats* stats) {
  TD3_ARG(batch > 0, "batch must be positive");
  TD3_ARG(n_demo >= 0 && n_demo <= batch, "n_demo must be in [0, batch]");
  TD3_ARG(h && rbh && demoh, "null handle");
  TD3_ARG(rbh != demoh, "rb and demo are the same ring (a mixed step draws from two rings)");
  Ring* r = reinterpret_cast<Ring*>(rbh);
  Ring* d = reinterpret_cast<Ring*>(demoh);
  TD3_RC(check_ring(h, r, kLearnerStep));
  TD3_RC(check_ring(h, d, kLearnerStep));
  TD3_ARG(!r->pri.on && !d->pri.on,
          "priorities are enabled on a ring of a mixed step (the mixed draw is uniform)");
  TD3_ARG(!h->comm && !h->local, "td3_train_step_mixed on a data-parallel handle (comm group attached)");
  TD3_ARG(inject_idx || ((n_demo == 0 || d->size > 0) && (n_demo == batch || r->size > 0)),
          "train on an empty replay buffer (a ring that contributes rows to the mixed batch is empty)");
  if (inject_idx)
    for (int i = 0; i < batch; ++i)
      TD3_ARG(inject_idx[i] >= 0 && inject_idx[i] < (i < n_demo ? d->cap : r->cap), "injected index out of range");
  TD3_HIP(hipSetDevice(h->cfg.device));
  TD3_RC(ensure_plan(h, batch));
  Plan* P = h->plan.get();
  if (P->particles) {                            // the encoders read the packed batch, not a ring
    const int np = h->N * h->D;
    set_particle_source(P, kBatchSource, P->pbatch, 2 * np, 0, np, P->d_iota);
  }
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  TD3_RC(ring_begin_read(r, s));                 // the adds queued on either ring before this step
  TD3_RC(ring_begin_read(d, s));
  if (inject_idx)
    TD3_HIP(hipMemcpyAsync(P->d_inject_idx, inject_idx, (size_t)batch * 8, hipMemcpyHostToDevice, s));
  if (inject_noise)
    TD3_HIP(hipMemcpyAsync(P->noise, inject_noise, (size_t)batch * h->ad * 4, hipMemcpyHostToDevice, s));
  const int actor_phase = ((h->total_it + 1) % h->cfg.policy_freq) == 0;
  TD3_RC(queue_bc_rows(h, actor_phase, n_demo, s));
  TD3_RC(input_from_rings(h, r, d, P, n_demo, inject_idx ? P->d_inject_idx : nullptr, s));
  TD3_RC(run_body(h, actor_phase, inject_noise ? 1 : 0, s, nullptr));
  TD3_RC(ring_end_read(r, s));                   // later adds to either ring wait for this step's reads
  TD3_RC(ring_end_read(d, s));
  if (inject_idx || inject_noise) TD3_HIP(hipStreamSynchronize(s));   // host sources are pageable
  TD3_RC(finish_step(h, actor_phase, s, stats));
  P->mixed_gen[0] = r->gen;
  P->mixed_gen[1] = d->gen;
  P->mixed_n_demo = n_demo;
  P->mixed_it = (int64_t)h->total_it;
  return 0;
}

int td3_debug_mixed_input(td3_handle* h, rb_handle* rbh, rb_handle* demoh, void* stream) {
  TD3_ARG(h && rbh && demoh, "null handle");
  Ring* r = reinterpret_cast<Ring*>(rbh);
  Ring* d = reinterpret_cast<Ring*>(demoh);
  Plan* P = h->plan.get();
  TD3_ARG(P && P->mixed_it != 0 && P->mixed_it == (int64_t)h->total_it && ring_alive(r, P->mixed_gen[0]) &&
              ring_alive(d, P->mixed_gen[1]),
          "run a mixed step on these two rings first (the plan's buffers hold its rows)");
  TD3_HIP(hipSetDevice(h->cfg.device));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  TD3_RC(ring_begin_read(r, s));
  TD3_RC(ring_begin_read(d, s));
  TD3_RC(input_from_rings(h, r, d, P, P->mixed_n_demo, P->d_idx, s));   // the rows of that step again
  TD3_RC(ring_end_read(r, s));
  return ring_end_read(d, s);
}

int td3_train_step_prioritized(td3_handle* h, rb_handle* rbh, int batch, double beta, void* stream,
                               const float* inject_u, const float* inject_noise, td3_step_stats* stats,
                               td3_per_stats* per) {
  TD3_ARG(h && rbh, "null handle");
  TD3_ARG(batch > 0, "batch must be positive");
  TD3_ARG(beta >= 0.0 && beta <= 1.0, "beta must be in [0, 1]");
  TD3_ARG(!h->particles, "td3_train_step_prioritized on a particle learner (use td3_train_step_prioritized_particles)");
  return prioritized_step(h, rbh, batch, beta, stream, inject_u, inject_noise, stats, per,
                          "td3_train_step_prioritized on a data-parallel handle (comm group attached)");
}

int td3_train_step_prioritized_particles(td3_handle* h, rb_handle* rbh, int batch, double beta, void* stream,
                                         const float* inject_u, const float* inject_noise,
                                         td3_step_stats* stats, td3_per_stats* per) {
  TD3_ARG(h && rbh, "null handle");
  TD3_ARG(batch > 0, "batch must be positive");
  TD3_ARG(beta >= 0.0 && beta <= 1.0, "beta must be in [0, 1]");
  TD3_ARG(h->particles, "td3_train_step_prioritized_particles on a featured learner (use td3_train_step_prioritized)");
  return prioritized_step(h, rbh, batch, beta, stream, inject_u, inject_noise, stats, per,
                          "td3_train_step_prioritized_particles on a data-parallel handle (comm group attached)");
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
  TD3_RC(queue_bc_rows(h, actor_phase, batch, s));
  TD3_RC(input_from_batch(h, P, state, action, next_state, reward, not_done, s));
  TD3_RC(run_body(h, actor_phase, inject_noise ? 1 : 0, s, nullptr));
  if (inject_noise) TD3_HIP(hipStreamSynchronize(s));
  return finish_step(h, actor_phase, s, stats);
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
  // (XQ[1] / XTQ[1] are null without CDQ: pack_kernel skips a null destination)
  TD3_RC(launch_pack(feat, F, B, Bp, {{P->XA, P->ld_a, c0}, {P->XAQ, P->ld_q, c0}, {P->XQ[0], P->ld_q, c0}}, s));
  TD3_RC(launch_pack(action, ad, B, Bp, {{P->XQ[0], P->ld_q, c0 + F}, {cdq ? P->XQ[1] : nullptr, P->ld_q, c0 + F}}, s));
  TD3_RC(launch_pack(next_feat, F, B, Bp, {{P->XTA, P->ld_a, c0}, {P->XTQ[0], P->ld_q, c0},
                                           {cdq ? P->XTQ[1] : nullptr, P->ld_q, c0}}, s));
  if (cdq) TD3_RC(launch_pack(feat, F, B, Bp, {{P->XQ[1], P->ld_q, c0}}, s));
  TD3_RC(launch_pack(part, np, B, Bp, {{P->pbatch, 2 * np, 0}}, s));
  TD3_RC(launch_pack(next_part, np, B, Bp, {{P->pbatch, 2 * np, np}}, s));
  TD3_RC(launch_pack(reward, 1, B, Bp, {{P->R, 1, 0}}, s));
  TD3_RC(launch_pack(not_done, 1, B, Bp, {{P->ND, 1, 0}}, s));
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
  TD3_RC(launch_pack(feat, F, B, Bp, {{P->XA, P->ld_a, c0}, {P->XAQ, P->ld_q, c0}}, s));
  TD3_RC(launch_pack(part, np, B, Bp, {{P->pbatch, 2 * np, 0}}, s));
  TD3_RC(run_stages(P->actor_learn, s));
  h->last_step_stream = s;
  h->actor_step += 1;
  TD3_RC(note_actor_update(h, s));
  if (h->clip_max[0] > 0.0) {                 // total_it does not move: the call reports under the current one
    h->clip_step[0] = h->total_it;
    h->clip_has[0] = true;
  }
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

}  // extern "C"
