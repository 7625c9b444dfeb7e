// The stage builders of the step and query plans: per-batch buffers, the GEMM / row / dW stage lists
// and the choices of their launch shapes, the k-quad weight images.
#include "learner.h"

namespace td3 {

int upload(td3_handle* h, std::vector<void*>& owned, const void* host, size_t bytes, void** out) {
  void* d = nullptr;
  TD3_HIP(hipMalloc(&d, bytes));
  TD3_HIP(hipMemcpy(d, host, bytes, hipMemcpyHostToDevice));
  owned.push_back(d);
  *out = d;
  (void)h;
  return 0;
}

void alloc_eval(Scratch& S, const NetL& n, int Bp, float* X, int ldx, bool bwd, bool norm, bool policy_or_q,
                EvalB& e) {
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

// Sizes and carves a plan's scratch: `carve` runs on a measuring Scratch, used + kScratchTail floats
// are allocated and zeroed, and `carve` runs again on the allocation.  mapped: the act plan whose
// IoCarve block lives in mapped host memory (null: the I/O buffers are carved from the scratch too).
int carve_scratch(const CarveFn& carve, ActPlan* mapped, float** scratch, size_t* scratch_bytes) {
  Scratch M;
  IoCarve mio{&M, mapped != nullptr};
  carve(M, mio);
  const size_t bytes = (M.used + kScratchTail) * sizeof(float);
  TD3_HIP(hipMalloc(scratch, bytes));
  TD3_HIP(hipMemset(*scratch, 0, bytes));
  TD3_HIP(hipDeviceSynchronize());   // null-stream memset vs the non-blocking step stream
  if (scratch_bytes) *scratch_bytes = bytes;
  Scratch S{*scratch};
  IoCarve io{&S, mapped != nullptr};
  if (mapped) TD3_RC(map_io(mapped, mio.used, &io));
  carve(S, io);
  if (S.used != M.used || io.used != mio.used) {
    set_error("internal: scratch carve took %zu + %zu floats, measured %zu + %zu", S.used, io.used, M.used, mio.used);
    return -2;
  }
  return 0;
}

static int gemm_lds_bytes(int Kp, int rt = 1) {
  int f = std::max(32 * rt * lds_stride(Kp), kGemmWaves * 32 * 33);
  return f * 4;
}

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

static int push_gemm_stage(std::vector<Stage>& st, std::vector<GemmProb>& probs, int mode, int wn, int pro, int Bp,
                           int lds, int blocks, double flops, const std::string& name, Counters* bump,
                           int bump_actor, const RingSide* rs = nullptr) {
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
bool merge_gemm_pair(std::vector<Stage>& st, size_t i, size_t j) {
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

int stage_index(const std::vector<Stage>& st, const std::string& name) {
  for (size_t k = 0; k < st.size(); ++k)
    if (st[k].name == name) return (int)k;
  return -1;
}

int push_row_stage(std::vector<Stage>& st, std::vector<GemmProb>& probs, int kind, int Bp, const std::string& name) {
  TD3_ARG(!probs.empty() && probs.size() <= (size_t)kMaxProbs, "too many problems in one row stage");
  GemmTable t{};
  for (size_t i = 0; i < probs.size(); ++i) t.p[i] = probs[i];
  t.nprob = (int)probs.size();
  char kname[64];
  snprintf(kname, sizeof(kname), "td3::row_kernel<%d>", kind);
  if (kind == kRowActorHeadBwdBc) snprintf(kname, sizeof(kname), "td3::row_bc_kernel");
  if (kind == kRowActorHeadBwdBcF) snprintf(kname, sizeof(kname), "td3::row_bcf_kernel");
  st.push_back({name, [=](hipStream_t s) { return launch_rows(kind, t, Bp, s); }, 0, kname});
  return 0;
}

// Two independent row stages in one launch: problems [0, n1) of kind1, the rest of kind2.
int push_row2_stage(std::vector<Stage>& st, std::vector<GemmProb>& probs, int kind1, int kind2, int n1, int Bp,
                    const std::string& name) {
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
int env_int(const char* name, int dflt) {
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
bool can_fuse_l0(const std::vector<FwdItem>& items) {
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
// data-parallel plans (flat Adam after the exchange), by a pack stage behind it (dp.hip push_w4_pack).
// Weight normalization (wn_kernel derives W) and the particle learner read the row-major arena.
// TD3_W4=0 turns them off.
bool w4_eligible(const td3_handle* h, int Bp) {
  (void)Bp;
  const bool on = env_int("TD3_W4", 1) != 0;     // read at every plan build (tests switch it)
  return on && !h->particles && h->cfg.norm != 2;
}

// The pack of a group's forward weights (layers 0-2: the heads are read by the row kernels) from P
// (and T) into their images
int w4_pack_args(const Group& g, bool with_t, W4PackArgs* out) {
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
int ensure_w4(td3_handle* h, hipStream_t s) {
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

int add_fwd_stages(const StageCtx& c, std::vector<Stage>& st, const std::vector<FwdItem>& items, const char* tag,
                   const FwdOpts& o) {
  td3_handle* h = c.h;
  const int Bp = c.Bp, B = c.B, bump_actor = o.bump_actor, o_r = o.o_r;
  Counters* bump = o.bump;
  const RingSide* ring = o.ring;
  const RingOut* ro = o.ro;
  const bool r16 = o.r16;
  const bool norm = h->cfg.norm == 1;
  const bool fuse_l0 = o.fuse_l0 && can_fuse_l0(items);
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
    TD3_RC(push_gemm_stage(st, probs, 0, wn, pro, Bp, lds, blocks, flops,
                           std::string(tag) + (l0 ? "_fwd01" : "_fwd" + std::to_string(l)),
                           l == bump_l ? bump : nullptr, bump_actor, gather ? ring : nullptr));
  }
  return 0;
}

// dU_1 = dZ_2 * W_2 (dZ_2 built by the fused head prologue `pro2`), dU_0 = dZ_1 * W_1
// (dZ_1 = relu'(LN_bwd(dU_1)) in the prologue), then dZ_0 rows when needed.
// need_in (TD3_particles): dU_in = dZ_0 * W_0 as well (dZ_0 formed in its prologue and kept),
// the input grad that feeds lnorm1's backward, the encoder and dQ1/da; replaces the dZ_0 rows.
int add_bwd_stages(const StageCtx& c, std::vector<Stage>& st, const std::vector<BwdItem>& items, const char* tag,
                   const BwdOpts& o) {
  td3_handle* h = c.h;
  const int Bp = c.Bp, B = c.B;
  const bool need_dz0 = o.need_dz0, need_in = o.need_in;
  std::vector<GemmProb>* lnbwd_rows = o.lnbwd_rows;
  const float head_bwd_scale = o.head_bwd_scale;
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
    TD3_RC(push_gemm_stage(st, probs, 1, wn, pro, Bp, lds, blocks,
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

// The optimizer's view of a group's arenas with optimizer `which`'s hyper-parameters
static AdamArgs group_adam(const td3_handle* h, const Group& g, int which) {
  AdamArgs a{};
  a.P = g.P; a.G = g.G; a.M = g.M; a.V = g.V; a.T = g.T;
  a.ctr = h->d_ctr;
  a.which = which;
  a.lr = h->adam[which].lr; a.eps = h->adam[which].eps;
  a.beta1 = h->adam[which].beta1; a.beta2 = h->adam[which].beta2;
  a.tau = (float)h->cfg.tau;
  a.grad_scale = 1.0f;
  a.P4 = h->w4_build ? g.P4 : nullptr;     // the dW kernels keep the k-quad images current
  a.T4 = h->w4_build ? g.T4 : nullptr;
  return a;
}

// The dW work of `items` (learner.h DwWork): one problem per layer of every network (weight, bias and
// LayerNorm affine grads), one more for a network's lnorm1 affine, and the roofline's accounting.
// o.unit_scale (featured critic): per item, the dense [Bp] row scale g_r of its unit-gradient
// backward rows (layers 0..2 and their LayerNorms; the head's dZ is the true gradient already).
static int make_dw_work(const StageCtx& c, const Group& g, const std::vector<BwdItem>& items, const DwOpts& o,
                        DwWork* out) {
  td3_handle* h = c.h;
  const int Bp = c.Bp;
  const bool norm = h->cfg.norm == 1;
  // B >= 512: 64x64 weight tiles with LDS-staged operands (dw64_kernel: half the operand
  // traffic, Humanoid C_dw 73 -> 63 us), else 32x32 register tiles (dw_kernel: more, shorter
  // workgroups for the latency-bound small batches)
  const bool tile64 = Bp >= 512;
  DwWork w{};
  DwArgs& a = w.a;
  double dw_operand_bytes = 0, dw_params = 0, dw_weights = 0;
  TD3_ARG(!o.unit_scale || o.unit_scale->size() == items.size(), "internal: one row scale per dW item");
  for (size_t k = 0; k < items.size(); ++k) {
    const BwdItem& it = items[k];
    const NetL& n = *it.net;
    const float* usc = o.unit_scale ? (*o.unit_scale)[k] : nullptr;
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
      p.tile_begin = w.blocks;
      w.blocks += (tile64 ? (L.Np + 63) / 64 : L.Np / 32) * p.ntk + L.Np / 32;   // matrix, then vector tiles
      w.flops += 2.0 * Bp * L.N * L.K;
      // operands once (dZ and U rows; the LayerNorm vector tiles also dU, H and the statistics),
      // then the optimizer's state per parameter (weight, bias, LN affine)
      dw_operand_bytes += 4.0 * Bp * ((double)L.N + L.K) + ((norm && l < 3) ? 4.0 * Bp * (2.0 * L.N + 2.0) : 0.0);
      dw_params += (double)L.N * L.K + L.N + ((norm && l < 3) ? 2.0 * L.N : 0.0);
      dw_weights += (double)L.N * L.K;
      TD3_ARG(a.nprob < kMaxDwProbs, "too many problems in one dw stage");
      a.probs[a.nprob++] = p;
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
      p.tile_begin = w.blocks;
      w.blocks += p.Np / 32;
      TD3_ARG(a.nprob < kMaxDwProbs, "too many problems in one dw stage");
      a.probs[a.nprob++] = p;
    }
  }
  a.Bp = Bp;
  TD3_ARG(!h->w4_build || (g.P4 && g.T4), "internal: k-quad images not allocated");
  a.adam = group_adam(h, g, o.which);
  // data parallel, weight normalization (dW -> (dg, dv) in wn_kernel) and a clipping group (the norm
  // needs the whole gradient before the first Adam update): the gradient only
  const bool grad_only = h->comm || h->local || g.wn.nlin > 0 || clip_on(h, o.which);
  a.mode = grad_only ? kDwGrad : o.polyak ? kDwAdamPolyak : kDwAdam;
  // a launch's algorithmic bytes: gradient-only dW writes 4 B per parameter; the fused Adam reads and
  // writes P, M, V (24 B; the gradient never leaves registers), Polyak reads and writes T (+8 B), and
  // the k-quad images take every updated weight once more (+4 B, +4 B more for T4 on Polyak steps)
  w.bytes = dw_operand_bytes +
            (a.mode == kDwGrad ? 4.0 * dw_params
                               : dw_params * (a.mode == kDwAdamPolyak ? 32.0 : 24.0) +
                                     (h->w4_build ? dw_weights * (a.mode == kDwAdamPolyak ? 8.0 : 4.0) : 0.0));
  a.tile64 = tile64 ? 1 : 0;
  a.scaled = o.unit_scale ? 1 : 0;
  w.split = tile64 && Bp % 64 == 0 && TD3_DWSK;
  *out = w;
  return 0;
}

// Network b's problems of `w` as a launch of their own (a bucket of dp.hip's overlapped schedule).
// They keep the tile_begin of the whole list: only the one-tile-per-workgroup kernels read it, and a
// bucket is a split-K launch.  Its bytes are not accounted.
DwWork dw_bucket(const DwWork& w, const std::vector<BwdItem>& items, size_t b) {
  auto count = [](const NetL& n) { return 4 + (n.lnin ? 1 : 0); };
  int p0 = 0;
  for (size_t k = 0; k < b; ++k) p0 += count(*items[k].net);
  const NetL& n = *items[b].net;
  DwWork out = w;
  out.a.nprob = count(n);
  for (int i = 0; i < out.a.nprob; ++i) out.a.probs[i] = w.a.probs[p0 + i];
  out.flops = out.bytes = 0;
  for (int l = 0; l < 4; ++l) out.flops += 2.0 * w.a.Bp * n.lin[l].N * n.lin[l].K;
  return out;
}

// One dW launch stage: the split-K pair where the work allows it (B >= 512), else one tile per
// workgroup.  The one place that spells a dW stage's kernel name.
int push_dw_stage(const StageCtx& c, std::vector<Stage>& st, const DwWork& w, SlabRef* slab, const std::string& name) {
  const DwArgs a = w.a;
  const int blocks = w.blocks;
  const std::string scaled = a.scaled ? "true" : "false";
  if (w.split) {
    DwSplit k{};
    TD3_RC(make_dw_split(c.h, c.owned, a, slab, k));
    st.push_back({name,
                  [=](hipStream_t s) {
                    DwSplit kk = k;
                    kk.slab = slab->p;
                    return launch_dw_split(a, kk, s);
                  },
                  w.flops, "td3::dwsk_kernel<" + scaled + (k.tm == 128 ? ", true>" : ", false>")});
  } else {
    st.push_back({name, [=](hipStream_t s) { return launch_dw(a, blocks, s); }, w.flops,
                  (a.tile64 ? "td3::dw64_kernel<" : "td3::dw_kernel<") + scaled + ">"});
  }
  st.back().bytes = w.bytes;
  return 0;
}

// TD3_particles: the encoder partial slabs of `items`, reduced and stepped in one launch
static int push_enc_adam_stage(std::vector<Stage>& st, const std::vector<BwdItem>& items, const DwWork& w,
                               int enc_nwg, const char* tag) {
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
  ea.adam = w.a.adam;
  ea.mode = w.a.mode;
  st.push_back({std::string(tag) + "_enc_adam", [=](hipStream_t s) { return launch_enc_adam(ea, s); }, 0,
                "td3::enc_adam_kernel"});
  return 0;
}

// Weight normalization's optimizer step: the dW stage's gradient -> (dg, dv), Adam (+ Polyak)
int push_wn_stage(std::vector<Stage>& st, const Group& g, const AdamArgs& adam, bool polyak, const char* tag) {
  WnArgs w = g.wn;
  w.adam = adam;
  w.mode = kWnAdam;
  w.polyak = polyak ? 1 : 0;
  st.push_back({std::string(tag) + "_wn", [=](hipStream_t s) { return launch_wn(w, s); }, 0, "td3::wn_kernel"});
  return 0;
}

// Weight / bias / LN grads of every layer of `items` (o.enc_nwg, TD3_particles: then the encoders'),
// then the optimizer step: fused into the dW launch on one GPU; wn_kernel under weight normalization;
// in a data-parallel plan the dW kernels write the gradient only and dp.hip's schedule follows; so they do
// for a group that clips its gradient (td3_set_grad_clip), and clip.hip's norm and Adam stages follow.
int add_dw_stage(const StageCtx& c, std::vector<Stage>& st, Group& g, const std::vector<BwdItem>& items,
                 const char* tag, const DwOpts& o) {
  DwWork w;
  TD3_RC(make_dw_work(c, g, items, o, &w));
  const bool dp = c.h->comm != nullptr || c.h->local != nullptr;
  if (dp && dp_buckets(c.h, g, items, o, w)) return add_dp_overlapped(c, st, g, items, tag, o, w);
  TD3_RC(push_dw_stage(c, st, w, o.slab, std::string(tag) + "_dw"));
  if (o.enc_nwg > 0) TD3_RC(push_enc_adam_stage(st, items, w, o.enc_nwg, tag));
  if (dp) return add_dp_optimizer(c.h, st, g, w.a.adam, o.polyak, tag);
  if (clip_on(c.h, o.which)) return add_clip_optimizer(c.h, st, g, w.a.adam, o.polyak, tag);
  if (g.wn.nlin > 0) return push_wn_stage(st, g, w.a.adam, o.polyak, tag);
  return 0;
}

int alloc_dw_slab(Plan* P) {
  if (!P->dwslab.bytes) return 0;
  void* d = nullptr;
  TD3_HIP(hipMalloc(&d, P->dwslab.bytes));
  P->tables.push_back(d);
  P->dwslab.p = static_cast<float*>(d);
  return 0;
}

void free_plan_tables(std::vector<void*>& t) {
  for (void* p : t) (void)hipFree(p);
  t.clear();
}

}  // namespace td3
