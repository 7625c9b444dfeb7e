// Learner state: parameter layouts and arenas, create / destroy, parameter and optimizer-state I/O
// of the td3_* C-ABI (include/td3.h).  The stage builders are in stages.hip, the train step in
// step.hip, the queries in act.hip, data parallel in dp.hip, profiling and debug entries in debug.hip.
//
// Reference mapping (/root/reference):
//   TD3_featured.TD3.__init__   :100-110  -> td3_create (param arenas, targets = copies)
//   TD3_base save/load         TD3_base.py:26-50 -> td3_get_params / td3_set_params
//
// HBM layout
//   * one fp32 arena per parameter group (actor: 1 MLP; critic: q1 then q2), five
//     parallel copies: params P, targets T, Adam exp_avg M, exp_avg_sq V, grads G.
//     Every Linear weight is stored [pad32(out)][pad32(in)] (zero pads, which stay
//     exactly zero through Adam and Polyak), biases / LayerNorm affines [pad32(out)].
#include "learner.h"

namespace td3 {

static thread_local char g_err[1024] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

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

}  // namespace td3

// ================================================================== C-ABI
using namespace td3;

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
  destroy_train_log(h);
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
  if (h->d_clip) (void)hipFree(h->d_clip);
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

// TD3+BC (include/td3.h, "TD3+BC"): alpha is a launch argument of the actor_head_bwd stage, so a new
// value rebuilds the plan (build_step reads h->bc_alpha) and with it the captured graphs.
int td3_set_bc(td3_handle* h, double alpha) {
  TD3_ARG(std::isfinite(alpha) && alpha >= 0.0, "alpha must be finite and >= 0");
  TD3_ARG(h != nullptr, "null handle");
  TD3_ARG(!h->particles, "td3_set_bc on a particle learner (the particle learner has no BC step yet)");
  TD3_ARG(!h->comm && !h->local,
          "td3_set_bc on a data-parallel handle (comm group attached): lambda would need the global batch's mean");
  TD3_HIP(hipSetDevice(h->cfg.device));
  TD3_HIP(hipStreamSynchronize(h->stream));
  if (h->bc_alpha == alpha) return 0;
  h->bc_alpha = alpha;
  h->bc_step = 0;
  if (h->plan) TD3_RC(build_plan(h, h->plan->B));
  return 0;
}

int td3_bc_info(td3_handle* h, td3_bc_info_t* info) {
  TD3_ARG(info != nullptr, "null info");
  TD3_ARG(h != nullptr, "null handle");
  *info = td3_bc_info_t{};
  info->enabled = h->bc_alpha > 0.0 ? 1 : 0;
  info->alpha = h->bc_alpha;
  const Plan* P = h->plan.get();
  if (!h->bc_step || !P || !P->bc) return 0;
  TD3_HIP(hipSetDevice(h->cfg.device));
  TD3_HIP(hipDeviceSynchronize());              // the last step may sit on a caller's stream
  float lam[2];
  std::vector<float> se((size_t)P->B);
  TD3_HIP(hipMemcpy(lam, P->bc_lam, sizeof(lam), hipMemcpyDeviceToHost));
  TD3_HIP(hipMemcpy(se.data(), P->bc_se, se.size() * 4, hipMemcpyDeviceToHost));
  double sum = 0;
  for (float v : se) sum += (double)v;
  info->step = h->bc_step;
  info->lambda = lam[0];
  info->q_abs_mean = lam[1];
  // (a filtered step: the rows that are not kept wrote 0, and the term is normalised by its n_d candidates)
  const double n_d = P->bcf ? (double)h->bcf_n_demo : (double)P->B;
  info->bc_loss = n_d > 0 ? sum / (n_d * h->ad) : 0.0;
  return 0;
}

// The BC term's row mask (include/td3.h, "BC on the demonstration rows, Q-filter"): the switches pick the
// row kind of the actor_head_bwd stage (build_step), so a change while BC is on rebuilds the plan.
int td3_set_bc_filter(td3_handle* h, int demo_rows, int q_filter) {
  TD3_ARG((demo_rows == 0 || demo_rows == 1) && (q_filter == 0 || q_filter == 1), "demo_rows and q_filter must be 0 or 1");
  TD3_ARG(h != nullptr, "null handle");
  TD3_ARG(!h->particles, "td3_set_bc_filter on a particle learner (the particle learner has no BC step yet)");
  TD3_ARG(!h->comm && !h->local,
          "td3_set_bc_filter on a data-parallel handle (comm group attached): BC is not supported there");
  if (h->bc_demo_rows == demo_rows && h->bc_q_filter == q_filter) return 0;
  if (!(h->bc_alpha > 0.0)) {                   // no plan reads them while BC is off
    h->bc_demo_rows = demo_rows;
    h->bc_q_filter = q_filter;
    return 0;
  }
  TD3_HIP(hipSetDevice(h->cfg.device));
  TD3_HIP(hipStreamSynchronize(h->stream));
  h->bc_demo_rows = demo_rows;
  h->bc_q_filter = q_filter;
  h->bc_step = 0;
  if (h->plan) TD3_RC(build_plan(h, h->plan->B));
  return 0;
}

int td3_bc_filter_info(td3_handle* h, td3_bc_filter_info_t* info) {
  TD3_ARG(info != nullptr, "null info");
  TD3_ARG(h != nullptr, "null handle");
  *info = td3_bc_filter_info_t{};
  info->demo_rows = h->bc_demo_rows;
  info->q_filter = h->bc_q_filter;
  const Plan* P = h->plan.get();
  if (!h->bc_step || !P || !P->bcf) return 0;
  TD3_HIP(hipSetDevice(h->cfg.device));
  TD3_HIP(hipDeviceSynchronize());              // the last step may sit on a caller's stream
  std::vector<float> se((size_t)P->B), keep((size_t)P->B);
  TD3_HIP(hipMemcpy(se.data(), P->bc_se, se.size() * 4, hipMemcpyDeviceToHost));
  TD3_HIP(hipMemcpy(keep.data(), P->bcf_keep, keep.size() * 4, hipMemcpyDeviceToHost));
  double sum = 0;
  int64_t kept = 0;
  for (int r = 0; r < P->B; ++r) {
    sum += (double)se[r];
    kept += keep[r] != 0.f;
  }
  info->step = h->bc_step;
  info->n_demo = h->bcf_n_demo;
  info->kept = kept;
  info->bc_loss = h->bcf_n_demo > 0 ? sum / ((double)h->bcf_n_demo * h->ad) : 0.0;
  return 0;
}

int td3_bc_filter_keep(td3_handle* h, float* keep, int n) {
  TD3_ARG(keep != nullptr, "null keep");
  TD3_ARG(h != nullptr, "null handle");
  const Plan* P = h->plan.get();
  TD3_ARG(h->bc_step && P && P->bcf, "no filtered BC step to report in the current step plan");
  TD3_ARG(n == P->B, "n must be the batch size of that step");
  TD3_HIP(hipSetDevice(h->cfg.device));
  TD3_HIP(hipDeviceSynchronize());
  TD3_HIP(hipMemcpy(keep, P->bcf_keep, (size_t)n * 4, hipMemcpyDeviceToHost));
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

}  // extern "C"
