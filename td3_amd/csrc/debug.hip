// Profiling and debug entry points of the C-ABI: per-stage timing, kernel probes, plan flags.
#include "learner.h"

using namespace td3;

extern "C" {

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
  TD3_RC(queue_bc_rows(h, actor_phase ? 1 : 0, batch, s));   // a profiled step draws from one ring: n_d = B
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
  note_bc_step(h, actor_phase);
  note_clip_step(h, actor_phase);
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

const char* td3_debug_last_stage(td3_handle* h, int i, int kernel) {
  if (!h || !h->last_body || i < 0 || i >= (int)h->last_body->size()) return "";
  const Stage& st = (*h->last_body)[i];
  return kernel ? st.kernel.c_str() : st.name.c_str();
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

int td3_debug_row_lds(void) { return last_row_lds(); }

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
