// The training log (include/td3.h, "training log"): per-step losses and Q statistics of the learner in
// a ring of td3_log_entry in device memory, one launch per logged step.
//
// train_log_kernel, ONE workgroup of 256 threads, queued by finish_step directly behind a step's body:
//   * it reads rows r < B of the plan's buffers as the body left them -- Plan::Y, Plan::Q[j].Qv
//     ([Bp][ldq], nq live columns), Plan::sqerr ([2][Bp]), Plan::AQ.Qv on actor steps, Plan::per_w on
//     prioritized steps -- a few tens of KB at most, so the launch is its cost and a second workgroup
//     would buy nothing;
//   * every quantity is reduced in fp64 in one fixed order: thread p takes elements (or rows) p, p + 256,
//     ... in increasing order, the 256 partials of all quantities go through LDS by one halving tree
//     (rs_tick_kernel's); no atomics, so an entry repeats bit for bit;
//   * thread 0 writes the entry to the slot the host chose (sequence number mod capacity).  The host
//     passes the step number and the flags as arguments: no device counter.
// The build compiles with -ffp-contract=off: no sum here is fused with the products by 0.5 / 1/(J*A).
#include "learner.h"

namespace td3 {
namespace {

constexpr int kLogThreads = 256;
constexpr int kLogMaxCap = 1 << 20;

// rows of the LDS partials: sums, then minima, then maxima
enum : int {
  kQ1, kQ2, kY, kGap, kBad, kAq, kS1, kS2, kTd, kW, kNumSum,
  kQMin = kNumSum, kYMin, kWMin, kNumMin,
  kQMax = kNumMin, kYMax, kTdMax, kNumAll
};

struct TrainLogArgs {
  const float* Y;        // [Bp][ldq]
  const float* Q1;       // [Bp][ldq]
  const float* Q2;       // [Bp][ldq]; null without a twin
  const float* sqerr;    // [2][Bp]
  const float* AQ;       // [Bp][ldq]; null on critic-only steps
  const float* W;        // [Bp]; null unless the step was prioritized
  td3_log_entry* out;    // the entry's slot
  int64_t step;
  double td_scale;       // 1 / (J * A)
  int B, Bp, nq, ldq;
};

__global__ __launch_bounds__(kLogThreads) void train_log_kernel(const TrainLogArgs a) {
  __shared__ double part[kNumAll][kLogThreads];
  const int p = threadIdx.x, B = a.B, nq = a.nq, n = B * nq;
  const bool twin = a.Q2 != nullptr, actor = a.AQ != nullptr, weighted = a.W != nullptr;
  // an absent input is read through a pointer that is valid anyway and its value dropped by a select, so
  // the loop bodies have no branch and the loads of the unrolled turns are issued together: a thread's
  // turns are otherwise a chain of load latencies, 48 of them at B = 4096, nq = 3.  The adds keep their
  // order; adding the 0.0 of an absent input changes no sum that is used.
  const float* Q2p = twin ? a.Q2 : a.Q1;
  const float* AQp = actor ? a.AQ : a.Q1;
  const float* Wp = weighted ? a.W : a.sqerr;
  const double inf = __builtin_huge_val();
  double q1s = 0.0, q2s = 0.0, ys = 0.0, gaps = 0.0, bad = 0.0, aqs = 0.0;
  double qmin = inf, ymin = inf, qmax = -inf, ymax = -inf;
#pragma unroll 8
  for (int e = p; e < n; e += kLogThreads) {
    const int r = e / nq, o = e - r * nq;
    const size_t k = (size_t)r * a.ldq + o;
    const double y = (double)a.Y[k], q1 = (double)a.Q1[k], q2 = (double)Q2p[k], aq = (double)AQp[k];
    q1s += q1;
    q2s += q2;
    ys += y;
    gaps += fabs(q1 - q2);
    bad += (double)((isfinite(y) ? 0 : 1) + (isfinite(q1) ? 0 : 1) + (twin && !isfinite(q2) ? 1 : 0));
    qmin = q1 < qmin ? q1 : qmin;
    qmin = q2 < qmin ? q2 : qmin;
    qmax = q1 > qmax ? q1 : qmax;
    qmax = q2 > qmax ? q2 : qmax;
    ymin = y < ymin ? y : ymin;
    ymax = y > ymax ? y : ymax;
    aqs += actor ? aq : 0.0;
  }
  double s1 = 0.0, s2 = 0.0, tds = 0.0, ws = 0.0, tdmax = -inf, wmin = inf;
#pragma unroll 4
  for (int r = p; r < B; r += kLogThreads) {
    const double e1 = (double)a.sqerr[r], e2 = (double)a.sqerr[(size_t)a.Bp + r], w = (double)Wp[r];
    s1 += e1;
    s2 += twin ? e2 : 0.0;
    const size_t k = (size_t)r * a.ldq;
    double t = 0.0, t2 = 0.0;
    for (int o = 0; o < nq; ++o) {
      const double y = (double)a.Y[k + o];
      t += fabs((double)a.Q1[k + o] - y);
      t2 += fabs((double)Q2p[k + o] - y);
    }
    t += twin ? t2 : 0.0;           // (t >= +0: adding 0.0 leaves its bits)
    t *= a.td_scale;
    tds += t;
    tdmax = t > tdmax ? t : tdmax;
    ws += w;
    wmin = w < wmin ? w : wmin;
  }
  part[kQ1][p] = q1s;
  part[kQ2][p] = q2s;
  part[kY][p] = ys;
  part[kGap][p] = gaps;
  part[kBad][p] = bad;
  part[kAq][p] = aqs;
  part[kS1][p] = s1;
  part[kS2][p] = s2;
  part[kTd][p] = tds;
  part[kW][p] = ws;
  part[kQMin][p] = qmin;
  part[kYMin][p] = ymin;
  part[kWMin][p] = wmin;
  part[kQMax][p] = qmax;
  part[kYMax][p] = ymax;
  part[kTdMax][p] = tdmax;
  for (int s = kLogThreads / 2; s >= 1; s >>= 1) {
    __syncthreads();
    if (p < s) {
#pragma unroll
      for (int i = 0; i < kNumSum; ++i) part[i][p] += part[i][p + s];
#pragma unroll
      for (int i = kNumSum; i < kNumMin; ++i)
        if (part[i][p + s] < part[i][p]) part[i][p] = part[i][p + s];
#pragma unroll
      for (int i = kNumMin; i < kNumAll; ++i)
        if (part[i][p + s] > part[i][p]) part[i][p] = part[i][p + s];
    }
  }
  if (p != 0) return;             // thread 0 wrote every part[i][0] last itself
  const double dn = (double)n, dB = (double)B;
  td3_log_entry e;
  e.step = a.step;
  e.batch = B;
  e.actor_step = actor ? 1 : 0;
  e.prioritized = weighted ? 1 : 0;
  e.nonfinite = (int32_t)part[kBad][0];           // exact: a count below 2^53
  e.critic_loss = twin ? part[kS1][0] / dn + part[kS2][0] / dn : part[kS1][0] / dn;
  e.actor_loss = actor ? -part[kAq][0] / dn : __builtin_nan("");
  e.q1_mean = part[kQ1][0] / dn;
  e.q2_mean = part[kQ2][0] / dn;
  e.y_mean = part[kY][0] / dn;
  e.q_min = part[kQMin][0];
  e.q_max = part[kQMax][0];
  e.y_min = part[kYMin][0];
  e.y_max = part[kYMax][0];
  e.q_gap_mean = part[kGap][0] / dn;
  e.td_abs_mean = part[kTd][0] / dB;
  e.td_abs_max = part[kTdMax][0];
  e.w_mean = weighted ? part[kW][0] / dB : 1.0;
  e.w_min = weighted ? part[kWMin][0] : 1.0;
  *a.out = e;
}

// Waits for the last log launch, wherever it was queued.
int wait_log(const TrainLog* L) {
  if (L->ev_recorded) TD3_HIP(hipEventSynchronize(L->ev));
  return 0;
}

}  // namespace

// One launch over the plan's buffers as they stand, into the slot of sequence number `seq`.
static int launch_log(const td3_handle* h, const TrainLog* L, int64_t seq, int64_t step, bool actor, bool prioritized,
                      hipStream_t s) {
  const Plan* P = h->plan.get();
  const bool twin = !P->particles || h->cdq;
  TrainLogArgs a{};
  a.Y = P->Y;
  a.Q1 = P->Q[0].Qv;
  a.Q2 = twin ? P->Q[1].Qv : nullptr;
  a.sqerr = P->sqerr;
  a.AQ = actor ? P->AQ.Qv : nullptr;
  a.W = prioritized ? P->per_w : nullptr;
  a.out = L->d + (seq % L->cap);
  a.step = step;
  a.td_scale = 1.0 / (double)((twin ? 2 : 1) * P->nq);
  a.B = P->B;
  a.Bp = P->Bp;
  a.nq = P->nq;
  a.ldq = P->ldq;
  hipLaunchKernelGGL(train_log_kernel, dim3(1), dim3(kLogThreads), 0, s, a);
  TD3_HIP(hipGetLastError());
  return 0;
}

int log_step(td3_handle* h, int actor_phase, bool prioritized, hipStream_t s) {
  TrainLog* L = h->log.get();
  TD3_RC(launch_log(h, L, L->count, h->total_it, actor_phase != 0, prioritized, s));
  L->count += 1;
  L->last_actor = actor_phase != 0;
  L->last_prioritized = prioritized;
  L->last_step = h->total_it;
  L->last_plan = h->plan.get();
  TD3_HIP(hipEventRecord(L->ev, s));
  L->ev_recorded = true;
  return 0;
}

void destroy_train_log(td3_handle* h) {
  TrainLog* L = h->log.get();
  if (!L) return;
  if (L->ev) {
    if (L->ev_recorded) (void)hipEventSynchronize(L->ev);   // a launch on a caller's stream may still write
    (void)hipEventDestroy(L->ev);
  }
  (void)hipFree(L->d);
  h->log.reset();
}

}  // namespace td3

using namespace td3;

extern "C" {

size_t td3_log_entry_size(void) { return sizeof(td3_log_entry); }

int td3_log_enable(td3_handle* h, int capacity, int every) {
  TD3_ARG(capacity >= 1 && capacity <= kLogMaxCap, "capacity must be in 1..2^20");
  TD3_ARG(every >= 1 && every <= kLogMaxCap, "every must be in 1..2^20");
  TD3_ARG(h != nullptr, "null handle");
  TD3_ARG(!h->log, "the training log is already enabled");
  TD3_ARG(!h->comm && !h->local,
          "td3_log_enable on a data-parallel handle (td3_comm_init / td3_comm_init_local group)");
  TD3_HIP(hipSetDevice(h->cfg.device));
  std::unique_ptr<TrainLog> L(new TrainLog());
  L->cap = capacity;
  L->every = every;
  const size_t bytes = sizeof(td3_log_entry) * (size_t)capacity;
  hipError_t e = hipMalloc(&L->d, bytes);
  if (e == hipSuccess) e = hipMemset(L->d, 0, bytes);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  // an ordering event (common.h TD3_EV_FLAGS): the entries are device memory written by a kernel, whose
  // end-of-kernel release makes them visible to the copy that reads them
  if (e == hipSuccess) e = hipEventCreateWithFlags(&L->ev, TD3_EV_FLAGS);
  if (e != hipSuccess) {
    set_error("td3_log_enable: %s", hipGetErrorString(e));
    (void)hipFree(L->d);
    return -2;
  }
  h->log = std::move(L);
  return 0;
}

int td3_log_info(const td3_handle* h, td3_log_info_t* info) {
  TD3_ARG(info != nullptr, "null info");
  TD3_ARG(h != nullptr, "null handle");
  const TrainLog* L = h->log.get();
  info->enabled = L ? 1 : 0;
  info->capacity = L ? L->cap : 0;
  info->every = L ? L->every : 0;
  info->count = L ? L->count : 0;
  return 0;
}

int td3_log_read(td3_handle* h, int64_t first, int64_t n, td3_log_entry* out, int64_t* first_out, int64_t* n_out) {
  TD3_ARG(first >= 0, "first must be >= 0");
  TD3_ARG(n >= 0, "n must be >= 0");
  TD3_ARG(out != nullptr || n == 0, "out is null");
  TD3_ARG(first_out != nullptr, "first_out is null");
  TD3_ARG(n_out != nullptr, "n_out is null");
  TD3_ARG(h != nullptr, "null handle");
  TD3_ARG(h->log != nullptr, "the training log is not enabled (td3_log_enable)");
  const TrainLog* L = h->log.get();
  const int64_t cap = L->cap, count = L->count;
  const int64_t oldest = std::max(count > cap ? count - cap : (int64_t)0, L->floor);
  const int64_t lo = first > oldest ? first : oldest;
  const int64_t want_hi = n > count - first ? count : first + n;   // first + n without overflow
  const int64_t cnt = want_hi > lo ? want_hi - lo : 0;
  *first_out = lo;
  *n_out = cnt;
  if (cnt == 0) return 0;
  TD3_HIP(hipSetDevice(h->cfg.device));
  TD3_RC(wait_log(L));
  const int64_t slot = lo % cap, head = cnt < cap - slot ? cnt : cap - slot;
  TD3_HIP(hipMemcpy(out, L->d + slot, sizeof(td3_log_entry) * (size_t)head, hipMemcpyDeviceToHost));
  if (cnt > head)
    TD3_HIP(hipMemcpy(out + head, L->d, sizeof(td3_log_entry) * (size_t)(cnt - head), hipMemcpyDeviceToHost));
  return 0;
}

int td3_log_set(td3_handle* h, const td3_log_entry* entries, int64_t n, int64_t count) {
  TD3_ARG(n >= 0, "n must be >= 0");
  TD3_ARG(entries != nullptr || n == 0, "entries is null");
  TD3_ARG(count >= n, "count must be >= n");
  TD3_ARG(h != nullptr, "null handle");
  TD3_ARG(h->log != nullptr, "the training log is not enabled (td3_log_enable)");
  TrainLog* L = h->log.get();
  TD3_ARG(n <= L->cap, "n must be <= capacity");
  TD3_HIP(hipSetDevice(h->cfg.device));
  TD3_RC(wait_log(L));
  if (n > 0) {
    const int64_t cap = L->cap, slot = (count - n) % cap, head = n < cap - slot ? n : cap - slot;
    TD3_HIP(hipMemcpy(L->d + slot, entries, sizeof(td3_log_entry) * (size_t)head, hipMemcpyHostToDevice));
    if (n > head)
      TD3_HIP(hipMemcpy(L->d, entries + head, sizeof(td3_log_entry) * (size_t)(n - head), hipMemcpyHostToDevice));
    TD3_HIP(hipDeviceSynchronize());
  }
  L->count = count;
  L->last_plan = nullptr;         // (td3_debug_log_launch: the last entry is no longer the last step's)
  L->floor = count - n;           // older slots hold whatever they held: not part of the log any more
  return 0;
}

int td3_debug_log_launch(td3_handle* h, void* stream) {
  TD3_ARG(h != nullptr, "null handle");
  TD3_ARG(h->log != nullptr, "the training log is not enabled (td3_log_enable)");
  TrainLog* L = h->log.get();
  TD3_ARG(L->count > 0 && L->last_plan == h->plan.get() && L->last_step == h->total_it,
          "log a step first (the plan's buffers hold its rows)");
  TD3_HIP(hipSetDevice(h->cfg.device));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  TD3_RC(launch_log(h, L, L->count - 1, L->last_step, L->last_actor, L->last_prioritized, s));
  TD3_HIP(hipEventRecord(L->ev, s));
  return 0;
}

}  // extern "C"
