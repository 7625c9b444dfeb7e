// Rollout statistics (include/td3.h, "rollout statistics"): running observation / return moments,
// normalisation and the episode log of a GPU-resident vector environment, one launch per tick.
//
// rs_tick_kernel, 1024 threads per workgroup, no workgroup waits on another:
//   * workgroup b < ncol owns observation columns [W b, W b + W).  Thread t is lane c = t mod W of row
//     phase p = t / W (P = 1024 / W phases): it sums its column over rows p, p + P, ... in fp64, in row
//     order; the P partials of a column are combined by a halving tree through LDS (partial p += partial
//     p + s for s = P/2, P/4, ..., 1).  W (rs_col_width) is the largest power of two <= 64 that leaves a
//     phase at most 8 rows (rows * W <= 8192), so a tall, narrow batch is spread over many workgroups
//     and a wide one reads 256-byte row segments.  The order is a function of (rows, obs_dim) alone and
//     there are no atomics, so results repeat bit for bit.  The
//     same threads then normalise the same columns of obs and next_obs, so an output may alias its input:
//     every read of a column by the reduction is behind a barrier before its first write.
//   * workgroup ncol (launched only when a reward is given) does the return moments, the reward
//     scaling and the episode bookkeeping over the rows; the row-ordered log slots come from a ballot
//     prefix count over `ended`.
// `count` is kept once per column workgroup (all copies equal) so that no workgroup reads a word another
// one writes in the same launch.
#include "rollout.h"

#include <cmath>
#include <new>
#include <vector>

namespace td3 {
namespace {

constexpr int kRsThreads = 1024;
constexpr int kRsMaxWidth = 64;
constexpr int kRsMaxLog = 1 << 24;

struct RsArgs {
  double* count_blk;   // [ncol]
  double* mean;        // [obs_dim]
  double* m2;          // [obs_dim]
  const uint8_t* mask; // [obs_dim]
  double* rscal;       // ret_count, ret_mean, ret_m2, ep_return_sum
  int64_t* iscal;      // ep_count, ep_len_sum, tick
  double* G;           // [rows]
  double* ep_return;   // [rows]
  int32_t* ep_len;     // [rows]
  rs_episode* log;     // [log_cap]
  const float* obs;
  const float* next_obs;
  const float* reward;
  const uint8_t* ended;
  float* obs_out;
  float* next_obs_out;
  float* reward_out;
  int rows, obs_dim, log_cap, ncol, W, update;
  double obs_eps, obs_clip, rew_eps, rew_clip, gamma;
};

// Sum of v over the threads t = c (mod W), returned to all of them: a halving tree in LDS, fixed order.
__device__ __forceinline__ double tree_sum(double* part, double v, int tid, int c, int W) {
  __syncthreads();                                  // earlier readers of part[] are done
  part[tid] = v;
  for (int s = kRsThreads / 2; s >= W; s >>= 1) {
    __syncthreads();
    if (tid < s) part[tid] += part[tid + s];
  }
  __syncthreads();
  return part[c];
}

__device__ __forceinline__ void normalise_cols(const float* in, float* out, int rows, int D, int col, int p, int P,
                                               bool on, double mean, double den, double lim) {
  if (!on) {                                        // masked column, or no moments yet: bit for bit
    if (out != in)
      for (int r = p; r < rows; r += P) out[(size_t)r * D + col] = in[(size_t)r * D + col];
    return;
  }
#pragma unroll 4
  for (int r = p; r < rows; r += P) {
    const size_t k = (size_t)r * D + col;
    out[k] = norm_elem(in[k], mean, den, lim);
  }
}

__device__ void rs_columns(const RsArgs& a, double* part) {
  const int tid = threadIdx.x, W = a.W, P = kRsThreads / W, c = tid & (W - 1), p = tid / W;
  const int blk = blockIdx.x, col = blk * W + c, rows = a.rows, D = a.obs_dim;
  const bool live = col < D;
  const bool on = live && a.mask[col] != 0;
  double cnt = a.count_blk[blk], mean = 0.0, m2 = 0.0;
  if (on) {
    mean = a.mean[col];
    m2 = a.m2[col];
  }
  if (a.update && a.obs) {                          // uniform over the launch
    double s = 0.0;
    if (on) {
#pragma unroll 8
      for (int r = p; r < rows; r += P) s += (double)a.obs[(size_t)r * D + col];
    }
    const double mb = tree_sum(part, s, tid, c, W) / (double)rows;
    double q = 0.0;
    if (on) {
#pragma unroll 8
      for (int r = p; r < rows; r += P) {
        const double d = (double)a.obs[(size_t)r * D + col] - mb;
        q += d * d;
      }
    }
    const double m2b = tree_sum(part, q, tid, c, W);
    chan_merge(cnt, mean, m2, (double)rows, mb, m2b);
    if (on && p == 0) {
      a.mean[col] = mean;
      a.m2[col] = m2;
    }
    if (tid == 0) a.count_blk[blk] = cnt;
  }
  if (!live) return;
  const bool norm = on && cnt > 0.0;
  const double den = norm ? norm_den(m2, cnt, a.obs_eps) : 1.0;
  if (a.obs && a.obs_out) normalise_cols(a.obs, a.obs_out, rows, D, col, p, P, norm, mean, den, a.obs_clip);
  if (a.next_obs && a.next_obs_out)
    normalise_cols(a.next_obs, a.next_obs_out, rows, D, col, p, P, norm, mean, den, a.obs_clip);
}

__device__ void rs_rewards(const RsArgs& a, double* part, int* wave_cnt) {
  const int tid = threadIdx.x, rows = a.rows;
  double rc = a.rscal[0], rm = a.rscal[1], rq = a.rscal[2];
  // row i belongs to thread i mod 1024 in every pass below
  double s = 0.0;
  for (int i = tid; i < rows; i += kRsThreads) {
    const double g = a.gamma * a.G[i] + (double)a.reward[i];
    a.G[i] = g;
    s += g;
  }
  if (a.update) {
    const double mb = tree_sum(part, s, tid, 0, 1) / (double)rows;
    double q = 0.0;
    for (int i = tid; i < rows; i += kRsThreads) {
      const double d = a.G[i] - mb;
      q += d * d;
    }
    const double m2b = tree_sum(part, q, tid, 0, 1);
    chan_merge(rc, rm, rq, (double)rows, mb, m2b);
    if (tid == 0) {
      a.rscal[0] = rc;
      a.rscal[1] = rm;
      a.rscal[2] = rq;
    }
  }
  const bool scale = rc > 0.0;
  const double den = scale ? sqrt(rq / rc + a.rew_eps) : 1.0;
  int ne = 0;
  for (int i = tid; i < rows; i += kRsThreads) {
    const float r = a.reward[i];
    a.ep_return[i] += (double)r;
    a.ep_len[i] += 1;
    if (a.ended && a.ended[i]) {
      a.G[i] = 0.0;
      ++ne;
    }
    if (a.reward_out) a.reward_out[i] = scale ? (float)clipd((double)r / den, a.rew_clip) : r;
  }
  const int64_t total = (int64_t)tree_sum(part, (double)ne, tid, 0, 1);   // exact: below 2^53
  const int64_t ep0 = a.iscal[0], tick = a.iscal[2];
  if (total > 0) {                                  // uniform
    const int lane = tid & 63, w = tid >> 6;
    int64_t run = 0, lens = 0;
    double rsum = a.rscal[3];
    for (int base = 0; base < rows; base += kRsThreads) {
      const int i = base + tid;
      const bool e = i < rows && a.ended[i] != 0;
      const unsigned long long b = __ballot(e);
      if (lane == 0) wave_cnt[w] = __popcll(b);
      __syncthreads();
      int before = __popcll(b & ((1ull << lane) - 1ull)), chunk = 0;
      for (int j = 0; j < kRsThreads / 64; ++j) {
        const int v = wave_cnt[j];
        if (j < w) before += v;
        chunk += v;
      }
      if (e) {
        const int64_t k = run + before;             // this episode's place among the tick's ends, row order
        const double ret = a.ep_return[i];
        const int32_t len = a.ep_len[i];
        if (total - 1 - k < (int64_t)a.log_cap)     // a slot written twice in one tick keeps the later row
          a.log[(ep0 + k) % a.log_cap] = rs_episode{(float)ret, len, (int32_t)i, 0, tick};
        part[before] = ret;
        lens += len;
        a.ep_return[i] = 0.0;
        a.ep_len[i] = 0;
      }
      __syncthreads();
      if (tid == 0) {                               // the return sum is added in row order, as the log is
#pragma unroll 8
        for (int j = 0; j < chunk; ++j) rsum += part[j];
      }
      run += chunk;
      __syncthreads();
    }
    const int64_t len_total = (int64_t)tree_sum(part, (double)lens, tid, 0, 1);
    if (tid == 0) {
      a.iscal[0] = ep0 + total;
      a.iscal[1] += len_total;
      a.rscal[3] = rsum;
    }
  }
  if (tid == 0) a.iscal[2] = tick + 1;
}

__global__ __launch_bounds__(kRsThreads) void rs_tick_kernel(const RsArgs a) {
  __shared__ double part[kRsThreads];
  __shared__ int wave_cnt[kRsThreads / 64];
  if ((int)blockIdx.x < a.ncol)
    rs_columns(a, part);
  else
    rs_rewards(a, part, wave_cnt);
}

inline size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

// Columns per workgroup: a power of two, at most 64, at most 8 rows per row phase (rows * W <= 8192)
// and no wider than the power of two that covers obs_dim.
int rs_col_width(int rows, int obs_dim) {
  int W = kRsMaxWidth;
  while (W > 1 && (int64_t)rows * W > 8192) W >>= 1;
  while (W > 1 && W / 2 >= obs_dim) W >>= 1;
  return W;
}

bool finite_ge0(double x) { return std::isfinite(x) && x >= 0.0; }
bool finite_gt0(double x) { return std::isfinite(x) && x > 0.0; }

int check_state_ptrs(const rs_state* st) {
  TD3_ARG(st != nullptr, "null st");
  TD3_ARG(st->mean != nullptr, "st->mean is null");
  TD3_ARG(st->m2 != nullptr, "st->m2 is null");
  TD3_ARG(st->G != nullptr, "st->G is null");
  TD3_ARG(st->ep_return != nullptr, "st->ep_return is null");
  TD3_ARG(st->ep_len != nullptr, "st->ep_len is null");
  TD3_ARG(st->log != nullptr, "st->log is null");
  return 0;
}

}  // namespace
}  // namespace td3

using namespace td3;

extern "C" {

int rs_create(int rows, int obs_dim, int log_cap, int device, const rs_config* cfg, rs_handle** out) {
  TD3_ARG(out != nullptr, "out is null");
  TD3_ARG(rows > 0 && rows <= (1 << 24), "rows must be in 1..2^24");
  TD3_ARG(obs_dim > 0 && obs_dim <= (1 << 20), "obs_dim must be in 1..2^20");
  TD3_ARG(log_cap > 0 && log_cap <= kRsMaxLog, "log_cap must be in 1..2^24");
  TD3_ARG(cfg != nullptr, "null cfg");
  TD3_ARG(finite_ge0(cfg->obs_eps), "cfg->obs_eps must be finite and >= 0");
  TD3_ARG(finite_gt0(cfg->obs_clip), "cfg->obs_clip must be finite and > 0");
  TD3_ARG(finite_ge0(cfg->rew_eps), "cfg->rew_eps must be finite and >= 0");
  TD3_ARG(finite_gt0(cfg->rew_clip), "cfg->rew_clip must be finite and > 0");
  TD3_ARG(cfg->gamma >= 0.0 && cfg->gamma <= 1.0, "cfg->gamma must be in [0, 1]");
  TD3_HIP(hipSetDevice(device));
  Stats* s = new (std::nothrow) Stats;
  TD3_ARG(s != nullptr, "out of host memory");
  s->device = device;
  s->rows = rows;
  s->obs_dim = obs_dim;
  s->log_cap = log_cap;
  s->cfg = *cfg;
  s->cfg.col_mask = nullptr;                        // the caller's array is read during this call only
  s->W = rs_col_width(rows, obs_dim);
  s->ncol = (obs_dim + s->W - 1) / s->W;
  const size_t R = (size_t)rows, D = (size_t)obs_dim;
  size_t off = 0;
  auto take = [&off](size_t bytes) {
    const size_t o = off;
    off += up16(bytes);
    return o;
  };
  const size_t o_cnt = take(8 * (size_t)s->ncol), o_mean = take(8 * D), o_m2 = take(8 * D), o_rs = take(8 * 4),
               o_is = take(8 * 3), o_G = take(8 * R), o_er = take(8 * R), o_el = take(4 * R),
               o_log = take(sizeof(rs_episode) * (size_t)log_cap), o_mask = take(D);
  hipError_t e = hipMalloc(&s->base, off);
  if (e == hipSuccess) e = hipMemset(s->base, 0, off);
  std::vector<uint8_t> mask(D, 1);
  if (cfg->col_mask)
    for (size_t j = 0; j < D; ++j) mask[j] = cfg->col_mask[j] ? 1 : 0;
  char* b = static_cast<char*>(s->base);
  if (e == hipSuccess) e = hipMemcpy(b + o_mask, mask.data(), D, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    set_error("rs_create: %s", hipGetErrorString(e));
    (void)hipFree(s->base);
    delete s;
    return -2;
  }
  s->count_blk = reinterpret_cast<double*>(b + o_cnt);
  s->mean = reinterpret_cast<double*>(b + o_mean);
  s->m2 = reinterpret_cast<double*>(b + o_m2);
  s->rscal = reinterpret_cast<double*>(b + o_rs);
  s->iscal = reinterpret_cast<int64_t*>(b + o_is);
  s->G = reinterpret_cast<double*>(b + o_G);
  s->ep_return = reinterpret_cast<double*>(b + o_er);
  s->ep_len = reinterpret_cast<int32_t*>(b + o_el);
  s->log = reinterpret_cast<rs_episode*>(b + o_log);
  s->mask = reinterpret_cast<uint8_t*>(b + o_mask);
  *out = reinterpret_cast<rs_handle*>(s);
  return 0;
}

int rs_destroy(rs_handle* h) {
  if (!h) return 0;
  Stats* s = reinterpret_cast<Stats*>(h);
  (void)hipSetDevice(s->device);
  (void)hipDeviceSynchronize();                     // no tick still in flight, whatever stream it was queued on
  (void)hipFree(s->base);
  delete s;
  return 0;
}

int rs_tick(rs_handle* h, const rs_tick_t* a, void* stream) {
  TD3_ARG(a != nullptr, "null a");
  TD3_ARG(a->update == 0 || a->update == 1, "a->update must be 0 or 1");
  TD3_ARG(a->obs_out == nullptr || a->obs != nullptr, "a->obs_out given without a->obs");
  TD3_ARG(a->next_obs_out == nullptr || a->next_obs != nullptr, "a->next_obs_out given without a->next_obs");
  TD3_ARG(a->reward_out == nullptr || a->reward != nullptr, "a->reward_out given without a->reward");
  TD3_ARG(a->ended == nullptr || a->reward != nullptr, "a->ended given without a->reward");
  TD3_ARG(h != nullptr, "null handle");
  Stats* s = reinterpret_cast<Stats*>(h);
  const int ncol = (a->obs || a->next_obs) ? s->ncol : 0;
  const int grid = ncol + (a->reward ? 1 : 0);
  if (grid == 0) return 0;                          // nothing given: nothing changes
  RsArgs k{};
  k.count_blk = s->count_blk;
  k.mean = s->mean;
  k.m2 = s->m2;
  k.mask = s->mask;
  k.rscal = s->rscal;
  k.iscal = s->iscal;
  k.G = s->G;
  k.ep_return = s->ep_return;
  k.ep_len = s->ep_len;
  k.log = s->log;
  k.obs = a->obs;
  k.next_obs = a->next_obs;
  k.reward = a->reward;
  k.ended = a->ended;
  k.obs_out = a->obs_out;
  k.next_obs_out = a->next_obs_out;
  k.reward_out = a->reward_out;
  k.rows = s->rows;
  k.obs_dim = s->obs_dim;
  k.log_cap = s->log_cap;
  k.ncol = ncol;
  k.W = s->W;
  k.update = a->update;
  k.obs_eps = s->cfg.obs_eps;
  k.obs_clip = s->cfg.obs_clip;
  k.rew_eps = s->cfg.rew_eps;
  k.rew_clip = s->cfg.rew_clip;
  k.gamma = s->cfg.gamma;
  TD3_HIP(hipSetDevice(s->device));
  hipStream_t st = static_cast<hipStream_t>(stream);   // NULL: HIP's default stream (torch's default too)
  hipLaunchKernelGGL(rs_tick_kernel, dim3(grid), dim3(kRsThreads), 0, st, k);   // the tick's one launch
  TD3_HIP(hipGetLastError());
  return 0;
}

int rs_info(const rs_handle* h, rs_info_t* info) {
  TD3_ARG(info != nullptr, "null info");
  TD3_ARG(h != nullptr, "null handle");
  const Stats* s = reinterpret_cast<const Stats*>(h);
  TD3_HIP(hipSetDevice(s->device));
  TD3_HIP(hipDeviceSynchronize());
  double rs[4];
  int64_t is[3];
  TD3_HIP(hipMemcpy(rs, s->rscal, sizeof rs, hipMemcpyDeviceToHost));
  TD3_HIP(hipMemcpy(is, s->iscal, sizeof is, hipMemcpyDeviceToHost));
  TD3_HIP(hipMemcpy(&info->count, s->count_blk, 8, hipMemcpyDeviceToHost));
  info->rows = s->rows;
  info->obs_dim = s->obs_dim;
  info->log_cap = s->log_cap;
  info->device = s->device;
  info->ret_count = rs[0];
  info->ep_return_sum = rs[3];
  info->ep_count = is[0];
  info->ep_len_sum = is[1];
  info->tick = is[2];
  return 0;
}

int rs_get_state(const rs_handle* h, rs_state* st) {
  TD3_RC(check_state_ptrs(st));
  TD3_ARG(h != nullptr, "null handle");
  const Stats* s = reinterpret_cast<const Stats*>(h);
  TD3_HIP(hipSetDevice(s->device));
  TD3_HIP(hipDeviceSynchronize());
  const size_t R = (size_t)s->rows, D = (size_t)s->obs_dim;
  double rs[4];
  int64_t is[3];
  TD3_HIP(hipMemcpy(rs, s->rscal, sizeof rs, hipMemcpyDeviceToHost));
  TD3_HIP(hipMemcpy(is, s->iscal, sizeof is, hipMemcpyDeviceToHost));
  TD3_HIP(hipMemcpy(&st->count, s->count_blk, 8, hipMemcpyDeviceToHost));
  TD3_HIP(hipMemcpy(st->mean, s->mean, 8 * D, hipMemcpyDeviceToHost));
  TD3_HIP(hipMemcpy(st->m2, s->m2, 8 * D, hipMemcpyDeviceToHost));
  TD3_HIP(hipMemcpy(st->G, s->G, 8 * R, hipMemcpyDeviceToHost));
  TD3_HIP(hipMemcpy(st->ep_return, s->ep_return, 8 * R, hipMemcpyDeviceToHost));
  TD3_HIP(hipMemcpy(st->ep_len, s->ep_len, 4 * R, hipMemcpyDeviceToHost));
  TD3_HIP(hipMemcpy(st->log, s->log, sizeof(rs_episode) * (size_t)s->log_cap, hipMemcpyDeviceToHost));
  st->ret_count = rs[0];
  st->ret_mean = rs[1];
  st->ret_m2 = rs[2];
  st->ep_return_sum = rs[3];
  st->ep_count = is[0];
  st->ep_len_sum = is[1];
  st->tick = is[2];
  return 0;
}

int rs_set_state(rs_handle* h, const rs_state* st) {
  TD3_RC(check_state_ptrs(st));
  TD3_ARG(finite_ge0(st->count), "st->count must be finite and >= 0");
  TD3_ARG(finite_ge0(st->ret_count), "st->ret_count must be finite and >= 0");
  TD3_ARG(st->ep_count >= 0, "st->ep_count must be >= 0");
  TD3_ARG(st->ep_len_sum >= 0, "st->ep_len_sum must be >= 0");
  TD3_ARG(st->tick >= 0, "st->tick must be >= 0");
  TD3_ARG(h != nullptr, "null handle");
  Stats* s = reinterpret_cast<Stats*>(h);
  TD3_HIP(hipSetDevice(s->device));
  TD3_HIP(hipDeviceSynchronize());
  const size_t R = (size_t)s->rows, D = (size_t)s->obs_dim;
  const double rs[4] = {st->ret_count, st->ret_mean, st->ret_m2, st->ep_return_sum};
  const int64_t is[3] = {st->ep_count, st->ep_len_sum, st->tick};
  const std::vector<double> cnt((size_t)s->ncol, st->count);
  TD3_HIP(hipMemcpy(s->rscal, rs, sizeof rs, hipMemcpyHostToDevice));
  TD3_HIP(hipMemcpy(s->iscal, is, sizeof is, hipMemcpyHostToDevice));
  TD3_HIP(hipMemcpy(s->count_blk, cnt.data(), 8 * cnt.size(), hipMemcpyHostToDevice));
  TD3_HIP(hipMemcpy(s->mean, st->mean, 8 * D, hipMemcpyHostToDevice));
  TD3_HIP(hipMemcpy(s->m2, st->m2, 8 * D, hipMemcpyHostToDevice));
  TD3_HIP(hipMemcpy(s->G, st->G, 8 * R, hipMemcpyHostToDevice));
  TD3_HIP(hipMemcpy(s->ep_return, st->ep_return, 8 * R, hipMemcpyHostToDevice));
  TD3_HIP(hipMemcpy(s->ep_len, st->ep_len, 4 * R, hipMemcpyHostToDevice));
  TD3_HIP(hipMemcpy(s->log, st->log, sizeof(rs_episode) * (size_t)s->log_cap, hipMemcpyHostToDevice));
  TD3_HIP(hipDeviceSynchronize());
  return 0;
}

int rs_read_episodes(const rs_handle* h, int64_t first, int64_t n, rs_episode* out, int64_t* first_out,
                     int64_t* n_out) {
  TD3_ARG(first >= 0, "first must be >= 0");
  TD3_ARG(n >= 0, "n must be >= 0");
  TD3_ARG(out != nullptr || n == 0, "out is null");
  TD3_ARG(first_out != nullptr, "first_out is null");
  TD3_ARG(n_out != nullptr, "n_out is null");
  TD3_ARG(h != nullptr, "null handle");
  const Stats* s = reinterpret_cast<const Stats*>(h);
  TD3_HIP(hipSetDevice(s->device));
  TD3_HIP(hipDeviceSynchronize());
  int64_t ep_count = 0;
  TD3_HIP(hipMemcpy(&ep_count, s->iscal, 8, hipMemcpyDeviceToHost));
  const int64_t cap = s->log_cap, oldest = ep_count > cap ? ep_count - cap : 0;
  const int64_t lo = first > oldest ? first : oldest;
  const int64_t want_hi = n > ep_count - first ? ep_count : first + n;   // first + n without overflow
  const int64_t cnt = want_hi > lo ? want_hi - lo : 0;
  *first_out = lo;
  *n_out = cnt;
  if (cnt == 0) return 0;
  const int64_t slot = lo % cap, head = cnt < cap - slot ? cnt : cap - slot;
  TD3_HIP(hipMemcpy(out, s->log + slot, sizeof(rs_episode) * (size_t)head, hipMemcpyDeviceToHost));
  if (cnt > head)
    TD3_HIP(hipMemcpy(out + head, s->log, sizeof(rs_episode) * (size_t)(cnt - head), hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
