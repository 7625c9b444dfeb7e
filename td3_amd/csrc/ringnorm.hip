// Dataset normalisation of a replay ring (include/td3.h, "dataset normalisation"): the fp64 moments of
// the ring's field 0 (state / features) into an rs_handle's observation moments, and the in-place
// normalisation of field 0 and its next-state twin with those moments -- the element expression of
// rs_tick step 2 (rollout.h norm_den / norm_elem), so a row normalised here and a row normalised by a
// tick have the same bits.
//
// rb_state_moments is two launches, no float atomics, no workgroup waiting on another:
//   nm_sweep_kernel   one workgroup per (row chunk, block of 256 columns).  A chunk is kNmChunk = 1024
//       consecutive ring rows, cut into micro-blocks of kNmMicro = 8 rows.  The rows are staged in LDS tile
//       by tile with 16-byte loads: whole records where the gap between two rows' field 0 is under one
//       128-byte line (every line of the ring is fetched anyway, and the read is one contiguous stream),
//       else only the field's own columns (a Humanoid record is half next-state, a particle record almost
//       all particles: those lines are never requested).  Thread (c, p) of the W x P = 256 threads (W the
//       power of two covering the block's columns) owns column c and the micro-blocks m = p (mod P) of the
//       chunk: per micro-block the sum in row order, mb = sum / rows, m2b = sum (x - mb)^2 in row order,
//       Chan-merged into the thread's partial in ascending m; the P partials of a column are then merged
//       by a halving tree (p takes p + s, s = P/2, ..., 1).  A partial's first block is taken as it is.
//   nm_merge_kernel   one wave per column: lane l merges the chunk partials l, l + 64, ... in ascending
//       order, the 64 lanes by the same halving tree; lane 0 replaces the handle's moments or merges
//       into them with rollout.h chan_merge, and workgroup 0 sets every count copy.
// The grouping depends on (size, obs_dim) alone -- not on the grid, the tile height or the record
// width -- so runs repeat bit for bit.
//
// rb_normalize_states is one launch: a thread owns one 16-byte unit of the record (fixed for the launch:
// its columns' mean and denominator stay in registers) and walks the rows, load - normalise - store.
// Only the units that hold a column of the two fields are touched.
#include "replay.h"
#include "rollout.h"

#include <algorithm>

namespace td3 {
namespace {

constexpr int kNmChunk = 1024;       // rows per chunk (rb_state_moments' documented row chunk)
constexpr int kNmMicro = 8;          // rows per micro-block
constexpr int kNmThreads = 256;
constexpr int kNmColBlock = 256;     // columns per workgroup
constexpr int kNmLdsFloats = 8192;   // the staged tile

struct NmSweepArgs {
  const float* data;
  const uint8_t* mask;
  const double* count_blk;
  double* part;            // [nchunk][sd] {mean, m2}
  double* old_count;       // the handle's count as it was before the call (read by nm_merge_kernel)
  int64_t size, nchunk;
  int rec, sd, whole;
};

// Merge partial b into a (either may be empty).
__device__ __forceinline__ void nm_merge(double& cnt, double& mean, double& m2, double nb, double mb, double qb) {
  if (nb == 0.0) return;
  if (cnt == 0.0) {
    cnt = nb;
    mean = mb;
    m2 = qb;
    return;
  }
  chan_merge(cnt, mean, m2, nb, mb, qb);
}

__global__ __launch_bounds__(kNmThreads) void nm_sweep_kernel(const NmSweepArgs a) {
  __shared__ float4 tile4[kNmLdsFloats / 4];
  float* tile = reinterpret_cast<float*>(tile4);
  double* red = reinterpret_cast<double*>(tile4);              // [3][256] after the last tile of a chunk
  const int tid = threadIdx.x;
  const int c0 = blockIdx.y * kNmColBlock, cw = min(kNmColBlock, a.sd - c0);
  int W = 1, sh = 0;
  while (W < cw) {
    W <<= 1;
    ++sh;
  }
  const int P = kNmThreads >> sh, c = tid & (W - 1), p = tid >> sh, col = c0 + c;
  const bool on = c < cw && a.mask[col] != 0;
  const int stride = a.whole ? a.rec : pad4(cw), seg4 = stride >> 2, rec4 = a.rec >> 2;
  const int coff4 = a.whole ? 0 : (c0 >> 2), lcol = a.whole ? col : c;
  const int T = min(kNmChunk, (kNmLdsFloats / stride) & ~(kNmMicro - 1));
  const float4* src4 = reinterpret_cast<const float4*>(a.data);
  if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) *a.old_count = a.count_blk[0];
  for (int64_t chunk = blockIdx.x; chunk < a.nchunk; chunk += gridDim.x) {
    const int64_t r0 = chunk * kNmChunk;
    const int nr = (int)min((int64_t)kNmChunk, a.size - r0);
    double cnt = 0.0, mean = 0.0, m2 = 0.0;
    for (int t0 = 0; t0 < nr; t0 += T) {
      const int tr = min(T, nr - t0), n4 = tr * seg4;
      const float4* base = src4 + (r0 + t0) * rec4 + coff4;
#pragma unroll 4
      for (int i = tid; i < n4; i += kNmThreads) {
        const int row = i / seg4, q = i - row * seg4;
        tile4[i] = a.whole ? base[i] : base[(int64_t)row * rec4 + q];
      }
      __syncthreads();
      if (on) {
        const int nmb = (tr + kNmMicro - 1) / kNmMicro, m0 = t0 / kNmMicro;
        for (int j = ((p - m0) % P + P) % P; j < nmb; j += P) {
          const int nb = min(kNmMicro, tr - j * kNmMicro);
          const float* x = tile + (size_t)j * kNmMicro * stride + lcol;
          double s = 0.0;
          for (int i = 0; i < nb; ++i) s += (double)x[i * stride];
          const double mb = s / (double)nb;
          double q = 0.0;
          for (int i = 0; i < nb; ++i) {
            const double d = (double)x[i * stride] - mb;
            q += d * d;
          }
          nm_merge(cnt, mean, m2, (double)nb, mb, q);
        }
      }
      __syncthreads();                                          // the tile is staged again, or reused below
    }
    red[tid] = cnt;
    red[kNmThreads + tid] = mean;
    red[2 * kNmThreads + tid] = m2;
    for (int s = kNmThreads / 2; s >= W; s >>= 1) {
      __syncthreads();
      if (tid < s) {
        double ca = red[tid], ma = red[kNmThreads + tid], qa = red[2 * kNmThreads + tid];
        nm_merge(ca, ma, qa, red[tid + s], red[kNmThreads + tid + s], red[2 * kNmThreads + tid + s]);
        red[tid] = ca;
        red[kNmThreads + tid] = ma;
        red[2 * kNmThreads + tid] = qa;
      }
    }
    __syncthreads();
    if (on && p == 0) {
      double* o = a.part + ((size_t)chunk * a.sd + col) * 2;
      o[0] = red[kNmThreads + tid];
      o[1] = red[2 * kNmThreads + tid];
    }
    __syncthreads();                                            // red[] is the next chunk's tile
  }
}

struct NmMergeArgs {
  const double* part;
  const double* old_count;
  const uint8_t* mask;
  double* count_blk;
  double* mean;
  double* m2;
  int64_t size, nchunk;
  int sd, ncount, merge;
};

__global__ __launch_bounds__(kNmThreads) void nm_merge_kernel(const NmMergeArgs a) {
  const int lane = threadIdx.x & 63, col = blockIdx.x * (kNmThreads / 64) + (threadIdx.x >> 6);
  const double old = *a.old_count;
  if (blockIdx.x == 0)
    for (int i = threadIdx.x; i < a.ncount; i += kNmThreads) a.count_blk[i] = a.merge ? old + (double)a.size : (double)a.size;
  if (col >= a.sd || a.mask[col] == 0) return;                  // uniform over the wave
  double cnt = 0.0, mean = 0.0, m2 = 0.0;
  for (int64_t k = lane; k < a.nchunk; k += 64) {
    const double nk = (double)min((int64_t)kNmChunk, a.size - k * kNmChunk);
    const double* pk = a.part + ((size_t)k * a.sd + col) * 2;
    nm_merge(cnt, mean, m2, nk, pk[0], pk[1]);
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    const double cb = __shfl_down(cnt, s, 64), mb = __shfl_down(mean, s, 64), qb = __shfl_down(m2, s, 64);
    if (lane < s) nm_merge(cnt, mean, m2, cb, mb, qb);
  }
  if (lane != 0) return;
  if (a.merge) {
    double c = old, m = a.mean[col], q = a.m2[col];
    chan_merge(c, m, q, cnt, mean, m2);
    mean = m;
    m2 = q;
  }
  a.mean[col] = mean;
  a.m2[col] = m2;
}

struct NmApplyArgs {
  float4* data;
  const double* count_blk;
  const double* mean;
  const double* m2;
  const uint8_t* mask;
  int64_t size;
  int rec4, sd, o_s2, nA, u2, nU, UW, ush;   // units [0, nA) hold field 0, [u2, u2 + nU - nA) the rest of its twin
  double eps, clip;
};

__global__ __launch_bounds__(kNmThreads) void nm_apply_kernel(const NmApplyArgs a) {
  const int tid = threadIdx.x, ui = blockIdx.y * a.UW + (tid & (a.UW - 1)), rp = tid >> a.ush, RP = kNmThreads >> a.ush;
  if (ui >= a.nU) return;
  const int unit = ui < a.nA ? ui : a.u2 + (ui - a.nA);
  const double cnt = a.count_blk[0];
  bool on[4], any = false;
  double mean[4], den[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c = unit * 4 + q;
    const int col = c < a.sd ? c : (c >= a.o_s2 && c < a.o_s2 + a.sd ? c - a.o_s2 : -1);
    on[q] = col >= 0 && cnt > 0.0 && a.mask[col] != 0;
    mean[q] = on[q] ? a.mean[col] : 0.0;
    den[q] = on[q] ? norm_den(a.m2[col], cnt, a.eps) : 1.0;
    any = any || on[q];
  }
  if (!any) return;                                             // masked, or no moments: bit for bit
  for (int64_t row = (int64_t)blockIdx.x * RP + rp; row < a.size; row += (int64_t)gridDim.x * RP) {
    float4* at = a.data + row * a.rec4 + unit;
    const float4 v = *at;
    float w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (on[q]) w[q] = norm_elem(w[q], mean[q], den[q], a.clip);
    *at = make_float4(w[0], w[1], w[2], w[3]);
  }
}

// The checks the two calls share, in the header's order (rb_normalize_states has no merge to check).
int norm_args(const rb_handle* rb, const rs_handle* rs, bool has_merge, int merge) {
  TD3_ARG(rb != nullptr, "null rb");
  TD3_ARG(rs != nullptr, "null rs");
  TD3_ARG(!has_merge || merge == 0 || merge == 1, "merge must be 0 or 1");
  const Ring* r = reinterpret_cast<const Ring*>(rb);
  const Stats* s = reinterpret_cast<const Stats*>(rs);
  TD3_ARG(s->obs_dim == r->sd, "dims: the statistics' obs_dim is not the ring's state (feature) width");
  TD3_ARG(s->device == r->device, "the statistics live on another device than the ring");
  TD3_ARG(r->size > 0, "empty ring");
  return 0;
}

}  // namespace
}  // namespace td3

using namespace td3;

extern "C" {

int rb_state_moments(rb_handle* rb, rs_handle* rs, int merge, void* stream) {
  TD3_RC(norm_args(rb, rs, true, merge));
  Ring* r = reinterpret_cast<Ring*>(rb);
  Stats* s = reinterpret_cast<Stats*>(rs);
  TD3_HIP(hipSetDevice(r->device));
  const int64_t nchunk = (r->size + kNmChunk - 1) / kNmChunk;
  const size_t need = (size_t)nchunk * r->sd * 2 + 2;
  if (need > r->nm_cap) {                                       // hipFree waits for the launches that still use it
    (void)hipFree(r->nm_part);
    r->nm_part = nullptr;
    r->nm_cap = 0;
    TD3_HIP(hipMalloc(&r->nm_part, need * sizeof(double)));
    r->nm_cap = need;
  }
  const int ncb = (r->sd + kNmColBlock - 1) / kNmColBlock;
  NmSweepArgs k{};
  k.data = r->data;
  k.mask = s->mask;
  k.count_blk = s->count_blk;
  k.part = r->nm_part;
  k.old_count = r->nm_part + (size_t)nchunk * r->sd * 2;
  k.size = r->size;
  k.nchunk = nchunk;
  k.rec = r->rec;
  k.sd = r->sd;
  k.whole = ncb == 1 && r->rec - pad4(r->sd) < 32;
  NmMergeArgs m{};
  m.part = k.part;
  m.old_count = k.old_count;
  m.mask = s->mask;
  m.count_blk = s->count_blk;
  m.mean = s->mean;
  m.m2 = s->m2;
  m.size = r->size;
  m.nchunk = nchunk;
  m.sd = r->sd;
  m.ncount = s->ncol;
  m.merge = merge;
  hipStream_t st = stream ? (hipStream_t)stream : r->stream;
  TD3_RC(ring_begin_read(r, st));
  hipLaunchKernelGGL(nm_sweep_kernel, dim3((unsigned)std::min<int64_t>(nchunk, 4096), ncb), dim3(kNmThreads), 0, st, k);
  hipLaunchKernelGGL(nm_merge_kernel, dim3((r->sd + 3) / 4), dim3(kNmThreads), 0, st, m);
  TD3_HIP(hipGetLastError());
  return ring_end_read(r, st);
}

int rb_normalize_states(rb_handle* rb, const rs_handle* rs, void* stream) {
  TD3_RC(norm_args(rb, rs, false, 0));
  Ring* r = reinterpret_cast<Ring*>(rb);
  const Stats* s = reinterpret_cast<const Stats*>(rs);
  TD3_ARG(!r->normalized, "the ring is already normalised (rb_write_records / rb_fill_synthetic make it raw again)");
  TD3_HIP(hipSetDevice(r->device));
  NmApplyArgs k{};
  k.data = reinterpret_cast<float4*>(r->data);
  k.count_blk = s->count_blk;
  k.mean = s->mean;
  k.m2 = s->m2;
  k.mask = s->mask;
  k.eps = s->cfg.obs_eps;
  k.clip = s->cfg.obs_clip;
  k.size = r->size;
  k.rec4 = r->rec / 4;
  k.sd = r->sd;
  k.o_s2 = r->o_s2;
  k.nA = (r->sd + 3) / 4;
  k.u2 = std::max(r->o_s2 / 4, k.nA);                           // the unit both fields share belongs to the first range
  k.nU = k.nA + std::max(0, (r->o_s2 + r->sd - 1) / 4 - k.u2 + 1);
  k.UW = 1;
  while (k.UW < k.nU && k.UW < kNmThreads) {
    k.UW <<= 1;
    ++k.ush;
  }
  const int RP = kNmThreads >> k.ush;
  const dim3 grid((unsigned)std::min<int64_t>((r->size + RP - 1) / RP, 2048), (k.nU + k.UW - 1) / k.UW);
  hipStream_t st = stream ? (hipStream_t)stream : r->stream;
  TD3_RC(ring_begin_write(r, st));
  hipLaunchKernelGGL(nm_apply_kernel, grid, dim3(kNmThreads), 0, st, k);
  TD3_HIP(hipGetLastError());
  r->ns_nhist = 0;                                              // as every write: the n-step lane ends
  r->normalized = 1;
  r->norm_rows = r->size;
  return ring_end_write(r, st);                                 // priorities are not touched (no ring_wrote)
}

int rb_norm_info(const rb_handle* rb, rb_norm_info_t* info) {
  TD3_ARG(info != nullptr, "null info");
  TD3_ARG(rb != nullptr, "null handle");
  const Ring* r = reinterpret_cast<const Ring*>(rb);
  info->normalized = r->normalized;
  info->obs_dim = r->sd;
  info->rows = r->normalized ? r->norm_rows : 0;
  return 0;
}

}  // extern "C"
