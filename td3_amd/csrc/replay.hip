// Replay ring kernels + the rb_* C-ABI (include/td3.h).
//
// Reference: /root/reference/my_replay_buffer.py
//   ReplayBuffer_featured.__init__  :73-89   -> rb_create
//   ReplayBuffer_featured.add       :109-117 -> rb_add (batched, pinned staging, async H2D),
//                                               rb_add_device (device rows, records built in the ring)
//   ReplayBuffer_featured.sample    :119-128 -> rb_sample / gather_kernel (Philox + HBM gather)
//   ReplayBuffer_featured.save/load :91-107  -> rb_read_records / rb_write_records
//   ReplayBuffer_particles          :6-69    -> rb_create_particles / rb_add_particles /
//                                               rb_sample_particles (same ring, wider record),
//                                               rb_add_particles_device (device rows)
//   main.py add_to_replay_buffer    :70-91   -> rb_add_device_hindsight / rb_add_particles_device_hindsight
//                                               (device rows, each stored with its K relabels)
//   (none: n-step returns)                   -> rb_add_device_nstep / rb_add_particles_device_nstep
//                                               (device rows of one tick; earlier ticks' rows mature in the ring)
//   (none: prioritized replay)               -> rb_enable_priorities / rb_set_priorities / rb_update_priorities /
//                                               rb_sample_prioritized (a 64-ary sum tree next to the ring; every
//                                               write of the ring gives its rows max_priority, ring_wrote)
//
// Both ring kinds are one ring whose record is a table of fields (replay.h Ring::field), filled with
// the named offsets by ring_layout, the only place that computes an offset.  The host side of the two
// kinds shares add_host (packing and pushing a host add), sample_fields (stand-alone samples),
// push_staged (staged records into HBM) and device_add (the launch of a device add); an rb_* entry
// point of a kind keeps its own argument checks and the kernel it launches.
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <set>

#include "replay.h"
#include "../../include/td3.h"

namespace td3 {

// ------------------------------------------------------------------ gather
// One wave per sampled row: the row index is drawn once per wave, the record
// (rec floats, 16-B aligned) is read as float4 (all of it in flight at once) into the
// wave's LDS slot and written to every destination segment.  A segment whose row start is
// 16-B aligned (every network-input segment: row strides are multiples of 32 floats) is
// stored as float4 -- four LDS dwords per lane, whatever the record offset, into one 16-B
// global store -- and its tail / unaligned segments as dwords.  Rows B..Bp-1 are
// zero-filled so padded batch rows stay finite and contribute nothing downstream.
// Bytes moved per live row: rec*4 read + sum(len)*4 written (step.hip input_from_ring).
__device__ __forceinline__ int64_t gather_row_index(const GatherArgs& a, int row) {
  if (a.inject_idx) return a.inject_idx[row];
  const uint64_t size = (uint64_t)*a.d_size;  // issued alongside the counter load
  const uint64_t step = a.ctr ? (uint64_t)(a.ctr->total_it + 1) : a.step;
  return (int64_t)philox_index(a.seed, step, (uint32_t)row, size);
}

template <bool STAGED>
__global__ __launch_bounds__(256) void gather_kernel(GatherArgs a) {
  __shared__ float rec_lds[STAGED ? 4 : 1][STAGED ? kMaxRecord : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wave;
  if (row >= a.Bp) return;
  const bool live = row < a.B;
  if constexpr (STAGED) {
    float* lr = rec_lds[wave];
    if (live) {
      const int64_t idx = gather_row_index(a, row);
      const float4* src = reinterpret_cast<const float4*>(a.data + (size_t)idx * a.rec);
      // All of the row's loads are issued before the first LDS write: a runtime-trip loop
      // waits out one HBM round trip per 64 float4 (4 serial trips for a 3 KB record).
      constexpr int kPer = kMaxRecord / 4 / 64;
      const int n4 = a.rec >> 2;
      float4 v[kPer];
#pragma unroll
      for (int i = 0; i < kPer; ++i) v[i] = src[min(lane + 64 * i, n4 - 1)];  // unguarded: clamped
#pragma unroll  // unguarded too (the slot holds kMaxRecord floats), or the loads sink into the guards
      for (int i = 0; i < kPer; ++i) reinterpret_cast<float4*>(lr)[lane + 64 * i] = v[i];
      if (a.idx_out && lane == 0) a.idx_out[row] = idx;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    for (int s = 0; s < a.nseg; ++s) {
      const GatherSeg g = a.seg[s];
      float* d = g.dst + (size_t)row * g.ld + g.col;
      const float* l = lr + g.src;
      const int n4 = (reinterpret_cast<uintptr_t>(d) & 15) == 0 ? (g.len >> 2) : 0;
      for (int q = lane; q < n4; q += 64) {
        const float4 v = live ? make_float4(l[4 * q], l[4 * q + 1], l[4 * q + 2], l[4 * q + 3])
                              : make_float4(0.f, 0.f, 0.f, 0.f);
        reinterpret_cast<float4*>(d)[q] = v;
      }
      for (int c = 4 * n4 + lane; c < g.len; c += 64) d[c] = live ? l[c] : 0.f;
    }
  } else {
    const float* src = nullptr;
    if (live) {
      const int64_t idx = gather_row_index(a, row);
      if (a.idx_out && lane == 0) a.idx_out[row] = idx;
      src = a.data + (size_t)idx * a.rec;
    }
    for (int s = 0; s < a.nseg; ++s) {
      const GatherSeg g = a.seg[s];
      float* d = g.dst + (size_t)row * g.ld + g.col;
      for (int c = lane; c < g.len; c += 64) d[c] = src ? src[g.src + c] : 0.f;
    }
  }
}

int launch_gather(const GatherArgs& a, hipStream_t s) {
  if (a.Bp <= 0) return 0;
  dim3 grid((a.Bp + 3) / 4);
  if (a.rec <= kMaxRecord) hipLaunchKernelGGL(gather_kernel<true>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(gather_kernel<false>, grid, dim3(256), 0, s, a);
  TD3_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ synthetic fill
// state, next_state ~ N(0,1); action ~ U(-max_action, max_action);
// reward ~ N(0,1); not_done = 1 with probability 0.99.  Philox keyed by (seed, row).
__global__ __launch_bounds__(256) void fill_kernel(float* data, int rec, int o_a, int ad, int o_r,
                                                   int o_nd, int64_t start, int64_t n, int64_t cap,
                                                   float max_action, uint64_t seed) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int64_t slot = (start + i) % cap;
  float* r = data + (size_t)slot * rec;
  for (int c0 = lane * 4; c0 < rec; c0 += 256) {
    float z[4];
    philox_normal4(seed, (uint64_t)i, kStreamFill, (uint32_t)c0, z);
    u32x4 u = philox4x32_10(u32x4{(uint32_t)c0, kStreamFill + 7u, (uint32_t)i, (uint32_t)(i >> 32)},
                            (uint32_t)seed, (uint32_t)(seed >> 32));
    uint32_t uu[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = c0 + j;
      if (c >= rec) break;
      float v;
      if (c > o_nd) v = 0.f;                                            // record pad
      else if (c == o_nd) v = ((float)(uu[j] >> 8) * (1.f / 16777216.f)) < 0.01f ? 0.f : 1.f;
      else if (c >= o_a && c < o_a + ad)
        v = max_action * (2.f * ((float)(uu[j] >> 8) * (1.f / 16777216.f)) - 1.f);
      else v = z[j];                                                    // states, particles, reward
      r[c] = v;
    }
  }
  (void)o_r;
}

__global__ void set_i64_kernel(int64_t* p, int64_t v) { *p = v; }

// Small adds: n staged records, read in place from mapped pinned host memory, into the ring rows
// ptr, ptr+1, ... (wrapping), and the new size -- one launch instead of a DMA copy per ring
// segment plus the size update.  rec is a multiple of 4 (replay.h), so records move as float4.
__global__ __launch_bounds__(256) void ring_put_kernel(float4* __restrict__ data, int64_t cap, int rec4,
                                                       const float4* __restrict__ src, int64_t n, int64_t ptr,
                                                       int64_t* d_size, int64_t new_size) {
  const int64_t total = n * rec4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / rec4, c = i - row * rec4;
    int64_t dst = ptr + row;
    if (dst >= cap) dst -= cap;
    data[dst * rec4 + c] = src[i];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *d_size = new_size;
}

// Adds of a few records travel in the kernel arguments (no host staging buffer whose reuse would
// need an event): rows [0, n) of `rows` (rec floats each) into ring rows ptr, ptr+1, .. (wrapping).
constexpr int kPutArgFloats = 960;
struct RingPutArgs {
  float4* data;
  int64_t* d_size;
  int64_t cap, ptr, n, new_size;
  int rec4;
  float rows[kPutArgFloats];
};
__global__ __launch_bounds__(256) void ring_put_args_kernel(RingPutArgs a) {
  const int64_t total = a.n * a.rec4;
  for (int64_t i = threadIdx.x; i < total; i += 256) {
    const int64_t row = i / a.rec4, c = i - row * a.rec4;
    int64_t dst = a.ptr + row;
    if (dst >= a.cap) dst -= a.cap;
    a.data[dst * a.rec4 + c] = reinterpret_cast<const float4*>(a.rows)[i];
  }
  if (threadIdx.x == 0) *a.d_size = a.new_size;
}

// Adds from device arrays (rb_add_device): the records [s | a | s' | r | not_done | pad] are assembled
// in the ring itself, one thread per float4 of a record.  Consecutive threads walk a record's columns
// and then the next row's, so each source array is read in order (row-major, unit stride inside a
// segment); source row `skip + row` goes to ring row ptr + row (wrapping once: n <= cap).
struct RingPutDeviceArgs {
  float4* data;
  int64_t* d_size;
  const float *state, *action, *next_state, *reward, *done;
  int64_t cap, ptr, n, skip, new_size;
  int sd, ad, o_s2, o_r, o_nd, rec4;
};
__device__ __forceinline__ float ring_put_device_elem(const RingPutDeviceArgs& a, int64_t r, int c) {
  if (c < a.sd) return a.state[r * a.sd + c];
  if (c < a.o_s2) return a.action[r * a.ad + (c - a.sd)];
  if (c < a.o_r) return a.next_state[r * a.sd + (c - a.o_s2)];
  if (c == a.o_r) return a.reward[r];
  if (c == a.o_nd) return 1.0f - a.done[r];               // my_replay_buffer.py:114
  return 0.f;                                             // record pad
}
__global__ __launch_bounds__(256) void ring_put_device_kernel(RingPutDeviceArgs a) {
  const int64_t total = a.n * a.rec4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / a.rec4;
    const int c = (int)(i - row * a.rec4) * 4;
    const int64_t r = a.skip + row;
    int64_t dst = a.ptr + row;
    if (dst >= a.cap) dst -= a.cap;
    a.data[dst * a.rec4 + (c >> 2)] = make_float4(ring_put_device_elem(a, r, c), ring_put_device_elem(a, r, c + 1),
                                                  ring_put_device_elem(a, r, c + 2), ring_put_device_elem(a, r, c + 3));
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *a.d_size = a.new_size;
}

// Particle adds from device arrays (rb_add_particles_device): the record
// [feat | particles | action | next_feat | next_particles | r | not_done | pad] is assembled in the ring
// from seven arrays.  Almost all of it is the two [N*D] particle blocks, whose record offset (o_p = F)
// and source rows (N*D floats) are in general not 16-byte aligned.  One workgroup per tile of
// kPutTile record columns: the work is split by SEGMENT (a table in the launch arguments, walked
// uniformly by the whole workgroup), so inside a segment consecutive lanes read consecutive source
// floats (dword loads, any alignment, every source float exactly once) into the tile's LDS image at
// their record column; the image then leaves as float4 stores aligned on the ring (rec and kPutTile
// are multiples of 4).  No per-float search for the segment a column belongs to.
constexpr int kPutTile = 1024;              // record columns per workgroup pass (4 per thread)
constexpr int kPutSegs = 7;
struct RingPutSeg {
  const float* src;                         // [n][len]
  int off, len;                             // record columns [off, off + len)
};
struct RingPutPartArgs {
  float4* data;
  int64_t* d_size;
  RingPutSeg seg[kPutSegs];                 // ascending and adjacent: seg[k + 1].off = seg[k].off + seg[k].len
  int64_t cap, ptr, n, skip, new_size;
  int rec, o_nd, ntile;                     // ntile = ceil(rec / kPutTile)
};
// Record columns [c0, c1) of source row r into the tile's LDS image (the caller's barrier follows).
__device__ __forceinline__ void ring_put_build_tile(const RingPutPartArgs& a, float* img, int64_t r, int c0, int c1,
                                                    int tid) {
#pragma unroll 1
  for (int k = 0; k < kPutSegs; ++k) {
    const RingPutSeg g = a.seg[k];
    const int lo = max(g.off, c0), hi = min(g.off + g.len, c1);
    if (lo >= hi) continue;                                   // uniform: the segment misses this tile
    const float* src = g.src + r * g.len;                     // the source row of this record
    const bool nd = g.off == a.o_nd;
    float v[4];                                               // the tile's loads in flight together
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = lo + tid + 256 * j;
      v[j] = c < hi ? src[c - g.off] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = lo + tid + 256 * j;
      if (c < hi) img[c - c0] = nd ? 1.0f - v[j] : v[j];      // my_replay_buffer.py:53
    }
  }
  for (int c = max(a.o_nd + 1, c0) + tid; c < c1; c += 256) img[c - c0] = 0.f;   // record pad
}
__global__ __launch_bounds__(256) void ring_put_particles_kernel(RingPutPartArgs a) {
  __shared__ float4 img4[kPutTile / 4];
  float* img = reinterpret_cast<float*>(img4);
  const int tid = threadIdx.x;
  const int64_t tiles = a.n * a.ntile;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t row = t / a.ntile;
    const int c0 = (int)(t - row * a.ntile) * kPutTile, c1 = min(c0 + kPutTile, a.rec);
    ring_put_build_tile(a, img, a.skip + row, c0, c1, tid);
    __syncthreads();
    int64_t dst = a.ptr + row;
    if (dst >= a.cap) dst -= a.cap;
    const int c = c0 + 4 * tid;
    if (c < c1) a.data[(dst * a.rec + c) >> 2] = img4[tid];
    __syncthreads();                                            // the image is reused by the next tile
  }
  if (blockIdx.x == 0 && tid == 0) *a.d_size = a.new_size;
}

// Hindsight fan-out adds (rb_add_device_hindsight / rb_add_particles_device_hindsight, main.py:70-91):
// source transition i is stored 1 + K times, as the expanded rows e = i * (1 + K) + j; copy j = 0 is
// the transition itself, copy j >= 1 has the G goal values goals[i][j - 1][.] in feature columns
// cols[.] of BOTH states and rewards[i][j - 1] as its reward.  Expanded row skip + row goes to ring
// row ptr + row (wrapping once), exactly as if the expanded rows had been given to the plain add.
constexpr int kMaxGoals = 8, kMaxRelabels = 64;
struct RingHindsight {
  const float *goals, *rewards;             // [n][k][g], [n][k]
  int k, g;
  int cols[kMaxGoals];
};
// The relabelled value of state column `sc` (an offset inside the state block) of copy j >= 1.
__device__ __forceinline__ float hindsight_goal(const RingHindsight& h, int64_t i, int j, int sc, float v) {
#pragma unroll
  for (int q = 0; q < kMaxGoals; ++q)
    if (q < h.g && h.cols[q] == sc) v = h.goals[((i * h.k) + (j - 1)) * h.g + q];
  return v;
}

struct RingPutDeviceHsArgs {
  RingPutDeviceArgs p;                      // p.n / p.skip count EXPANDED rows
  RingHindsight h;
};
__device__ __forceinline__ float ring_put_device_hs_elem(const RingPutDeviceHsArgs& a, int64_t i, int j, int c) {
  const RingPutDeviceArgs& p = a.p;
  if (j == 0 || c >= p.o_nd || (c >= p.sd && c < p.o_s2)) return ring_put_device_elem(p, i, c);
  if (c == p.o_r) return a.h.rewards[i * a.h.k + (j - 1)];
  if (c < p.sd) return hindsight_goal(a.h, i, j, c, p.state[i * p.sd + c]);
  return hindsight_goal(a.h, i, j, c - p.o_s2, p.next_state[i * p.sd + (c - p.o_s2)]);
}
__global__ __launch_bounds__(256) void ring_put_device_hs_kernel(RingPutDeviceHsArgs a) {
  const RingPutDeviceArgs& p = a.p;
  const int64_t total = p.n * p.rec4;
  const int copies = a.h.k + 1;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = t / p.rec4;
    const int c = (int)(t - row * p.rec4) * 4;
    const int64_t e = p.skip + row, i = e / copies;
    const int j = (int)(e - i * copies);
    int64_t dst = p.ptr + row;
    if (dst >= p.cap) dst -= p.cap;
    p.data[dst * p.rec4 + (c >> 2)] = make_float4(ring_put_device_hs_elem(a, i, j, c), ring_put_device_hs_elem(a, i, j, c + 1),
                                                  ring_put_device_hs_elem(a, i, j, c + 2), ring_put_device_hs_elem(a, i, j, c + 3));
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *p.d_size = p.new_size;
}

// The particle form: one workgroup per (source transition, tile), the tile's image built in LDS from
// the source exactly as ring_put_particles_kernel does -- every source float is read once per
// transition, not once per copy.  Each thread then takes the float4 of the image it stores into
// registers and writes it 1 + K times; for a relabel copy it first replaces, in a register copy, the
// goal columns of feat / next_feat and the reward column that fall inside its own float4.  The LDS
// image is never patched (copy 0 and every later copy start from the original values), so nothing is
// ordered between patching and storing, and a tile of particle columns alone stores one register
// value to 1 + K rows.  p.n / p.skip count EXPANDED rows; p.ptr is the ring row of expanded row skip.
struct RingPutPartHsArgs {
  RingPutPartArgs p;
  RingHindsight h;
  int o_s, o_s2, o_r, sd;                   // feat at [o_s, o_s + sd), next_feat at [o_s2, ..), reward
};
__global__ __launch_bounds__(256) void ring_put_particles_hs_kernel(RingPutPartHsArgs a) {
  __shared__ float4 img4[kPutTile / 4];
  float* img = reinterpret_cast<float*>(img4);
  const RingPutPartArgs& p = a.p;
  const int tid = threadIdx.x;
  const int copies = a.h.k + 1;
  const int64_t i0 = p.skip / copies;                             // first source transition with a surviving copy
  const int64_t e_end = p.skip + p.n;                             // = (source rows) * copies
  const int64_t tiles = (e_end / copies - i0) * p.ntile;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t srow = t / p.ntile;
    const int c0 = (int)(t - srow * p.ntile) * kPutTile, c1 = min(c0 + kPutTile, p.rec);
    const int64_t i = i0 + srow;
    ring_put_build_tile(p, img, i, c0, c1, tid);
    __syncthreads();
    const int c = c0 + 4 * tid;
    if (c < c1) {
      const float4 orig = img4[tid];
      // does this thread's float4 [c, c + 4) meet feat, next_feat or the reward?
      const bool in_f = c < a.o_s + a.sd && c + 4 > a.o_s, in_f2 = c < a.o_s2 + a.sd && c + 4 > a.o_s2;
      const bool in_r = a.o_r >= c && a.o_r < c + 4;
      const int64_t e0 = i * copies;
      for (int j = (int)max((int64_t)0, p.skip - e0); j < copies; ++j) {
        float w[4] = {orig.x, orig.y, orig.z, orig.w};
        if (j > 0 && (in_f || in_f2 || in_r)) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int cc = c + q;
            if (cc >= a.o_s && cc < a.o_s + a.sd) w[q] = hindsight_goal(a.h, i, j, cc - a.o_s, w[q]);
            else if (cc >= a.o_s2 && cc < a.o_s2 + a.sd) w[q] = hindsight_goal(a.h, i, j, cc - a.o_s2, w[q]);
            else if (cc == a.o_r) w[q] = a.h.rewards[i * a.h.k + (j - 1)];
          }
        }
        int64_t dst = p.ptr + (e0 + j - p.skip);
        if (dst >= p.cap) dst -= p.cap;
        p.data[(dst * p.rec + c) >> 2] = make_float4(w[0], w[1], w[2], w[3]);
      }
    }
    __syncthreads();                                            // the image is reused by the next tile
  }
  if (blockIdx.x == 0 && tid == 0) *p.d_size = p.new_size;
}

// N-step adds (rb_add_device_nstep / rb_add_particles_device_nstep): one launch stores this tick's
// one-step rows (copy 0, exactly the plain device add's records) and matures, in place, the rows the
// previous ticks of the lane stored for the same environment: copy j = 1..a_i is ring row
// hist[j - 1] + i (the row of source row i of the tick j ticks ago), whose reward gains
// gpow[j] * reward[i], whose next-state block becomes this tick's and whose not_done becomes
// gpow[j] * (1 - done[i]).  a_i = clamp(age_in[i], 0, nhist) is how many earlier ticks of environment
// i's episode are still maturing; age_out[i] is that count for the next tick (0 once the episode ended).
// age_in and age_out are different arrays (the host swaps them between ticks): every thread of a
// source row reads age_in, one thread writes age_out.  The host keeps the row ranges of the 1 + nhist
// ticks disjoint (n * rows <= cap), so each ring row belongs to one (i, j) and each of its 16-byte
// units to one thread: the thread that stores the reward column is the one that read its old value.
struct RingNstep {
  const int* age_in;
  int* age_out;
  const uint8_t* ended;                     // [rows]
  int64_t hist[kMaxNstep - 1];              // ring row of source row 0 of the tick j + 1 ticks ago, j < nhist
  float gpow[kMaxNstep];                    // gamma^j
  int nhist, nmax;                          // valid entries of hist; n - 1
};
__device__ __forceinline__ int nstep_age(const RingNstep& s, int64_t i) { return min(max(s.age_in[i], 0), s.nhist); }
__device__ __forceinline__ void nstep_age_out(const RingNstep& s, int64_t i, int age, float done) {
  s.age_out[i] = (s.ended[i] != 0 || done != 0.f) ? 0 : min(age + 1, s.nmax);
}
// Stores the four columns [c, c + 4) of a maturing row: one 16-byte store, or, in the unit that still
// holds columns before the next-state block (o_s2 is in general no multiple of 4), dword stores of the
// columns from o_s2 on -- the row's own action columns are not touched.
__device__ __forceinline__ void nstep_store_unit(float* row, int c, int o_s2, const float (&w)[4]) {
  if (c >= o_s2) {
    *reinterpret_cast<float4*>(row + c) = make_float4(w[0], w[1], w[2], w[3]);
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (c + q >= o_s2) row[c + q] = w[q];
  }
}

// The featured form: one thread per 16-byte unit of (source row, copy), as ring_put_device_kernel;
// per source row the rec4 units of copy 0, then for each of the nhist possible earlier ticks the
// units from the one holding column o_s2 on (u2 = o_s2 / 4).  A thread of a copy j > a_i has nothing
// to do: the grid is sized by the host, which does not know the ages.
struct RingPutDeviceNsArgs {
  RingPutDeviceArgs p;                      // p.n source rows, p.skip = 0 (a tick is never truncated)
  RingNstep s;
  int u2, per_row;                          // per_row = rec4 + nhist * (rec4 - u2)
};
__global__ __launch_bounds__(256) void ring_put_device_ns_kernel(RingPutDeviceNsArgs a) {
  const RingPutDeviceArgs& p = a.p;
  const int mu = p.rec4 - a.u2;
  const int64_t total = p.n * a.per_row;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / a.per_row;
    int u = (int)(t - i * a.per_row);
    const int age = nstep_age(a.s, i);
    if (u < p.rec4) {                                          // copy 0: the plain add's record
      const int c = u * 4;
      int64_t dst = p.ptr + i;
      if (dst >= p.cap) dst -= p.cap;
      p.data[dst * p.rec4 + u] = make_float4(ring_put_device_elem(p, i, c), ring_put_device_elem(p, i, c + 1),
                                             ring_put_device_elem(p, i, c + 2), ring_put_device_elem(p, i, c + 3));
      if (u == 0) nstep_age_out(a.s, i, age, p.done[i]);
      continue;
    }
    u -= p.rec4;
    const int j = 1 + u / mu;
    if (j > age) continue;
    const int c = (a.u2 + (u - (j - 1) * mu)) * 4;
    int64_t dst = a.s.hist[j - 1] + i;
    if (dst >= p.cap) dst -= p.cap;
    float* row = reinterpret_cast<float*>(p.data) + dst * (p.rec4 * 4);
    const float g = a.s.gpow[j];
    float w[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int cc = c + q;
      if (cc < p.o_s2) w[q] = 0.f;                             // not stored (nstep_store_unit)
      else if (cc < p.o_r) w[q] = p.next_state[i * p.sd + (cc - p.o_s2)];
      else if (cc == p.o_r) w[q] = row[cc] + g * p.reward[i];
      else if (cc == p.o_nd) w[q] = g * (1.0f - p.done[i]);
      else w[q] = 0.f;                                         // record pad
    }
    nstep_store_unit(row, c, p.o_s2, w);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *p.d_size = p.new_size;
}

// The particle form: one workgroup per (source row, tile) as ring_put_particles_hs_kernel -- the
// tile's image is built in LDS once, so every source float is read once per tick, each thread takes
// its float4 into registers and stores it to the new row and, where its unit reaches the next-state
// blocks, to the a_i maturing rows.  The reward (old value + gpow[j] * this tick's), not_done and a
// unit that straddles o_s2 are patched in a register copy; the LDS image is never patched.
struct RingPutPartNsArgs {
  RingPutPartArgs p;                        // p.n source rows, p.skip = 0
  RingNstep s;
  int o_s2, o_r;                            // next_feat, reward
};
__global__ __launch_bounds__(256) void ring_put_particles_ns_kernel(RingPutPartNsArgs a) {
  __shared__ float4 img4[kPutTile / 4];
  float* img = reinterpret_cast<float*>(img4);
  const RingPutPartArgs& p = a.p;
  const int tid = threadIdx.x;
  const int64_t tiles = p.n * p.ntile;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t i = t / p.ntile;
    const int c0 = (int)(t - i * p.ntile) * kPutTile, c1 = min(c0 + kPutTile, p.rec);
    ring_put_build_tile(p, img, i, c0, c1, tid);
    __syncthreads();
    const int age = nstep_age(a.s, i);
    const int c = c0 + 4 * tid;
    if (c < c1) {
      const float4 orig = img4[tid];
      int64_t dst = p.ptr + i;
      if (dst >= p.cap) dst -= p.cap;
      p.data[(dst * p.rec + c) >> 2] = orig;
      if (c + 4 > a.o_s2) {                                     // false for a whole tile below next_feat
        for (int j = 1; j <= age; ++j) {
          int64_t old = a.s.hist[j - 1] + i;
          if (old >= p.cap) old -= p.cap;
          float* row = reinterpret_cast<float*>(p.data) + old * p.rec;
          const float g = a.s.gpow[j];
          float w[4] = {orig.x, orig.y, orig.z, orig.w};
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if (c + q == a.o_r) w[q] = row[c + q] + g * w[q];
            else if (c + q == p.o_nd) w[q] = g * w[q];          // the image holds 1 - done
          }
          nstep_store_unit(row, c, a.o_s2, w);
        }
      }
    }
    if (c0 == 0 && tid == 0) nstep_age_out(a.s, i, age, p.seg[kPutSegs - 1].src[i]);
    __syncthreads();                                            // the image is reused by the next tile
  }
  if (blockIdx.x == 0 && tid == 0) *p.d_size = p.new_size;
}

// ------------------------------------------------------------------ priorities
// The 64-ary sum tree of replay.h PriTree.  Every kernel below gives one wave one group of 64
// siblings: a coalesced 256-byte load, an inclusive scan across the lanes.  A parent is stored as
// lane 63 of that scan, so the prefix sums a draw sees while it descends through a group end exactly
// at the value its parent holds.  Updates store the changed leaves and then recompute, level by
// level, every affected parent from all of its children: idempotent (duplicate indices store the same
// value twice), free of float atomics and therefore bitwise reproducible whatever the arrival order.
// A level is made visible to the next one by the launch boundary between them (one launch per level):
// a stored node is another workgroup's input one level up, and inside a launch that hand-off would
// need a release / acquire flag protocol across workgroups for a few microseconds of launch gaps.
__device__ __forceinline__ float pri_group_scan(float v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// Leaves [start, start + n) (wrapping at cap) = max_priority: the rows an add just wrote.
__global__ __launch_bounds__(256) void pri_fill_range_kernel(float* __restrict__ leaf, int64_t start, int64_t n,
                                                             int64_t cap, const float* __restrict__ d_max) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int64_t row = start + i;
  if (row >= cap) row -= cap;
  leaf[row] = *d_max;
}

// Leaves [0, size) = max_priority, [size, len) = 0: enable, rb_write_records.
__global__ __launch_bounds__(256) void pri_reset_kernel(float* __restrict__ leaf, int64_t size, int64_t len,
                                                        const float* __restrict__ d_max) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < len) leaf[i] = i < size ? *d_max : 0.f;
}

// Parents [p0a, p0a + na) and [p0b, p0b + nb) of one level from their children, one wave each.
__global__ __launch_bounds__(256) void pri_repair_range_kernel(const float* __restrict__ child,
                                                               float* __restrict__ parent, int64_t p0a, int64_t na,
                                                               int64_t p0b, int64_t nb) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= na + nb) return;
  const int64_t p = w < na ? p0a + w : p0b + (w - na);
  const float s = pri_group_scan(child[p * 64 + lane], lane);
  if (lane == 63) parent[p] = s;
}

// The parents idx[k] >> shift of one level, one wave per k (duplicates recompute the same value).
__global__ __launch_bounds__(256) void pri_repair_idx_kernel(const float* __restrict__ child,
                                                             float* __restrict__ parent,
                                                             const int64_t* __restrict__ idx, int64_t n, int shift) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= n) return;
  const int64_t p = idx[w] >> shift;
  const float s = pri_group_scan(child[p * 64 + lane], lane);
  if (lane == 63) parent[p] = s;
}

// Leaves idx[k] = p[k] (td = 0) or (p[k] + eps)^alpha (td = 1), in two launches: the leaves are
// cleared, then every entry raises its leaf by an integer atomicMax on the float's bits (priorities
// are non-negative: their bits order as they do).  A row that appears several times in one call
// (a batch can draw a row twice, with different target noise and so different TD errors) ends with
// the largest of its values whatever the order of arrival -- a plain store would keep whichever
// landed last.  max_priority is raised the same way, once per wave.  A non-finite |TD error| (a
// diverged critic) stores the current max_priority instead of poisoning every sum above the leaf.
__global__ __launch_bounds__(256) void pri_clear_kernel(float* __restrict__ leaf, const int64_t* __restrict__ idx,
                                                        int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) leaf[idx[i]] = 0.f;
}
__global__ __launch_bounds__(256) void pri_store_kernel(float* __restrict__ leaf, const int64_t* __restrict__ idx,
                                                        const float* __restrict__ p, int64_t n, int td, float alpha,
                                                        float eps, float* __restrict__ d_max) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float v = 0.f;
  if (i < n) {
    v = p[i];
    if (td) {
      v = powf(v + eps, alpha);
      if (!(v >= 0.f && v <= 3.0e38f)) v = *d_max;
    }
    v = v > 0.f ? v : 0.f;                                      // (-0.0f and NaN have large bits)
    atomicMax(reinterpret_cast<unsigned int*>(leaf + idx[i]), __float_as_uint(v));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0 && v > 0.f) atomicMax(reinterpret_cast<unsigned int*>(d_max), __float_as_uint(v));
}

// The stratified draw (rb_sample_prioritized), one wave per draw k: the mass m = u_k * total, with
// u_k = (k + U_k) / batch (U_k in [0, 1) from Philox) or inject_u[k], then down the tree -- at each
// level the first child whose inclusive prefix exceeds m, m less the prefix before it; where rounding
// leaves none, the last child with a non-zero value.  A child chosen by its prefix has a value > 0
// (its prefix exceeds its left neighbour's), so a row of priority 0 is never returned while any
// priority is positive.  The raw weight (size * p / total)^-beta goes to w_raw; pri_normalise_kernel
// divides the batch by its maximum.
struct PriDrawArgs {
  const float* level[kMaxPriLevels];
  int levels, batch;
  int64_t cap, size;
  float beta;
  const float* inject_u;
  int64_t *idx_out, *idx_out2;
  float* w_raw;
  uint64_t seed, step;
};
__global__ __launch_bounds__(256) void pri_draw_kernel(PriDrawArgs a) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= a.batch) return;
  float u;
  if (a.inject_u) {
    u = a.inject_u[k];
  } else {
    const u32x4 r = philox4x32_10(u32x4{(uint32_t)k, kStreamPriority, (uint32_t)a.step, (uint32_t)(a.step >> 32)},
                                  (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
    const float U = (float)(r.x >> 8) * (1.0f / 16777216.0f);                  // [0, 1)
    u = fminf(((float)k + U) / (float)a.batch, 0x1.fffffep-1f);                // (k + U) may round up to k + 1
  }
  float v = a.level[a.levels - 1][lane];
  float s = pri_group_scan(v, lane);
  const float total = __shfl(s, 63, 64);
  float m = u * total;
  int64_t node = 0;
  for (int l = a.levels - 1;; --l) {
    const unsigned long long over = __ballot(s > m), nz = __ballot(v > 0.f);
    int c = 0;
    if (over) c = __ffsll(over) - 1;
    else if (nz) c = 63 - __clzll(nz);
    const float before = __shfl(s, max(c - 1, 0), 64);
    if (c > 0) m -= before;
    node = node * 64 + c;
    if (l == 0) {
      v = __shfl(v, c, 64);
      break;
    }
    v = a.level[l - 1][node * 64 + lane];
    s = pri_group_scan(v, lane);
  }
  if (lane == 0) {
    node = min(node, a.cap - 1);                               // (all priorities zero: any row, in bounds)
    a.idx_out[k] = node;
    if (a.idx_out2) a.idx_out2[k] = node;
    a.w_raw[k] = powf((float)a.size * v / total, -a.beta);
  }
}

// w[k] = w_raw[k] / max_j w_raw[j]: one workgroup (a batch is a few hundred rows).
__global__ __launch_bounds__(256) void pri_normalise_kernel(const float* w_raw, float* w, int batch) {   // may alias
  __shared__ float wmax[4];
  float mx = 0.f;
  for (int i = threadIdx.x; i < batch; i += 256) mx = fmaxf(mx, w_raw[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
  for (int i = threadIdx.x; i < batch; i += 256) w[i] = w_raw[i] / mx;
}

// The lazy ordering of Ring::read_stream / write_stream: when `s` differs from the noted stream,
// an event recorded there now (it covers everything queued so far) is waited on by `s`.
static int order_after(hipStream_t s, hipStream_t noted, bool pending, hipEvent_t ev, hipStream_t& seen_by) {
  if (!pending || !noted || noted == s || seen_by == s) return 0;
  TD3_HIP(hipEventRecord(ev, noted));
  TD3_HIP(hipStreamWaitEvent(s, ev, 0));
  seen_by = s;
  return 0;
}

static std::mutex g_rings_mu;
static std::set<Ring*> g_rings;

void ring_forget_stream(hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_rings_mu);
  for (Ring* r : g_rings) {
    if (r->read_stream == s) {
      r->read_stream = nullptr;
      r->reads_pending = false;
    }
    if (r->write_stream == s) {
      r->write_stream = nullptr;
      r->writes_pending = false;
    }
    if (r->reads_seen_by == s) r->reads_seen_by = nullptr;
    if (r->writes_seen_by == s) r->writes_seen_by = nullptr;
  }
}

int ring_begin_read(Ring* r, hipStream_t s) {
  TD3_RC(order_after(s, r->write_stream, r->writes_pending, r->write_ev, r->writes_seen_by));  // adds so far
  TD3_RC(order_after(s, r->read_stream, r->reads_pending, r->read_ev, r->reads_seen_by));     // chained readers
  return 0;
}

int ring_end_read(Ring* r, hipStream_t s) {
  r->read_stream = s;
  r->reads_pending = true;
  r->reads_seen_by = nullptr;
  return 0;
}

// Writes (records, d_size) on `stream` start after every read and every other-stream write queued
// so far (Ring::read_stream / write_stream).
int ring_begin_write(Ring* r, hipStream_t stream) {
  TD3_RC(order_after(stream, r->read_stream, r->reads_pending, r->read_ev, r->reads_seen_by));
  TD3_RC(order_after(stream, r->write_stream, r->writes_pending, r->write_ev, r->writes_seen_by));
  return 0;
}

int ring_end_write(Ring* r, hipStream_t stream) {
  r->write_stream = stream;
  r->writes_pending = true;
  r->writes_seen_by = nullptr;
  return 0;
}

// ptr / size of an add of `rows` rows: only the last `cap` rows survive (the ring semantics of
// my_replay_buffer.py:115-116 applied `rows` times).  Returns the rows to write and leaves r->ptr at
// the ring row of the first of them (ring_wrote moves it past them); the first `skip` rows are dropped.
static int64_t ring_reserve(Ring* r, int64_t rows, int64_t& skip, int64_t& new_size) {
  skip = 0;
  if (rows > r->cap) {
    skip = rows - r->cap;
    r->ptr = (r->ptr + skip) % r->cap;
    rows = r->cap;
    r->size = r->cap;
  }
  new_size = std::min<int64_t>(r->size + rows, r->cap);
  return rows;
}

// Recompute, level by level (one launch each), the parents above leaves [start, start + n), wrapping
// at cap: per level the affected parents are one range, or two when the rows wrap.
static int pri_repair_ranges(const PriTree& t, int64_t start, int64_t n, int64_t cap, hipStream_t s) {
  const int64_t na0 = std::min(n, cap - start), nb0 = n - na0;     // leaves [start, start + na0) and [0, nb0)
  for (int l = 1; l < t.levels; ++l) {
    const int sh = 6 * l;
    const int64_t a0 = start >> sh, a1 = (start + na0 - 1) >> sh;
    int64_t b0 = 0, nb = nb0 > 0 ? ((nb0 - 1) >> sh) + 1 : 0;
    if (nb > a0) nb = a0;                                          // the two ranges meet: [0, a1] once
    const int64_t na = a1 - a0 + 1;
    hipLaunchKernelGGL(pri_repair_range_kernel, dim3((unsigned)((na + nb + 3) / 4)), dim3(256), 0, s,
                       t.level[l - 1], t.level[l], a0, na, b0, nb);
  }
  TD3_HIP(hipGetLastError());
  return 0;
}

// The rows an add just wrote get max_priority (a new transition is drawn at least once soon).
static int pri_wrote(Ring* r, int64_t start, int64_t rows, hipStream_t s) {
  const PriTree& t = r->pri;
  hipLaunchKernelGGL(pri_fill_range_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, t.level[0], start,
                     rows, r->cap, t.d_max);
  return pri_repair_ranges(t, start, rows, r->cap, s);
}

// Leaves [0, size) = max_priority, the rest 0, every parent recomputed.
static int pri_reset(Ring* r, int64_t size, hipStream_t s) {
  const PriTree& t = r->pri;
  hipLaunchKernelGGL(pri_reset_kernel, dim3((unsigned)((t.len[0] + 255) / 256)), dim3(256), 0, s, t.level[0], size,
                     t.len[0], t.d_max);
  return pri_repair_ranges(t, 0, r->cap, r->cap, s);
}

int ring_store_priorities(Ring* r, const int64_t* idx, const float* p, int64_t n, bool td, hipStream_t s) {
  const PriTree& t = r->pri;
  hipLaunchKernelGGL(pri_clear_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, t.level[0], idx, n);
  hipLaunchKernelGGL(pri_store_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, t.level[0], idx, p, n,
                     td ? 1 : 0, (float)t.alpha, (float)t.eps, t.d_max);
  for (int l = 1; l < t.levels; ++l)
    hipLaunchKernelGGL(pri_repair_idx_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, t.level[l - 1],
                       t.level[l], idx, n, 6 * l);
  TD3_HIP(hipGetLastError());
  return 0;
}

int ring_draw_prioritized(Ring* r, int batch, double beta, const float* inject_u, int64_t* idx_out,
                          int64_t* idx_out2, float* weight_out, hipStream_t s) {
  const PriTree& t = r->pri;
  PriDrawArgs a{};
  for (int l = 0; l < t.levels; ++l) a.level[l] = t.level[l];
  a.levels = t.levels;
  a.batch = batch;
  a.cap = r->cap;
  a.size = r->size;
  a.beta = (float)beta;
  a.inject_u = inject_u;
  a.idx_out = idx_out;
  a.idx_out2 = idx_out2;
  a.w_raw = weight_out;                                            // normalised in place
  a.seed = r->seed;
  a.step = ++r->sample_calls;
  hipLaunchKernelGGL(pri_draw_kernel, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(pri_normalise_kernel, dim3(1), dim3(256), 0, s, weight_out, weight_out, batch);
  TD3_HIP(hipGetLastError());
  return 0;
}

// After the launches that wrote `rows` rows at r->ptr.  Any write ends the n-step lane: the rows that
// follow are not the next tick of it (an n-step add sets its lane again after this).
static int ring_wrote(Ring* r, int64_t rows, int64_t new_size, hipStream_t s) {
  if (r->pri.on && rows > 0) TD3_RC(pri_wrote(r, r->ptr, rows, s));
  r->ptr = (r->ptr + rows) % r->cap;
  r->size = new_size;
  r->ns_nhist = 0;
  return ring_end_write(r, s);
}

// A device add whose launch arguments are built and whose rows are reserved: on the ring's device, on
// `stream` (or the ring's own) after the reads and writes queued so far; ptr / size then move past the rows.
template <class Args>
static int device_add(Ring* r, void (*kernel)(Args), const Args& a, int grid, int64_t rows, int64_t new_size,
                      void* stream) {
  TD3_HIP(hipSetDevice(r->device));
  hipStream_t s = stream ? (hipStream_t)stream : r->stream;
  TD3_RC(ring_begin_write(r, s));
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, s, a);
  TD3_HIP(hipGetLastError());
  return ring_wrote(r, rows, new_size, s);
}

bool ring_alive(const Ring* r, uint64_t gen) {
  std::lock_guard<std::mutex> lk(g_rings_mu);
  return r && g_rings.count(const_cast<Ring*>(r)) && r->gen == gen;
}

}  // namespace td3

using namespace td3;

// ================================================================== C-ABI
extern "C" {

static std::atomic<uint64_t> g_ring_gen{0};

// The record of a ring whose dimensions are set: the fields of its kind in C-ABI argument order (a
// featured ring has no particle blocks), one behind the other, padded to 16 B.
static void ring_layout(Ring* r) {
  const int np = r->N * r->D;
  const struct { int* off; int len; } fields[kRingFields] = {
      {&r->o_s, r->sd}, {&r->o_p, np}, {&r->o_a, r->ad}, {&r->o_s2, r->sd}, {&r->o_p2, np}, {&r->o_r, 1}, {&r->o_nd, 1}};
  int c = 0;
  r->nfield = 0;
  for (const auto& f : fields) {
    if (!f.len) continue;
    *f.off = c;
    r->field[r->nfield++] = RingField{c, f.len};
    c += f.len;
  }
  r->rec = pad4(c);
}

// The ring of the dimensions in `dims` (sd, ad and, for a particle ring, particles, N, D).
static int ring_alloc(const Ring& dims, int64_t max_size, int device, uint64_t seed, rb_handle** out) {
  TD3_HIP(hipSetDevice(device));
  Ring* r = new Ring(dims);
  ring_layout(r);
  r->gen = ++g_ring_gen;
  r->cap = max_size;
  r->seed = seed;
  r->device = device;
  hipError_t e = hipMalloc(&r->data, (size_t)max_size * r->rec * sizeof(float));
  if (e != hipSuccess) {
    set_error("rb_create: hipMalloc(%zu bytes) failed: %s",
              (size_t)max_size * r->rec * sizeof(float), hipGetErrorString(e));
    delete r;
    return -2;
  }
  TD3_HIP(hipMemset(r->data, 0, (size_t)max_size * r->rec * sizeof(float)));
  TD3_HIP(hipMalloc(&r->d_size, sizeof(int64_t)));
  TD3_HIP(hipMemset(r->d_size, 0, sizeof(int64_t)));
  // the memsets ran on the null stream, which does not order the ring's non-blocking stream:
  // finish them before any add / sample can be queued
  TD3_HIP(hipDeviceSynchronize());
  TD3_HIP(hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking));
  TD3_HIP(hipEventCreateWithFlags(&r->write_ev, TD3_EV_FLAGS));
  TD3_HIP(hipEventCreateWithFlags(&r->read_ev, TD3_EV_FLAGS));
  for (auto& ev : r->stage_buf_ev) TD3_HIP(hipEventCreateWithFlags(&ev, TD3_EV_FLAGS));
  {
    std::lock_guard<std::mutex> lk(g_rings_mu);
    g_rings.insert(r);
  }
  *out = reinterpret_cast<rb_handle*>(r);
  return 0;
}

int rb_create(int state_dim, int action_dim, int64_t max_size, int device, uint64_t seed,
              rb_handle** out) {
  TD3_ARG(out != nullptr, "out is null");
  TD3_ARG(state_dim > 0 && action_dim > 0, "dims must be positive");
  TD3_ARG(pad4(2 * state_dim + action_dim + 2) <= kMaxRecord, "record too wide");
  TD3_ARG(max_size > 0, "max_size must be positive");
  Ring dims;
  dims.sd = state_dim;
  dims.ad = action_dim;
  return ring_alloc(dims, max_size, device, seed, out);
}

int rb_create_particles(int feat_dim, int n_particles, int particle_dim, int action_dim, int64_t max_size,
                        int device, uint64_t seed, rb_handle** out) {
  TD3_ARG(out != nullptr, "out is null");
  TD3_ARG(feat_dim > 0 && n_particles > 0 && particle_dim > 0 && action_dim > 0, "dims must be positive");
  TD3_ARG(max_size > 0, "max_size must be positive");
  Ring dims;
  dims.particles = 1;
  dims.N = n_particles;
  dims.D = particle_dim;
  dims.sd = feat_dim;
  dims.ad = action_dim;
  return ring_alloc(dims, max_size, device, seed, out);
}

int rb_destroy(rb_handle* h) {
  if (!h) return 0;
  Ring* r = reinterpret_cast<Ring*>(h);
  (void)hipSetDevice(r->device);
  {
    std::lock_guard<std::mutex> lk(g_rings_mu);
    g_rings.erase(r);
  }
  // no reader or writer of the ring still in flight, whatever stream it was queued on
  (void)hipDeviceSynchronize();
  (void)hipFree(r->data);
  (void)hipFree(r->d_size);
  (void)hipFree(r->d_idx);
  (void)hipFree(r->pri.base);
  (void)hipFree(r->pri.d_max);
  (void)hipFree(r->nm_part);
  for (int* age : r->ns_age) (void)hipFree(age);
  for (int i = 0; i < 2; ++i) {
    if (r->stage_buf_ev[i]) (void)hipEventSynchronize(r->stage_buf_ev[i]);
    if (r->stage[i]) (void)hipHostFree(r->stage[i]);
    (void)hipEventDestroy(r->stage_buf_ev[i]);
  }
  (void)hipEventDestroy(r->write_ev);
  (void)hipEventDestroy(r->read_ev);
  (void)hipStreamDestroy(r->stream);
  delete r;
  return 0;
}

void* rb_stream(rb_handle* h) { return h ? (void*)reinterpret_cast<Ring*>(h)->stream : nullptr; }

int rb_info(const rb_handle* h, rb_info_t* info) {
  TD3_ARG(h && info, "null handle");
  const Ring* r = reinterpret_cast<const Ring*>(h);
  info->state_dim = r->sd;
  info->action_dim = r->ad;
  info->record_floats = r->rec;
  info->max_size = r->cap;
  info->ptr = r->ptr;
  info->size = r->size;
  info->data = r->data;
  info->device = r->device;
  info->n_particles = r->N;
  info->particle_dim = r->D;
  return 0;
}

// Pinned staging for the next add: alternate between two buffers so the host packs the next
// rows while the previous upload (which may be waiting behind a step that reads the ring) is
// still queued; only the upload before that one must have consumed its buffer.
static float* ensure_stage(Ring* r, size_t floats) {
  const int i = r->stage_cur;
  r->stage_cur ^= 1;
  if (hipEventSynchronize(r->stage_buf_ev[i]) != hipSuccess) return nullptr;
  if (floats > r->stage_cap[i]) {
    if (r->stage[i]) (void)hipHostFree(r->stage[i]);
    r->stage[i] = nullptr;
    r->stage_cap[i] = 0;
    const size_t cap = std::max(floats, (size_t)r->rec * 4096);
    hipError_t e = hipHostMalloc(&r->stage[i], cap * sizeof(float), hipHostMallocMapped);
    void* d = nullptr;
    if (e == hipSuccess) e = hipHostGetDevicePointer(&d, r->stage[i], 0);
    if (e != hipSuccess) {
      set_error("rb_add: hipHostMalloc(%zu bytes) failed: %s", cap * sizeof(float), hipGetErrorString(e));
      return nullptr;
    }
    r->stage_dev[i] = static_cast<float*>(d);
    r->stage_cap[i] = cap;
  }
  return r->stage[i];
}

static int stage_index(const Ring* r, const float* host) {
  for (int i = 0; i < 2; ++i)
    if (host == r->stage[i]) return i;
  return -1;
}

constexpr size_t kPutKernelBytes = 256 << 10;   // adds up to this size take ring_put_kernel

// Copy n packed records (host staging) into the ring at ptr, wrapping.
static int push_staged(Ring* r, const float* host, int64_t n, hipStream_t stream) {
  TD3_RC(ring_begin_write(r, stream));
  const int si = stage_index(r, host);
  int64_t skip, new_size;
  n = ring_reserve(r, n, skip, new_size);
  if ((int64_t)n * r->rec <= kPutArgFloats) {       // the records in the kernel arguments
    RingPutArgs pa;
    pa.data = reinterpret_cast<float4*>(r->data);
    pa.d_size = r->d_size;
    pa.cap = r->cap;
    pa.ptr = r->ptr;
    pa.n = n;
    pa.new_size = new_size;
    pa.rec4 = r->rec / 4;
    memcpy(pa.rows, host + (size_t)skip * r->rec, (size_t)n * r->rec * sizeof(float));
    hipLaunchKernelGGL(ring_put_args_kernel, dim3(1), dim3(256), 0, stream, pa);
    TD3_HIP(hipGetLastError());
    return ring_wrote(r, n, new_size, stream);
  }
  if (si >= 0 && (size_t)n * r->rec * sizeof(float) <= kPutKernelBytes) {
    const int64_t total4 = n * (r->rec / 4);
    const int grid = (int)std::min<int64_t>((total4 + 255) / 256, 256);
    hipLaunchKernelGGL(ring_put_kernel, dim3(grid), dim3(256), 0, stream, reinterpret_cast<float4*>(r->data),
                       r->cap, r->rec / 4, reinterpret_cast<const float4*>(r->stage_dev[si] + (size_t)skip * r->rec),
                       n, r->ptr, r->d_size, new_size);
    TD3_HIP(hipGetLastError());
  } else {
    const float* src = host + (size_t)skip * r->rec;
    for (int64_t done = 0, at = r->ptr; done < n; at = 0) {   // up to the end of the ring, then the rest
      const int64_t chunk = std::min<int64_t>(n - done, r->cap - at);
      TD3_HIP(hipMemcpyAsync(r->data + (size_t)at * r->rec, src + (size_t)done * r->rec,
                             (size_t)chunk * r->rec * sizeof(float), hipMemcpyHostToDevice, stream));
      done += chunk;
    }
    hipLaunchKernelGGL(set_i64_kernel, dim3(1), dim3(1), 0, stream, r->d_size, new_size);
    TD3_HIP(hipGetLastError());
  }
  if (si >= 0) TD3_HIP(hipEventRecord(r->stage_buf_ev[si], stream));   // the staging buffer is free
  return ring_wrote(r, n, new_size, stream);
}

// A host add of either kind: src[k] is the float64 array [n][field[k].len] of field k, the last one
// `done`.  The records are packed as fp32 (my_replay_buffer.py:46-56, :109-117) and pushed.
static int add_host(Ring* r, const double* const src[], int64_t n, void* stream) {
  TD3_HIP(hipSetDevice(r->device));
  float small[kPutArgFloats];                      // few records: packed here, shipped as launch arguments
  const bool few = n * r->rec <= kPutArgFloats;
  float* stage = few ? small : ensure_stage(r, (size_t)n * r->rec);
  if (!stage) return -2;
  const int last = r->nfield - 1;
  for (int64_t i = 0; i < n; ++i) {
    float* d = stage + (size_t)i * r->rec;
    for (int k = 0; k < last; ++k) {
      const RingField f = r->field[k];
      const double* x = src[k] + i * f.len;
      for (int c = 0; c < f.len; ++c) d[f.off + c] = (float)x[c];
    }
    d[r->o_nd] = (float)(1.0 - src[last][i]);             // my_replay_buffer.py:114
    for (int c = r->o_nd + 1; c < r->rec; ++c) d[c] = 0.f;
  }
  return push_staged(r, stage, n, stream ? (hipStream_t)stream : r->stream);
}

int rb_add(rb_handle* h, const double* state, const double* action, const double* next_state,
           const double* reward, const double* done, int64_t n, void* stream) {
  TD3_ARG(h != nullptr, "null handle");
  TD3_ARG(n >= 0, "n must be >= 0");
  if (n == 0) return 0;
  TD3_ARG(state && action && next_state && reward && done, "null input");
  Ring* r = reinterpret_cast<Ring*>(h);
  TD3_ARG(!r->particles, "rb_add on a particle ring (use rb_add_particles)");
  const double* const src[] = {state, action, next_state, reward, done};
  return add_host(r, src, n, stream);
}

int rb_add_particles(rb_handle* h, const double* feat, const double* part, const double* action,
                     const double* next_feat, const double* next_part, const double* reward,
                     const double* done, int64_t n, void* stream) {
  TD3_ARG(h != nullptr, "null handle");
  TD3_ARG(n >= 0, "n must be >= 0");
  if (n == 0) return 0;
  TD3_ARG(feat && part && action && next_feat && next_part && reward && done, "null input");
  Ring* r = reinterpret_cast<Ring*>(h);
  TD3_ARG(r->particles, "rb_add_particles on a featured ring");
  const double* const src[] = {feat, part, action, next_feat, next_part, reward, done};
  return add_host(r, src, n, stream);
}

int rb_add_records(rb_handle* h, const float* records, int64_t n, void* stream) {
  TD3_ARG(h != nullptr, "null handle");
  TD3_ARG(n >= 0, "n must be >= 0");
  if (n == 0) return 0;
  TD3_ARG(records != nullptr, "null records");
  Ring* r = reinterpret_cast<Ring*>(h);
  TD3_HIP(hipSetDevice(r->device));
  hipStream_t s = stream ? (hipStream_t)stream : r->stream;
  if (n * r->rec <= kPutArgFloats) return push_staged(r, records, n, s);   // launch arguments
  float* stage = ensure_stage(r, (size_t)n * r->rec);
  if (!stage) return -2;
  memcpy(stage, records, (size_t)n * r->rec * sizeof(float));
  return push_staged(r, stage, n, s);
}

// The launch arguments of a device add that stores `rows` ring rows (for a hindsight add: expanded rows).
static RingPutDeviceArgs ring_put_device_args(Ring* r, const float* state, const float* action,
                                              const float* next_state, const float* reward, const float* done,
                                              int64_t rows) {
  RingPutDeviceArgs a{};
  rows = ring_reserve(r, rows, a.skip, a.new_size);
  a.data = reinterpret_cast<float4*>(r->data);
  a.d_size = r->d_size;
  a.state = state;
  a.action = action;
  a.next_state = next_state;
  a.reward = reward;
  a.done = done;
  a.cap = r->cap;
  a.ptr = r->ptr;
  a.n = rows;
  a.sd = r->sd;
  a.ad = r->ad;
  a.o_s2 = r->o_s2;
  a.o_r = r->o_r;
  a.o_nd = r->o_nd;
  a.rec4 = r->rec / 4;
  return a;
}

static int ring_put_device_grid(const RingPutDeviceArgs& a) {
  return (int)std::min<int64_t>((a.n * a.rec4 + 255) / 256, 1024);
}

// The same for a particle ring: src[k] is the device array of field k (the last one, done, is stored as 1 - done).
static RingPutPartArgs ring_put_part_args(Ring* r, const float* const (&src)[kPutSegs], int64_t rows) {
  RingPutPartArgs a{};
  rows = ring_reserve(r, rows, a.skip, a.new_size);
  a.data = reinterpret_cast<float4*>(r->data);
  a.d_size = r->d_size;
  for (int k = 0; k < kPutSegs; ++k) a.seg[k] = RingPutSeg{src[k], r->field[k].off, r->field[k].len};
  a.cap = r->cap;
  a.ptr = r->ptr;
  a.n = rows;
  a.rec = r->rec;
  a.o_nd = r->o_nd;
  a.ntile = (r->rec + kPutTile - 1) / kPutTile;
  return a;
}

int rb_add_device(rb_handle* h, const float* state, const float* action, const float* next_state,
                  const float* reward, const float* done, int64_t n, void* stream) {
  TD3_ARG(n >= 0, "n must be >= 0");
  TD3_ARG(h != nullptr, "null handle");
  if (n == 0) return 0;
  TD3_ARG(state && action && next_state && reward && done, "null input");
  Ring* r = reinterpret_cast<Ring*>(h);
  TD3_ARG(!r->particles, "rb_add_device on a particle ring (use rb_add_particles_device)");
  const RingPutDeviceArgs a = ring_put_device_args(r, state, action, next_state, reward, done, n);
  return device_add(r, ring_put_device_kernel, a, ring_put_device_grid(a), a.n, a.new_size, stream);
}

int rb_add_particles_device(rb_handle* h, const float* feat, const float* part, const float* action,
                            const float* next_feat, const float* next_part, const float* reward,
                            const float* done, int64_t n, void* stream) {
  TD3_ARG(n >= 0, "n must be >= 0");
  TD3_ARG(h != nullptr, "null handle");
  if (n == 0) return 0;
  TD3_ARG(feat && part && action && next_feat && next_part && reward && done, "null input");
  Ring* r = reinterpret_cast<Ring*>(h);
  TD3_ARG(r->particles, "rb_add_particles_device on a featured ring (use rb_add_device)");
  const RingPutPartArgs a = ring_put_part_args(r, {feat, part, action, next_feat, next_part, reward, done}, n);
  const int grid = (int)std::min<int64_t>(a.n * a.ntile, 4096);
  return device_add(r, ring_put_particles_kernel, a, grid, a.n, a.new_size, stream);
}

// The checks of an rb_hindsight that need no ring (made before the handle is looked at).
static int hindsight_check(const rb_hindsight* hs) {
  TD3_ARG(hs != nullptr, "null hs");
  TD3_ARG(hs->k >= 1 && hs->k <= kMaxRelabels, "hs->k must be in 1..64");
  TD3_ARG(hs->g >= 1 && hs->g <= kMaxGoals, "hs->g must be in 1..8");
  TD3_ARG(hs->goals != nullptr, "null hs->goals");
  TD3_ARG(hs->rewards != nullptr, "null hs->rewards");
  for (int a = 0; a < hs->g; ++a) {
    TD3_ARG(hs->cols[a] >= 0, "hs->cols must be non-negative");
    for (int b = 0; b < a; ++b) TD3_ARG(hs->cols[a] != hs->cols[b], "hs->cols must be distinct");
  }
  return 0;
}

static RingHindsight hindsight_args(const rb_hindsight* hs) {
  RingHindsight h{};
  h.goals = hs->goals;
  h.rewards = hs->rewards;
  h.k = hs->k;
  h.g = hs->g;
  for (int a = 0; a < hs->g; ++a) h.cols[a] = hs->cols[a];
  return h;
}

int rb_add_device_hindsight(rb_handle* h, const float* state, const float* action, const float* next_state,
                            const float* reward, const float* done, int64_t n, const rb_hindsight* hs,
                            void* stream) {
  TD3_ARG(n >= 0, "n must be >= 0");
  TD3_RC(hindsight_check(hs));
  TD3_ARG(h != nullptr, "null handle");
  Ring* r = reinterpret_cast<Ring*>(h);
  TD3_ARG(!r->particles, "rb_add_device_hindsight on a particle ring (use rb_add_particles_device_hindsight)");
  for (int a = 0; a < hs->g; ++a) TD3_ARG(hs->cols[a] < r->sd, "hs->cols must be below state_dim");
  if (n == 0) return 0;
  TD3_ARG(state && action && next_state && reward && done, "null input");
  const RingPutDeviceHsArgs a{ring_put_device_args(r, state, action, next_state, reward, done, n * (1 + hs->k)),
                              hindsight_args(hs)};
  return device_add(r, ring_put_device_hs_kernel, a, ring_put_device_grid(a.p), a.p.n, a.p.new_size, stream);
}

int rb_add_particles_device_hindsight(rb_handle* h, const float* feat, const float* part, const float* action,
                                      const float* next_feat, const float* next_part, const float* reward,
                                      const float* done, int64_t n, const rb_hindsight* hs, void* stream) {
  TD3_ARG(n >= 0, "n must be >= 0");
  TD3_RC(hindsight_check(hs));
  TD3_ARG(h != nullptr, "null handle");
  Ring* r = reinterpret_cast<Ring*>(h);
  TD3_ARG(r->particles, "rb_add_particles_device_hindsight on a featured ring (use rb_add_device_hindsight)");
  for (int a = 0; a < hs->g; ++a) TD3_ARG(hs->cols[a] < r->sd, "hs->cols must be below feat_dim");
  if (n == 0) return 0;
  TD3_ARG(feat && part && action && next_feat && next_part && reward && done, "null input");
  const int copies = 1 + hs->k;
  const RingPutPartHsArgs a{
      ring_put_part_args(r, {feat, part, action, next_feat, next_part, reward, done}, n * copies),
      hindsight_args(hs), r->o_s, r->o_s2, r->o_r, r->sd};
  const int64_t src_rows = n - a.p.skip / copies;          // source transitions with a surviving copy
  const int grid = (int)std::min<int64_t>(src_rows * a.p.ntile, 4096);
  return device_add(r, ring_put_particles_hs_kernel, a, grid, a.p.n, a.p.new_size, stream);
}

// The checks of an rb_nstep that need no ring (made before the handle is looked at).
static int nstep_check(const rb_nstep* ns) {
  TD3_ARG(ns != nullptr, "null ns");
  TD3_ARG(ns->n >= 1 && ns->n <= kMaxNstep, "ns->n must be in 1..8");
  TD3_ARG(ns->gamma > 0.0 && ns->gamma <= 1.0, "ns->gamma must be in (0, 1]");
  TD3_ARG(ns->ended != nullptr, "null ns->ended");
  return 0;
}

// The lane a tick of `rows` rows continues (or starts: another rows / n / gamma than the lane's, or a
// lane some other write ended) and the launch arguments that describe it.
static int nstep_begin(Ring* r, int64_t rows, const rb_nstep* ns, RingNstep& s) {
  if (r->ns_rows != rows || r->ns_n != ns->n || r->ns_gamma != ns->gamma) r->ns_nhist = 0;
  if (r->ns_age_rows != rows) {
    TD3_HIP(hipSetDevice(r->device));
    for (int*& age : r->ns_age) {               // hipFree waits for the launches that still use them
      (void)hipFree(age);
      age = nullptr;
    }
    r->ns_age_rows = 0;
    for (int*& age : r->ns_age) TD3_HIP(hipMalloc(&age, (size_t)rows * sizeof(int)));
    r->ns_age_rows = rows;                      // contents unset: nhist = 0 clamps every age to 0
  }
  r->ns_rows = rows;
  r->ns_n = ns->n;
  r->ns_gamma = ns->gamma;
  s = RingNstep{};
  s.age_in = r->ns_age[0];
  s.age_out = r->ns_age[1];
  s.ended = ns->ended;
  s.nhist = r->ns_nhist;
  s.nmax = ns->n - 1;
  for (int j = 0; j < s.nhist; ++j) s.hist[j] = r->ns_hist[j];
  double g = 1.0;                               // gpow[j]: j factors of gamma multiplied left to right, in double
  for (int j = 0; j < kMaxNstep; ++j, g *= ns->gamma) s.gpow[j] = (float)g;
  return 0;
}

// After the launch of a tick that continued a lane of `nhist` ticks and stored its rows at `ptr`.
static void nstep_end(Ring* r, int nhist, int64_t ptr) {
  const int keep = std::min(nhist + 1, r->ns_n - 1);
  for (int j = keep - 1; j > 0; --j) r->ns_hist[j] = r->ns_hist[j - 1];
  if (keep > 0) r->ns_hist[0] = ptr;
  r->ns_nhist = keep;
  std::swap(r->ns_age[0], r->ns_age[1]);
}

int rb_add_device_nstep(rb_handle* h, const float* state, const float* action, const float* next_state,
                        const float* reward, const float* done, int64_t rows, const rb_nstep* ns, void* stream) {
  TD3_ARG(rows >= 0, "rows must be >= 0");
  TD3_RC(nstep_check(ns));
  TD3_ARG(h != nullptr, "null handle");
  Ring* r = reinterpret_cast<Ring*>(h);
  TD3_ARG(!r->particles, "rb_add_device_nstep on a particle ring (use rb_add_particles_device_nstep)");
  TD3_ARG(rows <= r->cap / ns->n, "ns->n * rows must not exceed max_size (an n-step tick is never truncated)");
  if (rows == 0) return 0;
  TD3_ARG(state && action && next_state && reward && done, "null input");
  RingPutDeviceNsArgs a{};
  TD3_RC(nstep_begin(r, rows, ns, a.s));
  a.p = ring_put_device_args(r, state, action, next_state, reward, done, rows);
  a.u2 = r->o_s2 / 4;
  a.per_row = a.p.rec4 + a.s.nhist * (a.p.rec4 - a.u2);
  const int64_t ptr = r->ptr;
  const int grid = (int)std::min<int64_t>((rows * a.per_row + 255) / 256, 1024);
  TD3_RC(device_add(r, ring_put_device_ns_kernel, a, grid, rows, a.p.new_size, stream));
  nstep_end(r, a.s.nhist, ptr);
  return 0;
}

int rb_add_particles_device_nstep(rb_handle* h, const float* feat, const float* part, const float* action,
                                  const float* next_feat, const float* next_part, const float* reward,
                                  const float* done, int64_t rows, const rb_nstep* ns, void* stream) {
  TD3_ARG(rows >= 0, "rows must be >= 0");
  TD3_RC(nstep_check(ns));
  TD3_ARG(h != nullptr, "null handle");
  Ring* r = reinterpret_cast<Ring*>(h);
  TD3_ARG(r->particles, "rb_add_particles_device_nstep on a featured ring (use rb_add_device_nstep)");
  TD3_ARG(rows <= r->cap / ns->n, "ns->n * rows must not exceed max_size (an n-step tick is never truncated)");
  if (rows == 0) return 0;
  TD3_ARG(feat && part && action && next_feat && next_part && reward && done, "null input");
  RingPutPartNsArgs a{};
  TD3_RC(nstep_begin(r, rows, ns, a.s));
  a.p = ring_put_part_args(r, {feat, part, action, next_feat, next_part, reward, done}, rows);
  a.o_s2 = r->o_s2;
  a.o_r = r->o_r;
  const int64_t ptr = r->ptr;
  const int grid = (int)std::min<int64_t>(rows * a.p.ntile, 4096);
  TD3_RC(device_add(r, ring_put_particles_ns_kernel, a, grid, rows, a.p.new_size, stream));
  nstep_end(r, a.s.nhist, ptr);
  return 0;
}

int rb_fill_synthetic(rb_handle* h, int64_t n, float max_action, uint64_t seed, void* stream) {
  TD3_ARG(h != nullptr, "null handle");
  TD3_ARG(n >= 0, "n must be >= 0");
  Ring* r = reinterpret_cast<Ring*>(h);
  TD3_HIP(hipSetDevice(r->device));
  hipStream_t s = stream ? (hipStream_t)stream : r->stream;
  if (n > r->cap) n = r->cap;
  r->normalized = 0;                                 // raw rows again (include/td3.h "dataset normalisation")
  TD3_RC(ring_begin_write(r, s));
  if (n > 0) {
    dim3 grid((unsigned)((n + 3) / 4));
    hipLaunchKernelGGL(fill_kernel, grid, dim3(256), 0, s, r->data, r->rec, r->o_a, r->ad, r->o_r, r->o_nd,
                       r->ptr, n, r->cap, max_action, seed);
    TD3_HIP(hipGetLastError());
  }
  const int64_t new_size = std::min<int64_t>(r->size + n, r->cap);
  hipLaunchKernelGGL(set_i64_kernel, dim3(1), dim3(1), 0, s, r->d_size, new_size);
  TD3_HIP(hipGetLastError());
  return ring_wrote(r, n, new_size, s);
}

// The stand-alone sample of either kind: field k of the drawn records into out[k] ([batch][field[k].len]).
static int sample_fields(Ring* r, float* const out[], int batch, const int64_t* inject_idx, int64_t* idx_out,
                         void* stream) {
  TD3_HIP(hipSetDevice(r->device));
  GatherArgs a = gather_base(r);
  for (int k = 0; k < r->nfield; ++k) a.seg[k] = GatherSeg{out[k], r->field[k].len, 0, r->field[k].off, r->field[k].len};
  a.nseg = r->nfield;
  a.B = a.Bp = batch;
  a.inject_idx = inject_idx;
  a.idx_out = idx_out;
  a.ctr = nullptr;
  a.step = ++r->sample_calls;
  hipStream_t s = stream ? (hipStream_t)stream : r->stream;
  TD3_RC(ring_begin_read(r, s));                     // add() before sample() (main.py:261, :269)
  TD3_RC(launch_gather(a, s));
  return ring_end_read(r, s);
}

int rb_sample(rb_handle* h, int batch, float* state, float* action, float* next_state,
              float* reward, float* not_done, const int64_t* inject_idx, int64_t* idx_out,
              void* stream) {
  TD3_ARG(h != nullptr, "null handle");
  Ring* r = reinterpret_cast<Ring*>(h);
  TD3_ARG(!r->particles, "rb_sample on a particle ring (use rb_sample_particles)");
  TD3_ARG(batch >= 0, "batch must be >= 0");
  TD3_ARG(r->size > 0 || batch == 0 || inject_idx, "sample from an empty buffer");
  TD3_ARG(state && action && next_state && reward && not_done, "null output");
  float* const out[] = {state, action, next_state, reward, not_done};
  return sample_fields(r, out, batch, inject_idx, idx_out, stream);
}

int rb_sample_particles(rb_handle* h, int batch, float* feat, float* part, float* action, float* next_feat,
                        float* next_part, float* reward, float* not_done, const int64_t* inject_idx,
                        int64_t* idx_out, void* stream) {
  TD3_ARG(h != nullptr, "null handle");
  Ring* r = reinterpret_cast<Ring*>(h);
  TD3_ARG(r->particles, "rb_sample_particles on a featured ring");
  TD3_ARG(batch >= 0, "batch must be >= 0");
  TD3_ARG(r->size > 0 || batch == 0 || inject_idx, "sample from an empty buffer");
  TD3_ARG(feat && part && action && next_feat && next_part && reward && not_done, "null output");
  float* const out[] = {feat, part, action, next_feat, next_part, reward, not_done};
  return sample_fields(r, out, batch, inject_idx, idx_out, stream);
}

// ------------------------------------------------------------------ priorities (C-ABI)
int rb_enable_priorities(rb_handle* h, double alpha, double eps, void* stream) {
  TD3_ARG(alpha >= 0.0 && alpha <= 1.0, "alpha must be in [0, 1]");
  TD3_ARG(eps > 0.0, "eps must be positive");
  TD3_ARG(h != nullptr, "null handle");
  Ring* r = reinterpret_cast<Ring*>(h);
  TD3_ARG(!r->pri.on, "priorities are already enabled on this ring");
  TD3_HIP(hipSetDevice(r->device));
  PriTree t;
  t.alpha = alpha;
  t.eps = eps;
  int64_t total = 0;
  for (int64_t n = r->cap;; n = (n + 63) / 64) {      // n nodes at this level, padded to whole groups
    TD3_ARG(t.levels < kMaxPriLevels, "max_size too large for the priority tree");
    t.len[t.levels++] = (n + 63) / 64 * 64;
    total += t.len[t.levels - 1];
    if (n <= 64) break;
  }
  TD3_HIP(hipMalloc(&t.base, (size_t)total * sizeof(float)));
  if (hipMalloc(&t.d_max, sizeof(float)) != hipSuccess) {
    (void)hipFree(t.base);
    set_error("rb_enable_priorities: hipMalloc failed");
    return -2;
  }
  float* at = t.base;
  for (int l = 0; l < t.levels; at += t.len[l++]) t.level[l] = at;
  hipStream_t s = stream ? (hipStream_t)stream : r->stream;
  const float one = 1.0f;
  TD3_HIP(hipMemsetAsync(t.base, 0, (size_t)total * sizeof(float), s));   // the pads stay zero for good
  TD3_HIP(hipMemcpyAsync(t.d_max, &one, sizeof(float), hipMemcpyHostToDevice, s));
  TD3_HIP(hipStreamSynchronize(s));                   // `one` is a pageable host source
  t.on = true;
  r->pri = t;
  TD3_RC(ring_begin_write(r, s));
  TD3_RC(pri_reset(r, r->size, s));
  return ring_end_write(r, s);
}

// The checks shared by rb_set_priorities / rb_update_priorities; *r is set when there is work.
static int priorities_args(rb_handle* h, const int64_t* idx, const float* p, int64_t n, Ring** r) {
  *r = nullptr;
  TD3_ARG(n >= 0, "n must be >= 0");
  TD3_ARG(n == 0 || (idx && p), "null idx / priority array");
  TD3_ARG(h != nullptr, "null handle");
  TD3_ARG(reinterpret_cast<Ring*>(h)->pri.on, "priorities are not enabled on this ring (rb_enable_priorities)");
  if (n > 0) *r = reinterpret_cast<Ring*>(h);
  return 0;
}

static int store_priorities(Ring* r, const int64_t* idx, const float* p, int64_t n, bool td, void* stream) {
  TD3_HIP(hipSetDevice(r->device));
  hipStream_t s = stream ? (hipStream_t)stream : r->stream;
  TD3_RC(ring_begin_write(r, s));
  TD3_RC(ring_store_priorities(r, idx, p, n, td, s));
  return ring_end_write(r, s);
}

int rb_set_priorities(rb_handle* h, const int64_t* idx, const float* p, int64_t n, void* stream) {
  Ring* r;
  TD3_RC(priorities_args(h, idx, p, n, &r));
  return r ? store_priorities(r, idx, p, n, false, stream) : 0;
}

int rb_update_priorities(rb_handle* h, const int64_t* idx, const float* td_abs, int64_t n, void* stream) {
  Ring* r;
  TD3_RC(priorities_args(h, idx, td_abs, n, &r));
  return r ? store_priorities(r, idx, td_abs, n, true, stream) : 0;
}

int rb_sample_prioritized(rb_handle* h, int batch, double beta, const float* inject_u, int64_t* idx_out,
                          float* weight_out, void* stream) {
  TD3_ARG(batch > 0, "batch must be positive");
  TD3_ARG(beta >= 0.0 && beta <= 1.0, "beta must be in [0, 1]");
  TD3_ARG(idx_out && weight_out, "null idx_out / weight_out");
  TD3_ARG(h != nullptr, "null handle");
  Ring* r = reinterpret_cast<Ring*>(h);
  TD3_ARG(r->pri.on, "priorities are not enabled on this ring (rb_enable_priorities)");
  TD3_ARG(r->size > 0, "sample from an empty buffer (size)");
  TD3_HIP(hipSetDevice(r->device));
  hipStream_t s = stream ? (hipStream_t)stream : r->stream;
  TD3_RC(ring_begin_read(r, s));
  TD3_RC(ring_draw_prioritized(r, batch, beta, inject_u, idx_out, nullptr, weight_out, s));
  return ring_end_read(r, s);
}

int rb_get_priorities(const rb_handle* h, int64_t start, int64_t n, float* host_out) {
  TD3_ARG(h && host_out, "null argument");
  const Ring* r = reinterpret_cast<const Ring*>(h);
  TD3_ARG(r->pri.on, "priorities are not enabled on this ring (rb_enable_priorities)");
  TD3_ARG(start >= 0 && n >= 0 && start + n <= r->cap, "range out of bounds");
  TD3_HIP(hipSetDevice(r->device));
  TD3_HIP(hipDeviceSynchronize());
  TD3_HIP(hipMemcpy(host_out, r->pri.level[0] + start, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

int rb_priority_info(const rb_handle* h, rb_priority_info_t* info) {
  TD3_ARG(h && info, "null argument");
  const Ring* r = reinterpret_cast<const Ring*>(h);
  const PriTree& t = r->pri;
  *info = rb_priority_info_t{};
  if (!t.on) return 0;
  info->enabled = 1;
  info->alpha = t.alpha;
  info->eps = t.eps;
  info->levels = t.levels;
  TD3_HIP(hipSetDevice(r->device));
  TD3_HIP(hipDeviceSynchronize());
  float root[64];
  TD3_HIP(hipMemcpy(root, t.level[t.levels - 1], sizeof(root), hipMemcpyDeviceToHost));
  TD3_HIP(hipMemcpy(&info->max_priority, t.d_max, sizeof(float), hipMemcpyDeviceToHost));
  // the sum a draw takes over the root group: lane 63 of pri_group_scan adds neighbours pairwise
  for (int w = 1; w < 64; w <<= 1)
    for (int i = 0; i < 64; i += 2 * w) root[i] = root[i] + root[i + w];
  info->total = (double)root[0];
  return 0;
}

int rb_read_records(const rb_handle* h, int64_t start, int64_t n, float* out) {
  TD3_ARG(h && out, "null argument");
  const Ring* r = reinterpret_cast<const Ring*>(h);
  TD3_ARG(start >= 0 && n >= 0 && start + n <= r->cap, "range out of bounds");
  TD3_HIP(hipSetDevice(r->device));
  TD3_HIP(hipStreamSynchronize(r->stream));
  TD3_HIP(hipDeviceSynchronize());
  TD3_HIP(hipMemcpy(out, r->data + (size_t)start * r->rec, (size_t)n * r->rec * sizeof(float),
                    hipMemcpyDeviceToHost));
  return 0;
}

int rb_write_records(rb_handle* h, int64_t start, int64_t n, const float* in, int64_t ptr,
                     int64_t size) {
  TD3_ARG(h && in, "null argument");
  Ring* r = reinterpret_cast<Ring*>(h);
  TD3_ARG(start >= 0 && n >= 0 && start + n <= r->cap, "range out of bounds");
  TD3_ARG(ptr >= 0 && ptr < r->cap && size >= 0 && size <= r->cap, "ptr/size out of bounds");
  TD3_HIP(hipSetDevice(r->device));
  TD3_HIP(hipDeviceSynchronize());
  TD3_HIP(hipMemcpy(r->data + (size_t)start * r->rec, in, (size_t)n * r->rec * sizeof(float),
                    hipMemcpyHostToDevice));
  r->ptr = ptr;
  r->size = size;
  r->ns_nhist = 0;                                   // the n-step lane ends with any other write
  r->normalized = 0;                                 // the caller's rows: raw until normalised again
  TD3_HIP(hipMemcpy(r->d_size, &r->size, sizeof(int64_t), hipMemcpyHostToDevice));
  if (r->pri.on) {                                   // the loaded rows are new rows: max_priority each
    TD3_RC(pri_reset(r, r->size, r->stream));
    TD3_HIP(hipStreamSynchronize(r->stream));
  }
  return 0;
}

int rb_sync(rb_handle* h) {
  TD3_ARG(h != nullptr, "null handle");
  Ring* r = reinterpret_cast<Ring*>(h);
  TD3_HIP(hipSetDevice(r->device));
  TD3_HIP(hipStreamSynchronize(r->stream));
  if (r->write_stream) TD3_HIP(hipStreamSynchronize(r->write_stream));   // adds flushed by a learner
  if (r->read_stream) TD3_HIP(hipStreamSynchronize(r->read_stream));
  return 0;
}

}  // extern "C"
