// Demonstration replay (include/td3.h, "Demonstration replay"): the input launch of td3_train_step_mixed,
// one gather that fills the plan's batch buffers from two rings.  A translation unit of its own: its two
// kernels are a code object of their own, and the code objects of replay.hip and kernels.hip -- every
// kernel a learner that never takes a mixed step launches -- are the ones they are without the feature.
#include "replay.h"

namespace td3 {

// One wave per batch row, as gather_kernel (replay.hip): row < n_demo reads side 0, else side 1.  The
// draw is gather_row_index's on the row's own ring: philox_index(seed, total_it + 1, row, size).
struct MixedRow {
  const float* rec;    // the sampled record, null for a pad row
};

__device__ __forceinline__ MixedRow mixed_row(const MixedArgs& a, int row, int lane) {
  if (row >= a.B) return MixedRow{nullptr};
  const bool demo = row < a.n_demo;
  const float* data = demo ? a.side[0].data : a.side[1].data;
  int64_t idx;
  if (a.inject_idx) {
    idx = a.inject_idx[row];
  } else {
    const int64_t* d_size = demo ? a.side[0].d_size : a.side[1].d_size;
    const uint64_t seed = demo ? a.side[0].seed : a.side[1].seed;
    const uint64_t size = (uint64_t)*d_size;      // issued alongside the counter load
    const uint64_t step = (uint64_t)(a.ctr->total_it + 1);
    idx = (int64_t)philox_index(seed, step, (uint32_t)row, size);
  }
  if (a.idx_out && lane == 0) a.idx_out[row] = idx;
  return MixedRow{data + (size_t)idx * a.rec};
}

// A particle block of an unstaged record (n floats, 4-B aligned at both ends: F and N*D are free) into
// its packed batch row.  Up to three head floats bring the source to 16 B (records are 16-B aligned);
// the body is read as float4, kInFlight loads per lane issued before the first store, so a 3000-float
// block is 2 HBM round trips instead of the 47 of a dword load-store loop.  Loads are clamped, not
// guarded, so none sinks behind a branch.  The destination keeps whatever alignment the head leaves
// it: float4 stores when that is 16 B, four dword stores per lane otherwise.  s null: zeros (pad rows).
constexpr int kInFlight = 8;
__device__ __forceinline__ void copy_block(float* __restrict__ d, const float* __restrict__ s, int n, int lane) {
  if (!s) {
    for (int c = lane; c < n; c += 64) d[c] = 0.f;
    return;
  }
  const int head = min(n, (int)((4 - ((reinterpret_cast<uintptr_t>(s) >> 2) & 3)) & 3));
  if (lane < head) d[lane] = s[lane];
  s += head;
  d += head;
  n -= head;
  const int n4 = n >> 2;
  const bool d16 = (reinterpret_cast<uintptr_t>(d) & 15) == 0;
  const float4* s4 = reinterpret_cast<const float4*>(s);
  for (int q0 = 0; q0 < n4; q0 += 64 * kInFlight) {
    float4 v[kInFlight];
#pragma unroll
    for (int i = 0; i < kInFlight; ++i) v[i] = s4[min(q0 + lane + 64 * i, n4 - 1)];
#pragma unroll
    for (int i = 0; i < kInFlight; ++i) {
      const int q = q0 + lane + 64 * i;
      if (q >= n4) continue;
      if (d16) {
        reinterpret_cast<float4*>(d)[q] = v[i];
      } else {
        d[4 * q] = v[i].x;
        d[4 * q + 1] = v[i].y;
        d[4 * q + 2] = v[i].z;
        d[4 * q + 3] = v[i].w;
      }
    }
  }
  const int c = 4 * n4 + lane;
  if (c < n) d[c] = s[c];
}

template <bool STAGED>
__global__ __launch_bounds__(256) void mixed_gather_kernel(MixedArgs a) {
  __shared__ float rec_lds[STAGED ? 4 : 1][STAGED ? kMaxRecord : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wave;
  if (row >= a.Bp) return;
  const MixedRow m = mixed_row(a, row, lane);
  const bool live = m.rec != nullptr;
  if constexpr (STAGED) {
    // the record through the wave's LDS slot, float4 stores to 16-B aligned segment rows (gather_kernel)
    float* lr = rec_lds[wave];
    if (live) {
      const float4* src = reinterpret_cast<const float4*>(m.rec);
      constexpr int kPer = kMaxRecord / 4 / 64;
      const int n4 = a.rec >> 2;
      float4 v[kPer];
#pragma unroll
      for (int i = 0; i < kPer; ++i) v[i] = src[min(lane + 64 * i, n4 - 1)];  // unguarded: clamped
#pragma unroll
      for (int i = 0; i < kPer; ++i) reinterpret_cast<float4*>(lr)[lane + 64 * i] = v[i];
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
    for (int s = 0; s < a.nseg; ++s) {
      const GatherSeg g = a.seg[s];
      float* d = g.dst + (size_t)row * g.ld + g.col;
      for (int c = lane; c < g.len; c += 64) d[c] = live ? m.rec[g.src + c] : 0.f;
    }
    if (a.pbatch) {
      float* d = a.pbatch + (size_t)row * 2 * a.np;
      copy_block(d, live ? m.rec + a.o_p : nullptr, a.np, lane);
      copy_block(d + a.np, live ? m.rec + a.o_p2 : nullptr, a.np, lane);
    }
  }
}

int launch_mixed_gather(const MixedArgs& args, hipStream_t s) {
  if (args.Bp <= 0) return 0;
  MixedArgs a = args;
  const dim3 grid((a.Bp + 3) / 4);
  if (a.rec <= kMaxRecord) {
    if (a.pbatch) {     // the blocks leave the LDS slot as two more segments
      a.seg[a.nseg++] = GatherSeg{a.pbatch, 2 * a.np, 0, a.o_p, a.np};
      a.seg[a.nseg++] = GatherSeg{a.pbatch, 2 * a.np, a.np, a.o_p2, a.np};
      a.pbatch = nullptr;
    }
    hipLaunchKernelGGL(mixed_gather_kernel<true>, grid, dim3(256), 0, s, a);
  } else {
    hipLaunchKernelGGL(mixed_gather_kernel<false>, grid, dim3(256), 0, s, a);
  }
  TD3_HIP(hipGetLastError());
  return 0;
}

}  // namespace td3
