// Part of kernels.hip: the flat passes of the data-parallel path (adam_flat_kernel, local_sum_kernel,
// polyak_flat_kernel) and weight normalisation (wn_kernel).
// Needs dev.h (AdamK, make_adam, adam_elem) and kernels.h (AdamArgs, W4Map, LocalSumArgs, WnArgs).
#pragma once
#include "adam_flat.h"
#include "dev.h"
#include "kernels.h"

namespace td3 {

// The flat optimizer pass of the data-parallel path (after the all-reduce): adam_flat_range (adam_flat.h).
__global__ __launch_bounds__(256) void adam_flat_kernel(AdamArgs a, int64_t n, int polyak, W4Map w) {
  adam_flat_range(a, n, polyak, w, make_adam(a));
}

__global__ __launch_bounds__(256) void local_sum_kernel(LocalSumArgs a) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.size; i += (int64_t)gridDim.x * 256) {
    float v = gld(a.a[0] + i);
    for (int k = 1; k < a.n; ++k) v = v + gld(a.a[k] + i);
    for (int k = 0; k < a.n; ++k) gst(a.a[k] + i, v);
  }
}

__global__ __launch_bounds__(256) void polyak_flat_kernel(float* T, const float* P, int64_t n, float tau,
                                                          float omt) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    gst(T + i, tau * gld(P + i) + omt * gld(T + i));
}

// ================================================================== weight normalization
// One wave per output row of a weight-normalised Linear (K <= 512: 8 columns per lane).
// kWnAdam: the row's dL/dW (G arena, dw_kernel in kDwGrad mode, all-reduced when data
// parallel) becomes torch's weight_norm backward
//   dg = (dW . v) / ||v||,   dv = (g / ||v||) dW - (g (dW . v) / ||v||^3) v
// then Adam on (bias, g, v) with the group's moments (adam_elem, + Polyak of the targets) and
// the row of W = v * (g / ||v||) is derived again from the updated parameters (and targets).
__device__ __forceinline__ float wn_norm(const float (&v)[8], int K, int lane) {
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (rcol(lane, j) < K) q += v[j] * v[j];
  return sqrtf(wsum(q));
}

__device__ __forceinline__ void wn_store_w(float* arena, const WnLinear& L, int i, int lane, float (&v)[8],
                                           float g) {
  const float sc = g / wn_norm(v, L.K, lane);
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = v[j] * sc;
  rv_store(arena + L.offW + (size_t)i * L.ld, L.K, lane, v);
}

__device__ __forceinline__ float lane0(float x) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 0));
}

__global__ __launch_bounds__(256) void wn_kernel(WnArgs a) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= a.rows) return;
  int l = 0;
  while (l + 1 < a.nlin && r >= a.lin[l + 1].row0) ++l;
  const WnLinear& L = a.lin[l];
  const int i = r - L.row0;
  float v[8];
  if (a.mode == kWnDerive) {
    for (float* arena : {a.arena, a.arena2}) {
      if (!arena) continue;
      rv_load(v, arena + L.offv + (size_t)i * L.ld, L.K, lane);
      wn_store_w(arena, L, i, lane, v, gld(arena + L.offg + i));
    }
    return;
  }
  const AdamArgs& A = a.adam;
  float* T = a.polyak ? A.T : nullptr;
  // every operand of the row requested up front: v, dW, the moments (and targets) of v, and on
  // lane 0 g, the bias and their optimizer state
  const size_t ov = L.offv + (size_t)i * L.ld;
  float gw[8], m[8], w2[8], vt[8];
  rv_load(v, A.P + ov, L.K, lane);
  rv_load(gw, A.G + L.offW + (size_t)i * L.ld, L.K, lane);
  rv_load(m, A.M + ov, L.K, lane);
  rv_load(w2, A.V + ov, L.K, lane);
  if (T) rv_load(vt, T + ov, L.K, lane);
  const size_t og = L.offg + i, ob = L.offb + i;
  float sg[4] = {0.f, 0.f, 0.f, 0.f}, sb[4] = {0.f, 0.f, 0.f, 0.f}, gb = 0.f;
  if (lane == 0) {
    sg[0] = gld(A.P + og); sg[1] = gld(A.M + og); sg[2] = gld(A.V + og);
    sb[0] = gld(A.P + ob); sb[1] = gld(A.M + ob); sb[2] = gld(A.V + ob);
    gb = gld(A.G + ob);
    if (T) { sg[3] = gld(T + og); sb[3] = gld(T + ob); }
  }
  const AdamK k = make_adam(A);
  const float g = lane0(sg[0]);
#pragma unroll
  for (int j = 0; j < 8; ++j) gw[j] *= k.gscale;
  const float n = wn_norm(v, L.K, lane);
  const float sdot = wsum(rv_pdot(gw, v, L.K, lane));
  const float ca = g / n;
  const float cb = ca * sdot / (n * n);
  const float dg = sdot / n;
  // v: element-wise Adam in registers (pads stay 0: zero grads and moments)
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float d = ca * gw[j] - cb * v[j];
    if (rcol(lane, j) < L.K) {
      adam_regs(v[j], m[j], w2[j], d, k);
      if (T) vt[j] = k.tau * v[j] + k.omt * vt[j];        // TD3_featured.py:167-171
    }
  }
  rv_store(A.P + ov, L.K, lane, v);
  rv_store(A.M + ov, L.K, lane, m);
  rv_store(A.V + ov, L.K, lane, w2);
  if (T) rv_store(T + ov, L.K, lane, vt);
  if (lane == 0) {
    adam_regs(sg[0], sg[1], sg[2], dg, k);
    adam_regs(sb[0], sb[1], sb[2], gb * k.gscale, k);
    pst(A.P + og, sg[0]); sst(A.M + og, sg[1]); sst(A.V + og, sg[2]);
    pst(A.P + ob, sb[0]); sst(A.M + ob, sb[1]); sst(A.V + ob, sb[2]);
    if (T) {
      sg[3] = k.tau * sg[0] + k.omt * sg[3];
      sb[3] = k.tau * sb[0] + k.omt * sb[3];
      gst(T + og, sg[3]);
      gst(T + ob, sb[3]);
    }
  }
  const float gn = lane0(sg[0]), gt = lane0(sg[3]);
  wn_store_w(A.P, L, i, lane, v, gn);
  if (T) wn_store_w(T, L, i, lane, vt, gt);
}

}  // namespace td3
