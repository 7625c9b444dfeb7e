// Part of kernels.hip: the query path (select_action / eval_q): head_kernel, the small-query hidden layers
// gemv_kernel and gemv01_kernel, and the one-launch act_kernel.
// Needs dev.h and kernels.h only (HeadArgs, GemvArgs, Gemv01Args, ActArgs); kernels_timeline.h for the marks.
#pragma once
#include "dev.h"
#include "kernels.h"
#include "kernels_timeline.h"

namespace td3 {

// ================================================================== act / eval_q heads
__global__ __launch_bounds__(256) void head_kernel(HeadArgs a) {
  const HeadProb P = a.probs[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.Bp) return;
  float x[1][8], g[8], bb[8], mean[1], rstd[1];
  const int ld = P.ldh;
  rv_load(x[0], P.H3 + (size_t)row * ld, ld, lane);
  if (P.lng) {
    rv_load(g, P.lng, ld, lane);
    rv_load(bb, P.lnb, ld, lane);
    ln_fwd_rows<1>(x, g, bb, P.K3, lane, mean, rstd);
    if (P.stats && lane == 0) {
      gst(P.stats + (row), mean[0]);
      gst(P.stats + (a.Bp + row), rstd[0]);
    }
  }
  if (P.U3) rv_store(P.U3 + (size_t)row * P.ldu, P.ldu, lane, x[0]);
  float zl = 0.f;
  for (int o = 0; o < P.nout; ++o) {
    float w[8];
    rv_load(w, P.W4 + (size_t)o * P.ldw, P.ldw, lane);
    const float z = wsum(rv_pdot(x[0], w, P.K3, lane)) + gld(P.b4 + (o));
    if (lane == o) zl = z;
  }
  if (lane >= P.nout) return;
  const int o = lane;
  const bool live = row < a.B;
  if (P.mode == kHeadPolicy) {
    const float th = tanhf(zl);
    gst(P.out + ((size_t)row * P.ldo + P.out_col + o), live ? a.max_action * th : 0.f);
    if (P.tanh_out) gst(P.tanh_out + ((size_t)row * 32 + o), th);
  } else {
    gst(P.out + ((size_t)row * P.ldo + o), zl);          // Q values [row][nout]
  }
}

// ================================================================== small-query hidden layers
// One wave per 4 output columns of one network (blockIdx.y): the wave loads its 4 weight rows
// and the R query rows (lane-sliced, K <= 512), applies the input LayerNorm (the GEMM prologue's
// packed form: pads of X, gamma, beta are zero) and reduces the 4R dot products.
template <int R>
__global__ __launch_bounds__(256) void gemv_kernel(GemvArgs a) {
  const GemvProb& P = a.p[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int o0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 4;
  if (o0 >= P.N) return;
  float w[4][8], x[R][8];
#pragma unroll
  for (int j = 0; j < 4; ++j) rv_load(w[j], P.W + (size_t)min(o0 + j, P.N - 1) * P.ldw, P.K, lane);
#pragma unroll
  for (int r = 0; r < R; ++r) rv_load(x[r], P.X + (size_t)min(r, a.B - 1) * P.ldx, P.K, lane);
  if (P.lng) {
    float g[8], bb[8], rm[8], mean[R], rstd[R];
    rv_load(g, P.lng, P.K, lane);
    rv_load(bb, P.lnb, P.K, lane);
    real_mask(rm, P.K, lane);
    ln_fwd_rows_pk<R>(x, g, bb, rm, 1.0f / (float)P.K, mean, rstd);
  }
  float z[4][R];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < R; ++r) z[j][r] = wsum(rv_pdot(x[r], w[j], P.K, lane));
  // lane 4r + j stores column o0 + j of row r
  const int j = lane & 3, r = lane >> 2;
  if (r < R && r < a.B && o0 + j < P.N) {
    float v = 0.f;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
      for (int rr = 0; rr < R; ++rr)
        if (jj == j && rr == r) v = z[jj][rr];
    gst(P.Y + (size_t)r * P.ldy + o0 + j, fmaxf(v + gld(P.b + o0 + j), 0.f));
  }
}

template <int R>
__global__ __launch_bounds__(256) void gemv01_kernel(Gemv01Args a) {
  __shared__ float h0[R][512];
  const GemvProb& P = a.l1.p[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int o0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 4;
  float w[4][8], x[R][8];
#pragma unroll
  for (int j = 0; j < 4; ++j) rv_load(w[j], P.W + (size_t)min(o0 + j, P.N - 1) * P.ldw, P.K, lane);
  // H0 (all N0 columns, zero pads) into LDS; W0 pads past K0 are zero, so the float4 steps may
  // read past a row's K0 query values (xq is zero past B*K0 and padded by 4)
  const float* W0 = a.W0[blockIdx.y];
  const float* b0 = a.b0[blockIdx.y];
  for (int o = threadIdx.x; o < 512; o += 256) {
    float z[R];
#pragma unroll
    for (int r = 0; r < R; ++r) z[r] = 0.f;
    if (o < a.N0) {
      const float* wr = W0 + (size_t)o * a.ldw0;
      for (int c = 0; c < a.K0; c += 4) {
        const float4 wv = gld4(wr + c);
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const float* q = a.xq + r * a.K0 + c;
          z[r] += wv.x * q[0];
          z[r] += wv.y * q[1];
          z[r] += wv.z * q[2];
          z[r] += wv.w * q[3];
        }
      }
      const float bo = gld(b0 + o);
#pragma unroll
      for (int r = 0; r < R; ++r) z[r] = fmaxf(z[r] + bo, 0.f);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) h0[r][o] = z[r];
  }
  __syncthreads();
  if (o0 >= P.N) return;
#pragma unroll
  for (int r = 0; r < R; ++r) rv_load_lds(x[r], h0[r], P.K, lane);
  if (P.lng) {
    float g[8], bb[8], rm[8], mean[R], rstd[R];
    rv_load(g, P.lng, P.K, lane);
    rv_load(bb, P.lnb, P.K, lane);
    real_mask(rm, P.K, lane);
    ln_fwd_rows_pk<R>(x, g, bb, rm, 1.0f / (float)P.K, mean, rstd);
  }
  float z[4][R];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < R; ++r) z[j][r] = wsum(rv_pdot(x[r], w[j], P.K, lane));
  const int j = lane & 3, r = lane >> 2;
  if (r < R && r < a.l1.B && o0 + j < P.N) {
    float v = 0.f;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
      for (int rr = 0; rr < R; ++rr)
        if (jj == j && rr == r) v = z[jj][rr];
    gst(P.Y + (size_t)r * P.ldy + o0 + j, fmaxf(v + gld(P.b + o0 + j), 0.f));
  }
}

// ================================================================== one-launch query (select_action)
// select_action / eval_q of n <= kGemvRows rows as ONE launch (TD3_featured.py:113-121; VERDICT
// r04 #6).  Grid (nb, networks) of 256-thread workgroups; workgroup b of network k:
//   1. requests its layer-1 and layer-2 weight rows (4 + 4 per wave: nothing in the launch writes
//      them), computes all of H0 = relu(W0 x + b0) into LDS (the query is in the arguments),
//   2. layer 1, columns 16b .. 16b+15 (LN0 in the prologue), stored write-through (sc1),
//   3. hands off: every storing wave drains its stores, the workgroup meets at a barrier, one lane
//      adds to the network's layer-1 counter; one lane polls it (sc1 loads) up to nb arrivals,
//   4. layer 2, the same 16 columns, from the H1 rows read with sc1 loads (LN1), stored sc1,
//   5. arrives on the network's second counter; the LAST arriver (the value its add returned) reads
//      H2 with sc1 loads, applies LN2 and the head, writes the outputs and zeroes both counters
//      (every workgroup has passed its layer-1 poll before its second add).
// The hand-off is MI355X_MICROARCH.md's sc1 form (stores and loads of the handed-off rows all sc1,
// each storing wave's vmcnt(0) before the workgroup barrier, one agent-scope atomic per workgroup).
// A poll that sees no progress for ~2^22 rounds gives up and the outputs are NaN (no hang).
__device__ __forceinline__ float ald(const float* p) {
  return __hip_atomic_load((const GAS float*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void ast(float* p, float v) {
  __hip_atomic_store((GAS float*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void rv_load_sc1(float (&v)[8], const float* row, int n, int lane) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = rcol(lane, j);
    v[j] = c < n ? ald(row + c) : 0.f;
  }
}

template <int R, int KQ>    // KQ: float4 steps of a layer-0 row (K0 <= 4 * KQ)
__global__ __launch_bounds__(256) void act_kernel(ActArgs a) {
  __shared__ float h0[R][512];
  __shared__ int s_flag;
  TL_MARK(0);
  const int k = blockIdx.y;
  const GemvProb& P1 = a.g.l1.p[k];
  const GemvProb& P2 = a.l2[k];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int B = a.g.l1.B;
  const int o0 = (blockIdx.x * 4 + wave) * 4;            // this wave's 4 columns of layers 1 and 2
  int* c1 = a.ctr + 2 * k;
  int* c2 = c1 + 1;
  // layer 0's weights first (H0 waits for them alone: vmcnt retires in order), coalesced: thread t
  // holds columns 4*kg .. 4*kg + 3 (kg = t % TPR) of rows rsub + RPP*i, a wave's loads whole
  // contiguous rows (one row per thread was a 64-line scatter per load: ~2 us of H0, act_tl.py)
  const float* W0 = a.g.W0[k];
  const float* b0 = a.g.b0[k];
  constexpr int LW = 4 * KQ;                  // W0 row stride (floats): 32 or 64
  constexpr int TPR = LW / 4, RPP = 256 / TPR, NPASS = 512 / RPP;
  const int kg = threadIdx.x % TPR, rsub = threadIdx.x / TPR;
  float4 w0r[NPASS];
  float b0r[NPASS];
#pragma unroll
  for (int i = 0; i < NPASS; ++i) {           // unconditional (rows past N0 clamp; pads are zero)
    const int o = min(rsub + RPP * i, a.g.N0 - 1);
    w0r[i] = gld4(W0 + (size_t)o * LW + 4 * kg);
    b0r[i] = gld(b0 + o);
  }
  float xr[R][4];                             // the query values of this thread's 4 columns (xq is
#pragma unroll                                // zero past B*K0; past K0 the weights are zero)
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) xr[r][jj] = a.g.xq[min(r * a.g.K0 + 4 * kg + jj, kGemvQ - 1)];
  // layer 1's operands; layer 2's and the head's are requested after the layer-1 hand-off (in
  // flight together with W0 they held H0 ~3 us behind the CU's ~70 GB/s L2 rate, act_tl.py)
  float w1[4][8], w2[4][8];
#pragma unroll
  for (int j = 0; j < 4; ++j) rv_load(w1[j], P1.W + (size_t)min(o0 + j, P1.N - 1) * P1.ldw, P1.K, lane);
  float g1[8], bb1[8], g2[8], bb2[8], rm1[8], rm2[8];
  if (P1.lng) {
    rv_load(g1, P1.lng, P1.K, lane);
    rv_load(bb1, P1.lnb, P1.K, lane);
  }
  real_mask(rm1, P1.K, lane);
  real_mask(rm2, P2.K, lane);
  const float bia1 = gld(P1.b + min(o0 + (lane & 3), P1.N - 1));
  const HeadProb& H = a.head[k];
  constexpr int kPre = 8;
  float w4[kPre][8], hg[8], hb[8];
  // 1. H0 of every query row: 4-column partial dot products, summed over the TPR threads of a row
  //    (butterfly), + b0, ReLU; rows past N0 are zero
#pragma unroll
  for (int i = 0; i < NPASS; ++i) {
    const int o = rsub + RPP * i;
    const float4 w = w0r[i];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float z = w.x * xr[r][0];
      z = z + w.y * xr[r][1];
      z = z + w.z * xr[r][2];
      z = z + w.w * xr[r][3];
#pragma unroll
      for (int m = TPR / 2; m >= 1; m >>= 1) z = z + __shfl_xor(z, m);
      if (kg == 0) h0[r][o] = o < a.g.N0 ? fmaxf(z + b0r[i], 0.f) : 0.f;
    }
  }
  __syncthreads();
  TL_MARK(5);
  const int j = lane & 3, rr = lane >> 2;                // lane 4r + j: column o0 + j of row r
  // 2. layer 1
  if (o0 < P1.N) {
    float x[R][8];
#pragma unroll
    for (int r = 0; r < R; ++r) rv_load_lds(x[r], h0[r], P1.K, lane);
    if (P1.lng) {
      float mean[R], rstd[R];
      ln_fwd_rows_pk<R>(x, g1, bb1, rm1, 1.0f / (float)P1.K, mean, rstd);
    }
    float z[4][R];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
      for (int r = 0; r < R; ++r) z[jj][r] = wsum(rv_pdot(x[r], w1[jj], P1.K, lane));
    if (rr < R && rr < B && o0 + j < P1.N) {
      float v = 0.f;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int r = 0; r < R; ++r)
          if (jj == j && r == rr) v = z[jj][r];
      ast(P1.Y + (size_t)rr * P1.ldy + o0 + j, fmaxf(v + bia1, 0.f));
    }
  }
  // 3. hand-off of H1 (every wave's stores drained before the barrier; one add per workgroup)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  TL_MARK(6);
  const int nb = (int)gridDim.x;
  if (threadIdx.x == 0) __hip_atomic_fetch_add((GAS int*)c1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // layer 2's operands and the head's (any workgroup may arrive last: rows 0..7 of W4, LN2 affine,
  // biases; a head of more outputs loads the rest in its loop), in flight during the poll
#pragma unroll
  for (int j = 0; j < 4; ++j) rv_load(w2[j], P2.W + (size_t)min(o0 + j, P2.N - 1) * P2.ldw, P2.K, lane);
  if (P2.lng) {
    rv_load(g2, P2.lng, P2.K, lane);
    rv_load(bb2, P2.lnb, P2.K, lane);
  }
  const float bia2 = gld(P2.b + min(o0 + (lane & 3), P2.N - 1));
#pragma unroll
  for (int o = 0; o < kPre; ++o) rv_load(w4[o], H.W4 + (size_t)min(o, H.nout - 1) * H.ldw, H.ldw, lane);
  if (H.lng) {
    rv_load(hg, H.lng, H.ldh, lane);
    rv_load(hb, H.lnb, H.ldh, lane);
  }
  const float b4 = lane < H.nout ? gld(H.b4 + lane) : 0.f;
  if (threadIdx.x == 0) {
    int ok = !(a.fail_test && blockIdx.x == 0);
    for (int spin = 0; ok && __hip_atomic_load((GAS int*)c1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < nb; ++spin) {
      if (spin > (1 << 22)) {
        ok = 0;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    s_flag = ok;
  }
  __syncthreads();
  TL_MARK(7);
  const bool ok1 = s_flag != 0;
  // 4. layer 2 on the H1 rows
  if (o0 < P2.N) {
    float x[R][8];
#pragma unroll
    for (int r = 0; r < R; ++r) rv_load_sc1(x[r], P2.X + (size_t)min(r, B - 1) * P2.ldx, P2.K, lane);
    if (P2.lng) {
      float mean[R], rstd[R];
      ln_fwd_rows_pk<R>(x, g2, bb2, rm2, 1.0f / (float)P2.K, mean, rstd);
    }
    float z[4][R];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
      for (int r = 0; r < R; ++r) z[jj][r] = wsum(rv_pdot(x[r], w2[jj], P2.K, lane));
    if (rr < R && rr < B && o0 + j < P2.N) {
      float v = 0.f;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int r = 0; r < R; ++r)
          if (jj == j && r == rr) v = z[jj][r];
      ast(P2.Y + (size_t)rr * P2.ldy + o0 + j, ok1 ? fmaxf(v + bia2, 0.f) : __builtin_nanf(""));
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  TL_MARK(1);
  // arrival on the layer-2 counter; a workgroup whose poll gave up adds kActFailInc too, so the last
  // arriver knows the H2 rows are not all valid and publishes the flag with kActFailed (the host
  // then reports an error and re-zeroes the counters) instead of a valid-looking result
  if (threadIdx.x == 0) {
    const int old = __hip_atomic_fetch_add((GAS int*)c2, ok1 ? 1 : 1 + kActFailInc, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
    const bool last = (old & (kActFailInc - 1)) == nb - 1;
    s_flag = last ? ((old >= kActFailInc || !ok1) ? 2 : 1) : 0;
  }
  __syncthreads();
  TL_MARK(2);
  if (!s_flag) return;
  const bool failed = s_flag == 2;
  // 5. the last arriver: LN2 + head of row `wave` (head_kernel's arithmetic on sc1 loads)
  if (wave < B) {
    float x[1][8], mean[1], rstd[1];
    rv_load_sc1(x[0], H.H3 + (size_t)wave * H.ldh, H.K3, lane);
    if (H.lng) ln_fwd_rows<1>(x, hg, hb, H.K3, lane, mean, rstd);
    float zl = 0.f;
#pragma unroll
    for (int o = 0; o < kPre; ++o) {
      if (o >= H.nout) break;
      const float z = wsum(rv_pdot(x[0], w4[o], H.K3, lane)) + __shfl(b4, o);
      if (lane == o) zl = z;
    }
    for (int o = kPre; o < H.nout; ++o) {
      float w[8];
      rv_load(w, H.W4 + (size_t)o * H.ldw, H.ldw, lane);
      const float z = wsum(rv_pdot(x[0], w, H.K3, lane)) + __shfl(b4, o);
      if (lane == o) zl = z;
    }
    if (lane < H.nout) {
      if (H.mode == kHeadPolicy) gst(H.out + ((size_t)wave * H.ldo + H.out_col + lane), a.max_action * tanhf(zl));
      else gst(H.out + ((size_t)wave * H.ldo + lane), zl);
    }
  }
  // publish: the outputs (mapped host memory) complete, a system-scope release, then this network's
  // flag = the launch's sequence number, which the host polls instead of a stream synchronize
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __hip_atomic_store((GAS int*)c1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next
    __hip_atomic_store((GAS int*)c2, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // launch (stream order)
    if (a.flag) {
      __threadfence_system();
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(a.flag + k, failed ? (a.seq | kActFailed) : a.seq, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  TL_MARK(3);
}

}  // namespace td3
