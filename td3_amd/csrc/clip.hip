// Global-norm gradient clipping (include/td3.h, "gradient clipping"): the norm reduction, the
// flat Adam pass that reads its scale from the device, the planner's clipped optimizer tail and the two
// calls above them.  A translation unit of its own: its kernels are a code object of their own, and the
// code object of kernels.hip -- every kernel a learner without clipping launches -- is the one it is
// without the feature (DESIGN.md §4a records why, for bc.hip).
#include "adam_flat.h"
#include "learner.h"

namespace td3 {

// The gnorm stage's grid, a function of the arena's size alone: one workgroup per 4096 floats, kClipMaxWg
// at the most.  The reduction order below depends on (n, W) only -- not on the batch, the launch mode or
// the dW kernel that produced G.
static int clip_wgs(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(kClipMaxWg, (n + 4095) / 4096)); }

// Workgroup b owns the float4s [b * per, min((b + 1) * per, n4)) of G.  Thread t widens and squares its
// float4s t, t + 256, ... of the slice in ascending order, each float4 as x, y, z, w, adding into one fp64
// accumulator (a product of two widened floats is exact in fp64); the 256 accumulators are added by a
// fixed binary tree in LDS (stride 128, 64, ... 1); thread 0 writes the workgroup's partial.
//
// The sum runs over the whole arena range [0, n), pads included, so it relies on every pad element of G
// being zero behind a gradient-only dW stage.  That holds because
//  - the arenas are zeroed when the handle is created (td3_create) and G has no writer but the dW stages
//    in kDwGrad mode (and the data-parallel sums of such arenas, which clipping refuses);
//  - the matrix tiles of dw_kernel / dw64_kernel and of dwsk_combine_kernel store whole [Np][Kp]
//    matrices: columns k >= kvalid are stored as 0.f explicitly, rows n >= N are sums over dZ's pad
//    columns, which the backward stages keep at zero (the layout invariant the GEMM prologues rely on);
//  - their vector tiles (bias, LayerNorm affine; apply_grads in kDwGrad mode) and enc_adam_kernel store
//    live elements only, so the pads between tensors keep the zeros of the allocation.
__global__ __launch_bounds__(256) void grad_sqsum_kernel(const float* G, int64_t n4, int64_t per, ClipDev* dev) {
  __shared__ double red[256];
  const int64_t b0 = (int64_t)blockIdx.x * per;
  const int64_t b1 = b0 + per < n4 ? b0 + per : n4;
  double acc = 0.0;
  for (int64_t i = b0 + threadIdx.x; i < b1; i += 256) {
    const float4 g = gld4(G + 4 * i);
    acc = acc + (double)g.x * (double)g.x;
    acc = acc + (double)g.y * (double)g.y;
    acc = acc + (double)g.z * (double)g.z;
    acc = acc + (double)g.w * (double)g.w;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) dev->partial[blockIdx.x] = red[0];
}

// adam_flat_kernel (kernels_optim.h; the loop both share is adam_flat_range, adam_flat.h) with the gradient's
// scale read from the device: every workgroup adds
// the W partials itself, in index order, and forms coef -- the same bits in every workgroup, no extra
// launch, no atomics (the precedent: TD3+BC's lambda).  clip_grad_norm_'s arithmetic in
// fp64: total = sqrt(sum), c = max_norm / (total + 1e-6), coef = c > 1 ? 1 : c (a NaN passes through, as
// torch's clamp does; there is no guard for a non-finite total), rounded to fp32 once.  Workgroup 0 leaves
// (total, coef) for td3_clip_info.  G is not scaled in place.
__global__ __launch_bounds__(256) void adam_flat_clip_kernel(AdamArgs a, int64_t n, int polyak, W4Map w,
                                                             ClipDev* dev, int W) {
  double sum = 0.0;
  for (int i = 0; i < W; ++i) sum = sum + dev->partial[i];
  const double total = sqrt(sum);
  const double c = dev->max_norm / (total + 1e-6);
  const float coef = (float)(c > 1.0 ? 1.0 : c);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    dev->total = total;
    dev->coef = coef;
  }
  AdamK k = make_adam(a);
  k.gscale = coef;
  adam_flat_range(a, n, polyak, w, k);
}

static int launch_grad_sqsum(const float* G, int64_t n, ClipDev* dev, hipStream_t s) {
  if ((n & 3) || ((uintptr_t)G & 15) || !dev) {
    set_error("launch_grad_sqsum: the arena must be float4-aligned (n %% 4 == 0, 16-B aligned)");
    return -1;
  }
  const int W = clip_wgs(n);
  const int64_t n4 = n >> 2, per = (n4 + W - 1) / W;
  hipLaunchKernelGGL(grad_sqsum_kernel, dim3(W), dim3(256), 0, s, G, n4, per, dev);
  TD3_HIP(hipGetLastError());
  return 0;
}

static int launch_adam_flat_clip(const AdamArgs& a, int64_t n, int polyak, const W4Map& wm, ClipDev* dev,
                                 hipStream_t s) {
  TD3_ARG(dev != nullptr, "internal: launch_adam_flat_clip without its device state");
  W4Map w;
  int blocks;
  TD3_RC(adam_flat_args("launch_adam_flat_clip", a, n, polyak, &wm, &w, &blocks));
  hipLaunchKernelGGL(adam_flat_clip_kernel, dim3(blocks), dim3(256), 0, s, a, n, polyak, w, dev, clip_wgs(n));
  TD3_HIP(hipGetLastError());
  return 0;
}

// The clipped optimizer tail of a group behind its gradient-only dW stage (`adam`: what the fused step would
// have used): <tag>_gnorm, then <tag>_adam with Polyak and the k-quad images as dp.hip's flat_adam arranges them.
int add_clip_optimizer(td3_handle* h, std::vector<Stage>& st, Group& g, const AdamArgs& adam, bool polyak,
                       const char* tag) {
  TD3_ARG(h->d_clip != nullptr && g.wn.nlin == 0, "internal: clipped optimizer tail without its device state");
  ClipDev* dev = h->d_clip + (adam.which == 1 ? 0 : 1);    // AdamArgs::which 1 = actor -> group 0
  const float* G = g.G;
  const int64_t n = g.size;
  W4Map wm{};
  TD3_RC(w4_map(h, g, 0, &wm));
  AdamArgs a = adam;
  a.grad_scale = 1.0f;                                     // the kernel takes coef in its place
  const int pol = polyak ? 1 : 0;
  st.push_back({std::string(tag) + "_gnorm", [=](hipStream_t s) { return launch_grad_sqsum(G, n, dev, s); }, 0,
                "td3::grad_sqsum_kernel"});
  st.back().bytes = 4.0 * (double)n;
  st.push_back({std::string(tag) + "_adam", [=](hipStream_t s) { return launch_adam_flat_clip(a, n, pol, wm, dev, s); },
                0, "td3::adam_flat_clip_kernel"});
  return 0;
}

}  // namespace td3

using namespace td3;

extern "C" {

// max_norm lives in the group's device scalar, so a new positive value leaves the plan and its captured
// graphs as they are; switching a group on or off changes its stage list and rebuilds them.
int td3_set_grad_clip(td3_handle* h, int group, double max_norm) {
  TD3_ARG(std::isfinite(max_norm) && max_norm >= 0.0, "max_norm must be finite and >= 0");
  TD3_ARG(group == 0 || group == 1, "group must be 0 (actor) or 1 (critic)");
  TD3_ARG(h != nullptr, "null handle");
  TD3_ARG(h->cfg.norm != 2,
          "td3_set_grad_clip on a weight-normalised learner (norm): its Adam runs on dg / dv inside wn_kernel");
  TD3_ARG(!h->comm && !h->local,
          "td3_set_grad_clip on a data-parallel handle (comm group attached): the norm would belong behind the "
          "all-reduce");
  if (h->clip_max[group] == max_norm) return 0;
  TD3_HIP(hipSetDevice(h->cfg.device));
  // ordered behind every queued step: the handle's stream and, if the last step ran on a caller's, that one
  TD3_HIP(hipStreamSynchronize(h->stream));
  if (h->last_step_stream && h->last_step_stream != h->stream) TD3_HIP(hipStreamSynchronize(h->last_step_stream));
  if (!h->d_clip) {
    TD3_HIP(hipMalloc(&h->d_clip, 2 * sizeof(ClipDev)));
    TD3_HIP(hipMemset(h->d_clip, 0, 2 * sizeof(ClipDev)));
  }
  const bool toggles = (h->clip_max[group] > 0.0) != (max_norm > 0.0);
  TD3_HIP(hipMemcpy(&h->d_clip[group].max_norm, &max_norm, sizeof(double), hipMemcpyHostToDevice));
  h->clip_max[group] = max_norm;
  if (!toggles) return 0;
  h->clip_step[group] = 0;
  h->clip_has[group] = false;
  if (h->plan) TD3_RC(build_plan(h, h->plan->B));
  return 0;
}

int td3_clip_info(td3_handle* h, td3_clip_info_t* info) {
  TD3_ARG(info != nullptr, "null info");
  TD3_ARG(h != nullptr, "null handle");
  *info = td3_clip_info_t{};
  for (int g = 0; g < 2; ++g) {
    info->enabled[g] = h->clip_max[g] > 0.0 ? 1 : 0;
    info->max_norm[g] = h->clip_max[g];
  }
  if (!h->d_clip || !h->plan || (!h->clip_has[0] && !h->clip_has[1])) return 0;
  TD3_HIP(hipSetDevice(h->cfg.device));
  TD3_HIP(hipDeviceSynchronize());              // the last step may sit on a caller's stream
  for (int g = 0; g < 2; ++g) {
    if (!h->clip_has[g] || h->clip_max[g] <= 0.0) continue;
    double total = 0.0;
    float coef = 0.f;
    TD3_HIP(hipMemcpy(&total, &h->d_clip[g].total, sizeof(double), hipMemcpyDeviceToHost));
    TD3_HIP(hipMemcpy(&coef, &h->d_clip[g].coef, sizeof(float), hipMemcpyDeviceToHost));
    info->step[g] = h->clip_step[g];
    info->grad_norm[g] = total;
    info->coef[g] = (double)coef;
  }
  return 0;
}

}  // extern "C"
