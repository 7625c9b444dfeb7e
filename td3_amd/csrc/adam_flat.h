// The flat optimizer pass's loop over a range of a group's arenas, shared by adam_flat_kernel (kernels.hip) and
// adam_flat_clip_kernel (clip.hip): one copy of the Adam / Polyak arithmetic and of the k-quad image scatter.
// Needs dev.h (AdamK, adam_regs, gld4 / sst4 / pst4) and kernels.h (AdamArgs, W4Map).
#pragma once
#include "dev.h"
#include "kernels.h"

namespace td3 {

// 4 elements per thread and array as one float4 (arenas and bucket ranges are multiples of 32 floats; the
// launchers check), every load of the 4 elements requested before the first store.  k.gscale scales g.
__device__ __forceinline__ void adam_flat_range(const AdamArgs& a, int64_t n, int polyak, const W4Map& w,
                                                const AdamK& k) {
  const int64_t n4 = n >> 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const int64_t e = 4 * i;
    const float4 g4 = gld4(a.G + e), m4 = gld4(a.M + e), v4 = gld4(a.V + e), p4 = gld4(a.P + e);
    const float4 t4 = gld4((polyak ? a.T : a.P) + e);
    float g[4] = {g4.x * k.gscale, g4.y * k.gscale, g4.z * k.gscale, g4.w * k.gscale};
    float mm[4] = {m4.x, m4.y, m4.z, m4.w}, vv[4] = {v4.x, v4.y, v4.z, v4.w};
    float pp[4] = {p4.x, p4.y, p4.z, p4.w}, tt[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      adam_regs(pp[j], mm[j], vv[j], g[j], k);
      tt[j] = k.tau * pp[j] + k.omt * tt[j];           // TD3_featured.py:167-171
    }
    sst4(a.M + e, make_float4(mm[0], mm[1], mm[2], mm[3]));
    sst4(a.V + e, make_float4(vv[0], vv[1], vv[2], vv[3]));
    pst4(a.P + e, make_float4(pp[0], pp[1], pp[2], pp[3]));
    if (polyak) pst4(a.T + e, make_float4(tt[0], tt[1], tt[2], tt[3]));
    if (w.P4) {                                      // the k-quad images of the weight matrices
      const int64_t j = w.base + e;
      for (int m = 0; m < w.nmat; ++m) {
        const int64_t r = j - w.off[m];
        if (r < 0 || r >= (int64_t)w.Np[m] * w.Kp[m]) continue;
        const int nn = (int)(r / w.Kp[m]), kq = (int)(r - (int64_t)nn * w.Kp[m]) >> 2;
        const int64_t iq = w.off[m] + ((int64_t)kq * w.Np[m] + nn) * 4;
        pst4(w.P4 + iq, make_float4(pp[0], pp[1], pp[2], pp[3]));
        if (polyak) pst4(w.T4 + iq, make_float4(tt[0], tt[1], tt[2], tt[3]));
        break;
      }
    }
  }
}

}  // namespace td3
