// The filtered BC term (include/td3.h, "BC on the demonstration rows, Q-filter"): the masked form of the
// actor-head backward row launch, kRowActorHeadBwdBcF.  A translation unit of its own, as bc.hip is: its four
// kernels are a code object of their own, and the code objects of kernels.hip and bc.hip -- every kernel a
// learner with both switches off launches -- are the ones they are without the feature.
#include "row_actor.h"

namespace td3 {

template <bool NORM, int RW = kRowWaves>
__global__ __launch_bounds__(64 * RW) void row_bcf_kernel(int Bp, GemmTable tab) {   // as row_kernel (kernels_rows.h)
  const GemmProb& P = tab.p[blockIdx.y];
  const RowCtx c{(int)(blockIdx.x * RW + (threadIdx.x >> 6)), (int)(threadIdx.x & 63), Bp};
  row_actor_head_bwd<NORM, RW, kBcFiltered>(P, c);
}

// d: the table with its wide problems marked, lds: the wide stage's bytes (launch_rows, kernels_launch.h)
int launch_rows_bcf(const GemmTable& d, int lds, int Bp, hipStream_t s) {
  const dim3 grid(Bp / kRowWaves, d.nprob), wgrid(Bp / kWideRows, d.nprob);
  if (d.p[0].norm) {
    if (lds) hipLaunchKernelGGL((row_bcf_kernel<true, kWideRows>), wgrid, dim3(64 * kWideRows), lds, s, Bp, d);
    else hipLaunchKernelGGL((row_bcf_kernel<true>), grid, dim3(64 * kRowWaves), 0, s, Bp, d);
  } else {
    if (lds) hipLaunchKernelGGL((row_bcf_kernel<false, kWideRows>), wgrid, dim3(64 * kWideRows), lds, s, Bp, d);
    else hipLaunchKernelGGL((row_bcf_kernel<false>), grid, dim3(64 * kRowWaves), 0, s, Bp, d);
  }
  return 0;
}

}  // namespace td3
