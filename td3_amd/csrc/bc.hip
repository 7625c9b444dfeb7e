// TD3+BC (include/td3.h, "TD3+BC"): the BC form of the actor-head backward row launch, kRowActorHeadBwdBc.
// A translation unit of its own: its four kernels are a code object of their own, and the code object of
// kernels.hip -- every kernel a learner without BC launches -- is the one it is without the feature.
#include "row_actor.h"

namespace td3 {

template <bool NORM, int RW = kRowWaves>
__global__ __launch_bounds__(64 * RW) void row_bc_kernel(int Bp, GemmTable tab) {   // as row_kernel (kernels_rows.h)
  const GemmProb& P = tab.p[blockIdx.y];
  const RowCtx c{(int)(blockIdx.x * RW + (threadIdx.x >> 6)), (int)(threadIdx.x & 63), Bp};
  row_actor_head_bwd<NORM, RW, true>(P, c);
}

// d: the table with its wide problems marked, lds: the wide stage's bytes (launch_rows, kernels_launch.h)
int launch_rows_bc(const GemmTable& d, int lds, int Bp, hipStream_t s) {
  const dim3 grid(Bp / kRowWaves, d.nprob), wgrid(Bp / kWideRows, d.nprob);
  if (d.p[0].norm) {
    if (lds) hipLaunchKernelGGL((row_bc_kernel<true, kWideRows>), wgrid, dim3(64 * kWideRows), lds, s, Bp, d);
    else hipLaunchKernelGGL((row_bc_kernel<true>), grid, dim3(64 * kRowWaves), 0, s, Bp, d);
  } else {
    if (lds) hipLaunchKernelGGL((row_bc_kernel<false, kWideRows>), wgrid, dim3(64 * kWideRows), lds, s, Bp, d);
    else hipLaunchKernelGGL((row_bc_kernel<false>), grid, dim3(64 * kRowWaves), 0, s, Bp, d);
  }
  return 0;
}

}  // namespace td3
