// Part of kernels.hip: the TD3_TL in-kernel phase timeline of experiment builds (the TL_MARK / TL_CLK_* /
// TL_FINE marks, which expand to nothing in the product) and the host readers of its device arrays.
// Needs dev.h only; the parts after it place the marks.
#pragma once
#include "dev.h"

namespace td3 {

// In-kernel phase timeline (experiment builds only: tools/build_exp.sh tl "-DTD3_TL"): per
// workgroup, s_memrealtime (100 MHz) at entry / after the prologue barrier / after the MFMA
// loop / after its own stores drained, plus the XCC id.  Read back with td3_tl_read.
#ifdef TD3_TL
__device__ unsigned long long td3_tl[8192][8];
// shader-clock counter (s_memtime) beside the 100 MHz marks 1 and 2 (prologue barrier, end of the
// MFMA loop): (clk[1] - clk[0]) / (tl[2] - tl[1]) * 100 MHz = the clock the MFMA phase ran at
__device__ unsigned long long td3_clk[8192][2];
__device__ __forceinline__ void tl_mark(int k) {
  const unsigned id = blockIdx.x + blockIdx.y * gridDim.x;
  if (threadIdx.x == 0 && id < 8192) {
    if (k == 3) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (k == 1 || k == 2) td3_clk[id][k - 1] = __builtin_amdgcn_s_memtime();
    td3_tl[id][k] = __builtin_amdgcn_s_memrealtime();
    if (k == 0) {
      unsigned x, hw;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
      td3_tl[id][4] = x | ((unsigned long long)hw << 32);
    }
  }
}
#define TL_MARK(k) tl_mark(k)
// every GEMM workgroup's MFMA phase (prologue barrier -> end of the MFMA loop) summed over launches:
// [0] shader-clock ticks (s_memtime), [1] 100 MHz ticks (s_memrealtime); read / cleared with
// td3_clk_sum_read (tools/clk_probe.py: the clock a run's MFMA phases ran at)
__device__ unsigned long long td3_clk_sum[2];
#define TL_CLK_BEGIN() const unsigned long long tl_c0 = __builtin_amdgcn_s_memtime(), tl_r0 = __builtin_amdgcn_s_memrealtime()
#define TL_CLK_END()                                                                             \
  do {                                                                                         \
    const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime(); \
    if (threadIdx.x == 0) {                                                                    \
      atomicAdd(&td3_clk_sum[0], c1 - tl_c0);                                                  \
      atomicAdd(&td3_clk_sum[1], r1 - tl_r0);                                                  \
    }                                                                                          \
  } while (0)
#else
#define TL_MARK(k)
#define TL_CLK_BEGIN()
#define TL_CLK_END()
#endif
#ifdef TD3_TL_FINE      // drain the loads at the mark (changes the overlap: phase attribution only)
#define TL_FINE(k) do { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); TL_MARK(k); } while (0)
#else
#define TL_FINE(k)
#endif

}  // namespace td3

#ifdef TD3_TL
// Experiment builds only: copy the gemm-stage timeline of the last launch (n workgroups).
extern "C" int td3_tl_read(unsigned long long* out, int n) {
  if (n > 8192) n = 8192;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(td3::td3_tl), (size_t)n * 8 * 8, 0, hipMemcpyDeviceToHost) != hipSuccess)
    return -1;
  return 0;
}
extern "C" int td3_clk_read(unsigned long long* out, int n) {
  if (n > 8192) n = 8192;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(td3::td3_clk), (size_t)n * 2 * 8, 0, hipMemcpyDeviceToHost) != hipSuccess)
    return -1;
  return 0;
}
extern "C" int td3_clk_sum_read(unsigned long long* out, int clear) {
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(td3::td3_clk_sum), 16, 0, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  static const unsigned long long z[2] = {0, 0};
  if (clear && hipMemcpyToSymbol(HIP_SYMBOL(td3::td3_clk_sum), z, 16, 0, hipMemcpyHostToDevice) != hipSuccess) return -1;
  return 0;
}
extern "C" int td3_tl_clear() {
  static unsigned long long z[8192][8];
  return hipMemcpyToSymbol(HIP_SYMBOL(td3::td3_tl), z, sizeof(z), 0, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}
#endif
