// What the rollout statistics (rollout.hip) share with the dataset normalisation of a replay ring
// (ringnorm.hip): the handle's device state, Chan's merge and the element expression of rs_tick step 2
// (include/td3.h).  Both translation units normalise through norm_den / norm_elem, so a row normalised
// by a tick and a row normalised in the ring have the same bits.
#pragma once
#include "common.h"
#include "../../include/td3.h"

namespace td3 {

// An rs_handle.
struct Stats {
  int device = 0, rows = 0, obs_dim = 0, log_cap = 0, ncol = 0, W = 0;
  rs_config cfg{};
  void* base = nullptr;            // one allocation; the pointers below point into it
  double* count_blk = nullptr;     // [ncol] copies of the observation count, all equal
  double* mean = nullptr;
  double* m2 = nullptr;
  double* rscal = nullptr;
  int64_t* iscal = nullptr;
  double* G = nullptr;
  double* ep_return = nullptr;
  int32_t* ep_len = nullptr;
  rs_episode* log = nullptr;
  uint8_t* mask = nullptr;
};

__device__ __forceinline__ double clipd(double y, double lim) { return y > lim ? lim : (y < -lim ? -lim : y); }

// Chan's merge of a batch (n rows, mean mb, sum of squared deviations m2b) into running moments.
__device__ __forceinline__ void chan_merge(double& count, double& mean, double& m2, double n, double mb, double m2b) {
  const double delta = mb - mean, tot = count + n;
  mean += delta * n / tot;
  m2 += m2b + delta * delta * count * n / tot;
  count = tot;
}

// rs_tick step 2 for one element of an enabled column with count > 0: fp64, rounded to fp32 once.
__device__ __forceinline__ double norm_den(double m2, double count, double eps) { return sqrt(m2 / count + eps); }
__device__ __forceinline__ float norm_elem(float x, double mean, double den, double lim) {
  return (float)clipd(((double)x - mean) / den, lim);
}

}  // namespace td3
