// numpy's 'linear' percentile of a sorted segment, for analysis_host.h's percentile_kernel (the
// level-1 summary of analysis.hip and the lifetime value of ltv.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace clv {

// numpy.percentile(a, q, method='linear') of a sorted segment (numpy/lib/_function_base_impl.py:
// virtual index (n-1) q, floor/next neighbours, _lerp with the t >= 0.5 branch); float32 segments
// (the percentile store) are widened to double before the interpolation, as numpy would on them.
template <class T>
__device__ double np_percentile_sorted(const T* a, int64_t n, double q_percent) {
  const double q = q_percent / 100.0;
  const double v = (double)(n - 1) * q;
  int64_t prev, next;
  if (v >= (double)(n - 1)) {
    prev = next = n - 1;
  } else if (v < 0.0) {
    prev = next = 0;
  } else {
    prev = (int64_t)floor(v);
    next = prev + 1;
  }
  const double gamma = v - floor(v);
  const double lo = (double)a[prev], hi = (double)a[next];
  const double diff = hi - lo;
  return gamma >= 0.5 ? hi - diff * (1.0 - gamma) : lo + diff * gamma;
}

}  // namespace clv
