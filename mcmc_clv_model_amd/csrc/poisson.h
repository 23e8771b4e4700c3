// The exact Poisson sampler of the posterior analysis (analysis.hip: predict, track; ppc.hip: the
// replicated calibration counts) and the Philox block it draws from.  Device code only; every
// translation unit that includes this gets its own copy.  tests/test_gpu_analysis_stream.py pins the
// bits of both (float64 model: tests/analysis_stream_ref.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "philox.h"

namespace clv {
namespace {

constexpr int POISSON_MAX_ITER = 1 << 16;   // bound for the inversion / rejection loops

__device__ __forceinline__ u32x4 pblock(uint32_t k0, uint32_t k1, uint32_t a, uint32_t d, uint32_t slot,
                                        uint32_t stream) {
  return philox4x32_10(u32x4{a, d, slot, stream}, k0, k1);
}

// Exact Poisson(m) sample.  m < 10: inversion by sequential search (one uniform); m >= 10: the
// transformed rejection PTRS of Hoermann (1993), as numpy's random_poisson_ptrs.  Each attempt
// uses Philox block (a, d, slot0 + attempt, stream).
__device__ int64_t poisson_draw(double m, uint32_t k0, uint32_t k1, uint32_t a, uint32_t d, uint32_t slot0,
                                uint32_t stream) {
  if (!(m > 0.0)) return 0;
  if (m < 10.0) {
    const u32x4 r = pblock(k0, k1, a, d, slot0, stream);
    const double u = u53(r.x, r.y);
    double p = exp(-m), F = p;
    int64_t k = 0;
    while (u > F && k < POISSON_MAX_ITER) {
      ++k;
      p *= m / (double)k;
      F += p;
    }
    return k;
  }
  const double slam = sqrt(m);
  const double loglam = log(m);
  const double b = 0.931 + 2.53 * slam;
  const double aa = -0.059 + 0.02483 * b;
  const double invalpha = 1.1239 + 1.1328 / (b - 3.4);
  const double vr = 0.9277 - 3.6224 / (b - 2.0);
  for (int it = 0; it < POISSON_MAX_ITER; ++it) {
    const u32x4 r = pblock(k0, k1, a, d, slot0 + (uint32_t)it, stream);
    const double U = u53(r.x, r.y) - 0.5;
    const double V = u53(r.z, r.w);
    const double us = 0.5 - fabs(U);
    const int64_t k = (int64_t)floor((2.0 * aa / us + b) * U + m + 0.43);
    if (us >= 0.07 && V <= vr) return k;
    if (k < 0 || (us < 0.013 && V > us)) continue;
    if (log(V) + log(invalpha) - log(aa / (us * us) + b) <= -m + (double)k * loglam - lgamma((double)k + 1.0)) return k;
  }
  return (int64_t)floor(m);  // unreachable in practice (acceptance > 0.85 per attempt)
}

}  // namespace
}  // namespace clv
