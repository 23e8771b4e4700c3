// Host pipeline shared by the posterior-analysis translation units (analysis.hip, ltv.hip, ic.hip,
// forecast.hip, diag.hip, score.hip): the exact per-segment sort and the percentile kernel that reads
// its output (staging a host array on the device is clv::upload of internal.h).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include <algorithm>
#include <cstdlib>
#include <string>

#include "internal.h"
#include "percentile.h"

namespace clv {

// per, lowered to the positive count the environment variable `name` holds, if it holds one: the
// tests' knob for a batch size (read at call time; it never raises a batch).
inline int64_t lowered_by_env(const char* name, int64_t per) {
  if (const char* e = std::getenv(name)) {
    const long long v = std::atoll(e);
    if (v > 0) per = std::min<int64_t>(per, v);
  }
  return per;
}

// The statistics of clv_psis_loo from a matrix [n_draws][n] already on the device (ic.hip; marginal.hip
// feeds it its own): ic_matrix_check is what needs no data (CLV_EINVAL before any device call),
// ic_matrix_dev queues the work on st, copies out [n][CLV_N_IC_STATS] to the host and synchronises.
int ic_matrix_check(int64_t n_draws, int64_t n, double reff);
int ic_matrix_dev(const double* d_loglik, int64_t n_draws, int64_t n, double reff, double* out, hipStream_t st);

// off[c] = c * len for c = 0 .. nc: the segment boundaries of nc segments of len keys.
template <class Off>
__global__ void seg_offsets_kernel(int64_t nc, int64_t len, Off* off) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c <= nc) off[c] = (Off)(c * len);
}

// Exact ascending sort of up to max_segs contiguous segments of len keys each (rocprim segmented
// radix sort over all of the key's bits).  Owns the sorted keys, the segment offsets and rocprim's
// temporary storage.  The storage is sized once, for max_segs segments, and reused for every
// smaller batch: this assumes that rocprim asks for no more when the keys and segments are fewer
// (its size is a function of those two counts alone); every sort passes the size it was given.
template <class K>
struct SegSorter {
  DevBuf sorted, off, tmp;
  size_t tmp_bytes = 0;
  int64_t len = 0, filled = -1;  // filled: the segment count the offsets hold
  hipStream_t st = nullptr;

  int call(void* t, size_t& bytes, const K* in, int64_t nc) {
    CLV_HIP(rocprim::segmented_radix_sort_keys(t, bytes, in, sorted.as<K>(), (unsigned)(nc * len), (unsigned)nc,
                                               off.as<uint32_t>(), off.as<uint32_t>() + 1, 0, 8 * sizeof(K), st));
    return CLV_OK;
  }

  int init(int64_t max_segs, int64_t seg_len, hipStream_t stream) {
    len = seg_len;
    st = stream;
    CLV_HIP(hipMalloc(&sorted.p, sizeof(K) * (size_t)(max_segs * len)));
    CLV_HIP(hipMalloc(&off.p, sizeof(uint32_t) * (size_t)(max_segs + 1)));
    int rc = call(nullptr, tmp_bytes, sorted.as<K>(), max_segs);
    if (rc) return rc;
    CLV_HIP(hipMalloc(&tmp.p, std::max<size_t>(tmp_bytes, 16)));
    return CLV_OK;
  }

  // *out <- the nc <= max_segs segments of in, each sorted (valid until the next sort).
  int sort(const K* in, int64_t nc, const K** out) {
    if (nc != filled) {
      hipLaunchKernelGGL(seg_offsets_kernel<uint32_t>, dim3((unsigned)((nc + 256) / 256)), dim3(256), 0, st, nc, len,
                         off.as<uint32_t>());
      CLV_HIP(hipGetLastError());
      filled = nc;
    }
    size_t bytes = tmp_bytes;
    *out = sorted.as<K>();
    return call(tmp.p, bytes, in, nc);
  }
};

// Up to 3 (percent, output column) pairs of percentile_kernel.
struct PctCols {
  int count;
  double q[3];
  int col[3];
};

// numpy's 'linear' percentiles pc of nc sorted segments of len keys -> out[(row0 + c) * stride + col].
template <class T>
__global__ __launch_bounds__(256) void percentile_kernel(const T* sorted, int64_t nc, int64_t len, PctCols pc,
                                                         int64_t row0, int64_t stride, double* out) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const T* a = sorted + c * len;
  double* o = out + (row0 + c) * stride;
  for (int k = 0; k < pc.count; ++k) o[pc.col[k]] = np_percentile_sorted(a, len, pc.q[k]);
}

template <class T>
int launch_percentiles(const T* sorted, int64_t nc, int64_t len, const PctCols& pc, int64_t row0, int64_t stride,
                       double* out, hipStream_t st) {
  hipLaunchKernelGGL(percentile_kernel<T>, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, st, sorted, nc, len, pc,
                     row0, stride, out);
  CLV_HIP(hipGetLastError());
  return CLV_OK;
}

}  // namespace clv
