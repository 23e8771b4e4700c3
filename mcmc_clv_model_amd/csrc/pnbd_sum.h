// What the maximum-likelihood translation units (csrc/pnbd.hip, csrc/gg.hip; DESIGN.md sections 4e, 4m)
// share.  The fixed-order sums: a 256-lane LDS tree per block, then one kernel that adds the block
// partials in a fixed order.  No float atomics, so the sums do not depend on the grid size and are
// bitwise the same on every call.  And the host side of an entry point: the device check and the
// "launch, final kernel, copy out" sequences.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "internal.h"

namespace {

constexpr int PNBD_MAX_GRID = 2048;

// Blocks of a launch over nb 256-customer blocks (the kernels stride over the rest).
inline unsigned grid_for(int64_t nb) { return (unsigned)std::min<int64_t>(nb, PNBD_MAX_GRID); }

// red[k][0] = sum over the 256 lanes of red[k][lane] for the rows k < m, tree offsets 128, 64, ..., 1.
// A row's tree does not see the other rows: its additions and their order are the same whatever m is.
__device__ __forceinline__ void tree256(double (*red)[256], int m) {
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off)
      for (int k = 0; k < m; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + off];
    __syncthreads();
  }
}

// out[row][k] = fixed-order sum over b < nb of part[(row * nb + b) * ns + k]; grid (ns, rows).
__global__ __launch_bounds__(256) void pnbd_final_kernel(const double* part, int64_t nb, int ns, double* out) {
  __shared__ double red[1][256];
  const int k = blockIdx.x;
  const int64_t row = blockIdx.y;
  double acc = 0.0;
  for (int64_t b = threadIdx.x; b < nb; b += 256) acc += part[(row * nb + b) * ns + k];
  red[0][threadIdx.x] = acc;
  tree256(red, 1);
  if (threadIdx.x == 0) out[row * ns + k] = red[0][0];
}

// A HIP device is visible (CLV_EHIP without one) and `device` is one of them, or negative for the
// current one (CLV_EINVAL "<prefix>: no such device").
inline int check_device(int32_t device, const char* prefix) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count < 1) return clv::fail(CLV_EHIP, "no HIP device visible");
  if (device >= count) return clv::fail(CLV_EINVAL, std::string(prefix) + ": no such device");
  return CLV_OK;
}

// The sum shape: launch() leaves block partials in d_part [rows][nb][ns]; res [rows][ns] <- their
// fixed-order sums by way of d_out.
template <class Launch>
int launch_sums(Launch launch, const double* d_part, int64_t nb, int ns, int64_t rows, double* d_out, double* res) {
  launch();
  CLV_HIP(hipGetLastError());
  hipLaunchKernelGGL(pnbd_final_kernel, dim3((unsigned)ns, (unsigned)rows), dim3(256), 0, nullptr, d_part, nb, ns,
                     d_out);
  CLV_HIP(hipGetLastError());
  CLV_HIP(hipMemcpy(res, d_out, sizeof(double) * (size_t)rows * (size_t)ns, hipMemcpyDeviceToHost));
  return CLV_OK;
}

// The per-row shape: launch(d) fills d [count] on the device; out <- d.
template <class Launch>
int launch_rows(size_t count, double* out, Launch launch) {
  clv::DevBuf bo;
  CLV_HIP(hipMalloc(&bo.p, sizeof(double) * count));
  launch(bo.as<double>());
  CLV_HIP(hipGetLastError());
  CLV_HIP(hipMemcpy(out, bo.p, sizeof(double) * count, hipMemcpyDeviceToHost));
  return CLV_OK;
}

}  // namespace
