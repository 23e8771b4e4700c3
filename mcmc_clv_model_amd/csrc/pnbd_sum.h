// The fixed-order sums of the maximum-likelihood kernels (csrc/pnbd.hip, csrc/gg.hip; DESIGN.md section
// 4e): a 256-lane LDS tree per block, then one kernel that adds the block partials in a fixed order.
// No float atomics, so the sums do not depend on the grid size and are bitwise the same on every call.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

// red[k][0] = sum over the 256 lanes of red[k][lane], tree offsets 128, 64, ..., 1.
template <int NSUM>
__device__ __forceinline__ void tree256(double (*red)[256]) {
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off)
      for (int k = 0; k < NSUM; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + off];
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
  tree256<1>(red);
  if (threadIdx.x == 0) out[row * ns + k] = red[0][0];
}

}  // namespace
