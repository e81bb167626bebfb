// Deterministic column reduction of an fp32 partial slab: the second pass
// of every "blocks write plain partials, a small kernel adds them" scheme
// in this library (LayerNorm / GroupNorm dw,db and the bias-gradient
// column sums). No atomics, no zero-init, fixed summation order.
#pragma once

#include "dcr_common.h"

namespace dcr {

#define DCR_SLAB_COLS 32   // columns per block: one 128 B line per slab row
#define DCR_SLAB_RLANES 8  // row lanes per block (256 threads)

// out[c] = sum_r slab[r * ld + c], c < cols, written in OT.
// Thread (tx, ty) adds rows ty, ty+8, ... of column tx in order; the 8
// row-lane partials are then added in order through LDS.
// `bx` is the block's index among the blocks doing this reduction (a
// kernel may give its first blocks other work); all 256 threads call it.
template <typename OT>
__device__ __forceinline__ void slab_colsum_block(const float* __restrict__ slab,
                                                  OT* __restrict__ out, long rows,
                                                  int cols, long ld, int bx) {
  __shared__ float part[DCR_SLAB_RLANES][DCR_SLAB_COLS];
  const int tx = threadIdx.x % DCR_SLAB_COLS;
  const int ty = threadIdx.x / DCR_SLAB_COLS;
  const int c = bx * DCR_SLAB_COLS + tx;
  float a = 0.f;
  if (c < cols) {
    long r = ty;
    // 8 independent loads in flight per thread (a one-load-at-a-time
    // loop over 512 slab rows measured 118 us per call)
    for (; r + 7 * DCR_SLAB_RLANES < rows; r += 8 * DCR_SLAB_RLANES) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = slab[(r + u * DCR_SLAB_RLANES) * ld + c];
#pragma unroll
      for (int u = 0; u < 8; ++u) a += v[u];
    }
    for (; r < rows; r += DCR_SLAB_RLANES) a += slab[r * ld + c];
  }
  part[ty][tx] = a;
  __syncthreads();
  if (ty == 0 && c < cols) {
    float s = part[0][tx];
#pragma unroll
    for (int i = 1; i < DCR_SLAB_RLANES; ++i) s += part[i][tx];
    out[c] = from_f32<OT>(s);
  }
}

template <typename OT>
__global__ __launch_bounds__(DCR_SLAB_COLS * DCR_SLAB_RLANES)
void slab_colsum_kernel(const float* __restrict__ slab, OT* __restrict__ out,
                        long rows, int cols, long ld) {
  slab_colsum_block<OT>(slab, out, rows, cols, ld, blockIdx.x);
}

template <typename OT>
static inline void slab_colsum_launch(const float* slab, void* out, long rows,
                                      int cols, long ld, hipStream_t s) {
  dim3 grid((cols + DCR_SLAB_COLS - 1) / DCR_SLAB_COLS);
  dim3 block(DCR_SLAB_COLS * DCR_SLAB_RLANES);
  hipLaunchKernelGGL((slab_colsum_kernel<OT>), grid, block, 0, s, slab,
                     (OT*)out, rows, cols, ld);
}

}  // namespace dcr
