// Fused patch max-similarity for split-product retrieval (MI355X / gfx950).
//
//   out[n, m] = max_{p < P, q < Q}  sum_c A[n, p, c] * B[m, q, c]
//
// A [N, P, C] and B [M, Q, C] are bf16, contiguous, C innermost; out is
// fp32 [N, M], pre-filled with -inf by the caller. Seen as flat row-major
// matrices [N*P, C] and [M*Q, C] this is an NT GEMM whose [N*P, M*Q] score
// matrix is reduced by max over P x Q blocks ("segments") and never stored:
// the largest global buffer the op touches is out itself.
//
// Main loop: the gemm.hip discipline. 128x128 score tile per block, 4 waves
// as 2x2 of 64x64 sub-tiles, v_mfma_f32_16x16x32_bf16 with fp32 accumulators,
// BK = 64, register-staged double-buffered LDS (next step's global loads are
// issued before the MFMAs, written after them, one barrier per step), LDS
// pitch BK+8. Rows past the operand's end and the contraction tail are staged
// as zeros: harmless to a dot product, and the epilogue never looks at them.
//
// Epilogue, per wave after one block barrier: the wave's 64x64
// fp32 sub-tile goes to a wave-private [64][65] LDS image that reuses the
// staging buffers. Lane c then walks column c down the rows, keeping a
// running max. Rows change segment (n = row / P) at the same place for
// every lane, so at each row-segment end, or at the last valid row, the
// wave holds 64 per-column maxima of one n. A segmented max-scan over the
// lanes (six shuffles, a lane only takes values from lanes of its own
// m = col / Q) leaves each column segment's max in its last lane, and that
// lane combines it into out[n, m] with an order-preserving integer atomic:
// signed max on the bit pattern of a value whose sign bit is clear,
// unsigned min when it is set. Max is exact and commutative, so the result
// does not depend on the order in which tiles arrive. Rows >= N*P are never
// walked and lanes of columns >= M*Q never publish or feed a valid lane,
// so padding cannot reach a maximum.

#include "dcr_stage.h"

namespace dcr_maxsim {

using namespace dcr_stage;  // staging types, geometry, stage_load/stage_store,
                            // atomic_max_f32

constexpr int GROUP = 16;               // A-tiles per block-order group

__global__ __launch_bounds__(256)
void patch_maxsim_kernel(const bf16_t* __restrict__ A,
                         const bf16_t* __restrict__ B, float* __restrict__ out,
                         long RA, long RB, long M, int P, int Q, int K,
                         long tiles_a, long tiles_b) {
  __shared__ __attribute__((aligned(16))) short smem[4 * STAGE];
  // images: A step buffers 0/1 at smem + {0, 1} * STAGE, B at {2, 3}

  // Block order: groups of GROUP A-tiles; inside a group the A-tile index
  // runs fastest, so blocks in flight together cover a compact patch of the
  // score matrix and share operand rows in cache (speed only).
  const long per_group = GROUP * tiles_b;
  const long grp = blockIdx.x / per_group;
  const long in_grp = blockIdx.x % per_group;
  const long first = grp * GROUP;
  const long gsz = min((long)GROUP, tiles_a - first);
  const long m0 = (first + in_grp % gsz) * 128;
  const long n0 = (in_grp / gsz) * 128;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l16 = lane & 15;
  const int kgrp = lane >> 4;
  const int wr = (wid >> 1) * 64;
  const int wc = (wid & 1) * 64;

  f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  const int nsteps = (K + BK - 1) / BK;
  uint4 av[NCH], bv[NCH];
  stage_load(A, RA, K, m0, 0, tid, av);
  stage_load(B, RB, K, n0, 0, tid, bv);
  stage_store(smem, tid, av);
  stage_store(smem + 2 * STAGE, tid, bv);
  __syncthreads();

  int cur = 0;
  for (int step = 0; step < nsteps; ++step) {
    const bool more = (step + 1 < nsteps);
    if (more) {
      stage_load(A, RA, K, m0, (step + 1) * BK, tid, av);
      stage_load(B, RB, K, n0, (step + 1) * BK, tid, bv);
    }

    const short* a_img = smem + cur * STAGE;
    const short* b_img = smem + (2 + cur) * STAGE;
#pragma unroll
    for (int kk = 0; kk < BK / 32; ++kk) {
      bf16x8 af[4], bf[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        af[i] = *reinterpret_cast<const bf16x8*>(
            a_img + (wr + i * 16 + l16) * PITCH + kk * 32 + kgrp * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        bf[j] = *reinterpret_cast<const bf16x8*>(
            b_img + (wc + j * 16 + l16) * PITCH + kk * 32 + kgrp * 8);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bf[j],
                                                              acc[i][j], 0, 0, 0);
    }

    if (more) {
      stage_store(smem + (cur ^ 1) * STAGE, tid, av);
      stage_store(smem + (2 + (cur ^ 1)) * STAGE, tid, bv);
      __syncthreads();
      cur ^= 1;
    }
  }

  // ---- epilogue: segmented max of the wave's 64x64 scores ----
  __syncthreads();  // every wave is done reading the staging buffers
  float* S = reinterpret_cast<float*>(smem) + wid * (64 * SP);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        S[(i * 16 + kgrp * 4 + rr) * SP + j * 16 + l16] = acc[i][j][rr];
  __syncthreads();  // the image is read across lanes

  const long gr0 = m0 + wr;              // first score row of this wave
  const long gc0 = n0 + wc;              // first score column
  const long rows_left = RA - gr0;
  if (rows_left <= 0) return;            // wave-uniform
  const int nrows = rows_left < 64 ? (int)rows_left : 64;

  const long gc = gc0 + lane;
  const bool cvalid = gc < RB;
  const long mcol = cvalid ? gc / Q : 0;
  const long seg0 = mcol * Q - gc0;      // local column where lane's m starts
  const int cs = seg0 > 0 ? (int)seg0 : 0;
  const bool cend = cvalid && (lane == 63 || gc + 1 == RB ||
                               gc + 1 == (mcol + 1) * Q);

  long nrow = gr0 / P;
  long next = (nrow + 1) * P - gr0;      // local row where nrow + 1 starts
  float v = -INFINITY;
  for (int r = 0; r < nrows; ++r) {
    v = fmaxf(v, S[r * SP + lane]);
    if (r + 1 == next || r + 1 == nrows) {
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const float u = __shfl_up(v, off, 64);
        if (lane - off >= cs) v = fmaxf(v, u);
      }
      if (cend) atomic_max_f32(out + nrow * M + mcol, v);
      v = -INFINITY;
      ++nrow;
      next += P;
    }
  }
}

}  // namespace dcr_maxsim

#include "dcr_launchers.h"

namespace dcr {

void patch_maxsim_launch(const void* A, const void* B, float* out, long N,
                         long M, int P, int Q, int K, hipStream_t st) {
  const long RA = N * P, RB = M * Q;
  const long ta = (RA + 127) / 128, tb = (RB + 127) / 128;
  hipLaunchKernelGGL(dcr_maxsim::patch_maxsim_kernel,
                     dim3((unsigned)(ta * tb)), dim3(256), 0, st,
                     (const dcr_maxsim::bf16_t*)A,
                     (const dcr_maxsim::bf16_t*)B, out, RA, RB, M, P, Q, K, ta,
                     tb);
}

}  // namespace dcr
