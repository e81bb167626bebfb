// Fused split-product similarity for aligned chunks and patches (MI355X /
// gfx950).
//
//   out[n, m] = max_{g < G}  sum_{l < L} A[n, g, l] * B[m, g, l]
//
// A [N, G, L] and B [M, G, L] are bf16, contiguous, L % 8 == 0; out is fp32
// [N, M]. Seen as row-major matrices [N, G*L] and [M, G*L] this is an NT
// GEMM whose contraction is cut into G segments: each segment's dot product
// is finished on its own and only the largest survives. The [N, M, G] block
// of per-group scores is never stored.
//
// Main loop: maxsim.hip's. 128x128 tile of out per block, 4 waves as 2x2 of
// 64x64 sub-tiles, v_mfma_f32_16x16x32_bf16 with fp32 accumulators, BK = 64,
// register-staged double-buffered LDS (the next step's global loads are
// issued before the MFMAs, written after them, one barrier per step), LDS
// pitch BK+8. The block walks one flat sequence of (group, k-step) pairs, so
// the prefetch runs across group boundaries. A k-step of group g stages
// columns [g*L, (g+1)*L) only: what is past the group's end in the step is
// zero, not the next group's data (stage_load_seg). At a group's last k-step
// the 64 accumulators of a lane are folded into 64 running maxima, which
// start at -inf, and the accumulators restart from zero.
//
// Every group's dot product runs the same k-step sequence wherever it lands,
// so the result does not depend on the tile, the split or how the caller
// chunks the rows of A.
//
// Splits: a tile's groups may be shared by S blocks, block s taking groups
// [s*G/S, (s+1)*G/S) (never empty for S <= G). With S == 1 the block stores
// its tile with plain stores. With S > 1 out is pre-filled with -inf by the
// caller and the blocks combine through atomic_max_f32, an exact and
// commutative max: the arrival order cannot change a bit.
//
// fmaxf returns the other operand when one is NaN, so a NaN group score is
// dropped unless every group of the entry is NaN (torch's amax would
// propagate it). Non-finite inputs are outside the op's contract.

#include "dcr_stage.h"

namespace dcr_splitsim {

using namespace dcr_stage;  // staging types, geometry, stage_load_seg,
                            // stage_store, atomic_max_f32

constexpr int TGROUP = 16;              // row tiles per block-order group

__global__ __launch_bounds__(256, 2)
void split_product_kernel(const bf16_t* __restrict__ A,
                          const bf16_t* __restrict__ B, float* __restrict__ out,
                          long N, long M, int G, int L, int S, long tiles_a,
                          long tiles_b) {
  __shared__ __attribute__((aligned(16))) short smem[4 * STAGE];
  // images: A step buffers 0/1 at smem + {0, 1} * STAGE, B at {2, 3}

  // Block order: the split index slowest; inside a split, groups of TGROUP
  // row tiles with the row-tile index fastest, so blocks in flight together
  // cover a compact patch of out and share operand rows in cache (speed
  // only).
  const long tiles = tiles_a * tiles_b;
  const int split = (int)(blockIdx.x / tiles);
  const long tile = blockIdx.x % tiles;
  const long per_group = TGROUP * tiles_b;
  const long grp = tile / per_group;
  const long in_grp = tile % per_group;
  const long first = grp * TGROUP;
  const long gsz = min((long)TGROUP, tiles_a - first);
  const long r0 = (first + in_grp % gsz) * 128;   // first row of out
  const long c0 = (in_grp / gsz) * 128;           // first column of out

  const int g0 = (int)((long)split * G / S);
  const int g1 = (int)((long)(split + 1) * G / S);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l16 = lane & 15;
  const int kgrp = lane >> 4;
  const int wr = (wid >> 1) * 64;
  const int wc = (wid & 1) * 64;

  f32x4_t acc[4][4], best[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc[i][j] = {0.f, 0.f, 0.f, 0.f};
      best[i][j] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    }

  const long ld = (long)G * L;
  const int spg = (L + BK - 1) / BK;      // k-steps per group
  uint4 av[NCH], bv[NCH];
  stage_load_seg(A, N, ld, L, r0, (long)g0 * L, 0, tid, av);
  stage_load_seg(B, M, ld, L, c0, (long)g0 * L, 0, tid, bv);
  stage_store(smem, tid, av);
  stage_store(smem + 2 * STAGE, tid, bv);
  __syncthreads();

  int cur = 0;
  int gn = g0, kn = 0;                    // the (group, k-step) being staged
  for (;;) {
    if (++kn == spg) { kn = 0; ++gn; }
    const bool last = (kn == 0);          // the step computed now ends a group
    const bool more = (gn < g1);
    if (more) {
      stage_load_seg(A, N, ld, L, r0, (long)gn * L, kn * BK, tid, av);
      stage_load_seg(B, M, ld, L, c0, (long)gn * L, kn * BK, tid, bv);
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

    if (last) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            best[i][j][rr] = fmaxf(best[i][j][rr], acc[i][j][rr]);
            acc[i][j][rr] = 0.f;
          }
    }

    if (!more) break;
    stage_store(smem + (cur ^ 1) * STAGE, tid, av);
    stage_store(smem + (2 + (cur ^ 1)) * STAGE, tid, bv);
    __syncthreads();
    cur ^= 1;
  }

  // ---- epilogue: the lane's 64 maxima go straight to out ----
  // lane holds rows i*16 + kgrp*4 + rr, column j*16 + l16 of the sub-tile
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const long row = r0 + wr + i * 16 + kgrp * 4 + rr;
      if (row >= N) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long col = c0 + wc + j * 16 + l16;
        if (col >= M) continue;
        float* dst = out + row * M + col;
        if (S > 1) atomic_max_f32(dst, best[i][j][rr]);
        else *dst = best[i][j][rr];
      }
    }
}

}  // namespace dcr_splitsim

#include "dcr_launchers.h"

namespace dcr {

// The launcher's rule for S (profiles/r10_splitsim.log, --sweep): the
// largest count that keeps the grid within one round of 2 blocks per CU on
// 256 CUs, at most G.
int split_product_splits(long N, long M, int G, int splits_req) {
  if (splits_req > 0) return splits_req < G ? splits_req : G;
  const long tiles = ((N + 127) / 128) * ((M + 127) / 128);
  long s = 512 / tiles;
  if (s < 1) s = 1;
  if (s > G) s = G;
  return (int)s;
}

void split_product_launch(const void* A, const void* B, float* out, long N,
                          long M, int G, int L, int S, hipStream_t st) {
  const long ta = (N + 127) / 128, tb = (M + 127) / 128;
  hipLaunchKernelGGL(dcr_splitsim::split_product_kernel,
                     dim3((unsigned)(ta * tb * S)), dim3(256), 0, st,
                     (const dcr_splitsim::bf16_t*)A,
                     (const dcr_splitsim::bf16_t*)B, out, N, M, G, L, S, ta,
                     tb);
}

}  // namespace dcr
