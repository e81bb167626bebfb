// Fused top-m similarity search (MI355X / gfx950).
//
//   for every query row n:  the m best (score, column) pairs of
//   score[n, c] = sum_k Qm[n, k] * X[c, k],  c < Nx,  1 <= m <= 16
//
// Qm [Nq, K] and X [Nx, K] are bf16, row-major, K % 8 == 0. The [Nq, Nx]
// score matrix is never stored: the largest buffers the op touches are the
// per-stripe candidate lists.
//
// Ordering rule: higher score first, among equal scores the lower column
// first; a NaN score is never inserted (and neither is -inf, the filler).
//
// Grid: one block per (query tile, stripe); a stripe is a contiguous run of
// 128-row index tiles. The query tile runs fastest, so the blocks in flight
// together walk the same index tiles and share them in cache; the query tile
// itself (128 x K bf16) is re-read through L2 for every index tile.
//
// Per index tile: maxsim.hip's main loop (128x128 tile, 4 waves as 2x2 of
// 64x64, v_mfma_f32_16x16x32_bf16, BK 64, register-staged double-buffered
// LDS at pitch 72, zero-staged rows past the end and contraction tail; the
// staging helpers are shared through dcr_stage.h). Every column's dot product
// therefore runs the same k-step sequence whatever tile, wave or stripe it
// lands in, and the result is bit-identical for any stripe count and any
// chunking of the query rows.
//
// Per-tile epilogue: each wave writes its 64x64 fp32 sub-tile to a
// wave-private [64][65] LDS image that reuses the staging buffers, then lane
// r walks ROW r across the valid columns (65r + c is distinct mod 64 over r:
// no bank conflict). A score enters the lane's list only when it beats the
// list's last entry. The list is sorted, lives in registers (capacity CAP, a
// template parameter >= m) and is updated by a fully unrolled shift chain
// with static indices only. Columns arrive in increasing order, so "strictly
// greater" keeps the lower column ahead among equal scores. Columns >= Nx
// are never offered; rows >= Nq are never written.
//
// The two waves that share a query row (column halves) keep their own
// lists. At the end of the stripe every wave stores its lists to
// part_scores / part_idx [Nq, 2S, CAP] (unfilled slots -inf / -1), and a
// second small kernel, one wave per row, merges a row's 2S*CAP candidates
// under the full (score, column) order into scores fp32 / idx int64 [Nq, m].
// No atomics anywhere.

#include "dcr_stage.h"

namespace dcr_topk {

using namespace dcr_stage;

// v is known to beat s[CAP-1]. Entries that v beats move down one slot.
template <int CAP>
__device__ __forceinline__ void list_insert(float (&s)[CAP], int (&ix)[CAP],
                                            float v, int c) {
#pragma unroll
  for (int j = CAP - 1; j >= 1; --j) {
    const bool up = v > s[j - 1];       // v lands above slot j
    const bool here = v > s[j];
    ix[j] = up ? ix[j - 1] : (here ? c : ix[j]);
    s[j] = up ? s[j - 1] : (here ? v : s[j]);
  }
  if (v > s[0]) { s[0] = v; ix[0] = c; }
}

// (v, c) ranks ahead of (s, i) under the ordering rule.
__device__ __forceinline__ bool ahead(float v, int c, float s, int i) {
  return v > s || (v == s && c < i);
}

template <int CAP>
__global__ __launch_bounds__(256, 2)
void topk_sim_kernel(const bf16_t* __restrict__ Qm,
                     const bf16_t* __restrict__ X,
                     float* __restrict__ part_s, int* __restrict__ part_i,
                     long Nq, long Nx, int K, int tiles_q, long tiles_x,
                     long tps, int nparts) {
  __shared__ __attribute__((aligned(16))) short smem[4 * STAGE];
  // images: query step buffers 0/1 at smem + {0, 1} * STAGE, index at {2, 3}

  const int qt = blockIdx.x % tiles_q;          // fastest: shares index rows
  const long stripe = blockIdx.x / tiles_q;
  const long m0 = (long)qt * 128;
  const long t_begin = stripe * tps;
  const long t_end = min(t_begin + tps, tiles_x);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l16 = lane & 15;
  const int kgrp = lane >> 4;
  const int wr = (wid >> 1) * 64;
  const int wc = (wid & 1) * 64;

  float ls[CAP];
  int li[CAP];
#pragma unroll
  for (int j = 0; j < CAP; ++j) { ls[j] = -INFINITY; li[j] = -1; }

  const int nsteps = (K + BK - 1) / BK;
  float* S = reinterpret_cast<float*>(smem) + wid * (64 * SP);
  uint4 av[NCH], bv[NCH];
  if (t_begin < t_end) {
    stage_load(Qm, Nq, K, m0, 0, tid, av);
    stage_load(X, Nx, K, t_begin * 128, 0, tid, bv);
  }

  for (long t = t_begin; t < t_end; ++t) {
    const long n0 = t * 128;
    f32x4_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

    stage_store(smem, tid, av);
    stage_store(smem + 2 * STAGE, tid, bv);
    __syncthreads();

    int cur = 0;
    for (int step = 0; step < nsteps; ++step) {
      const bool more = (step + 1 < nsteps);
      if (more) {
        stage_load(Qm, Nq, K, m0, (step + 1) * BK, tid, av);
        stage_load(X, Nx, K, n0, (step + 1) * BK, tid, bv);
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
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                af[i], bf[j], acc[i][j], 0, 0, 0);
      }

      if (more) {
        stage_store(smem + (cur ^ 1) * STAGE, tid, av);
        stage_store(smem + (2 + (cur ^ 1)) * STAGE, tid, bv);
        __syncthreads();
        cur ^= 1;
      }
    }

    // the next tile's first step is in flight during the epilogue
    if (t + 1 < t_end) {
      stage_load(Qm, Nq, K, m0, 0, tid, av);
      stage_load(X, Nx, K, n0 + 128, 0, tid, bv);
    }

    // ---- epilogue: offer the wave's 64x64 scores to the row lists ----
    __syncthreads();  // every wave is done reading the staging buffers
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          S[(i * 16 + kgrp * 4 + rr) * SP + j * 16 + l16] = acc[i][j][rr];
    __syncthreads();  // the image is read across lanes

    const long gc0 = n0 + wc;             // first score column of this wave
    const long left = Nx - gc0;
    const int ncols = left < 64 ? (left > 0 ? (int)left : 0) : 64;
    const float* row = S + lane * SP;
    for (int c = 0; c < ncols; ++c) {
      const float v = row[c];
      if (v > ls[CAP - 1]) list_insert<CAP>(ls, li, v, (int)gc0 + c);
    }
    __syncthreads();  // images are dead before the next tile is staged
  }

  const long r = m0 + wr + lane;
  if (r >= Nq) return;
  const long o = (r * nparts + 2 * stripe + (wid & 1)) * CAP;
#pragma unroll
  for (int j = 0; j < CAP; ++j) { part_s[o + j] = ls[j]; part_i[o + j] = li[j]; }
}

// One wave per query row: the row's n candidates -> the m best, in order.
// Lane l keeps the CAP best of candidates l, l+64, ... in a sorted register
// list under the full (score, column) order; then m rounds pick the best
// list head of the wave with a butterfly (the order is total and columns
// are unique, so every lane ends on the same winner) and its lane pops it.
template <int CAP>
__global__ __launch_bounds__(256)
void topk_merge_kernel(const float* __restrict__ part_s,
                       const int* __restrict__ part_i,
                       float* __restrict__ out_s, long* __restrict__ out_i,
                       long Nq, long n, int m) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= Nq) return;                  // wave-uniform
  float ls[CAP];
  int li[CAP];
#pragma unroll
  for (int j = 0; j < CAP; ++j) { ls[j] = -INFINITY; li[j] = -1; }
  const float* ps = part_s + r * n;
  const int* pi = part_i + r * n;
  for (long p = lane; p < n; p += 64) {
    const float v = ps[p];
    const int c = pi[p];
    if (c < 0 || !(li[CAP - 1] < 0 || ahead(v, c, ls[CAP - 1], li[CAP - 1])))
      continue;
#pragma unroll
    for (int j = CAP - 1; j >= 1; --j) {
      const bool up = li[j - 1] < 0 || ahead(v, c, ls[j - 1], li[j - 1]);
      const bool here = li[j] < 0 || ahead(v, c, ls[j], li[j]);
      const int pj = li[j - 1];
      const float sj = ls[j - 1];
      li[j] = up ? pj : (here ? c : li[j]);
      ls[j] = up ? sj : (here ? v : ls[j]);
    }
    if (li[0] < 0 || ahead(v, c, ls[0], li[0])) { ls[0] = v; li[0] = c; }
  }
  for (int j = 0; j < m; ++j) {
    float bv = ls[0];
    int bi = li[0];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off, 64);
      const int oi = __shfl_xor(bi, off, 64);
      if (oi >= 0 && (bi < 0 || ahead(ov, oi, bv, bi))) { bv = ov; bi = oi; }
    }
    if (lane == 0) { out_s[r * m + j] = bv; out_i[r * m + j] = bi; }
    if (bi >= 0 && li[0] == bi) {
#pragma unroll
      for (int t = 0; t + 1 < CAP; ++t) { ls[t] = ls[t + 1]; li[t] = li[t + 1]; }
      ls[CAP - 1] = -INFINITY;
      li[CAP - 1] = -1;
    }
  }
}

}  // namespace dcr_topk

#include "dcr_launchers.h"

namespace dcr {

void topk_sim_plan(long Nq, long Nx, int m, int stripes_req, int* cap,
                   int* stripes, long* tiles_per_stripe) {
  *cap = m <= 1 ? 1 : (m <= 4 ? 4 : (m <= 8 ? 8 : 16));
  const long tq = (Nq + 127) / 128, tx = (Nx + 127) / 128;
  long s = stripes_req;
  if (s <= 0) {
    // 256 CUs x 2 resident blocks: as many stripes as keep the whole grid
    // resident at once. One more block than that costs a second round of
    // the same length; fewer leave CUs idle (measured sweep: README).
    s = (2 * 256) / tq;
  }
  if (s > tx) s = tx;
  if (s < 1) s = 1;
  const long tps = (tx + s - 1) / s;
  *tiles_per_stripe = tps;
  *stripes = (int)((tx + tps - 1) / tps);   // no empty stripe
}

template <int CAP>
static void topk_sim_run(const void* Qm, const void* X, float* part_s,
                         int* part_i, float* out_s, long* out_i, long Nq,
                         long Nx, int K, int m, int stripes, long tps,
                         hipStream_t st) {
  const long tq = (Nq + 127) / 128, tx = (Nx + 127) / 128;
  const int nparts = 2 * stripes;
  hipLaunchKernelGGL(dcr_topk::topk_sim_kernel<CAP>,
                     dim3((unsigned)(tq * stripes)), dim3(256), 0, st,
                     (const dcr_topk::bf16_t*)Qm, (const dcr_topk::bf16_t*)X,
                     part_s, part_i, Nq, Nx, K, (int)tq, tx, tps, nparts);
  hipLaunchKernelGGL(dcr_topk::topk_merge_kernel<CAP>,
                     dim3((unsigned)((Nq + 3) / 4)), dim3(256), 0, st, part_s,
                     part_i, out_s, out_i, Nq, (long)nparts * CAP, m);
}

void topk_sim_launch(const void* Qm, const void* X, float* part_s, int* part_i,
                     float* out_s, long* out_i, long Nq, long Nx, int K, int m,
                     int cap, int stripes, long tiles_per_stripe,
                     hipStream_t st) {
  switch (cap) {
    case 1: topk_sim_run<1>(Qm, X, part_s, part_i, out_s, out_i, Nq, Nx, K, m,
                            stripes, tiles_per_stripe, st); break;
    case 4: topk_sim_run<4>(Qm, X, part_s, part_i, out_s, out_i, Nq, Nx, K, m,
                            stripes, tiles_per_stripe, st); break;
    case 8: topk_sim_run<8>(Qm, X, part_s, part_i, out_s, out_i, Nq, Nx, K, m,
                            stripes, tiles_per_stripe, st); break;
    default: topk_sim_run<16>(Qm, X, part_s, part_i, out_s, out_i, Nq, Nx, K,
                              m, stripes, tiles_per_stripe, st); break;
  }
}

}  // namespace dcr
