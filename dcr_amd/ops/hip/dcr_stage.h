// Operand staging shared by the 128x128 NT score-tile kernels (maxsim.hip,
// topk_sim.hip, splitsim.hip): types, LDS geometry and the global ->
// register -> LDS copy of one 128 x BK bf16 operand tile. Rows past the
// operand's end and the contraction tail are staged as zeros. Also the
// order-preserving float max atomic that maxsim.hip and splitsim.hip combine
// partial maxima with.
#pragma once

#include "dcr_common.h"

namespace dcr_stage {

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;

using bf16_t = __hip_bfloat16;

constexpr int BK = 64;
constexpr int PITCH = BK + 8;           // bf16 elements per staged row
constexpr int NCH = BK / 16;            // uint4s a thread stages per operand
constexpr int STAGE = 128 * PITCH;      // one operand tile, in bf16
constexpr int SP = 65;                  // fp32 pitch of the score image
static_assert(4 * 64 * SP * 4 <= 4 * STAGE * 2,
              "the score images reuse the staging LDS");

// rows [row0, row0+128) x k [k0, k0+BK) of a row-major [rows][K] operand:
// two threads a row, each BK/2 contiguous bf16 as uint4s. K % 8 == 0, so a
// uint4 is wholly inside the contraction or wholly past it.
__device__ __forceinline__ void stage_load(const bf16_t* __restrict__ src,
                                           long rows, int K, long row0, int k0,
                                           int tid, uint4 (&v)[NCH]) {
#pragma unroll
  for (int t = 0; t < NCH; ++t) v[t] = make_uint4(0, 0, 0, 0);
  const long r = row0 + (tid >> 1);
  const int kb = k0 + (tid & 1) * (BK / 2);
  if (r >= rows) return;
  const uint4* p = reinterpret_cast<const uint4*>(src + r * K + kb);
#pragma unroll
  for (int t = 0; t < NCH; ++t)
    if (kb + t * 8 + 8 <= K) v[t] = p[t];
}

// The same tile of an operand whose contraction is cut into groups
// (splitsim.hip): rows [row0, row0+128) x columns col0 + [k0, k0+BK) of a
// row-major operand with row stride ld, where col0 is the first column of
// the group and klim its length. Columns at col0 + klim and beyond belong to
// the next group and are staged as zeros. klim % 8 == 0 and col0 % 8 == 0.
__device__ __forceinline__ void stage_load_seg(const bf16_t* __restrict__ src,
                                               long rows, long ld, int klim,
                                               long row0, long col0, int k0,
                                               int tid, uint4 (&v)[NCH]) {
#pragma unroll
  for (int t = 0; t < NCH; ++t) v[t] = make_uint4(0, 0, 0, 0);
  const long r = row0 + (tid >> 1);
  const int kb = k0 + (tid & 1) * (BK / 2);
  if (r >= rows) return;
  const uint4* p = reinterpret_cast<const uint4*>(src + r * ld + col0 + kb);
#pragma unroll
  for (int t = 0; t < NCH; ++t)
    if (kb + t * 8 + 8 <= klim) v[t] = p[t];
}

__device__ __forceinline__ void stage_store(short* lds, int tid,
                                            const uint4 (&v)[NCH]) {
  uint4* d = reinterpret_cast<uint4*>(lds + (tid >> 1) * PITCH +
                                      (tid & 1) * (BK / 2));
#pragma unroll
  for (int t = 0; t < NCH; ++t) d[t] = v[t];
}

// out = max(out, v) for floats through integer atomics. Non-negative floats
// order like signed ints and beat every bit pattern with the sign set;
// negative floats order inversely to their unsigned patterns, which are all
// above the non-negative ones. -0.0 takes the unsigned path, +0.0 the signed.
__device__ __forceinline__ void atomic_max_f32(float* addr, float v) {
  const int bits = __float_as_int(v);
  if (bits >= 0) atomicMax(reinterpret_cast<int*>(addr), bits);
  else atomicMin(reinterpret_cast<unsigned*>(addr), (unsigned)bits);
}

}  // namespace dcr_stage
