// MFMA bf16 GEMM for the transformer linear layers (MI355X / gfx950).
//
// Reference ops this replaces: QKV/out projections,
// GEGLU FeedForward matmuls, proj_in/out of the spatial transformer —
// the rocBLAS/Tensile share of the SD-2.1 finetune step
// (/root/reference/diff_train.py:644 runs them through diffusers linears).
//
// One kernel template covers all three passes of torch.nn.Linear without
// materializing any transpose, because each operand can be staged from
// either a k-contiguous ("row-major") or a k-strided ("col-major") layout:
//
//   C[M,N] = sum_k A(m,k) * B(n,k)   (+ bias[n])        [out rows from A,
//                                                         out cols from B]
//   forward : A = x  [M,K]  (TA=0)   B = W  [N,K]  (TB=0)   + bias
//   dgrad   : A = dy [M,N'] (TA=0)   B = W' = mem[N'][K] read k-strided
//             (TB=1: contraction n', out-col k)         -> dx
//   wgrad   : A = dy^T (TA=1: mem [M][N], contraction m) and
//             B = x^T  (TB=1: mem [M][K])               -> dW (+ dbias,
//             the column-sum of dy fused into the A staging pass)
//
// Structure: the validated conv v3 discipline — 128x128 tile, 4 waves as
// 2x2 of 64x64 sub-tiles, v_mfma_f32_16x16x32_bf16, double-buffered LDS
// with register staging (next tile's global loads issued before the MFMA
// loop, write pass after it, ONE barrier per K-step), LDS pitch BK+8 so
// 16-lane ds_read_b128 groups land on 16 distinct banks. Split-K over the
// contraction (fp32 atomics + finalize) when the M/N grid starves 256 CUs.
//
// linear_wgrad_kernel, further down, is a separate weight-gradient kernel
// (natural-layout staging, transposed LDS reads, slab reduction): the one
// ops/linear.py dispatches by default.

#include "dcr_common.h"

namespace dcr_gemm {

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;

using bf16_t = __hip_bfloat16;

// Stage one operand tile [128 rows][BK k] into registers.
//  - !T : memory is row-major [rows][K] (k contiguous): 2 threads/row,
//         each loads BK/2 contiguous bf16 as uint4s.
//  - T  : memory is [K][rows] (rows contiguous): each thread owns one row
//         r = tid&127 and k-half (tid>>7); BK/2 coalesced 2-byte loads
//         (consecutive lanes -> consecutive rows), packed to uint4s.
// Out-of-range rows/k are zero-filled (contraction tail, ragged M/N).
template <int BK, bool T, bool COLSUM>
struct Stager {
  static constexpr int NCH = BK / 16;  // uint4s per thread (BK/2 bf16)
  const bf16_t* __restrict__ src;
  long ld;        // row stride (!T: = K) or r stride (T: = rows_total)
  long row0;      // first row of the tile
  long rows;      // total rows of the operand (M or N)
  int K;          // contraction extent
  int tid;
  float colsum;   // running sum of this thread's loaded values (wgrad dbias)

  __device__ void init(const bf16_t* s, long ld_, long row0_, long rows_,
                       int K_, int tid_) {
    src = s; ld = ld_; row0 = row0_; rows = rows_; K = K_; tid = tid_;
    colsum = 0.f;
  }
  __device__ int st_row() const { return T ? (tid & 127) : (tid >> 1); }
  __device__ int st_k() const {
    return T ? ((tid >> 7) * (BK / 2)) : ((tid & 1) * (BK / 2));
  }

  __device__ void load(int k0, uint4 (&v)[NCH]) {
#pragma unroll
    for (int t = 0; t < NCH; ++t) v[t] = make_uint4(0, 0, 0, 0);
    const long r = row0 + st_row();
    const int kb = k0 + st_k();
    if (r >= rows) return;
    if (!T) {
      const bf16_t* p = src + r * ld + kb;
      if (kb + BK / 2 <= K) {
#pragma unroll
        for (int t = 0; t < NCH; ++t)
          v[t] = reinterpret_cast<const uint4*>(p)[t];
      } else {
#pragma unroll
        for (int t = 0; t < NCH; ++t)
          if (kb + t * 8 + 8 <= K) v[t] = reinterpret_cast<const uint4*>(p)[t];
          else if (kb + t * 8 < K) {  // ragged 8-tail: scalar fill
            ushort tmp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int e = 0; e < 8 && kb + t * 8 + e < K; ++e)
              tmp[e] = reinterpret_cast<const ushort*>(p)[t * 8 + e];
            v[t] = *reinterpret_cast<const uint4*>(tmp);
          }
      }
    } else {
      // k-strided gather: BK/2 coalesced scalar loads down the k column
      ushort tmp[BK / 2];
      const bf16_t* p = src + (long)kb * ld + r;
#pragma unroll
      for (int j = 0; j < BK / 2; ++j) {
        tmp[j] = (kb + j < K) ? reinterpret_cast<const ushort*>(p)[(long)j * ld]
                              : (ushort)0;
      }
      if (COLSUM) {
#pragma unroll
        for (int j = 0; j < BK / 2; ++j) {
          __hip_bfloat16 h = *reinterpret_cast<__hip_bfloat16*>(&tmp[j]);
          colsum += __bfloat162float(h);
        }
      }
#pragma unroll
      for (int t = 0; t < NCH; ++t)
        v[t] = *reinterpret_cast<const uint4*>(&tmp[t * 8]);
    }
  }

  template <int PITCH>
  __device__ void store(short* lds, const uint4 (&v)[NCH]) {
    uint4* d = reinterpret_cast<uint4*>(lds + st_row() * PITCH + st_k());
#pragma unroll
    for (int t = 0; t < NCH; ++t) d[t] = v[t];
  }
};

template <int BK, bool TA, bool TB, bool DBIAS>
__global__ __launch_bounds__(256)
void gemm_bf16_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ B,
                      const float* __restrict__ bias, bf16_t* __restrict__ C,
                      float* __restrict__ ws, float* __restrict__ dbias,
                      long M, long N, int K, int splitz) {
  constexpr int PITCH = BK + 8;
  __shared__ short sA[2][128 * PITCH];
  __shared__ short sB[2][128 * PITCH];

  const long m0 = (long)blockIdx.x * 128;
  const long n0 = (long)blockIdx.y * 128;

  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int l16 = lane & 15;
  const int kgrp = lane >> 4;
  const int wr = (wid >> 1) * 64;
  const int wc = (wid & 1) * 64;

  f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  Stager<BK, TA, DBIAS> stA;
  Stager<BK, TB, false> stB;
  stA.init(A, TA ? M : (long)K, m0, M, K, (int)threadIdx.x);
  stB.init(B, TB ? N : (long)K, n0, N, K, (int)threadIdx.x);

  const int nsteps = (K + BK - 1) / BK;
  const int spz = (nsteps + splitz - 1) / splitz;
  const int step0 = blockIdx.z * spz;
  const int step1 = min(nsteps, step0 + spz);
  constexpr int NCH = BK / 16;

  uint4 av[NCH], bv[NCH];
  if (step0 < step1) {
    stA.load(step0 * BK, av);
    stB.load(step0 * BK, bv);
    stA.template store<PITCH>(sA[0], av);
    stB.template store<PITCH>(sB[0], bv);
  }
  __syncthreads();

  int cur = 0;
  for (int step = step0; step < step1; ++step) {
    const bool more = (step + 1 < step1);
    if (more) {
      stA.load((step + 1) * BK, av);
      stB.load((step + 1) * BK, bv);
    }

#pragma unroll
    for (int kk = 0; kk < BK / 32; ++kk) {
      bf16x8 af[4], bf[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        af[i] = *reinterpret_cast<const bf16x8*>(
            sA[cur] + (wr + i * 16 + l16) * PITCH + kk * 32 + kgrp * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        bf[j] = *reinterpret_cast<const bf16x8*>(
            sB[cur] + (wc + j * 16 + l16) * PITCH + kk * 32 + kgrp * 8);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bf[j],
                                                              acc[i][j], 0, 0, 0);
    }

    if (more) {
      stA.template store<PITCH>(sA[cur ^ 1], av);
      stB.template store<PITCH>(sB[cur ^ 1], bv);
      __syncthreads();
      cur ^= 1;
    }
  }

  // fused dbias (wgrad): A is dy^T, each staging thread has summed its
  // loaded dy values over the contraction; one tile of blocks (y==0)
  // covers every (m, n) pair exactly once per z-slice.
  if (DBIAS && blockIdx.y == 0) {
    const long r = m0 + stA.st_row();
    if (r < M && stA.colsum != 0.f) atomicAdd(&dbias[r], stA.colsum);
  }

#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const long m = m0 + wr + i * 16 + kgrp * 4 + rr;
      if (m >= M) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long n = n0 + wc + j * 16 + l16;
        if (n >= N) continue;
        if (splitz > 1) {
          atomicAdd(&ws[m * N + n], acc[i][j][rr]);
        } else {
          float v = acc[i][j][rr] + (bias ? bias[n] : 0.f);
          C[m * N + n] = __float2bfloat16(v);
        }
      }
    }
  }
}

__global__ void gemm_finalize_kernel(const float* __restrict__ ws,
                                     const float* __restrict__ bias,
                                     bf16_t* __restrict__ y, long total,
                                     long N) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    float v = ws[i] + (bias ? bias[i % N] : 0.f);
    y[i] = __float2bfloat16(v);
  }
}

// ---------------------------------------------------------------------------
// Split-contraction weight gradient: dW[N,K] = dy[M,N]^T x[M,K] (+ db[N]).
//
// Both operands are staged the way memory lays them out: rows of m, 16 B
// per lane along n (dy) and along k (x), into natural [m][cols] LDS images.
// The MFMA fragment "8 contraction elements at row lane&15" is a COLUMN of
// such an image, taken with two ds_read_b64_tr_b16 per 16x16x32 operand.
//
// A block owns a TN x 64 tile of dW and one slice of the contraction. A
// step stages WG_BM = 128 rows; wave w contracts rows 32w..32w+31 of the
// step into its own full-tile accumulators (one MFMA depth per wave per
// step, so every fragment read feeds TN/16 or 4 MFMAs). After the last
// step the four waves' accumulators are added in wave order through LDS
// and stored with plain float4 stores into the slice's row of a
// [split, N*K (+N)] fp32 slab; slab_colsum_kernel adds the slab rows in
// order and writes dw|db in the weight dtype. No atomics, no zero fill.
//
// LDS image of a [128][T] operand tile: 2*T-byte rows, the 32-byte column
// groups of a row XOR-permuted by wg_swz(row). One 32-lane half of a
// transposed read takes two 4-row blocks 8 rows apart in the same 16
// columns, 8 dwords per row: the XOR sends rows {r..r+3, r+8..r+11} to 8
// distinct 8-dword bank slots of the 64 (T=64: row parity picks the 32-bank
// half, bits 1 and 3 the slot; T=128: bits 0, 1 and 3 pick the slot), so
// the read is conflict-free. The staging write is one row segment of 128
// contiguous bytes per 8 lanes.
//
// Fused db: blocks of the first k-tile column sum the
// columns of the dy chunks they stage, in fp32. A thread always stages the
// same 8 columns, so it keeps 8 running sums; they are added in thread
// order through LDS at the end and go to the db tail of the slab row.

constexpr int WG_BM = 128;
constexpr int WG_TK = 64;

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

template <int T>
__device__ __forceinline__ int wg_swz(int row) {
  if (T == 64) return ((row >> 1) & 1) | (((row >> 3) & 1) << 1);
  return (row & 3) | (((row >> 3) & 1) << 2);
}

// byte offset of column `col` (multiple of 4) of row `row`
template <int T>
__device__ __forceinline__ int wg_off(int row, int col) {
  return row * (T * 2) + ((((col >> 4) ^ wg_swz<T>(row))) << 5) + (col & 15) * 2;
}

// global -> registers: chunk c = tid + 256 t is row c / (T/8), 16-byte
// column chunk c % (T/8). Buffer loads with the operand's byte size as the
// range: rows >= M come back zero from the hardware range check, with no
// branch around a load, so the compiler counts the loads it waits for
// (vmcnt(N)) instead of draining them all. Columns >= cols are read from
// column 0 instead: they reach only outputs that are never stored.
// A step past the slice's end (!live) loads from offset 2^31, out of range,
// so the loop issues the same loads every step and has no branch either.
// Byte offsets are 32-bit: the launcher requires M * ld * 2 < 2^31.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wg_rsrc(const bf16_t* p,
                                                          long bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(p), 0, (int)bytes,
                                           0x00020000);
}

template <int T>
__device__ __forceinline__ void wg_load(__amdgpu_buffer_rsrc_t src, long ld,
                                        long m0, bool live, int col0, int cols,
                                        int tid, uint4 (&v)[T / 16]) {
  constexpr int CPR = T / 8;
  const int col = col0 + (tid % CPR) * 8;
  const unsigned off0 =
      live ? (unsigned)((m0 + tid / CPR) * ld + (col < cols ? col : 0)) * 2u
           : 0x80000000u;
#pragma unroll
  for (int t = 0; t < T / 16; ++t) {
    const unsigned off = off0 + (unsigned)(t * (256 / CPR) * ld) * 2u;
    const u32x4 g = __builtin_amdgcn_raw_buffer_load_b128(src, (int)off, 0, 0);
    v[t] = make_uint4(g.x, g.y, g.z, g.w);
  }
}

template <int T>
__device__ __forceinline__ void wg_store(char* img, int tid,
                                         const uint4 (&v)[T / 16]) {
  constexpr int CPR = T / 8;
#pragma unroll
  for (int t = 0; t < T / 16; ++t) {
    const int row = tid / CPR + t * (256 / CPR);
    *reinterpret_cast<uint4*>(img + wg_off<T>(row, (tid % CPR) * 8)) = v[t];
  }
}

__device__ __forceinline__ void wg_colsum(const uint4& v, float (&cs)[8]) {
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    cs[2 * e] += __uint_as_float(w[e] << 16);
    cs[2 * e + 1] += __uint_as_float(w[e] & 0xffff0000u);
  }
}

// one 16x16x32 operand: columns c16..c16+15 of rows r32..r32+31 of an image
template <int T>
__device__ __forceinline__ bf16x8 wg_frag(const char* img, int r32, int c16,
                                          int lane) {
  const int row = r32 + (lane >> 4) * 8 + ((lane & 15) >> 2);
  const int col = c16 + (lane & 3) * 4;
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (lds_s16x4*)(img + wg_off<T>(row, col)));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (lds_s16x4*)(img + wg_off<T>(row + 4, col)));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

template <int TN, bool DB>
__global__ __launch_bounds__(256, TN == 64 ? 2 : 1)
void linear_wgrad_kernel(const bf16_t* __restrict__ dy,
                         const bf16_t* __restrict__ x, float* __restrict__ slab,
                         long M, int N, int K, int chunks_per_slice,
                         long slab_ld, int tiles_n, int tiles_k) {
  constexpr int NI = TN / 16, NJ = WG_TK / 16;
  constexpr int A_BYTES = WG_BM * TN * 2, B_BYTES = WG_BM * WG_TK * 2;
  constexpr int STAGE = A_BYTES + B_BYTES;
  constexpr int RED_BYTES = 4 * 16 * WG_TK * 4;  // 4 waves x [16][64] fp32
  static_assert(STAGE >= RED_BYTES, "reduction reuses the staging LDS");
  static_assert(STAGE >= (256 / (TN / 8)) * TN * 4, "db reduction too");
  __shared__ __attribute__((aligned(16))) char smem[STAGE];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  // Blocks are dealt round-robin to the 8 XCDs, each with its own L2. Give
  // each XCD a contiguous run of (slice, tile) work, tiles fastest, so the
  // tiles that share a slice's rows of dy and x read them from one L2
  // (bijective for any block count; placement is speed only).
  const int nwg = gridDim.x, ntile = tiles_n * tiles_k;
  const int xcd = blockIdx.x % 8, q = nwg / 8, r = nwg % 8;
  const int wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) +
                 blockIdx.x / 8;
  const int bz = wg / ntile, bt = wg % ntile;
  const int bx = bt % tiles_n, by = bt / tiles_n;
  const int n0 = bx * TN;
  const int k0 = by * WG_TK;
  const long nchunks = (M + WG_BM - 1) / WG_BM;
  const long c0 = (long)bz * chunks_per_slice;
  const long c1 = min(nchunks, c0 + chunks_per_slice);
  const bool do_db = DB && by == 0;  // block-uniform

  f32x4_t acc[NI][NJ];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};
  float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

  char* sa = smem;
  char* sb = smem + A_BYTES;
  // One LDS stage, two barriers a step; global loads run two steps ahead
  // in two register sets, so a block keeps two steps of operands in flight
  // across the MFMAs and the barriers.
  uint4 av0[TN / 16], bv0[WG_TK / 16], av1[TN / 16], bv1[WG_TK / 16];
  const __amdgpu_buffer_rsrc_t rdy = wg_rsrc(dy, M * N * 2);
  const __amdgpu_buffer_rsrc_t rx = wg_rsrc(x, M * K * 2);
  auto fetch = [&](long c, uint4 (&a)[TN / 16], uint4 (&b)[WG_TK / 16]) {
    wg_load<TN>(rdy, N, c * WG_BM, c < c1, n0, N, tid, a);
    wg_load<WG_TK>(rx, K, c * WG_BM, c < c1, k0, K, tid, b);
  };
  auto step = [&](long c, uint4 (&a)[TN / 16], uint4 (&b)[WG_TK / 16]) {
    wg_store<TN>(sa, tid, a);
    wg_store<WG_TK>(sb, tid, b);
    if (do_db) {
#pragma unroll
      for (int t = 0; t < TN / 16; ++t) wg_colsum(a[t], cs);
    }
    __syncthreads();
    fetch(c + 2, a, b);
    bf16x8 af[NI], bf[NJ];
#pragma unroll
    for (int i = 0; i < NI; ++i) af[i] = wg_frag<TN>(sa, wid * 32, i * 16, lane);
#pragma unroll
    for (int j = 0; j < NJ; ++j) bf[j] = wg_frag<WG_TK>(sb, wid * 32, j * 16, lane);
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bf[j],
                                                            acc[i][j], 0, 0, 0);
    __syncthreads();
  };
  fetch(c0, av0, bv0);
  fetch(c0 + 1, av1, bv1);
  // steps in pairs, no branch between them (a branch would make the
  // compiler drain every load at the join): an odd last step adds zeros
  for (long c = c0; c < c1; c += 2) {
    step(c, av0, bv0);
    step(c + 1, av1, bv1);
  }

  float* srow = slab + (long)bz * slab_ld;

  // the four waves' tiles, 16 rows of n at a time: red[w][16][64] fp32
  float* red = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        red[(wid * 16 + (lane >> 4) * 4 + r) * WG_TK + j * 16 + (lane & 15)] =
            acc[i][j][r];
    __syncthreads();
    const int rn = tid >> 4, ck = (tid & 15) * 4;
    float4 s = *reinterpret_cast<const float4*>(red + rn * WG_TK + ck);
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const float4 p =
          *reinterpret_cast<const float4*>(red + (w * 16 + rn) * WG_TK + ck);
      s.x += p.x; s.y += p.y; s.z += p.z; s.w += p.w;
    }
    const int n = n0 + i * 16 + rn, k = k0 + ck;
    if (n < N && k < K)
      *reinterpret_cast<float4*>(srow + (long)n * K + k) = s;
  }

  if (do_db) {
    // cred[256 / CPR][TN]: thread tid holds columns 8 (tid % CPR) .. +7
    constexpr int CPR = TN / 8, RT = 256 / CPR;
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 8; ++e)
      red[(tid / CPR) * TN + (tid % CPR) * 8 + e] = cs[e];
    __syncthreads();
    if (tid < TN && n0 + tid < N) {
      float s = red[tid];
      for (int r = 1; r < RT; ++r) s += red[r * TN + tid];
      srow[(long)N * K + n0 + tid] = s;
    }
  }
}

}  // namespace dcr_gemm

#include "dcr_launchers.h"
#include "dcr_reduce.h"

namespace dcr {

void gemm_bf16_launch(const void* A, const void* B, const float* bias,
                      void* C, float* ws, float* dbias, long M, long N, int K,
                      int ta, int tb, int want_dbias, int splitz,
                      hipStream_t st) {
  dim3 grid((unsigned)((M + 127) / 128), (unsigned)((N + 127) / 128),
            (unsigned)splitz),
      block(256);
  const auto* a = (const dcr_gemm::bf16_t*)A;
  const auto* b = (const dcr_gemm::bf16_t*)B;
  auto* c = (dcr_gemm::bf16_t*)C;

#define DCR_GEMM_LAUNCH(BK, TA, TB, DB)                                        \
  hipLaunchKernelGGL((dcr_gemm::gemm_bf16_kernel<BK, TA, TB, DB>), grid,       \
                     block, 0, st, a, b, bias, c, ws, dbias, M, N, K, splitz)

  const bool bk64 = (K % 64 == 0) || (K > 256);
  if (!ta && !tb) {
    if (bk64) DCR_GEMM_LAUNCH(64, false, false, false);
    else      DCR_GEMM_LAUNCH(32, false, false, false);
  } else if (!ta && tb) {
    if (bk64) DCR_GEMM_LAUNCH(64, false, true, false);
    else      DCR_GEMM_LAUNCH(32, false, true, false);
  } else if (ta && tb && want_dbias) {
    if (bk64) DCR_GEMM_LAUNCH(64, true, true, true);
    else      DCR_GEMM_LAUNCH(32, true, true, true);
  } else {
    if (bk64) DCR_GEMM_LAUNCH(64, true, true, false);
    else      DCR_GEMM_LAUNCH(32, true, true, false);
  }
#undef DCR_GEMM_LAUNCH

  if (splitz > 1) {
    long total = M * N;
    long blk = (total / 4 + 255) / 256;
    if (blk > 8192) blk = 8192;
    hipLaunchKernelGGL(dcr_gemm::gemm_finalize_kernel, dim3((unsigned)blk),
                       dim3(256), 0, st, ws, bias, c, total, N);
  }
}

// Tile and split for linear_wgrad. tile_req / split_req > 0 force them
// (the split clamped to the number of 128-row chunks); 0 asks for the rule.
// Tile: 64 x 64. The 128 x 64 tile halves the operand re-reads but holds
// 128 accumulator registers a lane and one block a CU, and measured slower
// at every flagship shape; it stays reachable for the sweep. Split: bring
// tiles x split to about WG_TARGET blocks (two fit a CU; beyond about 1.5 a
// CU the larger slab costs more than the extra blocks hide), while the
// fp32 slab, written once and read once, stays below twice the operand
// bytes. README "linear_wgrad sweep" has the measurements behind both.
#define WG_TARGET 400
void linear_wgrad_plan(long M, int N, int K, int tile_req, int split_req,
                       int* tile, int* split, int* chunks_per_slice) {
  const long nchunks = (M + dcr_gemm::WG_BM - 1) / dcr_gemm::WG_BM;
  const long kt = (K + dcr_gemm::WG_TK - 1) / dcr_gemm::WG_TK;
  const int tn = tile_req == 128 ? 128 : 64;
  const long tiles = ((N + tn - 1) / tn) * kt;
  long sp = split_req;
  if (sp <= 0) {
    sp = (WG_TARGET + tiles / 2) / tiles;
    const long cap = (M * ((long)N + K)) / ((long)N * K);
    if (sp > cap) sp = cap;
  }
  if (sp > nchunks) sp = nchunks;
  if (sp < 1) sp = 1;
  long cps = (nchunks + sp - 1) / sp;
  if (split_req <= 0 && cps > 1) cps += cps & 1;  // the kernel steps in pairs
  *tile = tn;
  *chunks_per_slice = (int)cps;
  *split = (int)((nchunks + cps - 1) / cps);  // no empty slice
}

void linear_wgrad_launch(const void* dy, const void* x, float* slab,
                         void* dwdb, long M, int N, int K, int want_db,
                         int tile, int split, int chunks_per_slice,
                         hipStream_t st) {
  const long ld = (long)N * K + (want_db ? N : 0);
  const int tn = (N + tile - 1) / tile;
  const int tk = (K + dcr_gemm::WG_TK - 1) / dcr_gemm::WG_TK;
  dim3 grid((unsigned)((long)tn * tk * split)), block(256);
  const auto* a = (const dcr_gemm::bf16_t*)dy;
  const auto* b = (const dcr_gemm::bf16_t*)x;
#define DCR_WGRAD_LAUNCH(TN, DB)                                               \
  hipLaunchKernelGGL((dcr_gemm::linear_wgrad_kernel<TN, DB>), grid, block, 0,  \
                     st, a, b, slab, M, N, K, chunks_per_slice, ld, tn, tk)
  if (tile == 128) {
    if (want_db) DCR_WGRAD_LAUNCH(128, true);
    else         DCR_WGRAD_LAUNCH(128, false);
  } else {
    if (want_db) DCR_WGRAD_LAUNCH(64, true);
    else         DCR_WGRAD_LAUNCH(64, false);
  }
#undef DCR_WGRAD_LAUNCH
  slab_colsum_launch<__hip_bfloat16>(slab, dwdb, split, (int)ld, ld, st);
}

}  // namespace dcr
