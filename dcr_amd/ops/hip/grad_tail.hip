// Optimizer tail before AdamW (FusedAdamW.gather_grads / clip_and_step):
// one launch copies a whole list of autograd gradients into the flat arena
// and takes their sum of squares on the way; a one-block kernel turns the
// per-block partials into the {sumsq, norm, coef} record that the clip-aware
// AdamW kernels (elementwise.hip) read. No atomics, no zero-fill, fixed
// summation order. Design and measurements: README.md "Gradient tail".
//
// Work unit: a virtual block = (parameter, chunk of `ch` elements). The
// per-call table (int64 x 4 per parameter, in device memory) holds
//   [0] source address  [1] destination element offset in the arena
//   [2] element count   [3] virtual blocks before this parameter
// and a block finds its parameter by binary search over column 3.
//
// Inside a chunk the elements are split by the DESTINATION's alignment only:
// head elements up to the first 16-byte boundary of the destination, then
// 16-byte groups, then a tail. Which lane takes which element, and the order
// a lane adds its squares in, depend on nothing else, so the sum over a
// chunk is the same bits whatever the source is: a gradient tensor (fused)
// or the arena itself (standalone pass, STORE=false). The source is read
// with the widest access of 16 / 8 / 4 / 2 bytes that divides the distance
// between source and destination; the destination group is always stored
// as one 16-byte access.
//
// ADD (gradient accumulation micro-steps): dst = T(float(dst) + float(src)),
// one fp32 add rounded once, which is what `_foreach_add_` computes for bf16
// and fp32. Same element-to-lane map and source widths; the destination
// group is one 16-byte load and one 16-byte store, GT_UNROLL loads of both
// operands in flight. There is no fused sum of squares in add mode: the sum
// of a step's gradient is taken by the standalone pass.

#include <cstdint>

#include "dcr_common.h"
#include "dcr_launchers.h"

using namespace dcr;

#define GT_THREADS 256
#define GT_UNROLL 4   // 16-byte loads in flight per lane

// 16 bytes from an address aligned to W bytes
template <int W>
__device__ __forceinline__ uint4 gt_load16(const char* __restrict__ p) {
  uint4 r;
  if (W == 16) {
    r = *reinterpret_cast<const uint4*>(p);
  } else if (W == 8) {
    uint2 a = reinterpret_cast<const uint2*>(p)[0];
    uint2 b = reinterpret_cast<const uint2*>(p)[1];
    r = make_uint4(a.x, a.y, b.x, b.y);
  } else if (W == 4) {
    const unsigned* q = reinterpret_cast<const unsigned*>(p);
    r = make_uint4(q[0], q[1], q[2], q[3]);
  } else {
    const unsigned short* q = reinterpret_cast<const unsigned short*>(p);
    r = make_uint4((unsigned)q[0] | ((unsigned)q[1] << 16),
                   (unsigned)q[2] | ((unsigned)q[3] << 16),
                   (unsigned)q[4] | ((unsigned)q[5] << 16),
                   (unsigned)q[6] | ((unsigned)q[7] << 16));
  }
  return r;
}

// sum of squares of one 16-byte group, as a fixed pairwise tree
template <typename T>
__device__ __forceinline__ float gt_group_sumsq(uint4 v);

template <>
__device__ __forceinline__ float gt_group_sumsq<float>(uint4 v) {
#pragma clang fp contract(off)
  float a = __uint_as_float(v.x), b = __uint_as_float(v.y);
  float c = __uint_as_float(v.z), d = __uint_as_float(v.w);
  return (a * a + b * b) + (c * c + d * d);
}

template <>
__device__ __forceinline__ float gt_group_sumsq<__hip_bfloat16>(uint4 v) {
#pragma clang fp contract(off)
  float q[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    unsigned w = (&v.x)[k];
    float lo = __uint_as_float(w << 16);
    float hi = __uint_as_float(w & 0xffff0000u);
    q[k] = lo * lo + hi * hi;
  }
  return (q[0] + q[1]) + (q[2] + q[3]);
}

// a + b over one 16-byte group, each element one fp32 add rounded to T
template <typename T>
__device__ __forceinline__ uint4 gt_group_add(uint4 a, uint4 b);

template <>
__device__ __forceinline__ uint4 gt_group_add<float>(uint4 a, uint4 b) {
  return make_uint4(__float_as_uint(__uint_as_float(a.x) + __uint_as_float(b.x)),
                    __float_as_uint(__uint_as_float(a.y) + __uint_as_float(b.y)),
                    __float_as_uint(__uint_as_float(a.z) + __uint_as_float(b.z)),
                    __float_as_uint(__uint_as_float(a.w) + __uint_as_float(b.w)));
}

__device__ __forceinline__ unsigned gt_bf16_bits(float f) {
  __hip_bfloat16 h = from_f32<__hip_bfloat16>(f);
  return (unsigned)*reinterpret_cast<unsigned short*>(&h);
}

template <>
__device__ __forceinline__ uint4 gt_group_add<__hip_bfloat16>(uint4 a, uint4 b) {
  uint4 r;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    unsigned x = (&a.x)[k], y = (&b.x)[k];
    float lo = __uint_as_float(x << 16) + __uint_as_float(y << 16);
    float hi = __uint_as_float(x & 0xffff0000u) + __uint_as_float(y & 0xffff0000u);
    (&r.x)[k] = gt_bf16_bits(lo) | (gt_bf16_bits(hi) << 16);
  }
  return r;
}

// the 16-byte groups of one chunk; lane t takes groups t, t+256, ... in order
template <typename T, int W, bool SUMSQ, bool STORE, bool ADD>
__device__ __forceinline__ float gt_body(const T* __restrict__ src,
                                         T* __restrict__ dst, int ng, float s) {
#pragma clang fp contract(off)
  constexpr int G = 16 / sizeof(T);
  int g = threadIdx.x;
  for (; g + (GT_UNROLL - 1) * GT_THREADS < ng; g += GT_UNROLL * GT_THREADS) {
    uint4 v[GT_UNROLL];
#pragma unroll
    for (int u = 0; u < GT_UNROLL; ++u)
      v[u] = gt_load16<W>(reinterpret_cast<const char*>(
          src + (long)(g + u * GT_THREADS) * G));
    if (ADD) {
      uint4 d[GT_UNROLL];
#pragma unroll
      for (int u = 0; u < GT_UNROLL; ++u)
        d[u] = *reinterpret_cast<const uint4*>(dst + (long)(g + u * GT_THREADS) * G);
#pragma unroll
      for (int u = 0; u < GT_UNROLL; ++u) v[u] = gt_group_add<T>(d[u], v[u]);
    }
    if (STORE) {
#pragma unroll
      for (int u = 0; u < GT_UNROLL; ++u)
        *reinterpret_cast<uint4*>(dst + (long)(g + u * GT_THREADS) * G) = v[u];
    }
    if (SUMSQ) {
#pragma unroll
      for (int u = 0; u < GT_UNROLL; ++u) s = s + gt_group_sumsq<T>(v[u]);
    }
  }
  for (; g < ng; g += GT_THREADS) {
    uint4 v = gt_load16<W>(reinterpret_cast<const char*>(src + (long)g * G));
    if (ADD)
      v = gt_group_add<T>(*reinterpret_cast<const uint4*>(dst + (long)g * G), v);
    if (STORE) *reinterpret_cast<uint4*>(dst + (long)g * G) = v;
    if (SUMSQ) s = s + gt_group_sumsq<T>(v);
  }
  return s;
}

template <typename T, bool SUMSQ, bool STORE, bool ADD = false>
__global__ __launch_bounds__(GT_THREADS)
void grad_gather_kernel(const long* __restrict__ table, int nparams, long nvb,
                        T* __restrict__ arena, float* __restrict__ partials,
                        int ch) {
  __shared__ float lds[2 * GT_THREADS / DCR_WAVE];
  constexpr int G = 16 / sizeof(T);
  const int t = threadIdx.x;
  for (long vb = blockIdx.x; vb < nvb; vb += gridDim.x) {
    // largest i with table[4i+3] <= vb (column 3 is non-decreasing, row 0 is 0)
    int lo = 0, hi = nparams - 1;
    while (lo < hi) {
      int mid = (lo + hi + 1) >> 1;
      if (table[4 * mid + 3] <= vb) lo = mid; else hi = mid - 1;
    }
    const long* row = table + 4 * lo;
    const long n = row[2];
    const long e0 = (vb - row[3]) * (long)ch;
    const long left = n - e0;
    const int len = left < (long)ch ? (int)left : ch;   // >= 1 by construction
    const T* src = reinterpret_cast<const T*>(row[0]) + e0;
    T* dst = arena + row[1] + e0;

    int h = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u)
                  / sizeof(T));
    if (h > len) h = len;
    const int ng = (len - h) / G;
    const int r = len - h - ng * G;

    float s = 0.f;
    if (t < h) {
#pragma clang fp contract(off)
      T x = src[t];
      if (ADD) x = from_f32<T>(to_f32<T>(dst[t]) + to_f32<T>(x));
      if (STORE) dst[t] = x;
      float f = to_f32<T>(x);
      if (SUMSQ) s = f * f;
    }
    const unsigned d = (unsigned)(reinterpret_cast<uintptr_t>(src) -
                                  reinterpret_cast<uintptr_t>(dst));
    const T* bs = src + h;
    T* bd = dst + h;
    if ((d & 15u) == 0)
      s = gt_body<T, 16, SUMSQ, STORE, ADD>(bs, bd, ng, s);
    else if ((d & 7u) == 0)
      s = gt_body<T, 8, SUMSQ, STORE, ADD>(bs, bd, ng, s);
    else if ((d & 3u) == 0)
      s = gt_body<T, 4, SUMSQ, STORE, ADD>(bs, bd, ng, s);
    else
      s = gt_body<T, sizeof(T) < 4 ? 2 : 4, SUMSQ, STORE, ADD>(bs, bd, ng, s);
    if (t < r) {
#pragma clang fp contract(off)
      const int i = h + ng * G + t;
      T x = src[i];
      if (ADD) x = from_f32<T>(to_f32<T>(dst[i]) + to_f32<T>(x));
      if (STORE) dst[i] = x;
      float f = to_f32<T>(x);
      if (SUMSQ) s = s + f * f;
    }
    if (SUMSQ) {
      float2 tot = block_reduce_sum2(s, 0.f, lds);
      if (t == 0) partials[vb] = tot.x;
    }
  }
}

// One block: partials -> {sumsq, norm, coef}. Thread t adds partials t,
// t+1024, ... in order (fp64), then a fixed LDS tree. coef follows
// FusedAdamW.clip_grad_norm_ step by step: `max_norm / (norm + 1e-6)` on a
// 0-dim fp32 tensor is reciprocal-then-multiply in torch, the comparison is
// a strict `>` (a NaN norm gives coef = 1).
#define GT_FIN_THREADS 1024
__global__ __launch_bounds__(GT_FIN_THREADS)
void sumsq_finalize_kernel(const float* __restrict__ partials, long nvb,
                           float max_norm, float* __restrict__ rec) {
  __shared__ double sh[GT_FIN_THREADS];
  const int t = threadIdx.x;
  double a = 0.0;
  long i = t;
  for (; i + 7L * GT_FIN_THREADS < nvb; i += 8L * GT_FIN_THREADS) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = partials[i + (long)u * GT_FIN_THREADS];
#pragma unroll
    for (int u = 0; u < 8; ++u) a += (double)v[u];
  }
  for (; i < nvb; i += GT_FIN_THREADS) a += (double)partials[i];
  sh[t] = a;
  __syncthreads();
  for (int off = GT_FIN_THREADS / 2; off > 0; off >>= 1) {
    if (t < off) sh[t] += sh[t + off];
    __syncthreads();
  }
  if (t == 0) {
#pragma clang fp contract(off)
    const float ss = (float)sh[0];
    const float norm = sqrtf(ss);
    float coef = 1.f;
    if (norm > max_norm) coef = (1.f / (norm + 1e-6f)) * max_norm;
    rec[0] = ss;
    rec[1] = norm;
    rec[2] = coef;
  }
}

namespace dcr {

int grad_gather_grid(long nvb, int grid_req) {
  // the grid walks the virtual blocks; 8192 was the best of the sweep
  // (README.md "Gradient tail"), by 2 % over 2048
  long g = grid_req > 0 ? grid_req : 8192;
  if (g > nvb) g = nvb;
  if (g < 1) g = 1;
  return (int)g;
}

template <typename T>
static void gather_dispatch(const long* table, int nparams, long nvb, void* arena,
                            float* partials, int ch, int grid, bool store,
                            bool add, hipStream_t s) {
  dim3 gr(grid), bl(GT_THREADS);
  T* a = (T*)arena;
  if (add)
    hipLaunchKernelGGL((grad_gather_kernel<T, false, true, true>), gr, bl, 0, s,
                       table, nparams, nvb, a, (float*)nullptr, ch);
  else if (store && partials)
    hipLaunchKernelGGL((grad_gather_kernel<T, true, true>), gr, bl, 0, s, table,
                       nparams, nvb, a, partials, ch);
  else if (store)
    hipLaunchKernelGGL((grad_gather_kernel<T, false, true>), gr, bl, 0, s, table,
                       nparams, nvb, a, partials, ch);
  else
    hipLaunchKernelGGL((grad_gather_kernel<T, true, false>), gr, bl, 0, s, table,
                       nparams, nvb, a, partials, ch);
}

void grad_gather_launch(DType dt, const long* table, int nparams, long nvb,
                        void* arena, float* partials, int ch, int grid,
                        bool store, bool add, hipStream_t s) {
  if (nvb <= 0 || nparams <= 0) return;
  if (dt == DT_BF16)
    gather_dispatch<__hip_bfloat16>(table, nparams, nvb, arena, partials, ch,
                                    grid, store, add, s);
  else
    gather_dispatch<float>(table, nparams, nvb, arena, partials, ch, grid,
                           store, add, s);
}

void sumsq_finalize_launch(const float* partials, long nvb, float max_norm,
                           float* rec, hipStream_t s) {
  hipLaunchKernelGGL(sumsq_finalize_kernel, dim3(1), dim3(GT_FIN_THREADS), 0, s,
                     partials, nvb, max_norm, rec);
}

}  // namespace dcr
