// Bias-gradient column sums for MI355X (gfx950).
//
// colsum:         dy [rows, C]  -> out [C]              (linear / conv dbias)
// colsum_grouped: dy [N, HW, C] -> out_n [N, C], out [C]
//                 (d_temb and the conv dbias from ONE read of dy; out is the
//                 fp32 sum of the unrounded per-sample sums)
// Row-major input is the layout of an NHWC conv dy and of a linear dy.
// fp32 accumulation, output in the input dtype, no atomics, fixed
// summation order (bit-reproducible).
//
// Pass 1 (colsum_partial_kernel): a 256-thread block is TX column-vector
// lanes x 256/TX row lanes; 16 B per lane along C, so a row lane group
// reads TX*16 B contiguous per row. Each thread adds its rows in registers
// (4 independent loads in flight), row lanes are added in order through
// LDS, and the block stores one fp32 partial per column into a
// [groups*chunks, C] slab — or, with a single chunk and no groups, the
// final value in the output dtype (one launch).
// Pass 2: slab_colsum_kernel, or colsum_grouped_finalize_kernel which
// also emits the per-sample rows.

#include "dcr_common.h"
#include "dcr_reduce.h"

using namespace dcr;

namespace dcr_reduce {

template <typename T, int V>
__device__ __forceinline__ void loadv(const T* __restrict__ p, float (&o)[V]) {
  if constexpr (V == 8) {
    f32x8 v = load8<T>(p);
#pragma unroll
    for (int k = 0; k < 4; ++k) { o[k] = (&v.lo.x)[k]; o[4 + k] = (&v.hi.x)[k]; }
  } else if constexpr (V == 4) {
    f32x4 v = load4<T>(p);
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = (&v.x)[k];
  } else {
    o[0] = to_f32<T>(p[0]);
  }
}

// grid (cblocks, groups*chunks). Block (bx, by): columns
// [bx*TX*V, (bx+1)*TX*V), group by / chunks, rows
// [(by % chunks) * rows_per_chunk, ...) of that group.
template <typename T, int V, int TX>
__global__ __launch_bounds__(256)
void colsum_partial_kernel(const T* __restrict__ x, float* __restrict__ slab,
                           T* __restrict__ direct, long rows_per_group, int C,
                           int chunks, long rows_per_chunk) {
  constexpr int RL = 256 / TX;
  __shared__ float part[RL][TX * V];
  const int tx = threadIdx.x % TX;
  const int ty = threadIdx.x / TX;
  const int c0 = (blockIdx.x * TX + tx) * V;
  const long grp = blockIdx.y / chunks;
  const long r0 = (long)(blockIdx.y % chunks) * rows_per_chunk;
  long r1 = r0 + rows_per_chunk;
  if (r1 > rows_per_group) r1 = rows_per_group;
  const T* base = x + grp * rows_per_group * C;

  float a[V];
#pragma unroll
  for (int k = 0; k < V; ++k) a[k] = 0.f;
  if (c0 < C) {
    long r = r0 + ty;
    for (; r + 3 * RL < r1; r += 4 * RL) {
      float v0[V], v1[V], v2[V], v3[V];
      loadv<T, V>(base + r * C + c0, v0);
      loadv<T, V>(base + (r + RL) * C + c0, v1);
      loadv<T, V>(base + (r + 2 * RL) * C + c0, v2);
      loadv<T, V>(base + (r + 3 * RL) * C + c0, v3);
#pragma unroll
      for (int k = 0; k < V; ++k) { a[k] += v0[k]; a[k] += v1[k]; a[k] += v2[k]; a[k] += v3[k]; }
    }
    for (; r < r1; r += RL) {
      float v0[V];
      loadv<T, V>(base + r * C + c0, v0);
#pragma unroll
      for (int k = 0; k < V; ++k) a[k] += v0[k];
    }
  }
#pragma unroll
  for (int k = 0; k < V; ++k) part[ty][tx * V + k] = a[k];
  __syncthreads();
  if (threadIdx.x < TX * V) {
    const int c = blockIdx.x * TX * V + threadIdx.x;
    if (c < C) {
      float s = part[0][threadIdx.x];
#pragma unroll 4
      for (int i = 1; i < RL; ++i) s += part[i][threadIdx.x];
      if (direct) direct[c] = from_f32<T>(s);
      else slab[(long)blockIdx.y * C + c] = s;
    }
  }
}

// slab [N*chunks, C] -> out_n [N, C] (each sample's chunks added in order,
// rounded once) and out [C] (the unrounded sample sums added in fp32:
// row lane ty adds samples ty, ty+8, ... in order, then the 8 lanes in order)
template <typename T>
__global__ __launch_bounds__(DCR_SLAB_COLS * DCR_SLAB_RLANES)
void colsum_grouped_finalize_kernel(const float* __restrict__ slab,
                                    T* __restrict__ out_n, T* __restrict__ out,
                                    int N, int chunks, int C) {
  __shared__ float part[DCR_SLAB_RLANES][DCR_SLAB_COLS];
  const int tx = threadIdx.x % DCR_SLAB_COLS;
  const int ty = threadIdx.x / DCR_SLAB_COLS;
  const int c = blockIdx.x * DCR_SLAB_COLS + tx;
  float tot = 0.f;
  if (c < C) {
    for (int n = ty; n < N; n += DCR_SLAB_RLANES) {
      float s = 0.f;
      for (int ch = 0; ch < chunks; ++ch) s += slab[((long)n * chunks + ch) * C + c];
      out_n[(long)n * C + c] = from_f32<T>(s);
      tot += s;
    }
  }
  part[ty][tx] = tot;
  __syncthreads();
  if (ty == 0 && c < C) {
    float s = part[0][tx];
#pragma unroll
    for (int i = 1; i < DCR_SLAB_RLANES; ++i) s += part[i][tx];
    out[c] = from_f32<T>(s);
  }
}

}  // namespace dcr_reduce

#include "dcr_launchers.h"

namespace dcr {

static inline int colsum_vec(DType dt, int C) {
  const int full = (dt == DT_F32) ? 4 : 8;     // 16 B per lane
  if (C % full == 0) return full;
  if (C % 4 == 0) return 4;
  return 1;
}

static inline int colsum_tx(int nvec) {
  if (nvec % 32 == 0) return 32;
  if (nvec % 16 == 0) return 16;
  if (nvec % 8 == 0) return 8;
  return 32;
}

// chunks per group: >= 4 rows per thread, about 1024 blocks at most, and at
// most `cap` partial rows per group for the second pass to add.
int colsum_chunks(int dt, long groups, long rows_per_group, int C, int cap) {
  const int V = colsum_vec((DType)dt, C);
  const int nvec = C / V;
  const int TX = colsum_tx(nvec);
  const long cblocks = (nvec + TX - 1) / TX;
  const long RL = 256 / TX;
  long chunks = (rows_per_group + RL * 4 - 1) / (RL * 4);
  // up to 8 rows per thread a second launch costs more than it saves
  // (64x1280 in two passes measured 8.4 us against aten's 6.1 us)
  if (rows_per_group <= RL * 8) chunks = 1;
  long room = (1024 + cblocks * groups - 1) / (cblocks * groups);
  if (chunks > room) chunks = room;
  if (chunks > cap) chunks = cap;
  if (chunks < 1) chunks = 1;
  return (int)chunks;
}

template <typename T, int V, int TX>
static void colsum_partial_tx(const void* x, float* slab, void* direct,
                              long groups, long rows_per_group, int C,
                              int chunks, hipStream_t s) {
  const int nvec = C / V;
  dim3 grid((nvec + TX - 1) / TX, (unsigned)(groups * chunks)), block(256);
  const long rpc = (rows_per_group + chunks - 1) / chunks;
  hipLaunchKernelGGL((dcr_reduce::colsum_partial_kernel<T, V, TX>), grid, block,
                     0, s, (const T*)x, slab, (T*)direct, rows_per_group, C,
                     chunks, rpc);
}

template <typename T, int V>
static void colsum_partial_v(const void* x, float* slab, void* direct,
                             long groups, long rows_per_group, int C,
                             int chunks, hipStream_t s) {
  switch (colsum_tx(C / V)) {
    case 8: colsum_partial_tx<T, V, 8>(x, slab, direct, groups, rows_per_group, C, chunks, s); break;
    case 16: colsum_partial_tx<T, V, 16>(x, slab, direct, groups, rows_per_group, C, chunks, s); break;
    default: colsum_partial_tx<T, V, 32>(x, slab, direct, groups, rows_per_group, C, chunks, s); break;
  }
}

template <typename T>
static void colsum_t(DType dt, const void* x, float* slab, void* out_n,
                     void* out, long groups, long rows_per_group, int C,
                     int chunks, hipStream_t s) {
  const bool grouped = out_n != nullptr;
  void* direct = (!grouped && chunks == 1) ? out : nullptr;
  switch (colsum_vec(dt, C)) {
    case 8:
      if constexpr (sizeof(T) == 2)
        colsum_partial_v<T, 8>(x, slab, direct, groups, rows_per_group, C, chunks, s);
      break;
    case 4: colsum_partial_v<T, 4>(x, slab, direct, groups, rows_per_group, C, chunks, s); break;
    default: colsum_partial_v<T, 1>(x, slab, direct, groups, rows_per_group, C, chunks, s); break;
  }
  if (grouped) {
    dim3 grid((C + DCR_SLAB_COLS - 1) / DCR_SLAB_COLS);
    hipLaunchKernelGGL((dcr_reduce::colsum_grouped_finalize_kernel<T>), grid,
                       dim3(DCR_SLAB_COLS * DCR_SLAB_RLANES), 0, s, slab,
                       (T*)out_n, (T*)out, (int)groups, chunks, C);
  } else if (chunks > 1) {
    slab_colsum_launch<T>(slab, out, chunks, C, (long)C, s);
  }
}

// x: [groups, rows_per_group, C]; out_n: [groups, C] or nullptr (then
// groups must be 1); slab: groups*chunks*C floats (unused when out_n is
// null and chunks == 1); chunks from colsum_chunks().
void colsum_launch(DType dt, const void* x, float* slab, void* out_n, void* out,
                   long groups, long rows_per_group, int C, int chunks,
                   hipStream_t s) {
  switch (dt) {
    case DT_F32: colsum_t<float>(dt, x, slab, out_n, out, groups, rows_per_group, C, chunks, s); break;
    case DT_F16: colsum_t<__half>(dt, x, slab, out_n, out, groups, rows_per_group, C, chunks, s); break;
    case DT_BF16: colsum_t<__hip_bfloat16>(dt, x, slab, out_n, out, groups, rows_per_group, C, chunks, s); break;
  }
}

}  // namespace dcr
