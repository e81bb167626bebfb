// GroupNorm(+fused SiLU) and LayerNorm forward/backward for MI355X (gfx950).
//
// Design (HBM3E-bound ops):
// * fp32 accumulation, bf16/f16/f32 IO, vec4 loads (dwordx4/dwordx2).
// * GroupNorm: one workgroup per (n, group) — the group's data is one
//   contiguous [C/G * H*W] segment of NCHW. Two-pass: block-reduce
//   mean/var, then normalize (+SiLU fused into the same kernel, saving a
//   full HBM round-trip per ResNet block).
// * Backward recomputes z from (x, mean, rstd); per-channel dw/db go
//   through an LDS accumulator, then one global atomicAdd per channel
//   per block.
// * LayerNorm: one wave per row, 4 waves per block.

#include "dcr_common.h"
#include "dcr_reduce.h"

using namespace dcr;

// ===========================================================================
// GroupNorm + SiLU forward
// ===========================================================================
template <typename T, typename WT, bool SILU>
__global__ void gn_fwd_kernel(const T* __restrict__ x, const WT* __restrict__ w,
                              const WT* __restrict__ b, T* __restrict__ y,
                              float* __restrict__ mean_out, float* __restrict__ rstd_out,
                              int G, int Cg, int HW, float eps) {
  const long base = (long)blockIdx.x * Cg * HW;
  const int L = Cg * HW;
  const int g = blockIdx.x % G;
  const int tid = threadIdx.x;
  const int nthr = blockDim.x;

  float s1 = 0.f, s2 = 0.f;
  if ((HW & 3) == 0) {
    for (int i = tid * 4; i < L; i += nthr * 4) {
      f32x4 v = load4<T>(x + base + i);
      s1 += v.x + v.y + v.z + v.w;
      s2 += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
  } else {
    for (int i = tid; i < L; i += nthr) {
      float v = to_f32<T>(x[base + i]);
      s1 += v; s2 += v * v;
    }
  }
  __shared__ float lds[2 * 16];
  float2 s = block_reduce_sum2(s1, s2, lds);
  const float m = s.x / L;
  const float var = fmaxf(s.y / L - m * m, 0.f);
  const float rs = rsqrtf(var + eps);
  if (tid == 0) { mean_out[blockIdx.x] = m; rstd_out[blockIdx.x] = rs; }

  const WT* wg = w + (long)g * Cg;
  const WT* bg = b + (long)g * Cg;
  if ((HW & 3) == 0) {
    for (int i = tid * 4; i < L; i += nthr * 4) {
      int c = i / HW;  // uniform across the 4 elements since HW % 4 == 0
      float wc = to_f32<WT>(wg[c]), bc = to_f32<WT>(bg[c]);
      f32x4 v = load4<T>(x + base + i);
      f32x4 o;
      o.x = (v.x - m) * rs * wc + bc;
      o.y = (v.y - m) * rs * wc + bc;
      o.z = (v.z - m) * rs * wc + bc;
      o.w = (v.w - m) * rs * wc + bc;
      if (SILU) { o.x = silu(o.x); o.y = silu(o.y); o.z = silu(o.z); o.w = silu(o.w); }
      store4<T>(y + base + i, o);
    }
  } else {
    for (int i = tid; i < L; i += nthr) {
      int c = i / HW;
      float z = (to_f32<T>(x[base + i]) - m) * rs * to_f32<WT>(wg[c]) + to_f32<WT>(bg[c]);
      if (SILU) z = silu(z);
      y[base + i] = from_f32<T>(z);
    }
  }
}

// ===========================================================================
// GroupNorm + SiLU backward
//   z  = yhat * w[c] + b[c],  yhat = (x - m) * rs
//   dz = dy * (SILU ? dsilu(z) : 1)
//   dx = rs * (w[c]*dz - mean(w*dz) - yhat * mean(w*dz*yhat))
//   dw[c] = sum dz*yhat ; db[c] = sum dz   (fp32 atomics, LDS-staged)
// ===========================================================================
template <typename T, typename WT, bool SILU>
__global__ void gn_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                              const WT* __restrict__ w, const WT* __restrict__ b,
                              const float* __restrict__ mean, const float* __restrict__ rstd,
                              T* __restrict__ dx, float* __restrict__ dw,
                              float* __restrict__ db, int G, int Cg, int HW) {
  extern __shared__ float smem[];  // [2*Cg] channel partials + [32] reduce scratch
  float* dw_l = smem;
  float* db_l = smem + Cg;
  float* red = smem + 2 * Cg;

  const long base = (long)blockIdx.x * Cg * HW;
  const int L = Cg * HW;
  const int g = blockIdx.x % G;
  const int tid = threadIdx.x;
  const int nthr = blockDim.x;
  const float m = mean[blockIdx.x];
  const float rs = rstd[blockIdx.x];
  const WT* wg = w + (long)g * Cg;
  const WT* bg = b + (long)g * Cg;

  for (int c = tid; c < Cg; c += nthr) { dw_l[c] = 0.f; db_l[c] = 0.f; }
  __syncthreads();

  const int lane = tid % DCR_WAVE;
  const bool wave_uniform_c = (HW % (DCR_WAVE * 4) == 0);

  float s1 = 0.f, s2 = 0.f;
  if ((HW & 3) == 0) {
    for (int i = tid * 4; i < L; i += nthr * 4) {
      int c = i / HW;
      float wc = to_f32<WT>(wg[c]), bc = to_f32<WT>(bg[c]);
      f32x4 xv = load4<T>(x + base + i);
      f32x4 gv = load4<T>(dy + base + i);
      float dwp = 0.f, dbp = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float xe = (&xv.x)[k], ge = (&gv.x)[k];
        float yh = (xe - m) * rs;
        float dz = ge;
        if (SILU) dz *= dsilu(yh * wc + bc);
        float gx = dz * wc;
        s1 += gx;
        s2 += gx * yh;
        dwp += dz * yh;
        dbp += dz;
      }
      if (wave_uniform_c) {
        float2 ws = wave_reduce_sum2(dwp, dbp);
        if (lane == 0) { atomicAdd(&dw_l[c], ws.x); atomicAdd(&db_l[c], ws.y); }
      } else {
        atomicAdd(&dw_l[c], dwp);
        atomicAdd(&db_l[c], dbp);
      }
    }
  } else {
    for (int i = tid; i < L; i += nthr) {
      int c = i / HW;
      float wc = to_f32<WT>(wg[c]), bc = to_f32<WT>(bg[c]);
      float xe = to_f32<T>(x[base + i]);
      float ge = to_f32<T>(dy[base + i]);
      float yh = (xe - m) * rs;
      float dz = ge;
      if (SILU) dz *= dsilu(yh * wc + bc);
      float gx = dz * wc;
      s1 += gx;
      s2 += gx * yh;
      atomicAdd(&dw_l[c], dz * yh);
      atomicAdd(&db_l[c], dz);
    }
  }
  __syncthreads();
  float2 s = block_reduce_sum2(s1, s2, red);
  const float m1 = s.x / L;
  const float m2 = s.y / L;

  if ((HW & 3) == 0) {
    for (int i = tid * 4; i < L; i += nthr * 4) {
      int c = i / HW;
      float wc = to_f32<WT>(wg[c]), bc = to_f32<WT>(bg[c]);
      f32x4 xv = load4<T>(x + base + i);
      f32x4 gv = load4<T>(dy + base + i);
      f32x4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float xe = (&xv.x)[k], ge = (&gv.x)[k];
        float yh = (xe - m) * rs;
        float dz = ge;
        if (SILU) dz *= dsilu(yh * wc + bc);
        float gx = dz * wc;
        (&o.x)[k] = rs * (gx - m1 - yh * m2);
      }
      store4<T>(dx + base + i, o);
    }
  } else {
    for (int i = tid; i < L; i += nthr) {
      int c = i / HW;
      float wc = to_f32<WT>(wg[c]), bc = to_f32<WT>(bg[c]);
      float xe = to_f32<T>(x[base + i]);
      float ge = to_f32<T>(dy[base + i]);
      float yh = (xe - m) * rs;
      float dz = ge;
      if (SILU) dz *= dsilu(yh * wc + bc);
      float gx = dz * wc;
      dx[base + i] = from_f32<T>(rs * (gx - m1 - yh * m2));
    }
  }
  __syncthreads();
  for (int c = tid; c < Cg; c += nthr) {
    atomicAdd(&dw[(long)g * Cg + c], dw_l[c]);
    atomicAdd(&db[(long)g * Cg + c], db_l[c]);
  }
}

// ===========================================================================
// LayerNorm forward: one wave per row
// ===========================================================================
template <typename T, typename WT>
__global__ void ln_fwd_kernel(const T* __restrict__ x, const WT* __restrict__ w,
                              const WT* __restrict__ b, T* __restrict__ y,
                              float* __restrict__ mean_out, float* __restrict__ rstd_out,
                              long M, int N, float eps) {
  const int wid = threadIdx.x / DCR_WAVE;
  const int lane = threadIdx.x % DCR_WAVE;
  const long row = (long)blockIdx.x * (blockDim.x / DCR_WAVE) + wid;
  if (row >= M) return;
  const T* xr = x + row * N;
  T* yr = y + row * N;

  float s1 = 0.f, s2 = 0.f;
  if ((N & 3) == 0) {
    for (int j = lane * 4; j < N; j += DCR_WAVE * 4) {
      f32x4 v = load4<T>(xr + j);
      s1 += v.x + v.y + v.z + v.w;
      s2 += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
  } else {
    for (int j = lane; j < N; j += DCR_WAVE) {
      float v = to_f32<T>(xr[j]);
      s1 += v; s2 += v * v;
    }
  }
  float2 s = wave_reduce_sum2(s1, s2);
  const float m = s.x / N;
  const float var = fmaxf(s.y / N - m * m, 0.f);
  const float rs = rsqrtf(var + eps);
  if (lane == 0) { mean_out[row] = m; rstd_out[row] = rs; }

  if ((N & 3) == 0) {
    for (int j = lane * 4; j < N; j += DCR_WAVE * 4) {
      f32x4 v = load4<T>(xr + j);
      f32x4 wv = load4<WT>(w + j);
      f32x4 bv = load4<WT>(b + j);
      f32x4 o;
      o.x = (v.x - m) * rs * wv.x + bv.x;
      o.y = (v.y - m) * rs * wv.y + bv.y;
      o.z = (v.z - m) * rs * wv.z + bv.z;
      o.w = (v.w - m) * rs * wv.w + bv.w;
      store4<T>(yr + j, o);
    }
  } else {
    for (int j = lane; j < N; j += DCR_WAVE) {
      yr[j] = from_f32<T>((to_f32<T>(xr[j]) - m) * rs * to_f32<WT>(w[j])
                          + to_f32<WT>(b[j]));
    }
  }
}

// ===========================================================================
// LayerNorm backward: one wave per row; dw/db via LDS[2N] then global atomics
// ===========================================================================
template <typename T, typename WT>
__global__ void ln_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                              const WT* __restrict__ w,
                              const float* __restrict__ mean, const float* __restrict__ rstd,
                              T* __restrict__ dx, float* __restrict__ dw,
                              float* __restrict__ db, long M, int N) {
  extern __shared__ float smem[];  // [2N]
  float* dw_l = smem;
  float* db_l = smem + N;
  const int wid = threadIdx.x / DCR_WAVE;
  const int lane = threadIdx.x % DCR_WAVE;
  const int waves = blockDim.x / DCR_WAVE;

  for (int j = threadIdx.x; j < 2 * N; j += blockDim.x) smem[j] = 0.f;
  __syncthreads();

  const long row = (long)blockIdx.x * waves + wid;
  if (row < M) {
    const T* xr = x + row * N;
    const T* gr = dy + row * N;
    T* dr = dx + row * N;
    const float m = mean[row];
    const float rs = rstd[row];

    float s1 = 0.f, s2 = 0.f;
    for (int j = lane; j < N; j += DCR_WAVE) {
      float g = to_f32<T>(gr[j]);
      float yh = (to_f32<T>(xr[j]) - m) * rs;
      float gw = g * to_f32<WT>(w[j]);
      s1 += gw;
      s2 += gw * yh;
      atomicAdd(&dw_l[j], g * yh);
      atomicAdd(&db_l[j], g);
    }
    float2 s = wave_reduce_sum2(s1, s2);
    const float m1 = s.x / N;
    const float m2 = s.y / N;
    for (int j = lane; j < N; j += DCR_WAVE) {
      float g = to_f32<T>(gr[j]);
      float yh = (to_f32<T>(xr[j]) - m) * rs;
      float gw = g * to_f32<WT>(w[j]);
      dr[j] = from_f32<T>(rs * (gw - m1 - yh * m2));
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < N; j += blockDim.x) {
    atomicAdd(&dw[j], dw_l[j]);
    atomicAdd(&db[j], db_l[j]);
  }
}

// ===========================================================================
// C++ launchers (instantiated per dtype; called from bindings.cpp)
// ===========================================================================
#define DCR_INST_T(T, WT)                                                              \
  template __global__ void gn_fwd_kernel<T, WT, true>(const T*, const WT*, const WT*,   \
      T*, float*, float*, int, int, int, float);                                        \
  template __global__ void gn_fwd_kernel<T, WT, false>(const T*, const WT*, const WT*,  \
      T*, float*, float*, int, int, int, float);                                        \
  template __global__ void gn_bwd_kernel<T, WT, true>(const T*, const T*, const WT*,    \
      const WT*, const float*, const float*, T*, float*, float*, int, int, int);        \
  template __global__ void gn_bwd_kernel<T, WT, false>(const T*, const T*, const WT*,   \
      const WT*, const float*, const float*, T*, float*, float*, int, int, int);        \
  template __global__ void ln_fwd_kernel<T, WT>(const T*, const WT*, const WT*, T*,     \
      float*, float*, long, int, float);                                                \
  template __global__ void ln_bwd_kernel<T, WT>(const T*, const T*, const WT*,          \
      const float*, const float*, T*, float*, float*, long, int);

DCR_INST_T(float, float)
DCR_INST_T(__hip_bfloat16, float)
DCR_INST_T(__hip_bfloat16, __hip_bfloat16)
DCR_INST_T(__half, float)
DCR_INST_T(__half, __half)

// ===========================================================================
// LayerNorm backward v2 (N <= 2048, N % 4 == 0): one wave per row with the
// row resident in registers (loaded once for both the reduction and dx).
// Shaped for bandwidth:
// * NC (256-column chunks per row) is a template parameter, so N=320 costs
//   2 chunks of registers and not 8: ~3x the waves per SIMD of a fixed
//   8-chunk kernel.
// * a wave walks rows row, row + waves_in_grid, ... and issues the loads of
//   its next row before the current row's wave reduction, so two rows of
//   x/dy per wave are in flight.
// * dw/db accumulate in registers across the wave's rows, the block's
//   waves are added in wave order through LDS, and the block writes one
//   plain [2N] fp32 row of a [blocks, 2N] slab; slab_colsum_kernel adds
//   the rows and writes dw|db in the weight dtype. No zero-init, no
//   atomics, bit-reproducible.
// The per-row arithmetic (element -> lane mapping, summation order, wave
// butterfly) is unchanged from the first v2 kernel, so dx keeps its bits.
// ===========================================================================
#define LNB2_WAVES 8

template <typename T> struct ln_raw4 { typedef uint2 type; };
template <> struct ln_raw4<float> { typedef float4 type; };

template <typename T>
__device__ __forceinline__ typename ln_raw4<T>::type ln_load_raw(const T* __restrict__ p) {
  return *reinterpret_cast<const typename ln_raw4<T>::type*>(p);
}

template <typename T>
__device__ __forceinline__ f32x4 ln_unpack(typename ln_raw4<T>::type r) {
  if constexpr (sizeof(T) == 4) {
    return {r.x, r.y, r.z, r.w};
  } else {
    const T* e = reinterpret_cast<const T*>(&r);
    return {to_f32<T>(e[0]), to_f32<T>(e[1]), to_f32<T>(e[2]), to_f32<T>(e[3])};
  }
}

template <typename T, typename WT, int NC>
__global__ __launch_bounds__(LNB2_WAVES * DCR_WAVE)
void ln_bwd_v2_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                      const WT* __restrict__ w,
                      const float* __restrict__ mean, const float* __restrict__ rstd,
                      T* __restrict__ dx, float* __restrict__ slab, long M, int N) {
  typedef typename ln_raw4<T>::type raw_t;
  extern __shared__ float smem[];  // [2N]: dw | db of this block

  const int wid = threadIdx.x / DCR_WAVE;
  const int lane = threadIdx.x % DCR_WAVE;

  float wv[NC][4], dwacc[NC][4], dbacc[NC][4];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int j = (c * DCR_WAVE + lane) * 4;
    f32x4 ww = {0.f, 0.f, 0.f, 0.f};
    if (j < N) ww = load4<WT>(w + j);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      wv[c][k] = (&ww.x)[k];
      dwacc[c][k] = 0.f;
      dbacc[c][k] = 0.f;
    }
  }

  const long rstride = (long)gridDim.x * LNB2_WAVES;
  long row = (long)blockIdx.x * LNB2_WAVES + wid;

  raw_t xr[NC], gr[NC];
  float m = 0.f, rs = 0.f;
  if (row < M) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int j = (c * DCR_WAVE + lane) * 4;
      if (j < N) {
        xr[c] = ln_load_raw<T>(x + row * N + j);
        gr[c] = ln_load_raw<T>(dy + row * N + j);
      }
    }
    m = mean[row];
    rs = rstd[row];
  }

  while (row < M) {
    // next row's loads go out before this row's reduction
    const long nrow = row + rstride;
    raw_t nxr[NC], ngr[NC];
    float nm = 0.f, nrs = 0.f;
    if (nrow < M) {
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int j = (c * DCR_WAVE + lane) * 4;
        if (j < N) {
          nxr[c] = ln_load_raw<T>(x + nrow * N + j);
          ngr[c] = ln_load_raw<T>(dy + nrow * N + j);
        }
      }
      nm = mean[nrow];
      nrs = rstd[nrow];
    }

    float xv[NC][4], gv[NC][4];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int j = (c * DCR_WAVE + lane) * 4;
      if (j < N) {
        f32x4 xx = ln_unpack<T>(xr[c]);
        f32x4 gg = ln_unpack<T>(gr[c]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          xv[c][k] = (&xx.x)[k];
          gv[c][k] = (&gg.x)[k];
          float yh = (xv[c][k] - m) * rs;
          float gw = gv[c][k] * wv[c][k];
          s1 += gw;
          s2 += gw * yh;
          dwacc[c][k] += gv[c][k] * yh;
          dbacc[c][k] += gv[c][k];
        }
      }
    }
    float2 s = wave_reduce_sum2(s1, s2);
    const float m1 = s.x / N;
    const float m2 = s.y / N;
    T* dr = dx + row * N;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int j = (c * DCR_WAVE + lane) * 4;
      if (j < N) {
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float yh = (xv[c][k] - m) * rs;
          float gw = gv[c][k] * wv[c][k];
          (&o.x)[k] = rs * (gw - m1 - yh * m2);
        }
        store4<T>(dr + j, o);
      }
    }

    row = nrow;
    m = nm;
    rs = nrs;
#pragma unroll
    for (int c = 0; c < NC; ++c) { xr[c] = nxr[c]; gr[c] = ngr[c]; }
  }

  // block combine, wave 0 first then 1, 2, ... (fixed order)
  for (int turn = 0; turn < LNB2_WAVES; ++turn) {
    if (wid == turn) {
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int j = (c * DCR_WAVE + lane) * 4;
        if (j < N) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (turn == 0) {
              smem[j + k] = dwacc[c][k];
              smem[N + j + k] = dbacc[c][k];
            } else {
              smem[j + k] += dwacc[c][k];
              smem[N + j + k] += dbacc[c][k];
            }
          }
        }
      }
    }
    __syncthreads();
  }
  float* srow = slab + (long)blockIdx.x * 2 * N;
  for (int j = threadIdx.x; j < 2 * N; j += blockDim.x) srow[j] = smem[j];
}

// ===========================================================================
// Host launchers
// ===========================================================================
#include "dcr_launchers.h"

namespace dcr {

template <typename T, typename WT>
static void gn_fwd_t(const void* x, const void* w, const void* b, void* y,
                     float* mean, float* rstd, int NG, int G, int Cg, int HW,
                     float eps, bool silu, hipStream_t s) {
  dim3 grid(NG), block(256);
  if (silu)
    hipLaunchKernelGGL((gn_fwd_kernel<T, WT, true>), grid, block, 0, s,
                       (const T*)x, (const WT*)w, (const WT*)b, (T*)y, mean, rstd, G, Cg, HW, eps);
  else
    hipLaunchKernelGGL((gn_fwd_kernel<T, WT, false>), grid, block, 0, s,
                       (const T*)x, (const WT*)w, (const WT*)b, (T*)y, mean, rstd, G, Cg, HW, eps);
}

void gn_fwd_launch(DType dt, const void* x, const void* w, const void* b,
                   bool w_f32, void* y, float* mean, float* rstd, int NG,
                   int G, int Cg, int HW, float eps, bool silu, hipStream_t s) {
  switch (dt) {
    case DT_F32: gn_fwd_t<float, float>(x, w, b, y, mean, rstd, NG, G, Cg, HW, eps, silu, s); break;
    case DT_F16:
      if (w_f32) gn_fwd_t<__half, float>(x, w, b, y, mean, rstd, NG, G, Cg, HW, eps, silu, s);
      else gn_fwd_t<__half, __half>(x, w, b, y, mean, rstd, NG, G, Cg, HW, eps, silu, s);
      break;
    case DT_BF16:
      if (w_f32) gn_fwd_t<__hip_bfloat16, float>(x, w, b, y, mean, rstd, NG, G, Cg, HW, eps, silu, s);
      else gn_fwd_t<__hip_bfloat16, __hip_bfloat16>(x, w, b, y, mean, rstd, NG, G, Cg, HW, eps, silu, s);
      break;
  }
}

template <typename T, typename WT>
static void gn_bwd_t(const void* dy, const void* x, const void* w, const void* b,
                     const float* mean, const float* rstd, void* dx, float* dw,
                     float* db, int NG, int G, int Cg, int HW, bool silu,
                     hipStream_t s) {
  dim3 grid(NG), block(256);
  size_t lds = (2 * Cg + 32) * sizeof(float);
  if (silu)
    hipLaunchKernelGGL((gn_bwd_kernel<T, WT, true>), grid, block, lds, s,
                       (const T*)dy, (const T*)x, (const WT*)w, (const WT*)b, mean, rstd, (T*)dx, dw, db, G, Cg, HW);
  else
    hipLaunchKernelGGL((gn_bwd_kernel<T, WT, false>), grid, block, lds, s,
                       (const T*)dy, (const T*)x, (const WT*)w, (const WT*)b, mean, rstd, (T*)dx, dw, db, G, Cg, HW);
}

void gn_bwd_launch(DType dt, const void* dy, const void* x, const void* w,
                   const void* b, bool w_f32, const float* mean, const float* rstd,
                   void* dx, float* dw, float* db, int NG, int G, int Cg,
                   int HW, bool silu, hipStream_t s) {
  switch (dt) {
    case DT_F32: gn_bwd_t<float, float>(dy, x, w, b, mean, rstd, dx, dw, db, NG, G, Cg, HW, silu, s); break;
    case DT_F16:
      if (w_f32) gn_bwd_t<__half, float>(dy, x, w, b, mean, rstd, dx, dw, db, NG, G, Cg, HW, silu, s);
      else gn_bwd_t<__half, __half>(dy, x, w, b, mean, rstd, dx, dw, db, NG, G, Cg, HW, silu, s);
      break;
    case DT_BF16:
      if (w_f32) gn_bwd_t<__hip_bfloat16, float>(dy, x, w, b, mean, rstd, dx, dw, db, NG, G, Cg, HW, silu, s);
      else gn_bwd_t<__hip_bfloat16, __hip_bfloat16>(dy, x, w, b, mean, rstd, dx, dw, db, NG, G, Cg, HW, silu, s);
      break;
  }
}

template <typename T, typename WT>
static void ln_fwd_t(const void* x, const void* w, const void* b, void* y,
                     float* mean, float* rstd, long M, int N, float eps,
                     hipStream_t s) {
  const int waves = 4;
  dim3 grid((M + waves - 1) / waves), block(waves * DCR_WAVE);
  hipLaunchKernelGGL((ln_fwd_kernel<T, WT>), grid, block, 0, s, (const T*)x,
                     (const WT*)w, (const WT*)b, (T*)y, mean, rstd, M, N, eps);
}

void ln_fwd_launch(DType dt, const void* x, const void* w, const void* b,
                   bool w_f32, void* y, float* mean, float* rstd, long M,
                   int N, float eps, hipStream_t s) {
  switch (dt) {
    case DT_F32: ln_fwd_t<float, float>(x, w, b, y, mean, rstd, M, N, eps, s); break;
    case DT_F16:
      if (w_f32) ln_fwd_t<__half, float>(x, w, b, y, mean, rstd, M, N, eps, s);
      else ln_fwd_t<__half, __half>(x, w, b, y, mean, rstd, M, N, eps, s);
      break;
    case DT_BF16:
      if (w_f32) ln_fwd_t<__hip_bfloat16, float>(x, w, b, y, mean, rstd, M, N, eps, s);
      else ln_fwd_t<__hip_bfloat16, __hip_bfloat16>(x, w, b, y, mean, rstd, M, N, eps, s);
      break;
  }
}

template <typename T, typename WT>
static void ln_bwd_t(const void* dy, const void* x, const void* w,
                     const float* mean, const float* rstd, void* dx, float* dw,
                     float* db, long M, int N, hipStream_t s) {
  // v1: zero-initialised dw/db, LDS + global atomics (N > 2048 or N % 4)
  size_t lds = 2 * (size_t)N * sizeof(float);
  const int waves = 4;
  dim3 grid((M + waves - 1) / waves), block(waves * DCR_WAVE);
  hipLaunchKernelGGL((ln_bwd_kernel<T, WT>), grid, block, lds, s, (const T*)dy,
                     (const T*)x, (const WT*)w, mean, rstd, (T*)dx, dw, db, M, N);
}

void ln_bwd_launch(DType dt, const void* dy, const void* x, const void* w,
                   bool w_f32, const float* mean, const float* rstd, void* dx,
                   float* dw, float* db, long M, int N, hipStream_t s) {
  switch (dt) {
    case DT_F32: ln_bwd_t<float, float>(dy, x, w, mean, rstd, dx, dw, db, M, N, s); break;
    case DT_F16:
      if (w_f32) ln_bwd_t<__half, float>(dy, x, w, mean, rstd, dx, dw, db, M, N, s);
      else ln_bwd_t<__half, __half>(dy, x, w, mean, rstd, dx, dw, db, M, N, s);
      break;
    case DT_BF16:
      if (w_f32) ln_bwd_t<__hip_bfloat16, float>(dy, x, w, mean, rstd, dx, dw, db, M, N, s);
      else ln_bwd_t<__hip_bfloat16, __hip_bfloat16>(dy, x, w, mean, rstd, dx, dw, db, M, N, s);
      break;
  }
}

// v2 grid: 8-wave blocks, 2 rows per wave until 512 blocks, then more rows
// per wave. The slab costs blocks * 2N * 4 B written and read once; at
// 512 blocks that is 8 % of the x/dy/dx traffic at 16384x320 and the
// grid still puts 4 waves on every SIMD.
int ln_bwd_v2_blocks(long M, int N) {
  if (N > 2048 || (N & 3) != 0) return 0;
  long blocks = (M + 2 * LNB2_WAVES - 1) / (2 * LNB2_WAVES);
  if (blocks > 512) blocks = 512;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}

template <typename T, typename WT, int NC>
static void ln_bwd_v2_nc(const void* dy, const void* x, const void* w,
                         const float* mean, const float* rstd, void* dx,
                         float* slab, int blocks, long M, int N, hipStream_t s) {
  size_t lds = 2 * (size_t)N * sizeof(float);
  hipLaunchKernelGGL((ln_bwd_v2_kernel<T, WT, NC>), dim3((unsigned)blocks),
                     dim3(LNB2_WAVES * DCR_WAVE), lds, s, (const T*)dy,
                     (const T*)x, (const WT*)w, mean, rstd, (T*)dx, slab, M, N);
}

template <typename T, typename WT>
static void ln_bwd_v2_t(const void* dy, const void* x, const void* w,
                        const float* mean, const float* rstd, void* dx,
                        float* slab, void* dwdb, int blocks, long M, int N,
                        hipStream_t s) {
  const int nchunk = (N + DCR_WAVE * 4 - 1) / (DCR_WAVE * 4);
  if (nchunk <= 2) ln_bwd_v2_nc<T, WT, 2>(dy, x, w, mean, rstd, dx, slab, blocks, M, N, s);
  else if (nchunk <= 3) ln_bwd_v2_nc<T, WT, 3>(dy, x, w, mean, rstd, dx, slab, blocks, M, N, s);
  else if (nchunk <= 5) ln_bwd_v2_nc<T, WT, 5>(dy, x, w, mean, rstd, dx, slab, blocks, M, N, s);
  else ln_bwd_v2_nc<T, WT, 8>(dy, x, w, mean, rstd, dx, slab, blocks, M, N, s);
  slab_colsum_launch<WT>(slab, dwdb, blocks, 2 * N, 2L * N, s);
}

void ln_bwd_v2_launch(DType dt, const void* dy, const void* x, const void* w,
                      bool w_f32, const float* mean, const float* rstd,
                      void* dx, float* slab, void* dwdb, int blocks, long M,
                      int N, hipStream_t s) {
  switch (dt) {
    case DT_F32: ln_bwd_v2_t<float, float>(dy, x, w, mean, rstd, dx, slab, dwdb, blocks, M, N, s); break;
    case DT_F16:
      if (w_f32) ln_bwd_v2_t<__half, float>(dy, x, w, mean, rstd, dx, slab, dwdb, blocks, M, N, s);
      else ln_bwd_v2_t<__half, __half>(dy, x, w, mean, rstd, dx, slab, dwdb, blocks, M, N, s);
      break;
    case DT_BF16:
      if (w_f32) ln_bwd_v2_t<__hip_bfloat16, float>(dy, x, w, mean, rstd, dx, slab, dwdb, blocks, M, N, s);
      else ln_bwd_v2_t<__hip_bfloat16, __hip_bfloat16>(dy, x, w, mean, rstd, dx, slab, dwdb, blocks, M, N, s);
      break;
  }
}

}  // namespace dcr
