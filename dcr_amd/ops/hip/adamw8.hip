// AdamW with block-scaled FP8 optimizer state (FusedAdamW state_bits=8).
//
// State format (normative; dcr_amd/ops/adamw.py quantize_blockwise is the
// CPU twin and ops/hip/README.md the description):
//   * quantisation block = 256 consecutive elements of the flat arena,
//     nblocks = ceil(n / 256); blocks ignore parameter boundaries
//   * codes uint8[nblocks*256] are OCP e4m3fn (gfx950's v_cvt_pk_*_fp8;
//     NOT gfx942's FNUZ), one fp32 absmax per block
//   * code = e4m3fn_rne(clamp(x * (448/absmax), -448, 448)); dequantise
//     float(code) * (absmax/448)
//   * a block whose 448/absmax is not finite (absmax == 0, or below
//     448/FLT_MAX ~ 1.3e-36 where the scale overflows) is stored as a zero
//     block: all codes 0, absmax 0
//   * first moment stored as is; second moment stored as r = sqrt(v)
//   * padding bytes past n are 0 and stay 0
//
// One pass over memory: dequantise, update m/v and the param in fp32
// registers (the update uses the UNquantised m', v'), reduce the block
// absmax across the wave with shuffles (no LDS, no atomics), requantise,
// store. One wave per block, 4 elements per lane: a dword of codes per
// moment, a dwordx2 of bf16 grads and a dwordx4 of master per lane, every
// instruction fully coalesced. (A 16-lanes-per-block, 16-elements-per-lane
// mapping with 16 B code accesses was measured and tied; see the rejected
// experiments in ops/hip/README.md.)
//
// FP contraction is OFF in this file: the CPU reference rounds every
// multiply and add separately, and an FMA on one side only moves values
// that sit near an FP8 rounding tie onto the neighbouring code.
//
// Non-finite gradients get no special handling, as in the fp32-state
// kernels: the parameter becomes NaN/inf. What is left in the state then
// differs from the CPU reference (here fmaxf drops a NaN from the absmax
// and the clamp turns a NaN product into the -448 code; torch's amax and
// clamp propagate the NaN). Neither is meaningful; the fp16 scaler path
// skips such steps before the optimizer runs.
#pragma clang fp contract(off)

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "dcr_common.h"
#include "dcr_launchers.h"

using namespace dcr;

namespace {

constexpr int QBLOCK = 256;
constexpr int EPL = QBLOCK / DCR_WAVE;   // elements per lane
constexpr int BPWG = 256 / DCR_WAVE;     // qblocks (= waves) per workgroup
constexpr float FP8_MAX = 448.f;
constexpr long MAX_WGS = 8192;           // grid cap, as ew_blocks

typedef float f32x2_t __attribute__((ext_vector_type(2)));

// 4 codes (one dword, element 0 in the low byte) -> 4 floats * s
__device__ __forceinline__ void dq4(unsigned w, float s, float* o) {
  f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
  f32x2_t hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  o[0] = lo.x * s; o[1] = lo.y * s; o[2] = hi.x * s; o[3] = hi.y * s;
}

__device__ __forceinline__ float clamp448(float x) {
  return fminf(fmaxf(x, -FP8_MAX), FP8_MAX);
}

// 4 floats -> 4 codes; the clamp is part of the format (x*s can round
// just above 448; saturation of the convert is not relied on)
__device__ __forceinline__ unsigned q4(const float* x, float s) {
  int w = 0;
  w = __builtin_amdgcn_cvt_pk_fp8_f32(clamp448(x[0] * s), clamp448(x[1] * s), w, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(clamp448(x[2] * s), clamp448(x[3] * s), w, true);
  return (unsigned)w;
}

__device__ __forceinline__ float wave_reduce_max(float v) {
#pragma unroll
  for (int off = DCR_WAVE / 2; off > 0; off >>= 1)
    v = fmaxf(v, __shfl_xor(v, off, DCR_WAVE));
  return v;
}

// P = float (params updated in place) or __hip_bfloat16 (bf16 params out,
// fp32 master in/out).
// CLIP follows adamw_kernel<CLIP> (elementwise.hip): the clip coefficient is
// rec[2] of the device record that sumsq_finalize_kernel (grad_tail.hip)
// wrote. When it is not 1 the kernel forms the clipped gradient as
// `flat_grad.mul_(coef.to(dtype))` would (fp32: g * coef; bf16: coef rounded
// to bf16, product in fp32, rounded to bf16, widened again), stores it back
// into the arena and updates from it; when it is 1 the arena is only read.
// The branch is uniform over the grid. CLIP=false never touches rec or
// writes g (g is const there): it is the kernel of step(), bit for bit.
template <typename P, bool CLIP>
__global__ __launch_bounds__(256) void adamw8_kernel(
    P* __restrict__ p,
    typename std::conditional<CLIP, P, const P>::type* __restrict__ g,
    float* __restrict__ master,
    uint8_t* __restrict__ mq, float* __restrict__ mabs,
    uint8_t* __restrict__ rq, float* __restrict__ rabs, long n, long nblocks,
    float lr, float beta1, float omb1, float beta2, float omb2, float eps,
    float wd, float inv_bc1, float inv_bc2, const float* __restrict__ rec) {
  constexpr bool BF16 = !std::is_same<P, float>::value;
  float coef = 1.f;
  if constexpr (CLIP) coef = rec[2];
  const bool clip = CLIP && coef != 1.f;
  // what aten's mul_ by a 0-dim tensor of the arena's dtype multiplies by
  const float cm = BF16 ? to_f32<P>(from_f32<P>(coef)) : coef;
  const int lane = threadIdx.x % DCR_WAVE;
  // fp32 params: the "master" IS the param arena
  float* __restrict__ w32 = BF16 ? master : reinterpret_cast<float*>(p);

  // qb is wave-uniform, so all 64 lanes reach the shuffles together
  const long stride = (long)gridDim.x * BPWG;
  for (long qb = (long)blockIdx.x * BPWG + threadIdx.x / DCR_WAVE;
       qb < nblocks; qb += stride) {
    const long e0 = qb * QBLOCK + (long)lane * EPL;
    const bool full = e0 + EPL <= n;   // false only in a partial last block

    float gv[EPL], pv[EPL], mv[EPL], rv[EPL];
    // ---- load -----------------------------------------------------------
    if (full) {
      f32x4 t = load4<P>(g + e0);
      gv[0] = t.x; gv[1] = t.y; gv[2] = t.z; gv[3] = t.w;
      f32x4 u = load4<float>(w32 + e0);
      pv[0] = u.x; pv[1] = u.y; pv[2] = u.z; pv[3] = u.w;
    } else {
      // masked elements neither load nor store p, g, master; with g = 0
      // and zero state they give m' = r' = 0 and so code 0
#pragma unroll
      for (int k = 0; k < EPL; ++k) {
        const bool ok = e0 + k < n;
        gv[k] = ok ? to_f32<P>(g[e0 + k]) : 0.f;
        pv[k] = ok ? w32[e0 + k] : 0.f;
      }
    }
    if constexpr (CLIP) {
      if (clip) {
        // masked elements stay 0 and are not stored
#pragma unroll
        for (int k = 0; k < EPL; ++k)
          if (full || e0 + k < n) gv[k] = to_f32<P>(from_f32<P>(gv[k] * cm));
        if (full) {
          f32x4 t = {gv[0], gv[1], gv[2], gv[3]};
          store4<P>(g + e0, t);
        } else {
#pragma unroll
          for (int k = 0; k < EPL; ++k)
            if (e0 + k < n) g[e0 + k] = from_f32<P>(gv[k]);
        }
      }
    }
    // codes are allocated to nblocks*256, padding included
    dq4(*reinterpret_cast<const unsigned*>(mq + e0), mabs[qb] / FP8_MAX, mv);
    dq4(*reinterpret_cast<const unsigned*>(rq + e0), rabs[qb] / FP8_MAX, rv);

    // ---- update (fp32, uses m', v' before requantising) -------------------
    float mmax = 0.f, rmax = 0.f;
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
      const float gg = gv[k];
      const float mm = beta1 * mv[k] + omb1 * gg;
      const float vv = beta2 * (rv[k] * rv[k]) + omb2 * (gg * gg);
      const float denom = sqrtf(vv * inv_bc2) + eps;
      const float upd = (mm * inv_bc1) / denom + wd * pv[k];
      pv[k] = pv[k] - lr * upd;
      const float rr = sqrtf(vv);
      mv[k] = mm; rv[k] = rr;
      mmax = fmaxf(mmax, fabsf(mm));
      rmax = fmaxf(rmax, rr);
    }
    mmax = wave_reduce_max(mmax);
    rmax = wave_reduce_max(rmax);

    // ---- store ------------------------------------------------------------
    if (full) {
      f32x4 u = {pv[0], pv[1], pv[2], pv[3]};
      store4<float>(w32 + e0, u);
      if constexpr (BF16) store4<P>(p + e0, u);
    } else {
#pragma unroll
      for (int k = 0; k < EPL; ++k) {
        if (e0 + k < n) {
          w32[e0 + k] = pv[k];
          if constexpr (BF16) p[e0 + k] = from_f32<P>(pv[k]);
        }
      }
    }
    // a scale that is not finite (absmax 0, or so small that 448/absmax
    // overflows: 0 * inf would be NaN) makes the block a zero block
    const float mqs = FP8_MAX / mmax, rqs = FP8_MAX / rmax;
    const bool mok = __builtin_isfinite(mqs), rok = __builtin_isfinite(rqs);
    *reinterpret_cast<unsigned*>(mq + e0) = mok ? q4(mv, mqs) : 0u;
    *reinterpret_cast<unsigned*>(rq + e0) = rok ? q4(rv, rqs) : 0u;
    if (lane == 0) { mabs[qb] = mok ? mmax : 0.f; rabs[qb] = rok ? rmax : 0.f; }
  }
}

// CLIP=false: the kernel of step(), g only read (rec unused, null);
// CLIP=true: the clip-aware kernel, which may write g
template <typename P, bool CLIP>
void launch(void* p, typename std::conditional<CLIP, void, const void>::type* g,
            float* master, uint8_t* mq, float* mabs, uint8_t* rq, float* rabs,
            long n, float lr, float b1, float omb1, float b2, float omb2,
            float eps, float wd, float ibc1, float ibc2, const float* rec,
            hipStream_t s) {
  using G = typename std::conditional<CLIP, P, const P>::type;
  const long nblocks = (n + QBLOCK - 1) / QBLOCK;
  long wgs = (nblocks + BPWG - 1) / BPWG;
  if (wgs > MAX_WGS) wgs = MAX_WGS;   // grid-stride covers the rest
  hipLaunchKernelGGL((adamw8_kernel<P, CLIP>), dim3((unsigned)wgs), dim3(256),
                     0, s, (P*)p, (G*)g, master, mq, mabs, rq, rabs, n, nblocks,
                     lr, b1, omb1, b2, omb2, eps, wd, ibc1, ibc2, rec);
}

template <bool CLIP>
void launch_dtype(int bf16, void* p,
                  typename std::conditional<CLIP, void, const void>::type* g,
                  float* master, uint8_t* mq, float* mabs, uint8_t* rq,
                  float* rabs, long n, double lr, double b1, double b2,
                  double eps, double wd, long step, const float* rec,
                  hipStream_t s) {
  if (n <= 0) return;
  // scalars are formed in double and rounded once, exactly as the CPU
  // reference does (python floats -> fp32 tensor scalars)
  const float omb1 = (float)(1.0 - b1), omb2 = (float)(1.0 - b2);
  const float ibc1 = (float)(1.0 / (1.0 - std::pow(b1, (double)step)));
  const float ibc2 = (float)(1.0 / (1.0 - std::pow(b2, (double)step)));
  if (bf16)
    launch<__hip_bfloat16, CLIP>(p, g, master, mq, mabs, rq, rabs, n, (float)lr,
                                 (float)b1, omb1, (float)b2, omb2, (float)eps,
                                 (float)wd, ibc1, ibc2, rec, s);
  else
    launch<float, CLIP>(p, g, master, mq, mabs, rq, rabs, n, (float)lr,
                        (float)b1, omb1, (float)b2, omb2, (float)eps, (float)wd,
                        ibc1, ibc2, rec, s);
}

}  // namespace

namespace dcr {

void adamw8_launch(int bf16, void* p, const void* g, float* master,
                   unsigned char* mq, float* mabs, unsigned char* rq,
                   float* rabs, long n, double lr, double b1, double b2,
                   double eps, double wd, long step, hipStream_t s) {
  launch_dtype<false>(bf16, p, g, master, mq, mabs, rq, rabs, n, lr, b1, b2,
                      eps, wd, step, nullptr, s);
}

void adamw8_clip_launch(int bf16, void* p, void* g, float* master,
                        unsigned char* mq, float* mabs, unsigned char* rq,
                        float* rabs, long n, double lr, double b1, double b2,
                        double eps, double wd, long step, const float* rec,
                        hipStream_t s) {
  launch_dtype<true>(bf16, p, g, master, mq, mabs, rq, rabs, n, lr, b1, b2, eps,
                     wd, step, rec, s);
}

}  // namespace dcr
