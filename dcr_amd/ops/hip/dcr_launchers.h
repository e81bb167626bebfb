// Host-side launcher API for the dcr_amd HIP kernels.
// bindings.cpp (built by the host compiler) calls these; definitions live
// in the .hip TUs compiled by hipcc for gfx950.
#pragma once

#include <hip/hip_runtime.h>

namespace dcr {

enum DType { DT_F32 = 0, DT_F16 = 1, DT_BF16 = 2 };

// norms.hip (w_f32: weights/bias are fp32; else same dtype as x)
void gn_fwd_launch(DType dt, const void* x, const void* w, const void* b,
                   bool w_f32, void* y, float* mean, float* rstd, int NG,
                   int G, int Cg, int HW, float eps, bool silu, hipStream_t s);
void gn_bwd_launch(DType dt, const void* dy, const void* x, const void* w,
                   const void* b, bool w_f32, const float* mean,
                   const float* rstd, void* dx, float* dw, float* db, int NG,
                   int G, int Cg, int HW, bool silu, hipStream_t s);
void ln_fwd_launch(DType dt, const void* x, const void* w, const void* b,
                   bool w_f32, void* y, float* mean, float* rstd, long M,
                   int N, float eps, hipStream_t s);
void ln_bwd_launch(DType dt, const void* dy, const void* x, const void* w,
                   bool w_f32, const float* mean, const float* rstd, void* dx,
                   float* dw, float* db, long M, int N, hipStream_t s);
// LN backward v2 (N <= 2048, N % 4 == 0): ln_bwd_v2_blocks() is the grid,
// or 0 when the shape needs ln_bwd_launch (zeroed fp32 dw/db, atomics).
// slab: blocks*2N floats, uninitialised; dwdb: [2N] in the weight dtype.
int ln_bwd_v2_blocks(long M, int N);
void ln_bwd_v2_launch(DType dt, const void* dy, const void* x, const void* w,
                      bool w_f32, const float* mean, const float* rstd,
                      void* dx, float* slab, void* dwdb, int blocks, long M,
                      int N, hipStream_t s);

// norms_nhwc.hip (channels_last GroupNorm; w_f32 as above).
// Workspaces are per-chunk partial slabs (plain stores, deterministic,
// no zero-init needed): fwd ws = chunks*N*G*2 floats; bwd ws =
// chunks*N*G*2 + chunks*N*2C + N*G*2 floats. chunks = gn_nhwc_chunks().
// bwd writes dw|db as one [2C] array in the weight dtype (dwdb).
int gn_nhwc_chunks(int N, int R);
void gn_nhwc_fwd_launch(DType dt, const void* x, const void* w, const void* b,
                        bool w_f32, void* y, float* ws, float* mean, float* rstd,
                        int N, int R, int C, int G, float eps, bool silu,
                        hipStream_t s);
void gn_nhwc_bwd_launch(DType dt, const void* dy, const void* x, const void* w,
                        const void* b, bool w_f32, const float* mean,
                        const float* rstd, float* ws, void* dx, void* dwdb,
                        int N, int R, int C, int G, bool silu,
                        hipStream_t s);

// reduce.hip — bias-gradient column sums of x [groups, rows_per_group, C].
// chunks = colsum_chunks(dt, groups, rows_per_group, C, cap); slab holds
// groups*chunks*C floats, uninitialised (unused when out_n is null and
// chunks == 1: one launch). out_n [groups, C] may be null (groups == 1).
int colsum_chunks(int dt, long groups, long rows_per_group, int C, int cap);
void colsum_launch(DType dt, const void* x, float* slab, void* out_n, void* out,
                   long groups, long rows_per_group, int C, int chunks,
                   hipStream_t s);

// elementwise.hip
void geglu_fwd_launch(DType dt, const void* x, void* y, long M, long N,
                      hipStream_t s);
void geglu_bwd_launch(DType dt, const void* dy, const void* x, void* dx,
                      long M, long N, hipStream_t s);
void adamw_launch(float* p, const float* g, float* m, float* v, long n,
                  float lr, float b1, float b2, float eps, float wd, long step,
                  hipStream_t s);
void adamw_bf16_launch(void* p, const void* g, float* master, float* m,
                       float* v, long n, float lr, float b1, float b2,
                       float eps, float wd, long step, hipStream_t s);
// clip-aware AdamW: rec = device float[3] {sumsq, norm, coef} written by
// sumsq_finalize_launch; when coef != 1 the clipped gradient is stored back
// into g and used for the update
void adamw_clip_launch(float* p, float* g, float* m, float* v, long n,
                       float lr, float b1, float b2, float eps, float wd,
                       long step, const float* rec, hipStream_t s);
void adamw_bf16_clip_launch(void* p, void* g, float* master, float* m,
                            float* v, long n, float lr, float b1, float b2,
                            float eps, float wd, long step, const float* rec,
                            hipStream_t s);
// grad_tail.hip — dt is DT_BF16 or DT_F32. table: device int64 [nparams, 4]
// = {source address, destination element offset in arena, element count,
// virtual blocks before this parameter}; a virtual block is `ch` elements
// of one parameter (ch % 8 == 0), nvb their total. store: copy source to
// arena; partials (nvb floats, uninitialised; may be null when store) gets
// each virtual block's sum of squares. !store needs partials and only reads.
// add (with store, partials ignored): arena = T(float(arena) + float(source))
// instead of the copy; no sum of squares.
int grad_gather_grid(long nvb, int grid_req);
void grad_gather_launch(DType dt, const long* table, int nparams, long nvb,
                        void* arena, float* partials, int ch, int grid,
                        bool store, bool add, hipStream_t s);
void sumsq_finalize_launch(const float* partials, long nvb, float max_norm,
                           float* rec, hipStream_t s);
// device-state AdamW (round-2 draft; hipGraph-capturable step)
void adamw_dev_launch(int bf16, void* p, const void* g, float* master,
                      float* m, float* v, long n, float b1, float b2,
                      float eps, float wd, float max_norm, float* hyper,
                      hipStream_t s);
// adamw8.hip — AdamW with block-scaled FP8 (e4m3fn) state; bf16 != 0:
// bf16 params + fp32 master, else fp32 params (master unused).
void adamw8_launch(int bf16, void* p, const void* g, float* master,
                   unsigned char* mq, float* mabs, unsigned char* rq,
                   float* rabs, long n, double lr, double b1, double b2,
                   double eps, double wd, long step, hipStream_t s);
// clip-aware: rec as for adamw_clip_launch; may rewrite g
void adamw8_clip_launch(int bf16, void* p, void* g, float* master,
                        unsigned char* mq, float* mabs, unsigned char* rq,
                        float* rabs, long n, double lr, double b1, double b2,
                        double eps, double wd, long step, const float* rec,
                        hipStream_t s);
void sched_launch(DType dt, int mode, const void* x0, const void* noise,
                  const float* ac, const long* t, void* out, long per_sample,
                  long total, hipStream_t s);
void cfg_launch(DType dt, const void* eu, const void* et, void* out, float s_,
                long total, hipStream_t s);
void lincomb_launch(DType dt, const void* X, const void* Y, const void* Z,
                    void* out, float a, float b, float c, long total,
                    hipStream_t s);

// attention.hip (bf16, head_dim 64)
void attn_fwd_launch(const void* q, const void* k, const void* v, void* o,
                     float* lse, int BH, int Lq, int Lk, int H, float scale,
                     bool causal, hipStream_t s);
// v2: masked-tail MFMA skip (round-2 draft; not dispatched)
void attn_fwd_v2_launch(const void* q, const void* k, const void* v, void* o,
                        float* lse, int BH, int Lq, int Lk, int H, float scale,
                        bool causal, hipStream_t s);
// v3: T14 async-stage + one barrier/tile + setprio (round-2 draft)
void attn_fwd_v3_launch(const void* q, const void* k, const void* v, void* o,
                        float* lse, int BH, int Lq, int Lk, int H, float scale,
                        bool causal, hipStream_t s);
// v4: swapped-QK^T in-register-softmax schedule (round-2)
void attn_fwd_v4_launch(const void* q, const void* k, const void* v, void* o,
                        float* lse, int BH, int Lq, int Lk, int H, float scale,
                        bool causal, hipStream_t s);
// generalized head-dim forward (SD-1.x 40/80/160); lse may be nullptr
void attn_fwd_gen_launch(const void* q, const void* k, const void* v, void* o,
                         float* lse, int BH, int Lq, int Lk, int H, int D,
                         float scale, bool causal, hipStream_t s);
// D=512 forward (VAE mid-block's single head): non-causal, no LSE
void attn_fwd_d512_launch(const void* q, const void* k, const void* v, void* o,
                          int BH, int Lq, int Lk, int H, float scale,
                          hipStream_t s);
// generalized head-dim backward (40/80/160): delta + dK/dV + dQ, no atomics
void attn_bwd_gen_launch(const void* q, const void* k, const void* v,
                         const void* o, const void* dO, const float* lse,
                         float* delta, void* dQ, void* dK, void* dV, int BH,
                         int Lq, int Lk, int H, int D, float scale,
                         bool causal, hipStream_t s);
void attn_bwd_launch(const void* q, const void* k, const void* v,
                     const void* o, const void* dO, const float* lse,
                     float* delta, void* dQ, void* dK, void* dV, int BH,
                     int Lq, int Lk, int H, float scale, bool causal,
                     hipStream_t s);
// backward v4 (swapped-operand schedule; DCR_ATTN_BWD_V4 draft)
void attn_bwd_v4_launch(const void* q, const void* k, const void* v,
                        const void* o, const void* dO, const float* lse,
                        float* delta, void* dQ, void* dK, void* dV, int BH,
                        int Lq, int Lk, int H, float scale, bool causal,
                        hipStream_t s);
void mfma_probe_launch(const void* A, const void* B, float* C, hipStream_t s);

// conv_nhwc.hip (implicit-GEMM conv fwd, opt-in); bias is fp32, or bf16
// when bias_bf16 (widened in the epilogue)
void conv_nhwc_fwd_launch(const void* x, const void* w, const void* bias,
                          bool bias_bf16, void* y, int Nb, int Hin, int Win, int C, int K,
                          int P, int Q, int R, int S, int stride, int pad,
                          hipStream_t st);
void conv_nhwc_fwd_v2_launch(const void* x, const void* w, const void* bias,
                             bool bias_bf16, void* y, float* ws, int splitz, const void* res,
                             const void* temb, int Nb, int Hin, int Win, int C,
                             int K, int P, int Q, int R, int S, int stride,
                             int pad, hipStream_t st);
// conv_nhwc_bwd.hip (dgrad + wgrad + fused bias-grad; DCR_NATIVE_CONV_BWD)
void conv_bwd_weight_launch(const void* dy, const void* x, float* dw_ws,
                            int Nb, int Hin, int Win, int C, int K, int P,
                            int Q, int R, int S, int stride, int pad,
                            int splits, void* dW_out, hipStream_t st);
void conv_bwd_data_launch(const void* dy, const void* w, void* dx, int Nb,
                          int Hin, int Win, int C, int K, int P, int Q, int R,
                          int S, int stride, int pad, hipStream_t st);
void conv_bias_grad_launch(const void* dy, float* db, long NPQ, int K,
                           hipStream_t st);

// gemm.hip — bf16 MFMA GEMM for transformer linears (fwd/dgrad/wgrad)
void gemm_bf16_launch(const void* A, const void* B, const float* bias,
                      void* C, float* ws, float* dbias, long M, long N, int K,
                      int ta, int tb, int want_dbias, int splitz,
                      hipStream_t st);
// split-contraction weight gradient dW = dy^T x (+ db = column sums of dy),
// bf16. slab: split * (N*K + (want_db ? N : 0)) floats, uninitialised;
// dwdb: N*K (+ N) bf16. tile/split/chunks_per_slice from linear_wgrad_plan.
void linear_wgrad_plan(long M, int N, int K, int tile_req, int split_req,
                       int* tile, int* split, int* chunks_per_slice);
void linear_wgrad_launch(const void* dy, const void* x, float* slab,
                         void* dwdb, long M, int N, int K, int want_db,
                         int tile, int split, int chunks_per_slice,
                         hipStream_t st);

// maxsim.hip — out[n,m] = max_{p,q} <A[n,p,:], B[m,q,:]>; A [N,P,K] and
// B [M,Q,K] bf16 contiguous, K % 8 == 0; out [N,M] fp32 pre-filled with
// -inf (partial maxima are combined with atomics). N, M >= 1.
void patch_maxsim_launch(const void* A, const void* B, float* out, long N,
                         long M, int P, int Q, int K, hipStream_t st);

// splitsim.hip — out[n,m] = max_g <A[n,g,:], B[m,g,:]>; A [N,G,L] and
// B [M,G,L] bf16 contiguous, L % 8 == 0, G*L < 2^31; out [N,M] fp32.
// S = split_product_splits(N, M, G, splits_req) blocks share a tile's groups
// (splits_req > 0 forces the count, clamped to G). S == 1: plain stores, out
// may be uninitialised. S > 1: out pre-filled with -inf, partial maxima are
// combined with atomics. N, M, G >= 1; ceil(N/128)*ceil(M/128)*S < 2^31.
int split_product_splits(long N, long M, int G, int splits_req);
void split_product_launch(const void* A, const void* B, float* out, long N,
                          long M, int G, int L, int S, hipStream_t st);

// topk_sim.hip — per row of Qm [Nq,K] the m best (score, column) pairs of
// Qm X^T over X [Nx,K]; bf16 contiguous, K % 8 == 0, 1 <= m <= 16, m <= Nx,
// Nx < 2^31. topk_sim_plan gives the list capacity (1/4/8/16 >= m), the
// stripe count (stripes_req > 0 forces it, clamped to the index tiles) and
// the 128-row tiles per stripe. part_s / part_i: Nq * 2*stripes * cap
// elements, uninitialised. out_s / out_i: [Nq, m]. No atomics.
void topk_sim_plan(long Nq, long Nx, int m, int stripes_req, int* cap,
                   int* stripes, long* tiles_per_stripe);
void topk_sim_launch(const void* Qm, const void* X, float* part_s, int* part_i,
                     float* out_s, long* out_i, long Nq, long Nx, int K, int m,
                     int cap, int stripes, long tiles_per_stripe,
                     hipStream_t st);

}  // namespace dcr
