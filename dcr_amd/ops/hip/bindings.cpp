// PyTorch bindings for the dcr_amd HIP kernel library (MI355X / gfx950).
// Host-only TU: dispatches dtypes + shapes and calls launchers from the
// .hip TUs. Fails loudly on unsupported layouts rather than silently
// falling back (bench validity: the HIP path must be the one that runs).

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <climits>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "dcr_launchers.h"

using namespace dcr;

namespace {

DType dtype_of(const at::Tensor& t) {
  switch (t.scalar_type()) {
    case at::kFloat: return DT_F32;
    case at::kHalf: return DT_F16;
    case at::kBFloat16: return DT_BF16;
    default: TORCH_CHECK(false, "dcr_hip: unsupported dtype ", t.scalar_type());
  }
}

hipStream_t cur_stream() {
  return at::cuda::getCurrentCUDAStream().stream();
}

at::Tensor as_f32(const at::Tensor& t) {
  return t.scalar_type() == at::kFloat ? t.contiguous()
                                       : t.to(at::kFloat).contiguous();
}

// weights may stay in the activation dtype (pure-bf16 training: avoids a
// cast kernel per norm call) or be fp32 (autocast); anything else -> fp32.
at::Tensor norm_weight(const at::Tensor& w, const at::Tensor& x, bool& w_f32) {
  if (w.scalar_type() == at::kFloat) {
    w_f32 = true;
    return w.contiguous();
  }
  if (w.scalar_type() == x.scalar_type()) {
    w_f32 = false;
    return w.contiguous();
  }
  w_f32 = true;
  return w.to(at::kFloat).contiguous();
}

}  // namespace

// ---------------------------------------------------------------- GroupNorm
std::vector<at::Tensor> groupnorm_silu_fwd(at::Tensor x, at::Tensor w, at::Tensor b,
                                           int64_t groups, double eps, bool silu) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous(), "gn: x must be contiguous CUDA");
  TORCH_CHECK(x.dim() >= 2, "gn: x must be [N, C, ...]");
  const int64_t N = x.size(0), C = x.size(1);
  const int64_t HW = x.numel() / (N * C);
  TORCH_CHECK(C % groups == 0, "gn: C % groups != 0");
  bool wf32;
  auto wf = norm_weight(w, x, wf32);
  bool bf32;
  auto bf = norm_weight(b, x, bf32);
  TORCH_CHECK(wf32 == bf32);
  auto y = at::empty_like(x);
  auto mean = at::empty({N * groups}, x.options().dtype(at::kFloat));
  auto rstd = at::empty_like(mean);
  gn_fwd_launch(dtype_of(x), x.data_ptr(), wf.data_ptr(), bf.data_ptr(), wf32,
                y.data_ptr(), mean.data_ptr<float>(), rstd.data_ptr<float>(),
                (int)(N * groups), (int)groups, (int)(C / groups), (int)HW,
                (float)eps, silu, cur_stream());
  return {y, mean, rstd};
}

std::vector<at::Tensor> groupnorm_silu_bwd(at::Tensor dy, at::Tensor x, at::Tensor w,
                                           at::Tensor b, at::Tensor mean, at::Tensor rstd,
                                           int64_t groups, bool silu) {
  TORCH_CHECK(dy.is_contiguous() && x.is_contiguous());
  const int64_t N = x.size(0), C = x.size(1);
  const int64_t HW = x.numel() / (N * C);
  bool wf32;
  auto wf = norm_weight(w, x, wf32);
  bool bf32;
  auto bf = norm_weight(b, x, bf32);
  auto dx = at::empty_like(x);
  auto dwdb = at::zeros({2 * C}, x.options().dtype(at::kFloat));
  auto dw = dwdb.narrow(0, 0, C);
  auto db = dwdb.narrow(0, C, C);
  gn_bwd_launch(dtype_of(x), dy.data_ptr(), x.data_ptr(), wf.data_ptr(),
                bf.data_ptr(), wf32, mean.data_ptr<float>(), rstd.data_ptr<float>(),
                dx.data_ptr(), dw.data_ptr<float>(), db.data_ptr<float>(),
                (int)(N * groups), (int)groups, (int)(C / groups), (int)HW,
                silu, cur_stream());
  return {dx, dw.to(w.scalar_type()), db.to(b.scalar_type())};
}

// channels_last GroupNorm: x is NHWC-contiguous, passed as [N, C, H, W]
// logical sizes with channels_last memory format.
std::vector<at::Tensor> groupnorm_silu_nhwc_fwd(at::Tensor x, at::Tensor w,
                                                at::Tensor b, int64_t groups,
                                                double eps, bool silu) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 &&
              x.is_contiguous(at::MemoryFormat::ChannelsLast),
              "gn_nhwc: channels_last 4D expected");
  const int64_t N = x.size(0), C = x.size(1);
  const int64_t R = x.size(2) * x.size(3);
  TORCH_CHECK(C % groups == 0 && C % 4 == 0);
  bool wf32;
  auto wf = norm_weight(w, x, wf32);
  bool bf32;
  auto bf = norm_weight(b, x, bf32);
  TORCH_CHECK(wf32 == bf32);
  auto y = at::empty_like(x);  // preserves channels_last
  const int64_t chunks = gn_nhwc_chunks((int)N, (int)R);
  // per-chunk partial slab, plain stores -> at::empty (no fill kernel)
  auto ws = at::empty({chunks * N * groups * 2},
                      x.options().dtype(at::kFloat));
  auto mean = at::empty({N * groups}, x.options().dtype(at::kFloat));
  auto rstd = at::empty_like(mean);
  gn_nhwc_fwd_launch(dtype_of(x), x.data_ptr(), wf.data_ptr(), bf.data_ptr(),
                     wf32, y.data_ptr(), ws.data_ptr<float>(),
                     mean.data_ptr<float>(), rstd.data_ptr<float>(), (int)N,
                     (int)R, (int)C, (int)groups, (float)eps, silu, cur_stream());
  return {y, mean, rstd};
}

std::vector<at::Tensor> groupnorm_silu_nhwc_bwd(at::Tensor dy, at::Tensor x,
                                                at::Tensor w, at::Tensor b,
                                                at::Tensor mean, at::Tensor rstd,
                                                int64_t groups, bool silu) {
  TORCH_CHECK(dy.is_contiguous(at::MemoryFormat::ChannelsLast) &&
              x.is_contiguous(at::MemoryFormat::ChannelsLast));
  const int64_t N = x.size(0), C = x.size(1);
  const int64_t R = x.size(2) * x.size(3);
  bool wf32;
  auto wf = norm_weight(w, x, wf32);
  bool bf32;
  auto bf = norm_weight(b, x, bf32);
  auto dx = at::empty_like(x);
  const int64_t chunks = gn_nhwc_chunks((int)N, (int)R);
  // [chunk-partial group sums | chunk-partial dw/db | finalized groups]
  // — every slot plain-stored, so no zero-init kernel. The finalize
  // kernel writes dw|db in the weight dtype: stats, finalize, apply.
  TORCH_CHECK(wf32 == bf32);
  auto ws = at::empty(
      {chunks * N * groups * 2 + chunks * N * 2 * C + N * groups * 2},
      x.options().dtype(at::kFloat));
  auto dwdb = at::empty({2 * C}, wf.options());
  gn_nhwc_bwd_launch(dtype_of(x), dy.data_ptr(), x.data_ptr(),
                     wf.data_ptr(), bf.data_ptr(), wf32,
                     mean.data_ptr<float>(), rstd.data_ptr<float>(),
                     ws.data_ptr<float>(), dx.data_ptr(), dwdb.data_ptr(),
                     (int)N, (int)R, (int)C, (int)groups, silu, cur_stream());
  return {dx, dwdb.narrow(0, 0, C).to(w.scalar_type()),
          dwdb.narrow(0, C, C).to(b.scalar_type())};
}

// ---------------------------------------------------------------- LayerNorm
std::vector<at::Tensor> layernorm_fwd(at::Tensor x, at::Tensor w, at::Tensor b,
                                      double eps) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous());
  const int64_t Nd = x.size(-1);
  const int64_t M = x.numel() / Nd;
  bool wf32;
  auto wf = norm_weight(w, x, wf32);
  bool bf32;
  auto bf = norm_weight(b, x, bf32);
  TORCH_CHECK(wf32 == bf32);
  auto y = at::empty_like(x);
  auto mean = at::empty({M}, x.options().dtype(at::kFloat));
  auto rstd = at::empty_like(mean);
  ln_fwd_launch(dtype_of(x), x.data_ptr(), wf.data_ptr(), bf.data_ptr(), wf32,
                y.data_ptr(), mean.data_ptr<float>(), rstd.data_ptr<float>(),
                M, (int)Nd, (float)eps, cur_stream());
  return {y, mean, rstd};
}

// blocks > 0 overrides the v2 grid (scripts/bench_norms.py sweeps it)
std::vector<at::Tensor> layernorm_bwd(at::Tensor dy, at::Tensor x, at::Tensor w,
                                      at::Tensor mean, at::Tensor rstd,
                                      int64_t blocks) {
  TORCH_CHECK(dy.is_contiguous() && x.is_contiguous());
  const int64_t Nd = x.size(-1);
  const int64_t M = x.numel() / Nd;
  TORCH_CHECK(Nd <= 16384, "ln_bwd: N too large for LDS accumulator");
  bool wf32;
  auto wf = norm_weight(w, x, wf32);
  auto dx = at::empty_like(x);
  int64_t nblk = ln_bwd_v2_blocks(M, (int)Nd);
  if (nblk > 0) {
    if (blocks > 0) nblk = std::min<int64_t>(blocks, 65535);
    // main kernel + slab reduce; dw|db leave the reduce in wf's dtype
    auto slab = at::empty({nblk * 2 * Nd}, x.options().dtype(at::kFloat));
    auto dwdb_t = at::empty({2 * Nd}, wf.options());
    ln_bwd_v2_launch(dtype_of(x), dy.data_ptr(), x.data_ptr(), wf.data_ptr(),
                     wf32, mean.data_ptr<float>(), rstd.data_ptr<float>(),
                     dx.data_ptr(), slab.data_ptr<float>(), dwdb_t.data_ptr(),
                     (int)nblk, M, (int)Nd, cur_stream());
    return {dx, dwdb_t.narrow(0, 0, Nd).to(w.scalar_type()),
            dwdb_t.narrow(0, Nd, Nd).to(w.scalar_type())};
  }
  auto dwdb = at::zeros({2 * Nd}, x.options().dtype(at::kFloat));
  auto dw = dwdb.narrow(0, 0, Nd);
  auto db = dwdb.narrow(0, Nd, Nd);
  ln_bwd_launch(dtype_of(x), dy.data_ptr(), x.data_ptr(), wf.data_ptr(), wf32,
                mean.data_ptr<float>(), rstd.data_ptr<float>(), dx.data_ptr(),
                dw.data_ptr<float>(), db.data_ptr<float>(), M, (int)Nd,
                cur_stream());
  return {dx, dw.to(w.scalar_type()), db.to(w.scalar_type())};
}

// ------------------------------------------------------ bias-grad column sums
// x: [rows, C] contiguous -> [C] (fp32 accumulation, x's dtype out)
at::Tensor colsum(at::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.is_contiguous(),
              "colsum: contiguous CUDA [rows, C] expected");
  const int64_t rows = x.size(0), C = x.size(1);
  TORCH_CHECK(rows >= 1 && C >= 1 && C < (1 << 30));
  const DType dt = dtype_of(x);
  const int chunks = colsum_chunks((int)dt, 1, rows, (int)C, 128);
  auto out = at::empty({C}, x.options());
  at::Tensor slab;
  float* sp = nullptr;
  if (chunks > 1) {
    slab = at::empty({chunks * C}, x.options().dtype(at::kFloat));
    sp = slab.data_ptr<float>();
  }
  colsum_launch(dt, x.data_ptr(), sp, nullptr, out.data_ptr(), 1, rows, (int)C,
                chunks, cur_stream());
  return out;
}

// x: [N, HW, C] contiguous -> ([N, C], [C]); the [C] output is the fp32 sum
// of the unrounded per-sample sums (d_temb and dbias from one read of dy)
std::vector<at::Tensor> colsum_grouped(at::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 3 && x.is_contiguous(),
              "colsum_grouped: contiguous CUDA [N, HW, C] expected");
  const int64_t N = x.size(0), HW = x.size(1), C = x.size(2);
  TORCH_CHECK(N >= 1 && HW >= 1 && C >= 1 && C < (1 << 30));
  const DType dt = dtype_of(x);
  const int chunks = colsum_chunks((int)dt, N, HW, (int)C, 16);
  auto out_n = at::empty({N, C}, x.options());
  auto out = at::empty({C}, x.options());
  auto slab = at::empty({N * chunks * C}, x.options().dtype(at::kFloat));
  colsum_launch(dt, x.data_ptr(), slab.data_ptr<float>(), out_n.data_ptr(),
                out.data_ptr(), N, HW, (int)C, chunks, cur_stream());
  return {out_n, out};
}

// ---------------------------------------------------------------- GEGLU
at::Tensor geglu_fwd(at::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous());
  const int64_t twoN = x.size(-1);
  TORCH_CHECK(twoN % 2 == 0);
  const int64_t N = twoN / 2;
  TORCH_CHECK(N % 4 == 0, "geglu: inner dim must be divisible by 4");
  const int64_t M = x.numel() / twoN;
  auto sizes = x.sizes().vec();
  sizes.back() = N;
  auto y = at::empty(sizes, x.options());
  geglu_fwd_launch(dtype_of(x), x.data_ptr(), y.data_ptr(), M, N, cur_stream());
  return y;
}

at::Tensor geglu_bwd(at::Tensor dy, at::Tensor x) {
  TORCH_CHECK(dy.is_contiguous() && x.is_contiguous());
  const int64_t twoN = x.size(-1);
  const int64_t N = twoN / 2;
  const int64_t M = x.numel() / twoN;
  auto dx = at::empty_like(x);
  geglu_bwd_launch(dtype_of(x), dy.data_ptr(), x.data_ptr(), dx.data_ptr(), M, N,
                   cur_stream());
  return dx;
}

// ---------------------------------------------------------------- AdamW
void adamw_step(at::Tensor p, at::Tensor g, at::Tensor m, at::Tensor v,
                double lr, double beta1, double beta2, double eps, double wd,
                int64_t step) {
  TORCH_CHECK(p.is_cuda() && p.scalar_type() == at::kFloat,
              "adamw: fp32 flat params expected");
  TORCH_CHECK(p.is_contiguous() && g.is_contiguous() && m.is_contiguous() &&
              v.is_contiguous());
  adamw_launch(p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(),
               v.data_ptr<float>(), p.numel(), (float)lr, (float)beta1,
               (float)beta2, (float)eps, (float)wd, step, cur_stream());
}

void adamw_step_bf16(at::Tensor p, at::Tensor g, at::Tensor master,
                     at::Tensor m, at::Tensor v, double lr, double beta1,
                     double beta2, double eps, double wd, int64_t step) {
  TORCH_CHECK(p.is_cuda() && p.scalar_type() == at::kBFloat16);
  TORCH_CHECK(master.scalar_type() == at::kFloat);
  TORCH_CHECK(p.is_contiguous() && g.is_contiguous() && master.is_contiguous());
  adamw_bf16_launch(p.data_ptr(), g.data_ptr(), master.data_ptr<float>(),
                    m.data_ptr<float>(), v.data_ptr<float>(), p.numel(),
                    (float)lr, (float)beta1, (float)beta2, (float)eps,
                    (float)wd, step, cur_stream());
}

// ---------------------------------------------------------------- grad tail
// grad_tail.hip: one-launch gradient gather with a fused sum of squares, the
// finalize that turns it into {sumsq, norm, coef}, and the AdamW kernels
// that read coef from that record.
namespace {

void gt_check_arena(const at::Tensor& arena, int64_t ch) {
  TORCH_CHECK(arena.is_cuda() && arena.dim() == 1 && arena.is_contiguous(),
              "grad tail: the arena must be a flat contiguous GPU tensor");
  TORCH_CHECK(arena.scalar_type() == at::kBFloat16 ||
              arena.scalar_type() == at::kFloat,
              "grad tail: bf16 or fp32 arena expected");
  TORCH_CHECK(ch >= 8 && ch % 8 == 0 && ch <= (1 << 24),
              "grad tail: chunk must be a multiple of 8 elements, got ", ch);
}

// element offset of an arena view; checks that it lies inside the arena
int64_t gt_view_offset(const at::Tensor& arena, const at::Tensor& view) {
  TORCH_CHECK(view.scalar_type() == arena.scalar_type() &&
              view.device() == arena.device() &&
              view.is_non_overlapping_and_dense(),
              "grad tail: not a dense view of the arena");
  const int64_t es = arena.element_size();
  const int64_t byte_off = (const char*)view.data_ptr() - (const char*)arena.data_ptr();
  TORCH_CHECK(byte_off >= 0 && byte_off % es == 0 &&
              byte_off / es + view.numel() <= arena.numel(),
              "grad tail: view outside the arena");
  return byte_off / es;
}

// raw copy is right when both hold the same elements in the same memory
// order: same dtype, dense, equal strides on every dimension of size > 1
// (a [K,C,1,1] weight is contiguous in both memory formats and may carry
// either stride tuple)
bool gt_qualifies(const at::Tensor& g, const at::Tensor& view) {
  if (!g.defined() || g.device() != view.device() ||
      g.scalar_type() != view.scalar_type() || g.sizes() != view.sizes() ||
      !g.is_non_overlapping_and_dense())
    return false;
  for (int64_t d = 0; d < g.dim(); ++d)
    if (g.size(d) > 1 && g.stride(d) != view.stride(d)) return false;
  return reinterpret_cast<uintptr_t>(g.data_ptr()) % g.element_size() == 0;
}

// rows of {source address, destination offset, count, block prefix}: filled
// into pinned memory and sent with one non-blocking copy, so the caching
// host allocator keeps the block from reuse until the copy has run
at::Tensor gt_upload(const at::Tensor& arena, const std::vector<int64_t>& rows) {
  auto host = at::empty({(int64_t)rows.size()},
                        at::TensorOptions().dtype(at::kLong).pinned_memory(true));
  std::memcpy(host.data_ptr<int64_t>(), rows.data(), rows.size() * sizeof(int64_t));
  auto dev = at::empty({(int64_t)rows.size()}, arena.options().dtype(at::kLong));
  dev.copy_(host, /*non_blocking=*/true);
  return dev;
}

float* gt_partials(const c10::optional<at::Tensor>& partials,
                   const at::Tensor& arena, int64_t nvb) {
  if (!partials.has_value()) return nullptr;
  TORCH_CHECK(partials->is_cuda() && partials->device() == arena.device() &&
              partials->scalar_type() == at::kFloat &&
              partials->is_contiguous() && partials->numel() >= nvb,
              "grad tail: partials must hold ", nvb, " floats on the GPU");
  return partials->data_ptr<float>();
}

}  // namespace

// Copies every qualifying grads[i] into views[i] (views of `arena`) in one
// launch; with `partials` also writes each virtual block's sum of squares.
// Returns the indices that did not qualify: the caller copies those.
// add: views[i] += grads[i] (one fp32 add rounded once, as _foreach_add_)
// instead of the copy, same eligibility rule; takes no partials. The caller
// runs view.add_(g) for the indices returned.
std::vector<int64_t> grad_gather(at::Tensor arena, std::vector<at::Tensor> views,
                                 std::vector<at::Tensor> grads,
                                 c10::optional<at::Tensor> partials,
                                 int64_t ch, int64_t grid, bool add) {
  gt_check_arena(arena, ch);
  TORCH_CHECK(views.size() == grads.size(), "grad_gather: list lengths differ");
  TORCH_CHECK(!add || !partials.has_value(),
              "grad_gather: add mode takes no sum of squares");
  std::vector<int64_t> rows, rejected;
  rows.reserve(4 * views.size());
  int64_t nvb = 0;
  for (size_t i = 0; i < views.size(); ++i) {
    if (!gt_qualifies(grads[i], views[i])) {
      rejected.push_back((int64_t)i);
      continue;
    }
    const int64_t n = views[i].numel();
    if (n == 0) continue;
    const int64_t off = gt_view_offset(arena, views[i]);
    rows.push_back((int64_t)reinterpret_cast<uintptr_t>(grads[i].data_ptr()));
    rows.push_back(off);
    rows.push_back(n);
    rows.push_back(nvb);
    nvb += (n + ch - 1) / ch;
  }
  if (rows.empty()) return rejected;
  float* pp = gt_partials(partials, arena, nvb);
  auto table = gt_upload(arena, rows);
  grad_gather_launch(dtype_of(arena), (const long*)table.data_ptr<int64_t>(),
                     (int)(rows.size() / 4), nvb, arena.data_ptr(), pp, (int)ch,
                     grad_gather_grid(nvb, (int)grid), /*store=*/true, add,
                     cur_stream());
  return rejected;
}

// Standalone sum of squares of the arena slices `views`, over the same
// virtual-block partition grad_gather uses for the same list: same bits.
// Returns the number of partials written.
int64_t grad_sumsq(at::Tensor arena, std::vector<at::Tensor> views,
                   at::Tensor partials, int64_t ch, int64_t grid) {
  gt_check_arena(arena, ch);
  std::vector<int64_t> rows;
  rows.reserve(4 * views.size());
  int64_t nvb = 0;
  for (const auto& v : views) {
    const int64_t n = v.numel();
    if (n == 0) continue;
    const int64_t off = gt_view_offset(arena, v);
    rows.push_back((int64_t)reinterpret_cast<uintptr_t>(
        (const char*)arena.data_ptr() + off * arena.element_size()));
    rows.push_back(off);
    rows.push_back(n);
    rows.push_back(nvb);
    nvb += (n + ch - 1) / ch;
  }
  float* pp = gt_partials(partials, arena, nvb);
  if (rows.empty()) return 0;
  auto table = gt_upload(arena, rows);
  grad_gather_launch(dtype_of(arena), (const long*)table.data_ptr<int64_t>(),
                     (int)(rows.size() / 4), nvb, arena.data_ptr(), pp, (int)ch,
                     grad_gather_grid(nvb, (int)grid), /*store=*/false,
                     /*add=*/false, cur_stream());
  return nvb;
}

// partials[0:nvb] -> rec = {sumsq, norm, coef} (float[3] on the GPU)
void sumsq_finalize(at::Tensor partials, int64_t nvb, double max_norm,
                    at::Tensor rec) {
  TORCH_CHECK(partials.is_cuda() && partials.scalar_type() == at::kFloat &&
              partials.is_contiguous() && nvb >= 0 && partials.numel() >= nvb,
              "sumsq_finalize: partials must hold nvb floats on the GPU");
  TORCH_CHECK(rec.is_cuda() && rec.scalar_type() == at::kFloat &&
              rec.is_contiguous() && rec.numel() == 3,
              "sumsq_finalize: rec must be float[3] on the GPU");
  sumsq_finalize_launch(partials.data_ptr<float>(), nvb, (float)max_norm,
                        rec.data_ptr<float>(), cur_stream());
}

static void gt_check_rec(const at::Tensor& rec, const at::Tensor& p) {
  TORCH_CHECK(rec.is_cuda() && rec.device() == p.device() &&
              rec.scalar_type() == at::kFloat && rec.is_contiguous() &&
              rec.numel() == 3, "adamw_clip: rec must be float[3] on the GPU");
}

void adamw_step_clip(at::Tensor p, at::Tensor g, at::Tensor m, at::Tensor v,
                     double lr, double beta1, double beta2, double eps,
                     double wd, int64_t step, at::Tensor rec) {
  TORCH_CHECK(p.is_cuda() && p.scalar_type() == at::kFloat &&
              g.scalar_type() == at::kFloat && g.numel() == p.numel(),
              "adamw_clip: fp32 flat params and grads expected");
  TORCH_CHECK(p.is_contiguous() && g.is_contiguous() && m.is_contiguous() &&
              v.is_contiguous());
  gt_check_rec(rec, p);
  adamw_clip_launch(p.data_ptr<float>(), g.data_ptr<float>(),
                    m.data_ptr<float>(), v.data_ptr<float>(), p.numel(),
                    (float)lr, (float)beta1, (float)beta2, (float)eps,
                    (float)wd, step, rec.data_ptr<float>(), cur_stream());
}

void adamw_step_bf16_clip(at::Tensor p, at::Tensor g, at::Tensor master,
                          at::Tensor m, at::Tensor v, double lr, double beta1,
                          double beta2, double eps, double wd, int64_t step,
                          at::Tensor rec) {
  TORCH_CHECK(p.is_cuda() && p.scalar_type() == at::kBFloat16 &&
              g.scalar_type() == at::kBFloat16 && g.numel() == p.numel());
  TORCH_CHECK(master.scalar_type() == at::kFloat);
  TORCH_CHECK(p.is_contiguous() && g.is_contiguous() && master.is_contiguous());
  gt_check_rec(rec, p);
  adamw_bf16_clip_launch(p.data_ptr(), g.data_ptr(), master.data_ptr<float>(),
                         m.data_ptr<float>(), v.data_ptr<float>(), p.numel(),
                         (float)lr, (float)beta1, (float)beta2, (float)eps,
                         (float)wd, step, rec.data_ptr<float>(), cur_stream());
}

// device-state AdamW (round-2 draft): hyper = float[8] cuda tensor
// {lr, b1^t, b2^t, inv_bc1, inv_bc2, clip_coef, gnorm_sq, step};
// init {lr, 1, 1, 1, 1, 1, 0, 0}. The 3-kernel sequence is stream-ordered
// and hipGraph-capturable; update hyper[0] (lr) from the host between
// replays. Gated validation: DCR_DEV_ADAMW=1 tests.
void adamw_step_dev(at::Tensor p, at::Tensor g, c10::optional<at::Tensor> master,
                    at::Tensor m, at::Tensor v, at::Tensor hyper, double beta1,
                    double beta2, double eps, double wd, double max_norm) {
  TORCH_CHECK(hyper.is_cuda() && hyper.scalar_type() == at::kFloat &&
              hyper.numel() == 8 && hyper.is_contiguous());
  TORCH_CHECK(p.is_contiguous() && g.is_contiguous());
  const bool bf16 = p.scalar_type() == at::kBFloat16;
  float* mp = nullptr;
  if (bf16) {
    TORCH_CHECK(master.has_value() && master->scalar_type() == at::kFloat,
                "bf16 device-state adamw needs the fp32 master");
    mp = master->data_ptr<float>();
  } else {
    TORCH_CHECK(p.scalar_type() == at::kFloat);
  }
  adamw_dev_launch(bf16 ? 1 : 0, p.data_ptr(), g.data_ptr(), mp,
                   m.data_ptr<float>(), v.data_ptr<float>(), p.numel(),
                   (float)beta1, (float)beta2, (float)eps, (float)wd,
                   (float)max_norm, hyper.data_ptr<float>(), cur_stream());
}

// AdamW with block-scaled FP8 state (adamw8.hip; format in ops/hip/README.md).
// State: codes uint8[nblocks*256] + absmax float[nblocks] per moment,
// nblocks = ceil(numel/256).
static void adamw8_check_state(const at::Tensor& p, const at::Tensor& mq,
                               const at::Tensor& mabs, const at::Tensor& rq,
                               const at::Tensor& rabs) {
  const int64_t n = p.numel();
  const int64_t nblocks = (n + 255) / 256;
  TORCH_CHECK(mq.is_cuda() && mabs.is_cuda() && rq.is_cuda() && rabs.is_cuda(),
              "adamw8: state must be on the GPU");
  TORCH_CHECK(mq.scalar_type() == at::kByte && rq.scalar_type() == at::kByte,
              "adamw8: codes must be uint8");
  TORCH_CHECK(mabs.scalar_type() == at::kFloat &&
              rabs.scalar_type() == at::kFloat, "adamw8: absmax must be fp32");
  TORCH_CHECK(mq.is_contiguous() && mabs.is_contiguous() &&
              rq.is_contiguous() && rabs.is_contiguous(),
              "adamw8: state must be contiguous");
  TORCH_CHECK(mq.numel() == nblocks * 256 && rq.numel() == nblocks * 256,
              "adamw8: codes must hold nblocks*256 = ", nblocks * 256,
              " bytes for numel ", n);
  TORCH_CHECK(mabs.numel() == nblocks && rabs.numel() == nblocks,
              "adamw8: absmax must hold nblocks = ", nblocks, " floats");
}

void adamw8_step(at::Tensor p, at::Tensor g, at::Tensor mq, at::Tensor mabs,
                 at::Tensor rq, at::Tensor rabs, double lr, double beta1,
                 double beta2, double eps, double wd, int64_t step) {
  TORCH_CHECK(p.is_cuda() && p.scalar_type() == at::kFloat,
              "adamw8: fp32 flat params expected");
  TORCH_CHECK(g.is_cuda() && g.scalar_type() == at::kFloat &&
              g.numel() == p.numel(), "adamw8: fp32 grads of the same numel");
  TORCH_CHECK(p.is_contiguous() && g.is_contiguous(),
              "adamw8: arenas must be contiguous");
  adamw8_check_state(p, mq, mabs, rq, rabs);
  adamw8_launch(0, p.data_ptr(), g.data_ptr(), nullptr,
                mq.data_ptr<uint8_t>(), mabs.data_ptr<float>(),
                rq.data_ptr<uint8_t>(), rabs.data_ptr<float>(), p.numel(), lr,
                beta1, beta2, eps, wd, step, cur_stream());
}

void adamw8_step_bf16(at::Tensor p, at::Tensor g, at::Tensor master,
                      at::Tensor mq, at::Tensor mabs, at::Tensor rq,
                      at::Tensor rabs, double lr, double beta1, double beta2,
                      double eps, double wd, int64_t step) {
  TORCH_CHECK(p.is_cuda() && p.scalar_type() == at::kBFloat16,
              "adamw8_bf16: bf16 flat params expected");
  TORCH_CHECK(g.is_cuda() && g.scalar_type() == at::kBFloat16 &&
              g.numel() == p.numel(), "adamw8_bf16: bf16 grads of the same numel");
  TORCH_CHECK(master.is_cuda() && master.scalar_type() == at::kFloat &&
              master.numel() == p.numel(),
              "adamw8_bf16: fp32 master of the same numel");
  TORCH_CHECK(p.is_contiguous() && g.is_contiguous() && master.is_contiguous(),
              "adamw8_bf16: arenas must be contiguous");
  adamw8_check_state(p, mq, mabs, rq, rabs);
  adamw8_launch(1, p.data_ptr(), g.data_ptr(), master.data_ptr<float>(),
                mq.data_ptr<uint8_t>(), mabs.data_ptr<float>(),
                rq.data_ptr<uint8_t>(), rabs.data_ptr<float>(), p.numel(), lr,
                beta1, beta2, eps, wd, step, cur_stream());
}

// clip-aware: rec = {sumsq, norm, coef} from sumsq_finalize; when coef != 1
// the clipped gradient is stored back into g
void adamw8_step_clip(at::Tensor p, at::Tensor g, at::Tensor mq,
                      at::Tensor mabs, at::Tensor rq, at::Tensor rabs,
                      double lr, double beta1, double beta2, double eps,
                      double wd, int64_t step, at::Tensor rec) {
  TORCH_CHECK(p.is_cuda() && p.scalar_type() == at::kFloat,
              "adamw8_clip: fp32 flat params expected");
  TORCH_CHECK(g.is_cuda() && g.scalar_type() == at::kFloat &&
              g.numel() == p.numel(), "adamw8_clip: fp32 grads of the same numel");
  TORCH_CHECK(p.is_contiguous() && g.is_contiguous(),
              "adamw8_clip: arenas must be contiguous");
  adamw8_check_state(p, mq, mabs, rq, rabs);
  gt_check_rec(rec, p);
  adamw8_clip_launch(0, p.data_ptr(), g.data_ptr(), nullptr,
                     mq.data_ptr<uint8_t>(), mabs.data_ptr<float>(),
                     rq.data_ptr<uint8_t>(), rabs.data_ptr<float>(), p.numel(),
                     lr, beta1, beta2, eps, wd, step, rec.data_ptr<float>(),
                     cur_stream());
}

void adamw8_step_bf16_clip(at::Tensor p, at::Tensor g, at::Tensor master,
                           at::Tensor mq, at::Tensor mabs, at::Tensor rq,
                           at::Tensor rabs, double lr, double beta1,
                           double beta2, double eps, double wd, int64_t step,
                           at::Tensor rec) {
  TORCH_CHECK(p.is_cuda() && p.scalar_type() == at::kBFloat16,
              "adamw8_bf16_clip: bf16 flat params expected");
  TORCH_CHECK(g.is_cuda() && g.scalar_type() == at::kBFloat16 &&
              g.numel() == p.numel(),
              "adamw8_bf16_clip: bf16 grads of the same numel");
  TORCH_CHECK(master.is_cuda() && master.scalar_type() == at::kFloat &&
              master.numel() == p.numel(),
              "adamw8_bf16_clip: fp32 master of the same numel");
  TORCH_CHECK(p.is_contiguous() && g.is_contiguous() && master.is_contiguous(),
              "adamw8_bf16_clip: arenas must be contiguous");
  adamw8_check_state(p, mq, mabs, rq, rabs);
  gt_check_rec(rec, p);
  adamw8_clip_launch(1, p.data_ptr(), g.data_ptr(), master.data_ptr<float>(),
                     mq.data_ptr<uint8_t>(), mabs.data_ptr<float>(),
                     rq.data_ptr<uint8_t>(), rabs.data_ptr<float>(), p.numel(),
                     lr, beta1, beta2, eps, wd, step, rec.data_ptr<float>(),
                     cur_stream());
}

// ------------------------------------------------------------- scheduler math
static at::Tensor sched_common(int mode, at::Tensor a, at::Tensor b, at::Tensor ac,
                               at::Tensor t) {
  TORCH_CHECK(a.is_cuda() && a.is_contiguous() && b.is_contiguous());
  TORCH_CHECK(ac.scalar_type() == at::kFloat && t.scalar_type() == at::kLong);
  const int64_t B = t.size(0);
  const int64_t per = a.numel() / B;
  TORCH_CHECK(per % 4 == 0, "sched: per-sample numel must be divisible by 4");
  auto out = at::empty_like(a);
  sched_launch(dtype_of(a), mode, a.data_ptr(), b.data_ptr(), ac.data_ptr<float>(),
               t.data_ptr<int64_t>(), out.data_ptr(), per, a.numel(), cur_stream());
  return out;
}

at::Tensor add_noise(at::Tensor x0, at::Tensor noise, at::Tensor ac, at::Tensor t) {
  return sched_common(0, x0, noise, ac, t);
}

at::Tensor get_velocity(at::Tensor x0, at::Tensor noise, at::Tensor ac, at::Tensor t) {
  return sched_common(1, x0, noise, ac, t);
}

// elementwise over any DENSE layout (NCHW or channels_last) as long as
// every operand shares the same strides — the kernel walks raw memory.
static bool same_dense(const at::Tensor& a, const at::Tensor& b) {
  return a.is_non_overlapping_and_dense() && b.is_non_overlapping_and_dense() &&
         a.strides() == b.strides();
}

at::Tensor lincomb(at::Tensor X, at::Tensor Y,
                   c10::optional<at::Tensor> Z, double a, double b, double c) {
  TORCH_CHECK(X.is_cuda());
  TORCH_CHECK(same_dense(X, Y), "lincomb: X/Y layout mismatch");
  TORCH_CHECK(X.numel() % 4 == 0);
  auto out = at::empty_like(X);  // preserves layout
  const void* zp = nullptr;
  at::Tensor Zc;
  if (Z.has_value()) {
    TORCH_CHECK(same_dense(X, *Z), "lincomb: X/Z layout mismatch");
    Zc = *Z;
    zp = Zc.data_ptr();
  }
  lincomb_launch(dtype_of(X), X.data_ptr(), Y.data_ptr(), zp, out.data_ptr(),
                 (float)a, (float)b, (float)c, X.numel(), cur_stream());
  return out;
}

at::Tensor cfg_combine(at::Tensor eu, at::Tensor et, double scale) {
  TORCH_CHECK(eu.is_cuda());
  TORCH_CHECK(same_dense(eu, et), "cfg: layout mismatch");
  TORCH_CHECK(eu.numel() % 4 == 0);
  auto out = at::empty_like(eu);
  cfg_launch(dtype_of(eu), eu.data_ptr(), et.data_ptr(), out.data_ptr(),
             (float)scale, eu.numel(), cur_stream());
  return out;
}

// ---------------------------------------------------------------- attention
// q/k/v: [B, L, H, 64] (transpose-free BLHD layout; pass 3D [BH, L, 64]
// for the packed per-head layout — treated as B'=BH, H=1).
static void attn_dims(const at::Tensor& q, const at::Tensor& k,
                      int64_t& B, int64_t& H, int64_t& Lq, int64_t& Lk) {
  TORCH_CHECK(q.size(-1) == 64 && k.size(-1) == 64, "attn: head_dim 64 only");
  if (q.dim() == 4) {
    B = q.size(0); Lq = q.size(1); H = q.size(2); Lk = k.size(1);
    TORCH_CHECK(k.dim() == 4 && k.size(2) == H, "attn: head mismatch");
  } else {
    TORCH_CHECK(q.dim() == 3);
    B = q.size(0); Lq = q.size(1); H = 1; Lk = k.size(1);
  }
}

std::vector<at::Tensor> attn_fwd(at::Tensor q, at::Tensor k, at::Tensor v,
                                 double scale, bool causal) {
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == at::kBFloat16,
              "attn: bf16 CUDA only");
  TORCH_CHECK(q.is_contiguous() && k.is_contiguous() && v.is_contiguous());
  int64_t B, H, Lq, Lk;
  attn_dims(q, k, B, H, Lq, Lk);
  auto o = at::empty_like(q);
  auto lse = at::empty({B * H, Lq}, q.options().dtype(at::kFloat));
  attn_fwd_launch(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                  lse.data_ptr<float>(), (int)(B * H), (int)Lq, (int)Lk,
                  (int)H, (float)scale, causal, cur_stream());
  return {o, lse};
}

// generalized head-dim kernels (SD-1.x 40/80/160). q/k/v: [B, L, H, D]
// or packed [BH, L, D].
static void attn_gen_dims(const at::Tensor& q, const at::Tensor& k,
                          const at::Tensor& v, int64_t& B, int64_t& H,
                          int64_t& Lq, int64_t& Lk, int64_t& D) {
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == at::kBFloat16,
              "attn_gen: bf16 CUDA only");
  TORCH_CHECK(q.is_contiguous() && k.is_contiguous() && v.is_contiguous());
  D = q.size(-1);
  TORCH_CHECK(D == 40 || D == 80 || D == 160,
              "attn_gen: head_dim 40/80/160 only (64 has the main kernel)");
  if (q.dim() == 4) {
    B = q.size(0); Lq = q.size(1); H = q.size(2); Lk = k.size(1);
    TORCH_CHECK(k.dim() == 4 && k.size(2) == H && k.size(-1) == D);
  } else {
    TORCH_CHECK(q.dim() == 3);
    B = q.size(0); Lq = q.size(1); H = 1; Lk = k.size(1);
  }
}

static at::Tensor attn_fwd_gen_impl(const at::Tensor& q, const at::Tensor& k,
                                    const at::Tensor& v, double scale,
                                    bool causal, at::Tensor* lse) {
  int64_t B, H, Lq, Lk, D;
  attn_gen_dims(q, k, v, B, H, Lq, Lk, D);
  auto o = at::empty_like(q);
  float* lse_p = nullptr;
  if (lse != nullptr) {
    *lse = at::empty({B * H, Lq}, q.options().dtype(at::kFloat));
    lse_p = lse->data_ptr<float>();
  }
  attn_fwd_gen_launch(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                      lse_p, (int)(B * H), (int)Lq, (int)Lk, (int)H, (int)D,
                      (float)scale, causal, cur_stream());
  return o;
}

// forward without LSE (sampling under no_grad)
at::Tensor attn_fwd_gen(at::Tensor q, at::Tensor k, at::Tensor v,
                        double scale, bool causal) {
  return attn_fwd_gen_impl(q, k, v, scale, causal, nullptr);
}

// training forward: same kernel, also writes lse [B*H, Lq] fp32
std::vector<at::Tensor> attn_fwd_gen_lse(at::Tensor q, at::Tensor k,
                                         at::Tensor v, double scale,
                                         bool causal) {
  at::Tensor lse;
  auto o = attn_fwd_gen_impl(q, k, v, scale, causal, &lse);
  return {o, lse};
}

// D=512 forward (VAE mid-block's single head). q/k/v: [B, L, H, 512] or
// packed [BH, L, 512]. Everything is checked here, before any launch.
static void attn_d512_dims(const at::Tensor& q, const at::Tensor& k,
                           const at::Tensor& v, int64_t& B, int64_t& H,
                           int64_t& Lq, int64_t& Lk) {
  TORCH_CHECK(q.is_cuda() && k.is_cuda() && v.is_cuda() &&
              q.scalar_type() == at::kBFloat16 &&
              k.scalar_type() == at::kBFloat16 &&
              v.scalar_type() == at::kBFloat16,
              "attn_fwd_d512: bf16 CUDA tensors only");
  TORCH_CHECK(q.get_device() == k.get_device() &&
              q.get_device() == v.get_device(),
              "attn_fwd_d512: q/k/v on different devices");
  TORCH_CHECK(q.is_contiguous() && k.is_contiguous() && v.is_contiguous(),
              "attn_fwd_d512: q/k/v must be contiguous");
  TORCH_CHECK(q.dim() == 3 || q.dim() == 4,
              "attn_fwd_d512: [B,L,H,512] or [BH,L,512]");
  TORCH_CHECK(k.dim() == q.dim(), "attn_fwd_d512: q/k rank mismatch");
  TORCH_CHECK(q.size(-1) == 512 && k.size(-1) == 512,
              "attn_fwd_d512: head_dim 512 only");
  TORCH_CHECK(k.sizes() == v.sizes(), "attn_fwd_d512: k/v shape mismatch");
  TORCH_CHECK(k.size(0) == q.size(0), "attn_fwd_d512: q/k batch mismatch");
  B = q.size(0); Lq = q.size(1); Lk = k.size(1);
  H = 1;
  if (q.dim() == 4) {
    H = q.size(2);
    TORCH_CHECK(k.size(2) == H, "attn_fwd_d512: q/k head count mismatch");
  }
  TORCH_CHECK(Lk > 0 || q.numel() == 0, "attn_fwd_d512: no keys");
  TORCH_CHECK(Lq <= INT_MAX - 64 && Lk <= INT_MAX - 64 && H <= INT_MAX &&
              B * H <= 65535,
              "attn_fwd_d512: grid out of range (B*H <= 65535)");
}

at::Tensor attn_fwd_d512(at::Tensor q, at::Tensor k, at::Tensor v,
                         double scale) {
  int64_t B, H, Lq, Lk;
  attn_d512_dims(q, k, v, B, H, Lq, Lk);
  auto o = at::empty_like(q);
  if (q.numel() == 0) return o;
  attn_fwd_d512_launch(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                       (int)(B * H), (int)Lq, (int)Lk, (int)H, (float)scale,
                       cur_stream());
  return o;
}

std::vector<at::Tensor> attn_bwd_gen(at::Tensor q, at::Tensor k, at::Tensor v,
                                     at::Tensor o, at::Tensor dO,
                                     at::Tensor lse, double scale,
                                     bool causal) {
  int64_t B, H, Lq, Lk, D;
  attn_gen_dims(q, k, v, B, H, Lq, Lk, D);
  TORCH_CHECK(k.sizes() == v.sizes(), "attn_bwd_gen: k/v shape mismatch");
  TORCH_CHECK(o.sizes() == q.sizes() && dO.sizes() == q.sizes(),
              "attn_bwd_gen: o/dO must have q's shape");
  TORCH_CHECK(o.is_cuda() && dO.is_cuda() && lse.is_cuda() &&
              o.scalar_type() == at::kBFloat16 &&
              dO.scalar_type() == at::kBFloat16 &&
              o.is_contiguous() && dO.is_contiguous(),
              "attn_bwd_gen: o/dO must be contiguous bf16 CUDA tensors");
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.is_contiguous() &&
              lse.dim() == 2 && lse.size(0) == B * H && lse.size(1) == Lq,
              "attn_bwd_gen: lse must be contiguous fp32 [B*H, Lq]");
  auto dQ = at::empty_like(q);
  auto dK = at::empty_like(k);
  auto dV = at::empty_like(v);
  auto delta = at::empty({B * H, Lq}, q.options().dtype(at::kFloat));
  attn_bwd_gen_launch(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                      dO.data_ptr(), lse.data_ptr<float>(),
                      delta.data_ptr<float>(), dQ.data_ptr(), dK.data_ptr(),
                      dV.data_ptr(), (int)(B * H), (int)Lq, (int)Lk, (int)H,
                      (int)D, (float)scale, causal, cur_stream());
  return {dQ, dK, dV};
}

// round-2 draft: T14 async K/V staging + one barrier per tile + setprio
// (DCR_ATTN_V3=1 gates its tests and dispatch)
std::vector<at::Tensor> attn_fwd_v4(at::Tensor q, at::Tensor k, at::Tensor v,
                                    double scale, bool causal) {
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == at::kBFloat16,
              "attn: bf16 CUDA only");
  TORCH_CHECK(q.is_contiguous() && k.is_contiguous() && v.is_contiguous());
  int64_t B, H, Lq, Lk;
  attn_dims(q, k, B, H, Lq, Lk);
  auto o = at::empty_like(q);
  auto lse = at::empty({B * H, Lq}, q.options().dtype(at::kFloat));
  attn_fwd_v4_launch(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                     lse.data_ptr<float>(), (int)(B * H), (int)Lq, (int)Lk,
                     (int)H, (float)scale, causal, cur_stream());
  return {o, lse};
}

std::vector<at::Tensor> attn_fwd_v3(at::Tensor q, at::Tensor k, at::Tensor v,
                                    double scale, bool causal) {
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == at::kBFloat16,
              "attn: bf16 CUDA only");
  TORCH_CHECK(q.is_contiguous() && k.is_contiguous() && v.is_contiguous());
  int64_t B, H, Lq, Lk;
  attn_dims(q, k, B, H, Lq, Lk);
  auto o = at::empty_like(q);
  auto lse = at::empty({B * H, Lq}, q.options().dtype(at::kFloat));
  attn_fwd_v3_launch(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                     lse.data_ptr<float>(), (int)(B * H), (int)Lq, (int)Lk,
                     (int)H, (float)scale, causal, cur_stream());
  return {o, lse};
}

std::vector<at::Tensor> attn_fwd_v2(at::Tensor q, at::Tensor k, at::Tensor v,
                                    double scale, bool causal) {
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == at::kBFloat16,
              "attn: bf16 CUDA only");
  TORCH_CHECK(q.is_contiguous() && k.is_contiguous() && v.is_contiguous());
  int64_t B, H, Lq, Lk;
  attn_dims(q, k, B, H, Lq, Lk);
  auto o = at::empty_like(q);
  auto lse = at::empty({B * H, Lq}, q.options().dtype(at::kFloat));
  attn_fwd_v2_launch(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                     lse.data_ptr<float>(), (int)(B * H), (int)Lq, (int)Lk,
                     (int)H, (float)scale, causal, cur_stream());
  return {o, lse};
}

std::vector<at::Tensor> attn_bwd(at::Tensor q, at::Tensor k, at::Tensor v,
                                 at::Tensor o, at::Tensor dO, at::Tensor lse,
                                 double scale, bool causal) {
  int64_t B, H, Lq, Lk;
  attn_dims(q, k, B, H, Lq, Lk);
  auto dQ = at::empty_like(q);
  auto dK = at::empty_like(k);
  auto dV = at::empty_like(v);
  auto delta = at::empty({B * H, Lq}, q.options().dtype(at::kFloat));
  attn_bwd_launch(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                  dO.contiguous().data_ptr(), lse.data_ptr<float>(),
                  delta.data_ptr<float>(), dQ.data_ptr(), dK.data_ptr(),
                  dV.data_ptr(), (int)(B * H), (int)Lq, (int)Lk, (int)H,
                  (float)scale, causal, cur_stream());
  return {dQ, dK, dV};
}

// backward v4 draft (DCR_ATTN_BWD_V4): swapped-operand schedule
std::vector<at::Tensor> attn_bwd_v4(at::Tensor q, at::Tensor k, at::Tensor v,
                                 at::Tensor o, at::Tensor dO, at::Tensor lse,
                                 double scale, bool causal) {
  int64_t B, H, Lq, Lk;
  attn_dims(q, k, B, H, Lq, Lk);
  auto dQ = at::empty_like(q);
  auto dK = at::empty_like(k);
  auto dV = at::empty_like(v);
  auto delta = at::empty({B * H, Lq}, q.options().dtype(at::kFloat));
  attn_bwd_v4_launch(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                  dO.contiguous().data_ptr(), lse.data_ptr<float>(),
                  delta.data_ptr<float>(), dQ.data_ptr(), dK.data_ptr(),
                  dV.data_ptr(), (int)(B * H), (int)Lq, (int)Lk, (int)H,
                  (float)scale, causal, cur_stream());
  return {dQ, dK, dV};
}


at::Tensor mfma_probe(at::Tensor A, at::Tensor B) {
  TORCH_CHECK(A.is_cuda() && A.scalar_type() == at::kBFloat16);
  TORCH_CHECK(A.sizes() == at::IntArrayRef({16, 32}) &&
              B.sizes() == at::IntArrayRef({32, 16}));
  auto C = at::zeros({16, 16}, A.options().dtype(at::kFloat));
  mfma_probe_launch(A.contiguous().data_ptr(), B.contiguous().data_ptr(),
                    C.data_ptr<float>(), cur_stream());
  return C;
}

// ---------------------------------------------------------------- conv
// The conv kernels read the bias as bf16 or fp32 and widen it in the
// epilogue, so the parameter goes in as it is: no cast kernel per call.
// `keep` holds the tensor the returned pointer belongs to.
static const void* conv_bias_ptr(const c10::optional<at::Tensor>& bias,
                                 at::Tensor& keep, bool& is_bf16) {
  is_bf16 = false;
  if (!bias.has_value()) return nullptr;
  if (bias->scalar_type() == at::kBFloat16) {
    is_bf16 = true;
    keep = bias->contiguous();
  } else {
    keep = as_f32(*bias);
  }
  return keep.data_ptr();
}

at::Tensor conv2d_nhwc_fwd(at::Tensor x, at::Tensor w,
                           c10::optional<at::Tensor> bias, int64_t stride,
                           int64_t pad) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16);
  TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast) &&
              w.is_contiguous(at::MemoryFormat::ChannelsLast),
              "conv_nhwc: channels_last only");
  const int64_t Nb = x.size(0), C = x.size(1), Hin = x.size(2), Win = x.size(3);
  const int64_t K = w.size(0), R = w.size(2), S = w.size(3);
  TORCH_CHECK(w.size(1) == C && C % 32 == 0 && K % 64 == 0);
  TORCH_CHECK((R == 3 && S == 3) || (R == 1 && S == 1));
  const int64_t P = (Hin + 2 * pad - R) / stride + 1;
  const int64_t Q = (Win + 2 * pad - S) / stride + 1;
  auto y = at::empty({Nb, K, P, Q},
                     x.options().memory_format(at::MemoryFormat::ChannelsLast));
  at::Tensor bf;
  bool b_bf16 = false;
  const void* bp = conv_bias_ptr(bias, bf, b_bf16);
  conv_nhwc_fwd_launch(x.data_ptr(), w.data_ptr(), bp, b_bf16, y.data_ptr(), (int)Nb,
                       (int)Hin, (int)Win, (int)C, (int)K, (int)P, (int)Q,
                       (int)R, (int)S, (int)stride, (int)pad, cur_stream());
  return y;
}

static at::Tensor conv2d_nhwc_fwd_v2_impl(at::Tensor x, at::Tensor w,
                                          c10::optional<at::Tensor> bias,
                                          int64_t stride, int64_t pad,
                                          c10::optional<at::Tensor> res,
                                          c10::optional<at::Tensor> temb) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16);
  TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast) &&
              w.is_contiguous(at::MemoryFormat::ChannelsLast));
  const int64_t Nb = x.size(0), C = x.size(1), Hin = x.size(2), Win = x.size(3);
  const int64_t K = w.size(0), R = w.size(2), S = w.size(3);
  TORCH_CHECK(w.size(1) == C && C % 32 == 0 && K % 64 == 0);
  TORCH_CHECK((R == 3 && S == 3) || (R == 1 && S == 1));
  const int64_t P = (Hin + 2 * pad - R) / stride + 1;
  const int64_t Q = (Win + 2 * pad - S) / stride + 1;
  auto y = at::empty({Nb, K, P, Q},
                     x.options().memory_format(at::MemoryFormat::ChannelsLast));
  at::Tensor bf;
  bool b_bf16 = false;
  const void* bp = conv_bias_ptr(bias, bf, b_bf16);
  // split-K when the (pixels/128) x (K/128) grid starves the 256 CUs
  const int64_t NPQ = Nb * P * Q;
  int64_t blocks = ((NPQ + 127) / 128) * ((K + 127) / 128);
  int64_t nsteps = C * R * S / ((C % 64 == 0) ? 64 : 32);
  int splitz = 1;
  if (blocks < 384) {
    splitz = (int)std::min<int64_t>({(384 + blocks - 1) / blocks, nsteps, 16});
    if (splitz < 1) splitz = 1;
  }
  at::Tensor ws;
  float* wsp = nullptr;
  if (splitz > 1) {
    ws = at::zeros({NPQ * K}, x.options().dtype(at::kFloat));
    wsp = ws.data_ptr<float>();
  }
  const void* rp = nullptr;
  const void* tp = nullptr;
  if (res.has_value()) {
    TORCH_CHECK(res->scalar_type() == at::kBFloat16 &&
                res->is_contiguous(at::MemoryFormat::ChannelsLast) &&
                res->sizes() == y.sizes(), "conv res: NHWC bf16 same shape");
    rp = res->data_ptr();
  }
  if (temb.has_value()) {
    TORCH_CHECK(temb->scalar_type() == at::kBFloat16 &&
                temb->is_contiguous() && temb->dim() == 2 &&
                temb->size(0) == Nb && temb->size(1) == K,
                "conv temb: contiguous bf16 [N, K]");
    tp = temb->data_ptr();
  }
  conv_nhwc_fwd_v2_launch(x.data_ptr(), w.data_ptr(), bp, b_bf16, y.data_ptr(), wsp,
         splitz, rp, tp, (int)Nb, (int)Hin, (int)Win, (int)C, (int)K,
         (int)P, (int)Q, (int)R, (int)S, (int)stride,
         (int)pad, cur_stream());
  return y;
}

at::Tensor conv2d_nhwc_fwd_v2(at::Tensor x, at::Tensor w,
                              c10::optional<at::Tensor> bias, int64_t stride,
                              int64_t pad,
                              c10::optional<at::Tensor> res = c10::nullopt,
                              c10::optional<at::Tensor> temb = c10::nullopt) {
  return conv2d_nhwc_fwd_v2_impl(x, w, bias, stride, pad, res, temb);
}

// conv backward drafts (round-2; validated before any dispatch)
std::vector<at::Tensor> conv2d_nhwc_bwd(at::Tensor dy, at::Tensor x,
                                        at::Tensor w, int64_t stride,
                                        int64_t pad) {
  TORCH_CHECK(dy.is_cuda() && dy.scalar_type() == at::kBFloat16);
  TORCH_CHECK(dy.is_contiguous(at::MemoryFormat::ChannelsLast) &&
              x.is_contiguous(at::MemoryFormat::ChannelsLast) &&
              w.is_contiguous(at::MemoryFormat::ChannelsLast));
  const int64_t Nb = x.size(0), C = x.size(1), Hin = x.size(2), Win = x.size(3);
  const int64_t K = w.size(0), R = w.size(2), S = w.size(3);
  TORCH_CHECK(C % 64 == 0 && K % 64 == 0);
  const int64_t P = dy.size(2), Q = dy.size(3);
  const int64_t NPQ = Nb * P * Q;
  int splits = (int)std::min<int64_t>(std::max<int64_t>(
      384 / std::max<int64_t>((K / 64) * (R * S * C / 32), 1), 1), 16);
  auto dw_ws = at::zeros({K * R * S * C}, x.options().dtype(at::kFloat));
  auto dW = at::empty_like(w);
  conv_bwd_weight_launch(dy.data_ptr(), x.data_ptr(), dw_ws.data_ptr<float>(),
                         (int)Nb, (int)Hin, (int)Win, (int)C, (int)K, (int)P,
                         (int)Q, (int)R, (int)S, (int)stride, (int)pad,
                         splits, dW.data_ptr(), cur_stream());
  auto dx = at::empty_like(x);
  conv_bwd_data_launch(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), (int)Nb,
                       (int)Hin, (int)Win, (int)C, (int)K, (int)P, (int)Q,
                       (int)R, (int)S, (int)stride, (int)pad, cur_stream());
  auto db = at::zeros({K}, x.options().dtype(at::kFloat));
  conv_bias_grad_launch(dy.data_ptr(), db.data_ptr<float>(), NPQ, (int)K,
                        cur_stream());
  return {dx, dW, db};
}

// ---------------------------------------------------------------- GEMM
// C[M,N] = sum_k A(m,k)*B(n,k) (+bias[n]); ta/tb: operand memory is
// [K][rows] (k-strided) instead of [rows][K]. want_dbias (wgrad): also
// return the column-sum of A's underlying dy (fused into staging).
std::vector<at::Tensor> gemm_bf16(at::Tensor A, at::Tensor B,
                                  c10::optional<at::Tensor> bias,
                                  bool ta, bool tb, bool want_dbias) {
  TORCH_CHECK(A.is_cuda() && A.scalar_type() == at::kBFloat16 &&
              B.scalar_type() == at::kBFloat16, "gemm_bf16: bf16 CUDA only");
  TORCH_CHECK(A.is_contiguous() && B.is_contiguous());
  TORCH_CHECK(A.dim() == 2 && B.dim() == 2);
  const int64_t M = ta ? A.size(1) : A.size(0);
  const int64_t K = ta ? A.size(0) : A.size(1);
  const int64_t N = tb ? B.size(1) : B.size(0);
  TORCH_CHECK((tb ? B.size(0) : B.size(1)) == K, "gemm_bf16: K mismatch");
  TORCH_CHECK(K % 8 == 0, "gemm_bf16: K % 8 != 0");
  auto C = at::empty({M, N}, A.options());
  at::Tensor bf;
  const float* bp = nullptr;
  if (bias.has_value()) {
    bf = bias->to(at::kFloat).contiguous();
    bp = bf.data_ptr<float>();
  }
  // split the contraction when the tile grid starves the 256 CUs
  const int64_t blocks = ((M + 127) / 128) * ((N + 127) / 128);
  const int64_t nsteps = (K + 63) / 64;
  int splitz = 1;
  if (blocks < 384)
    splitz = (int)std::min<int64_t>({(384 + blocks - 1) / blocks, nsteps, 16});
  if (splitz < 1) splitz = 1;
  at::Tensor ws;
  float* wsp = nullptr;
  if (splitz > 1) {
    ws = at::zeros({M * N}, A.options().dtype(at::kFloat));
    wsp = ws.data_ptr<float>();
  }
  at::Tensor db;
  float* dbp = nullptr;
  if (want_dbias) {
    TORCH_CHECK(ta, "gemm_bf16: dbias fusion needs ta (wgrad layout)");
    db = at::zeros({M}, A.options().dtype(at::kFloat));
    dbp = db.data_ptr<float>();
  }
  gemm_bf16_launch(A.data_ptr(), B.data_ptr(), bp, C.data_ptr(), wsp, dbp,
                   M, N, (int)K, ta ? 1 : 0, tb ? 1 : 0, want_dbias ? 1 : 0,
                   splitz, cur_stream());
  if (want_dbias) return {C, db};
  return {C};
}

// dw[N,K] = dy2d[M,N]^T x2d[M,K] (+ db[N] = column sums of dy2d), bf16 with
// fp32 accumulation: one split-contraction MFMA launch into an fp32 slab and
// one ordered slab reduction. split = 0 / tile = 0 take the launcher's rule.
// dw and db are views of one [N*K (+N)] buffer.
std::vector<at::Tensor> linear_wgrad(at::Tensor dy, at::Tensor x, bool want_db,
                                     int64_t split, int64_t tile) {
  TORCH_CHECK(dy.is_cuda() && x.is_cuda() &&
              dy.scalar_type() == at::kBFloat16 &&
              x.scalar_type() == at::kBFloat16, "linear_wgrad: bf16 CUDA only");
  TORCH_CHECK(dy.dim() == 2 && x.dim() == 2 && dy.is_contiguous() &&
              x.is_contiguous(), "linear_wgrad: contiguous 2-D expected");
  const int64_t M = dy.size(0), N = dy.size(1), K = x.size(1);
  TORCH_CHECK(x.size(0) == M, "linear_wgrad: row mismatch");
  TORCH_CHECK(M >= 1 && N % 8 == 0 && K % 8 == 0 && N >= 8 && K >= 8,
              "linear_wgrad: N % 8 == 0 and K % 8 == 0 expected");
  TORCH_CHECK(N * K + N < (1LL << 31) && split >= 0 && split < (1 << 16));
  TORCH_CHECK(M * std::max(N, K) < (1LL << 30),
              "linear_wgrad: operands of 2 GiB and more are not supported "
              "(32-bit buffer offsets)");
  int tn, sp, cps;
  linear_wgrad_plan(M, (int)N, (int)K, (int)tile, (int)split, &tn, &sp, &cps);
  const int64_t ld = N * K + (want_db ? N : 0);
  auto slab = at::empty({sp * ld}, dy.options().dtype(at::kFloat));
  auto out = at::empty({ld}, dy.options());
  linear_wgrad_launch(dy.data_ptr(), x.data_ptr(), slab.data_ptr<float>(),
                      out.data_ptr(), M, (int)N, (int)K, want_db ? 1 : 0, tn,
                      sp, cps, cur_stream());
  auto dw = out.narrow(0, 0, N * K).view({N, K});
  if (want_db) return {dw, out.narrow(0, N * K, N)};
  return {dw};
}

// ---------------------------------------------------------------- maxsim
// out[n, m] = max over patch pairs (p, q) of <A[n, p, :], B[m, q, :]>, fp32.
// One fused launch: the [N*P, M*Q] score matrix is never stored.
at::Tensor patch_maxsim(at::Tensor A, at::Tensor B) {
  TORCH_CHECK(A.is_cuda() && B.is_cuda() && A.device() == B.device(),
              "patch_maxsim: CUDA tensors on one device expected");
  TORCH_CHECK(A.scalar_type() == at::kBFloat16 &&
              B.scalar_type() == at::kBFloat16, "patch_maxsim: bf16 only");
  TORCH_CHECK(A.dim() == 3 && B.dim() == 3,
              "patch_maxsim: A [N, P, C] and B [M, Q, C] expected");
  TORCH_CHECK(A.is_contiguous() && B.is_contiguous(),
              "patch_maxsim: contiguous operands expected");
  const int64_t N = A.size(0), P = A.size(1), C = A.size(2);
  const int64_t M = B.size(0), Q = B.size(1);
  TORCH_CHECK(B.size(2) == C, "patch_maxsim: C mismatch");
  TORCH_CHECK(C >= 8 && C % 8 == 0, "patch_maxsim: C % 8 != 0");
  TORCH_CHECK(P >= 1 && Q >= 1, "patch_maxsim: P >= 1 and Q >= 1 expected");
  TORCH_CHECK(P < (1LL << 30) && Q < (1LL << 30) && C < (1LL << 30),
              "patch_maxsim: P, Q, C must stay below 2^30");
  auto out = at::full({N, M}, -std::numeric_limits<float>::infinity(),
                      A.options().dtype(at::kFloat));
  if (N == 0 || M == 0) return out;
  TORCH_CHECK(reinterpret_cast<uintptr_t>(A.data_ptr()) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(B.data_ptr()) % 16 == 0,
              "patch_maxsim: operands must be 16-byte aligned");
  const int64_t tiles = ((N * P + 127) / 128) * ((M * Q + 127) / 128);
  TORCH_CHECK(tiles < (1LL << 31),
              "patch_maxsim: too many score tiles for one launch; "
              "pass fewer rows of A per call");
  patch_maxsim_launch(A.data_ptr(), B.data_ptr(), out.data_ptr<float>(), N, M,
                      (int)P, (int)Q, (int)C, cur_stream());
  return out;
}

// ---------------------------------------------------------------- splitsim
// out[n, m] = max over groups g of <A[n, g, :], B[m, g, :]>, fp32. One fused
// launch: the [N, M, G] block of per-group scores is never stored. splits =
// 0 takes the launcher's rule; any value gives the same bits.
at::Tensor split_product(at::Tensor A, at::Tensor B, int64_t splits) {
  TORCH_CHECK(A.is_cuda() && B.is_cuda() && A.device() == B.device(),
              "split_product: CUDA tensors on one device expected");
  TORCH_CHECK(A.scalar_type() == at::kBFloat16 &&
              B.scalar_type() == at::kBFloat16, "split_product: bf16 only");
  TORCH_CHECK(A.dim() == 3 && B.dim() == 3,
              "split_product: A [N, G, L] and B [M, G, L] expected");
  TORCH_CHECK(A.is_contiguous() && B.is_contiguous(),
              "split_product: contiguous operands expected");
  const int64_t N = A.size(0), G = A.size(1), L = A.size(2);
  const int64_t M = B.size(0);
  TORCH_CHECK(B.size(1) == G, "split_product: G mismatch");
  TORCH_CHECK(B.size(2) == L, "split_product: L mismatch");
  TORCH_CHECK(L >= 8 && L % 8 == 0, "split_product: L % 8 != 0");
  TORCH_CHECK(G >= 1, "split_product: G >= 1 expected");
  TORCH_CHECK(G < (1LL << 30) && L < (1LL << 30) && G * L < (1LL << 31),
              "split_product: G * L must stay below 2^31");
  TORCH_CHECK(N < (1LL << 31) && M < (1LL << 31),
              "split_product: N and M must stay below 2^31");
  TORCH_CHECK(splits >= 0 && splits <= G,
              "split_product: 0 <= splits <= G expected");
  const auto opts = A.options().dtype(at::kFloat);
  if (N == 0 || M == 0) return at::empty({N, M}, opts);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(A.data_ptr()) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(B.data_ptr()) % 16 == 0,
              "split_product: operands must be 16-byte aligned");
  const int S = split_product_splits(N, M, (int)G, (int)splits);
  const int64_t tiles = ((N + 127) / 128) * ((M + 127) / 128);
  TORCH_CHECK(tiles * S < (1LL << 31),
              "split_product: too many blocks for one launch; pass fewer "
              "rows of A per call");
  auto out = S > 1
      ? at::full({N, M}, -std::numeric_limits<float>::infinity(), opts)
      : at::empty({N, M}, opts);
  split_product_launch(A.data_ptr(), B.data_ptr(), out.data_ptr<float>(), N, M,
                       (int)G, (int)L, S, cur_stream());
  return out;
}

// ---------------------------------------------------------------- topk_sim
// Per row of q [Nq, D] the m best (score, column) pairs of q x^T over
// x [Nx, D], higher score first and the lower column first among equals:
// {scores fp32 [Nq, m], idx int64 [Nq, m]}. The score matrix is never
// stored. stripes = 0 takes the launcher's rule; any value gives the same
// bits.
std::vector<at::Tensor> topk_sim(at::Tensor q, at::Tensor x, int64_t m,
                                 int64_t stripes) {
  TORCH_CHECK(q.is_cuda() && x.is_cuda() && q.device() == x.device(),
              "topk_sim: CUDA tensors on one device expected");
  TORCH_CHECK(q.scalar_type() == at::kBFloat16 &&
              x.scalar_type() == at::kBFloat16, "topk_sim: bf16 only");
  TORCH_CHECK(q.dim() == 2 && x.dim() == 2,
              "topk_sim: q [Nq, D] and x [Nx, D] expected");
  const int64_t Nq = q.size(0), D = q.size(1), Nx = x.size(0);
  TORCH_CHECK(Nx < (1LL << 31), "topk_sim: Nx must stay below 2^31");
  TORCH_CHECK(Nq < (1LL << 31),
              "topk_sim: pass fewer than 2^31 query rows per call");
  TORCH_CHECK(q.is_contiguous() && x.is_contiguous(),
              "topk_sim: contiguous operands expected");
  TORCH_CHECK(x.size(1) == D, "topk_sim: D mismatch");
  TORCH_CHECK(D >= 8 && D % 8 == 0 && D < (1LL << 30),
              "topk_sim: D % 8 != 0");
  TORCH_CHECK(m >= 1 && m <= 16, "topk_sim: 1 <= m <= 16 expected");
  TORCH_CHECK(m <= Nx, "topk_sim: m exceeds the number of index rows");
  TORCH_CHECK(stripes >= 0 && stripes < (1LL << 24),
              "topk_sim: stripes out of range");
  auto scores = at::empty({Nq, m}, q.options().dtype(at::kFloat));
  auto idx = at::empty({Nq, m}, q.options().dtype(at::kLong));
  if (Nq == 0) return {scores, idx};
  TORCH_CHECK(reinterpret_cast<uintptr_t>(q.data_ptr()) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "topk_sim: operands must be 16-byte aligned");
  int cap, ns;
  long tps;
  topk_sim_plan(Nq, Nx, (int)m, (int)stripes, &cap, &ns, &tps);
  TORCH_CHECK(((Nq + 127) / 128) * ns < (1LL << 31),
              "topk_sim: too many blocks for one launch; pass fewer query "
              "rows per call");
  auto part_s = at::empty({Nq, 2 * ns, cap}, q.options().dtype(at::kFloat));
  auto part_i = at::empty({Nq, 2 * ns, cap}, q.options().dtype(at::kInt));
  topk_sim_launch(q.data_ptr(), x.data_ptr(), part_s.data_ptr<float>(),
                  part_i.data_ptr<int>(), scores.data_ptr<float>(),
                  reinterpret_cast<long*>(idx.data_ptr<int64_t>()), Nq, Nx,
                  (int)D, (int)m, cap, ns, tps, cur_stream());
  return {scores, idx};
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, mod) {
  mod.def("topk_sim", &topk_sim, pybind11::arg("q"), pybind11::arg("x"),
          pybind11::arg("m"), pybind11::arg("stripes") = 0);
  mod.def("gemm_bf16", &gemm_bf16);
  mod.def("patch_maxsim", &patch_maxsim);
  mod.def("split_product", &split_product, pybind11::arg("A"),
          pybind11::arg("B"), pybind11::arg("splits") = 0);
  mod.def("linear_wgrad", &linear_wgrad, pybind11::arg("dy2d"),
          pybind11::arg("x2d"), pybind11::arg("want_db"),
          pybind11::arg("split") = 0, pybind11::arg("tile") = 0);
  mod.def("conv2d_nhwc_bwd", &conv2d_nhwc_bwd);
  mod.def("conv2d_nhwc_fwd", &conv2d_nhwc_fwd);
  mod.def("conv2d_nhwc_fwd_v2", &conv2d_nhwc_fwd_v2,
          pybind11::arg("x"), pybind11::arg("w"), pybind11::arg("bias"),
          pybind11::arg("stride"), pybind11::arg("pad"),
          pybind11::arg("res") = c10::nullopt,
          pybind11::arg("temb") = c10::nullopt);
  mod.def("attn_fwd", &attn_fwd);
  mod.def("attn_fwd_gen", &attn_fwd_gen);
  mod.def("attn_fwd_gen_lse", &attn_fwd_gen_lse);
  mod.def("attn_fwd_d512", &attn_fwd_d512);
  mod.def("attn_bwd_gen", &attn_bwd_gen);
  mod.def("attn_fwd_v2", &attn_fwd_v2);
  mod.def("attn_fwd_v3", &attn_fwd_v3);
  mod.def("attn_fwd_v4", &attn_fwd_v4);
  mod.def("attn_bwd", &attn_bwd);
  mod.def("attn_bwd_v4", &attn_bwd_v4);
  mod.def("mfma_probe", &mfma_probe);
  mod.def("groupnorm_silu_fwd", &groupnorm_silu_fwd);
  mod.def("groupnorm_silu_bwd", &groupnorm_silu_bwd);
  mod.def("groupnorm_silu_nhwc_fwd", &groupnorm_silu_nhwc_fwd);
  mod.def("groupnorm_silu_nhwc_bwd", &groupnorm_silu_nhwc_bwd);
  mod.def("layernorm_fwd", &layernorm_fwd);
  mod.def("layernorm_bwd", &layernorm_bwd, py::arg("dy"), py::arg("x"),
          py::arg("w"), py::arg("mean"), py::arg("rstd"),
          py::arg("blocks") = 0);
  mod.def("colsum", &colsum);
  mod.def("colsum_grouped", &colsum_grouped);
  mod.def("geglu_fwd", &geglu_fwd);
  mod.def("geglu_bwd", &geglu_bwd);
  mod.def("adamw_step", &adamw_step);
  mod.def("adamw_step_bf16", &adamw_step_bf16);
  mod.def("adamw_step_dev", &adamw_step_dev);
  mod.def("adamw_step_clip", &adamw_step_clip);
  mod.def("adamw_step_bf16_clip", &adamw_step_bf16_clip);
  mod.def("grad_gather", &grad_gather, py::arg("arena"), py::arg("views"),
          py::arg("grads"), py::arg("partials") = py::none(),
          py::arg("ch") = 16384, py::arg("grid") = 0, py::arg("add") = false);
  mod.def("grad_sumsq", &grad_sumsq, py::arg("arena"), py::arg("views"),
          py::arg("partials"), py::arg("ch") = 16384, py::arg("grid") = 0);
  mod.def("sumsq_finalize", &sumsq_finalize);
  mod.def("adamw8_step", &adamw8_step, py::arg("p"), py::arg("g"),
          py::arg("exp_avg_q"), py::arg("exp_avg_absmax"),
          py::arg("exp_avg_sq_q"), py::arg("exp_avg_sq_absmax"), py::arg("lr"),
          py::arg("beta1"), py::arg("beta2"), py::arg("eps"), py::arg("wd"),
          py::arg("step"));
  mod.def("adamw8_step_bf16", &adamw8_step_bf16, py::arg("p"), py::arg("g"),
          py::arg("master"), py::arg("exp_avg_q"), py::arg("exp_avg_absmax"),
          py::arg("exp_avg_sq_q"), py::arg("exp_avg_sq_absmax"), py::arg("lr"),
          py::arg("beta1"), py::arg("beta2"), py::arg("eps"), py::arg("wd"),
          py::arg("step"));
  mod.def("adamw8_step_clip", &adamw8_step_clip, py::arg("p"), py::arg("g"),
          py::arg("exp_avg_q"), py::arg("exp_avg_absmax"),
          py::arg("exp_avg_sq_q"), py::arg("exp_avg_sq_absmax"), py::arg("lr"),
          py::arg("beta1"), py::arg("beta2"), py::arg("eps"), py::arg("wd"),
          py::arg("step"), py::arg("rec"));
  mod.def("adamw8_step_bf16_clip", &adamw8_step_bf16_clip, py::arg("p"),
          py::arg("g"), py::arg("master"), py::arg("exp_avg_q"),
          py::arg("exp_avg_absmax"), py::arg("exp_avg_sq_q"),
          py::arg("exp_avg_sq_absmax"), py::arg("lr"), py::arg("beta1"),
          py::arg("beta2"), py::arg("eps"), py::arg("wd"), py::arg("step"),
          py::arg("rec"));
  mod.def("add_noise", &add_noise);
  mod.def("get_velocity", &get_velocity);
  mod.def("cfg_combine", &cfg_combine);
  mod.def("lincomb", &lincomb);
}
