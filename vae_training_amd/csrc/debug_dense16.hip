// Diagnostic entry (not part of include/vaek.h; tests/test_gpu_dense16.py, tests/test_gpu_dense32.py): run ONE Dense launcher --
// of dtype = VAEK_BF16 the round-1 kernels of gemm_bf16.hip, the bf16-storage kernels of gemm_bf16s.hip and gemm_skinny16.hip and
// the bf16-stored forms of gemm_f32.hip; of dtype = VAEK_F32 the all-f32 kernels of gemm_f32.hip (the f32_* ops) -- on caller tensors through the step's own code (api.hip): the op names a layer kind and a launch function
// (dense_fwd / dense_dx / dense_dw), weights are prepared by prep_weights into the caller's scratch, dW|db slabs summed by
// launch_sum_slabs into the flat-gradient layout [(n_in + 1), n_out].  Every predicate the launcher relies on is checked before
// the first launch, and so is the step's route: a shape dense_kind gives another kind launches nothing.
#include <algorithm>

#include "vaek_internal.h"

enum {
    VAEK_D16_DENSE_FWD_BF16 = 0, VAEK_D16_DENSE_FWD_REPARAM_BF16, VAEK_D16_DENSE_DX_BF16, VAEK_D16_DENSE_DW_BF16,     // gemm_bf16.hip
    VAEK_D16_HS_FWD, VAEK_D16_HS_DX, VAEK_D16_HS_DW,                                                                 // gemm_bf16s.hip
    VAEK_D16_SK_FIRST_FWD, VAEK_D16_SK_LAST_FWD, VAEK_D16_SK_LAST_FWD_REPARAM, VAEK_D16_SK_LAST_FWD_ELBO,            // gemm_skinny16.hip
    VAEK_D16_SK_FIRST_DX, VAEK_D16_SK_LAST_BWD, VAEK_D16_SK_FIRST_BWD,
    VAEK_D16_FWD_OUT16, VAEK_D16_FWD_IN16, VAEK_D16_FWD_REPARAM_IN16, VAEK_D16_FWD_ELBO_IN16,                        // gemm_f32.hip
    VAEK_D16_DX_OUT16, VAEK_D16_DX_IN16, VAEK_D16_DW_X16, VAEK_D16_DW_DY16,
    VAEK_D16_F32_FWD, VAEK_D16_F32_FWD_REPARAM, VAEK_D16_F32_FWD_ELBO, VAEK_D16_F32_DX, VAEK_D16_F32_DW,             // gemm_f32.hip, all f32
    VAEK_D16_COUNT
};

// Tensors are row-major and contiguous; "bf16" ones are __bf16.  x: the layer input [rows, n_in]; dy: the gradient of its output
// [rows, n_out]; w: f32 [n_in, n_out] as the parameters hold it, b: f32 [n_out].  The skinny ops name their layer the same way:
// first layer n_in = d, n_out = H; last layer n_in = H, n_out = d.  The f32_* ops demand no alignment of any tensor (the public ABI
// demands none: a layer's kernel sits wherever the layers before it end in the flat parameter vector); scratch stays 256-aligned.
struct vaek_dense16_args {
    int32_t rows, n_in, n_out;
    int32_t relu, accumulate;            // relu: forward activation / dX mask (ops that have the choice); accumulate: dX ops
    int32_t S, rows_per_split;           // dW|db ops: batch split (the skinny ones use S only: S * 64 workgroups)
    int32_t form;                        // out: sk_last_bwd / sk_first_bwd 1 = matrix-core form, 0 = per-lane form; else -1
    const void* x; const float* w; const float* b; const void* dy;
    const void* x_post;                  // dX relu-mask source (f32 for gemm_bf16, bf16 otherwise; may be null for gemm_bf16)
    const float* z1; const float* lv;    // reparameterisation epilogues: samples = mu + exp(lv / 2) z1
    const float* xdata; const float* z2; const float* eps_param; float eps_cli, inv_bt;      // ELBO epilogues
    void* out;                           // y / mu / dX / dL/dx_hat (sk_last_bwd: dh)
    float* out2;                         // samples (reparameterisation).  ELBO ops: null, or where the {mse, d eps} pair of every
                                         // output tile goes instead of scratch, in the kernel's tile order: the caller provides
                                         // 2 * ceil(rows / 32) * ceil(n_out / 32) floats (tiles are at least 32 x 32; a kernel with
                                         // larger tiles writes the first 2 * tiles of them)
    float* dwb;                          // summed dW|db [(n_in + 1), n_out]
    void* scratch; int64_t scratch_bytes;     // scratch == null: the bytes needed are written to scratch_bytes
};

namespace vaek {
namespace {

// each op as the step reaches it: the layer kind, and which launch function (api.hip) with which epilogue
enum Dir { FWD, DX, DW };
struct Route { Kind kind; Dir dir; Epi epi = Epi::NONE; };
constexpr Route kRoute[VAEK_D16_COUNT] = {
    {Kind::BF16, FWD}, {Kind::BF16, FWD, Epi::REPARAM}, {Kind::BF16, DX}, {Kind::BF16, DW},
    {Kind::HIDDEN16, FWD}, {Kind::HIDDEN16, DX}, {Kind::HIDDEN16, DW},
    {Kind::FIRST_SK, FWD}, {Kind::LAST_SK, FWD}, {Kind::LAST_SK, FWD, Epi::REPARAM}, {Kind::LAST_SK, FWD, Epi::ELBO},
    {Kind::FIRST_SK, DX}, {Kind::LAST_SK, DW}, {Kind::FIRST_SK, DW},
    {Kind::FIRST16, FWD}, {Kind::LAST16, FWD}, {Kind::LAST16, FWD, Epi::REPARAM}, {Kind::LAST16, FWD, Epi::ELBO},
    {Kind::LAST16, DX}, {Kind::FIRST16, DX}, {Kind::LAST16, DW}, {Kind::FIRST16, DW},
    {Kind::F32, FWD}, {Kind::F32, FWD, Epi::REPARAM}, {Kind::F32, FWD, Epi::ELBO}, {Kind::F32, DX}, {Kind::F32, DW},
};
Pos position(Kind k) {       // the f32-storage kinds' choice does not depend on it
    return k == Kind::FIRST_SK || k == Kind::FIRST16 ? Pos::FIRST : k == Kind::LAST_SK || k == Kind::LAST16 ? Pos::LAST : Pos::HIDDEN;
}
// the ops whose launch reads the layer's bf16 kernel copies (DenseW::w16)
bool reads_w16(const Route& r) {
    return (r.kind == Kind::HIDDEN16 && r.dir != DW) || (r.kind == Kind::LAST_SK && r.dir == FWD) || (r.kind == Kind::FIRST_SK && r.dir == DX);
}

size_t up256(size_t v) { return (v + 255) / 256 * 256; }

struct D16Scratch { size_t wb, skw, slabs, skpart, epart, total; int64_t slab_stride; };

D16Scratch scratch_layout(const Route& r, const Layer& l, int rows) {
    D16Scratch s{};
    size_t off = 0;
    s.wb = off;
    if (reads_w16(r) && r.kind == Kind::HIDDEN16) off = up256(off + 2 * (size_t)l.n_in * l.n_out * sizeof(__bf16));
    s.skw = off;
    if (reads_w16(r) && is_sk(r.kind)) off = up256(off + 32 * (size_t)sk_H(l) * sizeof(__bf16));
    s.slab_stride = (int64_t)(((size_t)(l.n_in + 1) * l.n_out + 63) / 64 * 64);
    s.slabs = off;
    if (r.dir == DW) off = up256(off + (size_t)l.S * s.slab_stride * sizeof(float));
    s.skpart = off;
    if (r.dir == DW && is_sk(r.kind)) off = up256(off + sk_partial_bytes(sk_d(l), sk_H(l), l.S));
    s.epart = off;     // {mse, d eps} per output tile: tiles are at least 32 x 32
    if (r.epi == Epi::ELBO) off = up256(off + (size_t)((rows + 31) / 32) * ((l.n_out + 31) / 32) * 2 * sizeof(float));
    s.total = off;
    return s;
}

// The launchers' predicates and the step's route, checked up front.
int validate(int op, const vaek_dense16_args& a) {
    auto bad = [](const char* why) { set_error("vaek_debug_dense16: %s", why); return VAEK_ERR_INVALID; };
    if (op < 0 || op >= VAEK_D16_COUNT) return bad("unknown op");
    if (a.rows <= 0 || a.n_in <= 0 || a.n_out <= 0) return bad("rows, n_in and n_out must be positive");
    const Route r = kRoute[op];
    const bool fwd = r.dir == FWD, dx = r.dir == DX, dw = r.dir == DW, sk_bwd = dw && r.kind == Kind::LAST_SK;
    if (!a.w && (!dw || sk_bwd)) return bad("w is required");
    if ((fwd || dw) && !a.x) return bad("x is required");
    if ((dx || dw) && !a.dy) return bad("dy is required");
    if (fwd && !a.b) return bad("b is required");
    if ((fwd || dx || sk_bwd) && !a.out) return bad("out is required");
    if (dw && !a.dwb) return bad("dwb is required");
    if (r.epi == Epi::REPARAM && (!a.out2 || !a.z1 || !a.lv)) return bad("out2, z1 and lv are required");
    if (r.epi == Epi::ELBO && (!a.xdata || !a.z2)) return bad("xdata and z2 are required");
    if (dx && (r.kind == Kind::HIDDEN16 || r.kind == Kind::LAST16) && !a.x_post) return bad("x_post is required");
    if (a.accumulate && !(dx && r.kind != Kind::HIDDEN16)) return bad("this op does not accumulate");
    // the step's route: dense_kind gives this kind to this shape at this position, in a stack that can hold the layer
    const Pos pos = position(r.kind);
    const bool b16 = r.kind != Kind::F32 && r.kind != Kind::BF16;
    const int dtype = r.kind == Kind::F32 ? VAEK_F32 : VAEK_BF16;
    if (dense_kind(dtype, b16, pos, a.n_in, a.n_out) != r.kind) return bad("the step runs another kernel on this layer");
    if (b16 && ((pos != Pos::FIRST && !b16_width(a.n_in)) || (pos != Pos::LAST && !b16_width(a.n_out))))
        return bad("the hidden widths of a bf16-storage stack are multiples of 64");
    const bool has_relu = (fwd && r.epi == Epi::NONE && pos != Pos::LAST) || (dx && (r.kind == Kind::BF16 || r.kind == Kind::F32));
    if (a.relu && !has_relu) return bad("this op has no relu switch");
    if (dw) {
        if (a.S < 1) return bad("S must be >= 1");
        if (is_sk(r.kind)) {
            if (a.S > 64) return bad("skinny dW: S <= 64");
        } else {
            if (a.rows_per_split <= 0 || a.rows_per_split % 64) return bad("rows_per_split must be a positive multiple of 64");
            if ((int64_t)a.S * a.rows_per_split < a.rows || (int64_t)(a.S - 1) * a.rows_per_split >= a.rows)
                return bad("S must be ceil(rows / rows_per_split)");
        }
    }
    return VAEK_OK;
}

template <typename T> T* at(void* base, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(base) + off); }

}  // namespace
}  // namespace vaek

extern "C" int vaek_debug_dense16(vaek_ctx* ctx, int32_t op, vaek_dense16_args* args, void* stream) {
    using namespace vaek;
    if (!args) { set_error("vaek_debug_dense16: null args"); return VAEK_ERR_INVALID; }
    vaek_dense16_args& a = *args;
    a.form = -1;
    int rc = validate(op, a);
    if (rc) return rc;
    const Route r = kRoute[op];
    // the one layer: its [W | b] at offset 0 of the caller's w, its bf16 copies at offset 0 of their scratch areas
    Layer l;
    l.n_in = a.n_in; l.n_out = a.n_out; l.w_off = 0; l.relu = a.relu != 0; l.kind = r.kind; l.S = a.S; l.rows_per_split = a.rows_per_split;
    const D16Scratch s = scratch_layout(r, l, a.rows);
    if (!a.scratch) { a.scratch_bytes = (int64_t)s.total; return VAEK_OK; }
    if (a.scratch_bytes < (int64_t)s.total || (reinterpret_cast<uintptr_t>(a.scratch) & 255)) {
        set_error("vaek_debug_dense16: scratch must be 256-byte aligned and hold %zu bytes", s.total);
        return VAEK_ERR_WORKSPACE;
    }
    if (!ctx) { set_error("vaek_debug_dense16: null context"); return VAEK_ERR_INVALID; }
    ProfBind pb(ctx);
    hipStream_t st = (hipStream_t)stream;
    const Layer* ls[1] = {&l};
    // weight prep, as convert_weights (api.hip) runs it for the step
    if (reads_w16(r) && (rc = prep_weights(a.w, ls, 1, at<__bf16>(a.scratch, s.wb), at<__bf16>(a.scratch, s.skw), st))) return rc;
    const DenseW p{a.w, a.b, at<__bf16>(a.scratch, r.kind == Kind::HIDDEN16 ? s.wb : s.skw)};
    if (r.dir == FWD) {
        float* part = r.epi == Epi::ELBO && a.out2 ? a.out2 : at<float>(a.scratch, s.epart);
        Epilogue e{r.epi, a.out2, a.z1, a.lv, a.xdata, a.z2, a.eps_param, a.eps_cli, a.inv_bt, part, 0, 0};
        return dense_fwd(l, p, a.x, a.out, a.rows, &e, st);
    }
    if (r.dir == DX) return dense_dx(l, p, a.dy, a.x_post, a.out, a.rows, a.relu != 0, a.accumulate != 0, st);
    if (is_sk(r.kind)) a.form = sk_bwd_mfma_form(a.rows, sk_H(l), sk_d(l), a.S) ? 1 : 0;
    float* slabs = at<float>(a.scratch, s.slabs);
    if ((rc = dense_dw(l, p, a.x, a.dy, a.out, slabs, s.slab_stride, at<float>(a.scratch, s.skpart), a.rows, st))) return rc;
    return launch_sum_slabs(slabs, s.slab_stride, a.S, a.dwb, (int64_t)(a.n_in + 1) * a.n_out, st);
}
