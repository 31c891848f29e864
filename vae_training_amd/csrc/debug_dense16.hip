// Diagnostic entry (not part of include/vaek.h; tests/test_gpu_dense16.py): run ONE Dense launcher of dtype = VAEK_BF16 -- the
// round-1 kernels of gemm_bf16.hip, the bf16-storage kernels of gemm_bf16s.hip and gemm_skinny16.hip, and the bf16-stored forms
// of gemm_f32.hip -- on caller tensors, exactly as net_forward / net_backward (api.hip) call it: the same launch_* function with
// the same argument conventions, weights prepared by the step's own prep kernels (launch_cvt_weights, launch_sk_prep) into the
// caller's scratch, dW|db slabs summed by launch_sum_slabs into the flat-gradient layout [(n_in + 1), n_out].  Every predicate
// the launcher or the step relies on is checked before the first launch; a shape the step would not send launches nothing.
#include <algorithm>

#include "vaek_internal.h"

enum {
    VAEK_D16_DENSE_FWD_BF16 = 0, VAEK_D16_DENSE_FWD_REPARAM_BF16, VAEK_D16_DENSE_DX_BF16, VAEK_D16_DENSE_DW_BF16,     // gemm_bf16.hip
    VAEK_D16_HS_FWD, VAEK_D16_HS_DX, VAEK_D16_HS_DW,                                                                 // gemm_bf16s.hip
    VAEK_D16_SK_FIRST_FWD, VAEK_D16_SK_LAST_FWD, VAEK_D16_SK_LAST_FWD_REPARAM, VAEK_D16_SK_LAST_FWD_ELBO,            // gemm_skinny16.hip
    VAEK_D16_SK_FIRST_DX, VAEK_D16_SK_LAST_BWD, VAEK_D16_SK_FIRST_BWD,
    VAEK_D16_FWD_OUT16, VAEK_D16_FWD_IN16, VAEK_D16_FWD_REPARAM_IN16, VAEK_D16_FWD_ELBO_IN16,                        // gemm_f32.hip
    VAEK_D16_DX_OUT16, VAEK_D16_DX_IN16, VAEK_D16_DW_X16, VAEK_D16_DW_DY16,
    VAEK_D16_COUNT
};

// Tensors are row-major and contiguous; "bf16" ones are __bf16.  x: the layer input [rows, n_in]; dy: the gradient of its output
// [rows, n_out]; w: f32 [n_in, n_out] as the parameters hold it, b: f32 [n_out].  The skinny ops name their layer the same way:
// first layer n_in = d, n_out = H; last layer n_in = H, n_out = d.
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
    float* out2;                         // samples (reparameterisation)
    float* dwb;                          // summed dW|db [(n_in + 1), n_out]
    void* scratch; int64_t scratch_bytes;     // scratch == null: the bytes needed are written to scratch_bytes
};

namespace vaek {
namespace {

size_t up256(size_t v) { return (v + 255) / 256 * 256; }

struct D16Scratch { size_t wb, sk, slabs, skpart, epart, total; int64_t slab_stride; };

bool is_dw(int op) {
    return op == VAEK_D16_DENSE_DW_BF16 || op == VAEK_D16_HS_DW || op == VAEK_D16_SK_LAST_BWD || op == VAEK_D16_SK_FIRST_BWD ||
           op == VAEK_D16_DW_X16 || op == VAEK_D16_DW_DY16;
}
bool is_sk(int op) { return op >= VAEK_D16_SK_FIRST_FWD && op <= VAEK_D16_SK_FIRST_BWD; }
bool sk_first(int op) { return op == VAEK_D16_SK_FIRST_FWD || op == VAEK_D16_SK_FIRST_DX || op == VAEK_D16_SK_FIRST_BWD; }

D16Scratch scratch_layout(int op, const vaek_dense16_args& a) {
    D16Scratch s{};
    const int d = sk_first(op) ? a.n_in : a.n_out, H = sk_first(op) ? a.n_out : a.n_in;
    size_t off = 0;
    s.wb = off;
    if (op == VAEK_D16_HS_FWD || op == VAEK_D16_HS_DX) off = up256(off + 2 * (size_t)a.n_in * a.n_out * sizeof(__bf16));
    s.sk = off;
    if (op == VAEK_D16_SK_LAST_FWD || op == VAEK_D16_SK_LAST_FWD_REPARAM || op == VAEK_D16_SK_LAST_FWD_ELBO || op == VAEK_D16_SK_FIRST_DX)
        off = up256(off + 32 * (size_t)H * sizeof(__bf16));
    s.slab_stride = (int64_t)(((size_t)(a.n_in + 1) * a.n_out + 63) / 64 * 64);
    s.slabs = off;
    if (is_dw(op)) off = up256(off + (size_t)a.S * s.slab_stride * sizeof(float));
    s.skpart = off;
    if (op == VAEK_D16_SK_LAST_BWD || op == VAEK_D16_SK_FIRST_BWD) off = up256(off + sk_partial_bytes(d, H, a.S));
    s.epart = off;     // {mse, d eps} per output tile: tiles are at least 32 x 32
    if (op == VAEK_D16_SK_LAST_FWD_ELBO || op == VAEK_D16_FWD_ELBO_IN16)
        off = up256(off + (size_t)((a.rows + 31) / 32) * ((a.n_out + 31) / 32) * 2 * sizeof(float));
    s.total = off;
    return s;
}

// The step's predicates (api.hip vaek_ctx_create, net_forward, net_backward) and the launchers' own, checked up front.
int validate(int op, const vaek_dense16_args& a) {
    auto bad = [](const char* why) { set_error("vaek_debug_dense16: %s", why); return VAEK_ERR_INVALID; };
    if (op < 0 || op >= VAEK_D16_COUNT) return bad("unknown op");
    if (a.rows <= 0 || a.n_in <= 0 || a.n_out <= 0) return bad("rows, n_in and n_out must be positive");
    const bool fwd = op == VAEK_D16_DENSE_FWD_BF16 || op == VAEK_D16_DENSE_FWD_REPARAM_BF16 || op == VAEK_D16_HS_FWD ||
                     op == VAEK_D16_SK_FIRST_FWD || op == VAEK_D16_SK_LAST_FWD || op == VAEK_D16_SK_LAST_FWD_REPARAM ||
                     op == VAEK_D16_SK_LAST_FWD_ELBO || op == VAEK_D16_FWD_OUT16 || op == VAEK_D16_FWD_IN16 ||
                     op == VAEK_D16_FWD_REPARAM_IN16 || op == VAEK_D16_FWD_ELBO_IN16;
    const bool dx = op == VAEK_D16_DENSE_DX_BF16 || op == VAEK_D16_HS_DX || op == VAEK_D16_SK_FIRST_DX || op == VAEK_D16_DX_OUT16 ||
                    op == VAEK_D16_DX_IN16;
    const bool reparam = op == VAEK_D16_DENSE_FWD_REPARAM_BF16 || op == VAEK_D16_SK_LAST_FWD_REPARAM || op == VAEK_D16_FWD_REPARAM_IN16;
    const bool elbo = op == VAEK_D16_SK_LAST_FWD_ELBO || op == VAEK_D16_FWD_ELBO_IN16;
    if (!a.w && (!is_dw(op) || op == VAEK_D16_SK_LAST_BWD)) return bad("w is required");
    if ((fwd || is_dw(op) || op == VAEK_D16_SK_LAST_BWD) && !a.x) return bad("x is required");
    if ((dx || is_dw(op)) && !a.dy) return bad("dy is required");
    if (fwd && !a.b) return bad("b is required");
    if ((fwd || dx || op == VAEK_D16_SK_LAST_BWD) && !a.out) return bad("out is required");
    if (is_dw(op) && !a.dwb) return bad("dwb is required");
    if (reparam && (!a.out2 || !a.z1 || !a.lv)) return bad("out2, z1 and lv are required");
    if (elbo && (!a.xdata || !a.z2)) return bad("xdata and z2 are required");
    if ((op == VAEK_D16_HS_DX || op == VAEK_D16_DX_OUT16) && !a.x_post) return bad("x_post is required");
    if (a.accumulate && !(op == VAEK_D16_DENSE_DX_BF16 || op == VAEK_D16_SK_FIRST_DX || op == VAEK_D16_DX_OUT16 || op == VAEK_D16_DX_IN16))
        return bad("this op does not accumulate");
    // the width classes the step sends to each family
    if (op <= VAEK_D16_DENSE_DW_BF16 && (a.n_in < 64 || a.n_out < 64)) return bad("gemm_bf16 layers have both widths >= 64");
    if (op >= VAEK_D16_HS_FWD && op <= VAEK_D16_HS_DW && (a.n_in % 64 || a.n_out % 64))
        return bad("bf16-storage hidden layers have widths that are multiples of 64");
    if (is_sk(op)) {
        const int d = sk_first(op) ? a.n_in : a.n_out, H = sk_first(op) ? a.n_out : a.n_in;
        if (!sk_supported(d, H)) return bad("skinny kernels need 1 <= d <= 16 and H a multiple of 64 in [64, 2048]");
    }
    if (op >= VAEK_D16_FWD_OUT16) {        // the first (out16, dx_in16, dw_dy16) or last layer of a b16 stack that sk_supported refused
        const bool first = op == VAEK_D16_FWD_OUT16 || op == VAEK_D16_DX_IN16 || op == VAEK_D16_DW_DY16;
        const int d = first ? a.n_in : a.n_out, H = first ? a.n_out : a.n_in;
        if (H % 64) return bad("the bf16-stored side is a hidden width, a multiple of 64");
        if (sk_supported(d, H)) return bad("this layer runs on the skinny kernels in the step");
    }
    const bool has_relu = op == VAEK_D16_DENSE_FWD_BF16 || op == VAEK_D16_DENSE_DX_BF16 || op == VAEK_D16_HS_FWD ||
                          op == VAEK_D16_SK_FIRST_FWD || op == VAEK_D16_FWD_OUT16;
    if (a.relu && !has_relu) return bad("this op has no relu switch");
    if (is_dw(op)) {
        if (a.S < 1) return bad("S must be >= 1");
        if (op == VAEK_D16_SK_LAST_BWD || op == VAEK_D16_SK_FIRST_BWD) {
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
    const D16Scratch s = scratch_layout(op, a);
    if (!a.scratch) { a.scratch_bytes = (int64_t)s.total; return VAEK_OK; }
    if (a.scratch_bytes < (int64_t)s.total || (reinterpret_cast<uintptr_t>(a.scratch) & 255)) {
        set_error("vaek_debug_dense16: scratch must be 256-byte aligned and hold %zu bytes", s.total);
        return VAEK_ERR_WORKSPACE;
    }
    if (!ctx) { set_error("vaek_debug_dense16: null context"); return VAEK_ERR_INVALID; }
    ProfBind pb(ctx);
    hipStream_t st = (hipStream_t)stream;
    const int rows = a.rows, n_in = a.n_in, n_out = a.n_out;
    const float* xf = static_cast<const float*>(a.x);
    const __bf16* x16 = static_cast<const __bf16*>(a.x);
    const float* dyf = static_cast<const float*>(a.dy);
    const __bf16* dy16 = static_cast<const __bf16*>(a.dy);
    float* outf = static_cast<float*>(a.out);
    __bf16* out16 = static_cast<__bf16*>(a.out);
    float* slabs = at<float>(a.scratch, s.slabs);
    float* epart = at<float>(a.scratch, s.epart);
    int bm = 0, nbx = 0;

    // weight prep, as convert_weights (api.hip) runs it for the step: the parameters are the one layer's [W | b] at offset 0
    if (op == VAEK_D16_HS_FWD || op == VAEK_D16_HS_DX) {
        const int K[1] = {n_in}, N[1] = {n_out};
        const int64_t woff[1] = {0}, ooff[1] = {0};
        if ((rc = launch_cvt_weights(a.w, at<__bf16>(a.scratch, s.wb), K, N, woff, ooff, 1, st))) return rc;
    }
    __bf16* wp = at<__bf16>(a.scratch, s.sk);
    if (op == VAEK_D16_SK_LAST_FWD || op == VAEK_D16_SK_LAST_FWD_REPARAM || op == VAEK_D16_SK_LAST_FWD_ELBO || op == VAEK_D16_SK_FIRST_DX) {
        const bool first = op == VAEK_D16_SK_FIRST_DX;
        const int H[1] = {first ? n_out : n_in}, d[1] = {first ? n_in : n_out}, tr[1] = {first ? 0 : 1};
        const int64_t woff[1] = {0}, ooff[1] = {0};
        if ((rc = launch_sk_prep(a.w, wp, H, d, tr, woff, ooff, 1, st))) return rc;
    }
    const __bf16* wb16 = at<__bf16>(a.scratch, s.wb);
    const __bf16* wT16 = wb16 + (int64_t)n_in * n_out;

    switch (op) {
    case VAEK_D16_DENSE_FWD_BF16: rc = launch_dense_fwd_bf16(xf, a.w, a.b, outf, rows, n_in, n_out, a.relu != 0, st); break;
    case VAEK_D16_DENSE_FWD_REPARAM_BF16:
        rc = launch_dense_fwd_reparam_bf16(xf, a.w, a.b, outf, a.out2, a.z1, a.lv, rows, n_in, n_out, st); break;
    case VAEK_D16_DENSE_DX_BF16:
        rc = launch_dense_bwd_dx_bf16(dyf, a.w, static_cast<const float*>(a.x_post), outf, rows, n_in, n_out, a.relu != 0, a.accumulate != 0, st);
        break;
    case VAEK_D16_DENSE_DW_BF16:
        rc = launch_dense_bwd_dw_bf16(xf, dyf, slabs, s.slab_stride, a.S, a.rows_per_split, rows, n_in, n_out, st); break;
    case VAEK_D16_HS_FWD: rc = launch_hs_fwd(x16, wT16, a.b, out16, rows, n_in, n_out, a.relu != 0, st); break;
    case VAEK_D16_HS_DX: rc = launch_hs_dx(dy16, wb16, static_cast<const __bf16*>(a.x_post), out16, rows, n_in, n_out, st); break;
    case VAEK_D16_HS_DW: rc = launch_hs_dw(x16, dy16, slabs, s.slab_stride, a.S, a.rows_per_split, rows, n_in, n_out, st); break;
    case VAEK_D16_SK_FIRST_FWD: rc = launch_sk_first_fwd(xf, a.w, a.b, out16, rows, n_in, n_out, a.relu != 0, st); break;
    case VAEK_D16_SK_LAST_FWD: rc = launch_sk_last_fwd(x16, wp, a.b, outf, rows, n_in, n_out, st); break;
    case VAEK_D16_SK_LAST_FWD_REPARAM:
        rc = launch_sk_last_fwd_reparam(x16, wp, a.b, outf, a.out2, a.z1, a.lv, rows, n_in, n_out, st); break;
    case VAEK_D16_SK_LAST_FWD_ELBO:
        rc = launch_sk_last_fwd_elbo(x16, wp, a.b, outf, a.xdata, a.z2, a.eps_param, a.eps_cli, a.inv_bt, epart, rows, n_in, n_out, &bm, &nbx, st);
        break;
    case VAEK_D16_SK_FIRST_DX: rc = launch_sk_first_dx(dy16, wp, outf, rows, n_out, n_in, a.accumulate != 0, st); break;
    case VAEK_D16_SK_LAST_BWD:
        a.form = sk_bwd_mfma_form(rows, n_in, n_out, a.S) ? 1 : 0;
        rc = launch_sk_last_bwd(x16, dyf, a.w, out16, at<float>(a.scratch, s.skpart), slabs, s.slab_stride, a.S, rows, n_in, n_out, st);
        break;
    case VAEK_D16_SK_FIRST_BWD:
        a.form = sk_bwd_mfma_form(rows, n_out, n_in, a.S) ? 1 : 0;
        rc = launch_sk_first_bwd(xf, dy16, at<float>(a.scratch, s.skpart), slabs, s.slab_stride, a.S, rows, n_out, n_in, st);
        break;
    case VAEK_D16_FWD_OUT16: rc = launch_dense_fwd_out16(xf, a.w, a.b, out16, rows, n_in, n_out, a.relu != 0, st); break;
    case VAEK_D16_FWD_IN16: rc = launch_dense_fwd_in16(x16, a.w, a.b, outf, rows, n_in, n_out, st); break;
    case VAEK_D16_FWD_REPARAM_IN16:
        rc = launch_dense_fwd_reparam_in16(x16, a.w, a.b, outf, a.out2, a.z1, a.lv, rows, n_in, n_out, st); break;
    case VAEK_D16_FWD_ELBO_IN16:
        rc = launch_dense_fwd_elbo_in16(x16, a.w, a.b, outf, a.xdata, a.z2, a.eps_param, a.eps_cli, a.inv_bt, epart, rows, n_in, n_out, &bm, &nbx,
                                        st);
        break;
    case VAEK_D16_DX_OUT16:
        rc = launch_dense_bwd_dx_out16(dyf, a.w, static_cast<const __bf16*>(a.x_post), out16, rows, n_in, n_out, a.accumulate != 0, st); break;
    case VAEK_D16_DX_IN16: rc = launch_dense_bwd_dx_in16(dy16, a.w, outf, rows, n_in, n_out, a.accumulate != 0, st); break;
    case VAEK_D16_DW_X16:
        rc = launch_dense_bwd_dw_x16(x16, dyf, slabs, s.slab_stride, a.S, a.rows_per_split, rows, n_in, n_out, st); break;
    case VAEK_D16_DW_DY16:
        rc = launch_dense_bwd_dw_dy16(xf, dy16, slabs, s.slab_stride, a.S, a.rows_per_split, rows, n_in, n_out, st); break;
    }
    if (rc) return rc;
    if (is_dw(op)) return launch_sum_slabs(slabs, s.slab_stride, a.S, a.dwb, (int64_t)(n_in + 1) * n_out, st);
    return VAEK_OK;
}
