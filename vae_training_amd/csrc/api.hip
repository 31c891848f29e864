// C ABI of libvaek.so (include/vaek.h): context, flat parameter layout, workspace carving and the
// layer-by-layer orchestration of VAE.train_step / VAE.loss / VAE.apply
// (/root/reference/networks.py:87-101, :103-113, :61-84).
#include <stdarg.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <utility>

#include "eval_check.h"      // the checks of the training entry points and their order; vaek_internal.h through it

namespace vaek {

static thread_local char g_err[512] = "";
thread_local Profiler* g_prof = nullptr;
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
constexpr int kElboBlockSplits = 512;           // row splits of the ELBO block entry point (vaek_elbo_fwd_bwd)

static void add_net(vaek_ctx* c, Net& net, const char* name, int fan_in, const int* hidden, int n_hidden, int last) {
    int k = fan_in;
    for (int i = 0; i <= n_hidden; ++i) {
        const int n = i < n_hidden ? hidden[i] : last;
        Layer l;
        l.n_in = k; l.n_out = n; l.w_off = c->P; l.relu = i < n_hidden;
        char nm[64];
        snprintf(nm, sizeof(nm), "%s/FC%d/kernel", name, i);
        c->leaves.push_back({nm, c->P, k, n});
        c->P += (int64_t)k * n;
        snprintf(nm, sizeof(nm), "%s/FC%d/bias", name, i);
        c->leaves.push_back({nm, c->P, 1, n});
        c->P += n;
        net.layers.push_back(l);
        c->max_width = std::max(c->max_width, std::max(k, n));
        k = n;
    }
}

static size_t carve_acts(vaek_ctx* c, Net& net, size_t off) {
    for (auto& l : net.layers) {
        net.act_off.push_back(off);
        off = align_up(off + (size_t)c->B * l.n_out * sizeof(float), 256);
    }
    return off;
}

static int check_ws(const vaek_ctx* c, const void* ws) {
    if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255)) {
        set_error("workspace must be a non-null, 256-byte aligned device pointer of vaek_workspace_bytes() bytes");
        return VAEK_ERR_WORKSPACE;
    }
    (void)c;
    return VAEK_OK;
}

// dW|db slabs are flat-gradient images at a 64-float-aligned pitch (16-byte loads in the streaming reductions)
static inline int64_t slab_stride(const vaek_ctx* c) { return (int64_t)align_up((size_t)c->P, 64); }

template <typename T>
static T* at(void* ws, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(ws) + off); }

// ---- a Dense layer's kernels: its kind, decided once per layer in vaek_ctx_create ---------------------------------------------
// dtype = VAEK_BF16 routes the WIDE layers (both dims >= 64) of an f32-storage stack through the bf16 matrix-core kernels; skinny
// input/output layers (D, L of a handful of features) stay on the exact f32 kernels -- they are bandwidth-bound and carry the
// reparameterisation / ELBO inputs.  A b16 stack's ends keep an exact f32 product too, with the hidden side stored as bf16.
Kind dense_kind(int dtype, bool b16, Pos pos, int n_in, int n_out) {
    if (!b16) return dtype == VAEK_BF16 && n_in >= 64 && n_out >= 64 ? Kind::BF16 : Kind::F32;
    if (pos == Pos::FIRST) return sk_supported(n_in, n_out) ? Kind::FIRST_SK : Kind::FIRST16;
    if (pos == Pos::LAST) return sk_supported(n_out, n_in) ? Kind::LAST_SK : Kind::LAST16;
    return Kind::HIDDEN16;
}
// bf16-STORAGE mode of a stack: with at least two hidden layers whose widths are all multiples of 64, the hidden activations /
// gradients are kept as bf16 and the hidden -> hidden layers run gemm_bf16s.hip.  Other stacks under dtype = VAEK_BF16 keep f32
// storage and the round-1 kernels (gemm_bf16.hip) for their wide layers.
static bool net_is_b16(int dtype, const Net& net) {
    if (dtype != VAEK_BF16 || net.layers.size() < 3) return false;
    for (size_t i = 0; i + 1 < net.layers.size(); ++i)
        if (!b16_width(net.layers[i].n_out)) return false;
    return true;
}
// batch split of the layer's dW|db launch: slabs sized so that (tiles x S) fills the chip
static void plan_split(Layer& l, int B) {
    if (is_sk(l.kind)) {
        // gemm_skinny16.hip: S slabs, each the fixed-order sum of 64 workgroups' partial images
        l.S = std::min(8, std::max(1, B / 4096));
        l.rows_per_split = (B + l.S - 1) / l.S;
        return;
    }
    int s_target;
    if (l.kind == Kind::HIDDEN16) {
        // gemm_bf16s.hip, 128 x 128 tiles, 64-row k-tiles: ~512 workgroups
        const int tiles = ((l.n_in + 127) / 128) * ((l.n_out + 127) / 128);
        s_target = std::min(256, std::max(1, 512 / tiles));
    } else {
        // wide layers run 128 x 128 tiles (gemm_f32.hip) and want ~3 workgroups per CU; the rest 64-wide tiles
        const bool wide = l.n_in + 1 >= 128 && l.n_out >= 128;
        // ... counted in the tile shape gemm_f32.hip's launch() picks: 128 x 128, 128 x 32 (n_out <= 32), 32 x 128 (n_in < 32)
        const int tiles = wide ? ((l.n_in + 1 + 127) / 128) * ((l.n_out + 127) / 128)
                        : l.n_out <= 32 ? (l.n_in + 1 + 127) / 128
                        : l.n_in + 1 <= 32 ? (l.n_out + 127) / 128
                        : ((l.n_in + 1 + 63) / 64) * ((l.n_out + 63) / 64);
        // at most 64 slabs: the fixed-order slab sum (bulk_finalize_kernel) is a chain of S / 8 memory round trips per output,
        // and a 256-slab skinny layer (C3's 6 -> 512) held the whole finalize launch for ~60 us
        s_target = std::min(64, std::max(4, (wide ? 768 : 1024) / tiles));
    }
    l.rows_per_split = std::max(64, (int)align_up((size_t)(B + s_target - 1) / s_target, 64));
    l.S = (B + l.rows_per_split - 1) / l.rows_per_split;
}

int prep_weights(const float* params, const Layer* const* ls, int count, __bf16* wb16, __bf16* sk16, hipStream_t st) {
    int K[24], N[24], n = 0, H[16], d[16], tr[16], m = 0;
    int64_t woff[24], ooff[24], sw[16], so[16];
    for (int i = 0; i < count; ++i) {
        const Layer& l = *ls[i];
        if ((l.kind == Kind::HIDDEN16 && n == 24) || (is_sk(l.kind) && m == 16)) { set_error("too many bf16 layers"); return VAEK_ERR_INVALID; }
        if (l.kind == Kind::HIDDEN16) { K[n] = l.n_in; N[n] = l.n_out; woff[n] = l.w_off; ooff[n] = l.w16_off; ++n; }
        if (is_sk(l.kind)) { H[m] = sk_H(l); d[m] = sk_d(l); tr[m] = l.kind == Kind::LAST_SK; sw[m] = l.w_off; so[m] = l.w16_off; ++m; }
    }
    int rc = launch_cvt_weights(params, wb16, K, N, woff, ooff, n, st);
    return rc ? rc : launch_sk_prep(params, sk16, H, d, tr, sw, so, m, st);
}
// bf16 copies of every b16 layer's kernel, once per entry point that runs the layer-by-layer step
static int convert_weights(vaek_ctx* c, const float* params, void* ws, hipStream_t st) {
    const Layer* ls[32];
    int n = 0;
    for (const Net* net : {&c->enc, &c->dec, &c->sig})
        for (const Layer& l : net->layers) ls[n++] = &l;
    return prep_weights(params, ls, n, at<__bf16>(ws, c->ws_wb16), at<__bf16>(ws, c->ws_sk16), st);
}
static DenseW layer_weights(const vaek_ctx* c, const float* params, void* ws, const Layer& l) {
    const float* w = params + l.w_off;
    return {w, w + (int64_t)l.n_in * l.n_out, at<__bf16>(ws, l.kind == Kind::HIDDEN16 ? c->ws_wb16 : c->ws_sk16) + l.w16_off};
}

// ---- the launch functions: the only code that knows each kind's launchers and their argument conventions ------------------
int dense_fwd(const Layer& l, const DenseW& p, const void* x, void* y, int rows, Epilogue* e, hipStream_t st) {
    const Epi epi = e ? e->kind : Epi::NONE;
    const float* xf = static_cast<const float*>(x);
    const __bf16* x16 = static_cast<const __bf16*>(x);
    float* yf = static_cast<float*>(y);
    __bf16* y16 = static_cast<__bf16*>(y);
    switch (l.kind) {
    case Kind::F32:
        if (epi == Epi::ELBO)
            return launch_dense_fwd_elbo(xf, p.w, p.b, yf, e->x, e->z2, e->eps_param, e->eps_cli, e->inv_bt, e->part, rows, l.n_in,
                                         l.n_out, &e->bm, &e->nbx, st);
        if (epi == Epi::REPARAM) return launch_dense_fwd_reparam(xf, p.w, p.b, yf, e->samples, e->z1, e->lv, rows, l.n_in, l.n_out, st);
        return launch_dense_fwd(xf, p.w, p.b, yf, rows, l.n_in, l.n_out, l.relu, st);
    case Kind::BF16:
        if (epi == Epi::ELBO) break;          // gemm_bf16.hip has none: generic_grads runs the ELBO pass on its own
        if (epi == Epi::REPARAM)
            return launch_dense_fwd_reparam_bf16(xf, p.w, p.b, yf, e->samples, e->z1, e->lv, rows, l.n_in, l.n_out, st);
        return launch_dense_fwd_bf16(xf, p.w, p.b, yf, rows, l.n_in, l.n_out, l.relu, st);
    // a b16 stack's first and hidden layers are never the last: no epilogue
    case Kind::FIRST_SK: return launch_sk_first_fwd(xf, p.w, p.b, y16, rows, l.n_in, l.n_out, l.relu, st);
    case Kind::FIRST16: return launch_dense_fwd_out16(xf, p.w, p.b, y16, rows, l.n_in, l.n_out, l.relu, st);
    case Kind::HIDDEN16: return launch_hs_fwd(x16, p.w16 + (int64_t)l.n_in * l.n_out, p.b, y16, rows, l.n_in, l.n_out, l.relu, st);
    case Kind::LAST_SK:
        if (epi == Epi::ELBO)
            return launch_sk_last_fwd_elbo(x16, p.w16, p.b, yf, e->x, e->z2, e->eps_param, e->eps_cli, e->inv_bt, e->part, rows, l.n_in,
                                           l.n_out, &e->bm, &e->nbx, st);
        if (epi == Epi::REPARAM)
            return launch_sk_last_fwd_reparam(x16, p.w16, p.b, yf, e->samples, e->z1, e->lv, rows, l.n_in, l.n_out, st);
        return launch_sk_last_fwd(x16, p.w16, p.b, yf, rows, l.n_in, l.n_out, st);
    case Kind::LAST16:
        if (epi == Epi::ELBO)
            return launch_dense_fwd_elbo_in16(x16, p.w, p.b, yf, e->x, e->z2, e->eps_param, e->eps_cli, e->inv_bt, e->part, rows, l.n_in,
                                              l.n_out, &e->bm, &e->nbx, st);
        if (epi == Epi::REPARAM)
            return launch_dense_fwd_reparam_in16(x16, p.w, p.b, yf, e->samples, e->z1, e->lv, rows, l.n_in, l.n_out, st);
        return launch_dense_fwd_in16(x16, p.w, p.b, yf, rows, l.n_in, l.n_out, st);
    }
    set_error("dense_fwd: no ELBO epilogue on gemm_bf16.hip");
    return VAEK_ERR_INVALID;
}

int dense_dx(const Layer& l, const DenseW& p, const void* dy, const void* x_post, void* dx, int rows, bool relu, bool accumulate,
             hipStream_t st) {
    const float* dyf = static_cast<const float*>(dy);
    const __bf16* dy16 = static_cast<const __bf16*>(dy);
    float* dxf = static_cast<float*>(dx);
    __bf16* dx16 = static_cast<__bf16*>(dx);
    switch (l.kind) {
    case Kind::F32:
        return launch_dense_bwd_dx(dyf, p.w, static_cast<const float*>(x_post), dxf, rows, l.n_in, l.n_out, relu, accumulate, st);
    case Kind::BF16:
        return launch_dense_bwd_dx_bf16(dyf, p.w, static_cast<const float*>(x_post), dxf, rows, l.n_in, l.n_out, relu, accumulate, st);
    case Kind::FIRST_SK: return launch_sk_first_dx(dy16, p.w16, dxf, rows, l.n_out, l.n_in, accumulate, st);
    case Kind::FIRST16: return launch_dense_bwd_dx_in16(dy16, p.w, dxf, rows, l.n_in, l.n_out, accumulate, st);
    case Kind::HIDDEN16:
        return launch_hs_dx(dy16, p.w16, static_cast<const __bf16*>(x_post), dx16, rows, l.n_in, l.n_out, st);
    case Kind::LAST_SK: return VAEK_OK;          // dense_dw's launch_sk_last_bwd wrote it
    case Kind::LAST16:
        return launch_dense_bwd_dx_out16(dyf, p.w, static_cast<const __bf16*>(x_post), dx16, rows, l.n_in, l.n_out, accumulate, st);
    }
    return VAEK_ERR_INVALID;
}

int dense_dw(const Layer& l, const DenseW& p, const void* x, const void* dy, void* dx, float* slab0, int64_t slab_stride, float* skpart,
             int rows, hipStream_t st) {
    const float* xf = static_cast<const float*>(x);
    const __bf16* x16 = static_cast<const __bf16*>(x);
    const float* dyf = static_cast<const float*>(dy);
    const __bf16* dy16 = static_cast<const __bf16*>(dy);
    switch (l.kind) {
    case Kind::F32: return launch_dense_bwd_dw(xf, dyf, slab0, slab_stride, l.S, l.rows_per_split, rows, l.n_in, l.n_out, st);
    case Kind::BF16: return launch_dense_bwd_dw_bf16(xf, dyf, slab0, slab_stride, l.S, l.rows_per_split, rows, l.n_in, l.n_out, st);
    case Kind::FIRST_SK: return launch_sk_first_bwd(xf, dy16, skpart, slab0, slab_stride, l.S, rows, l.n_out, l.n_in, st);
    case Kind::FIRST16: return launch_dense_bwd_dw_dy16(xf, dy16, slab0, slab_stride, l.S, l.rows_per_split, rows, l.n_in, l.n_out, st);
    case Kind::HIDDEN16: return launch_hs_dw(x16, dy16, slab0, slab_stride, l.S, l.rows_per_split, rows, l.n_in, l.n_out, st);
    case Kind::LAST_SK:          // dW|db AND dX from one pass over x
        return launch_sk_last_bwd(x16, dyf, p.w, static_cast<__bf16*>(dx), skpart, slab0, slab_stride, l.S, rows, l.n_in, l.n_out, st);
    case Kind::LAST16: return launch_dense_bwd_dw_x16(x16, dyf, slab0, slab_stride, l.S, l.rows_per_split, rows, l.n_in, l.n_out, st);
    }
    return VAEK_ERR_INVALID;
}

// ---- forward through one Dense/relu stack; `reparam` fuses networks.py:73-74 into the last layer, `ef` the ELBO pass
static int net_forward(vaek_ctx* c, const Net& net, const float* params, const float* in, void* ws, int rows,
                       bool reparam, const float* z1, hipStream_t st, Epilogue* ef = nullptr) {
    Epilogue rp{Epi::REPARAM, at<float>(ws, c->ws_samples), z1, params + c->off_epsp};
    const void* h = in;
    for (size_t i = 0; i < net.layers.size(); ++i) {
        const Layer& l = net.layers[i];
        float* y = at<float>(ws, net.act_off[i]);
        Epilogue* e = i + 1 < net.layers.size() ? nullptr : ef ? ef : reparam ? &rp : nullptr;
        if (int rc = dense_fwd(l, layer_weights(c, params, ws, l), h, y, rows, e, st)) return rc;
        h = y;
    }
    return VAEK_OK;
}

// ---- backward through one stack.  d_out: gradient w.r.t. the last Dense output (lives in the
// stack's last activation buffer).  dx_first: where dL/d(input) goes (nullptr: not needed).
struct BucketSink {          // bucketed mode: where finished layers go and which event announces them
    float* grads; void* const* events; int next;
};

static int net_backward(vaek_ctx* c, const Net& net, const float* params, const float* in, float* d_out, void* ws,
                        float* dx_first, bool accumulate_first, hipStream_t st, BucketSink* sink = nullptr) {
    const void* d = d_out;
    float* gb[2] = {at<float>(ws, c->ws_gbuf0), at<float>(ws, c->ws_gbuf1)};
    int tog = 0;
    float* slabs = at<float>(ws, c->ws_slabs);
    for (int i = (int)net.layers.size() - 1; i >= 0; --i) {
        const Layer& l = net.layers[i];
        const DenseW p = layer_weights(c, params, ws, l);
        const float* h_in = i == 0 ? in : at<float>(ws, net.act_off[i - 1]);
        float* dx = i > 0 ? gb[tog] : dx_first;      // a hidden layer's dX: the ping-pong buffers
        int rc = dense_dw(l, p, h_in, d, dx, slabs + l.w_off, slab_stride(c), at<float>(ws, c->ws_skpart), c->B, st);
        if (rc) return rc;
        if (sink) {     // this layer's [kernel | bias] slice is final once its slabs are summed: announce it
            const int64_t cnt = (int64_t)(l.n_in + 1) * l.n_out;
            if ((rc = launch_sum_slabs(slabs + l.w_off, slab_stride(c), l.S, sink->grads + l.w_off, cnt, st))) return rc;
            VAEK_HIP_CHECK(hipEventRecord((hipEvent_t)sink->events[sink->next++], st));
        }
        // dX through relu' of the layer below; the first layer's (to dx_first) unmasked, optionally added
        if (dx && (rc = dense_dx(l, p, d, i > 0 ? h_in : nullptr, dx, c->B, i > 0, i == 0 && accumulate_first, st))) return rc;
        if (i > 0) { d = dx; tog ^= 1; }
    }
    return VAEK_OK;
}

static int generic_grads(vaek_ctx* c, const float* params, int32_t* step_dev, const float* x, const float* z1,
                         const float* z2, void* ws, hipStream_t st, BucketSink* sink = nullptr) {
    const bool sig = c->cfg.sigmoid_decoder != 0;
    const float inv_bt = (float)(1.0 / (double)c->Bt);
    int rc;
    if ((rc = convert_weights(c, params, ws, st))) return rc;
    if ((rc = net_forward(c, c->enc, params, x, ws, c->B, true, z1, st))) return rc;
    const float* samples = at<float>(ws, c->ws_samples);
    float* mu = at<float>(ws, c->enc.act_off.back());
    float* y_lin = at<float>(ws, c->dec.act_off.back());
    const float* eps_param = c->off_eps >= 0 ? params + c->off_eps : nullptr;
    const Layer& last = c->dec.layers.back();
    if (c->lwd) {
        // wide linear decoder: x and z2 read ONCE for the decoder's forward, the ELBO pass, dL/d samples and the decoder's kernel
        // gradient (linear_wide.hip); dL/d x_hat never exists in memory
        const float* wd = params + last.w_off;
        float* slabs = at<float>(ws, c->ws_slabs);
        float* part = at<float>(ws, c->ws_eblk);
        float* gpart = at<float>(ws, c->ws_lwd);
        if ((rc = launch_lwd(samples, wd, wd + (int64_t)last.n_in * last.n_out, x, z2, eps_param, c->cfg.eps_cli, inv_bt, gpart, slabs + last.w_off,
                             slab_stride(c), part, c->B, c->D, c->L, c->lwd_rb, st)))
            return rc;
        if (sink) {
            const int64_t cnt = (int64_t)(last.n_in + 1) * last.n_out;
            if ((rc = launch_sum_slabs(slabs + last.w_off, slab_stride(c), last.S, sink->grads + last.w_off, cnt, st))) return rc;
            VAEK_HIP_CHECK(hipEventRecord((hipEvent_t)sink->events[sink->next++], st));
        }
        float* dsamp = at<float>(ws, c->ws_dsamp);
        if ((rc = launch_lwd_second(gpart, c->D / 256, dsamp, mu, z1, at<float>(ws, c->ws_rpart), c->B, c->L, c->Se, c->rows_per_esplit, inv_bt, part,
                                    last.S * (c->D / 256), at<float>(ws, c->ws_epart), step_dev, st)))
            return rc;
        return net_backward(c, c->enc, params, x, dsamp, ws, nullptr, false, st, sink);
    }
    if (!sig && last.kind != Kind::BF16) {
        // one decoder, exact f32 output layer: the ELBO's elementwise pass runs in that layer's epilogue -- its output never
        // goes to HBM, dL/dx_hat lands where the backward pass expects it
        Epilogue ef{Epi::ELBO, nullptr, nullptr, nullptr, x, z2, eps_param, c->cfg.eps_cli, inv_bt, at<float>(ws, c->ws_eblk), 0, 0};
        if ((rc = net_forward(c, c->dec, params, samples, ws, c->B, false, nullptr, st, &ef))) return rc;
        if ((rc = launch_elbo_reduce(ef.part, ef.bm, ef.nbx, mu, at<float>(ws, c->ws_epart), c->B, c->L, c->Se, c->rows_per_esplit,
                                     step_dev, st)))
            return rc;
        float* dsamp = at<float>(ws, c->ws_dsamp);
        if ((rc = net_backward(c, c->dec, params, samples, y_lin, ws, dsamp, false, st, sink))) return rc;
        if ((rc = launch_reparam_bwd(dsamp, mu, z1, at<float>(ws, c->ws_rpart), c->B, c->L, c->Se, c->rows_per_esplit, inv_bt, st)))
            return rc;
        return net_backward(c, c->enc, params, x, dsamp, ws, nullptr, false, st, sink);
    }
    if ((rc = net_forward(c, c->dec, params, samples, ws, c->B, false, nullptr, st))) return rc;
    if (sig && (rc = net_forward(c, c->sig, params, samples, ws, c->B, false, nullptr, st))) return rc;
    float* y_sig = sig ? at<float>(ws, c->sig.act_off.back()) : nullptr;
    ElboArgs e{};
    e.x = x; e.y_lin = y_lin; e.y_sig = y_sig; e.z2 = z2; e.mu = mu;
    e.eps_param = eps_param;
    e.eps_cli = c->cfg.eps_cli;
    e.d_lin = y_lin; e.d_sig = y_sig;
    e.partial = at<float>(ws, c->ws_epart);
    e.rows = c->B; e.D = c->D; e.L = c->L; e.S = c->Se; e.rows_per_split = c->rows_per_esplit;
    e.inv_bt = inv_bt; e.step_dev = step_dev;
    if ((rc = launch_elbo(e, st))) return rc;
    float* dsamp = at<float>(ws, c->ws_dsamp);
    if ((rc = net_backward(c, c->dec, params, samples, y_lin, ws, dsamp, false, st, sink))) return rc;
    if (sig && (rc = net_backward(c, c->sig, params, samples, y_sig, ws, dsamp, true, st, sink))) return rc;
    if ((rc = launch_reparam_bwd(dsamp, mu, z1, at<float>(ws, c->ws_rpart), c->B, c->L, c->Se, c->rows_per_esplit,
                                 inv_bt, st)))
        return rc;
    return net_backward(c, c->enc, params, x, dsamp, ws, nullptr, false, st, sink);
}

// the whole-network step of a context with c->fused; `exchange` (the in-kernel P2P sum) exists on fused_train_step's kernels only
static int whole_step(vaek_ctx* c, float* params, float* grads, float* m, float* v, int32_t* step_dev, const float* x, const float* z1,
                      const float* z2, float lr, bool apply_adam, bool exchange, void* ws, hipStream_t st, const BatchArgs* gen = nullptr) {
    if (!c->mlp3) return fused_train_step(c, params, grads, m, v, step_dev, x, z1, z2, lr, apply_adam, exchange, ws, st, gen);
    if (exchange) { set_error("the three-hidden-layer whole-network step has no in-kernel exchange"); return VAEK_ERR_INVALID; }
    return mlp3_train_step(c, params, grads, m, v, step_dev, x, z1, z2, lr, apply_adam, ws, st, gen);
}

constexpr int64_t kBulkFinalizeMin = 65536;      // parameters below which the 64-output finalize alone is faster

// The launch sequence of the finalisation on filled-in arguments (the step below; vaek_debug_tail, debug_tail.hip): the outputs
// [0, hi) as a streaming pass with Adam (hi = 0: none) and the 64-output finalize above them, else the 64-output finalize from
// f.lo; Adam (f.params_rw) inside the finalize kernel when `fuse`, else a separate launch over what the bulk pass left.
int finalize_launches(const FinalizeArgs& args, int64_t hi, bool fuse, hipStream_t st) {
    FinalizeArgs f = args;
    float* const params_rw = f.params_rw;
    int rc;
    int64_t adam_from = 0;
    if (hi > 0) {
        // big models: weights and biases as a streaming pass (with Adam), the 64-output finalize only for the tail
        if ((rc = launch_bulk_finalize(f, hi, st))) return rc;
        f.lo = adam_from = hi;
    }
    if (!fuse) f.params_rw = nullptr;
    if ((rc = launch_finalize(f, st)) || params_rw == nullptr || fuse) return rc;
    return launch_adam(params_rw + adam_from, f.grads + adam_from, f.m + adam_from, f.v + adam_from, f.P - adam_from, f.lr, 0, f.step_dev, 1.f, st);
}

// the finalisation's arguments as the context and its workspace give them
static FinalizeArgs finalize_args(vaek_ctx* c, const float* params, float* grads, float* params_rw, float* m, float* v,
                                  const int32_t* step_dev, float lr, void* ws, int64_t lo) {
    FinalizeArgs f{};
    f.lo = lo;
    f.slabs = at<float>(ws, c->ws_slabs); f.slab_stride = slab_stride(c); f.S = c->S;
    f.nseg = 0;
    for (const Net* net : {&c->enc, &c->dec, &c->sig})
        for (const auto& l : net->layers) {
            f.seg_end[f.nseg] = (int)(l.w_off + (int64_t)(l.n_in + 1) * l.n_out);
            f.seg_S[f.nseg++] = l.S;
        }
    f.epart = at<float>(ws, c->ws_epart); f.rpart = at<float>(ws, c->ws_rpart); f.Se = c->Se;
    f.P = c->P; f.off_epsp = c->off_epsp; f.off_eps = c->off_eps; f.L = c->L; f.D = c->D;
    f.params = params; f.eps_cli = c->cfg.eps_cli;
    f.rows_over_bt = (float)((double)c->B / (double)c->Bt); f.inv_bt = (float)(1.0 / (double)c->Bt);
    f.rows = (float)c->B;
    f.grads = grads; f.params_rw = params_rw; f.m = m; f.v = v; f.step_dev = step_dev; f.lr = lr;
    f.loss_hist = c->cfg.world == 1 ? c->loss_hist : nullptr; f.loss_hist_cap = c->loss_hist_cap;
    if (!f.step_dev) f.loss_hist = nullptr;
    return f;
}

static int generic_finalize(vaek_ctx* c, const float* params, float* grads, float* params_rw, float* m, float* v,
                            const int32_t* step_dev, float lr, void* ws, hipStream_t st, int64_t lo = 0) {
    const FinalizeArgs f = finalize_args(c, params, grads, params_rw, m, v, step_dev, lr, ws, lo);
    // Adam is fused into the finalize kernel only while epsilon_p, epsilon and the scalar sums all sit
    // in its block 0 (64 outputs): the loss lanes read epsilon_p, so its Adam writers must be behind the
    // same block-local barrier.  Wider latents take a separate Adam launch.
    const bool fuse = params_rw != nullptr && c->L + 5 <= 64;
    const int64_t hi = lo == 0 && c->off_epsp >= kBulkFinalizeMin ? c->off_epsp : 0;
    return finalize_launches(f, hi, fuse, st);
}

}  // namespace vaek

using namespace vaek;

extern "C" {

int vaek_version(void) { return VAEK_VERSION; }
const char* vaek_last_error(void) { return g_err; }

int vaek_ctx_create(const vaek_config* cfg, vaek_ctx** out) {
    if (!cfg || !out) { set_error("null argument"); return VAEK_ERR_INVALID; }
    if (cfg->struct_size != (int32_t)sizeof(vaek_config)) {
        set_error("vaek_config.struct_size %d != %zu (header/library mismatch)", cfg->struct_size, sizeof(vaek_config));
        return VAEK_ERR_INVALID;
    }
    if (cfg->batch <= 0 || cfg->data_dim <= 0 || cfg->latent_dim <= 0 || cfg->n_enc_hidden < 0 ||
        cfg->n_enc_hidden > VAEK_MAX_HIDDEN || cfg->n_dec_hidden < 0 || cfg->n_dec_hidden > VAEK_MAX_HIDDEN ||
        cfg->world < 1 || cfg->rank < 0 || cfg->rank >= cfg->world) {
        set_error("invalid geometry: batch=%d D=%d L=%d n_enc=%d n_dec=%d world=%d rank=%d", cfg->batch,
                  cfg->data_dim, cfg->latent_dim, cfg->n_enc_hidden, cfg->n_dec_hidden, cfg->world, cfg->rank);
        return VAEK_ERR_INVALID;
    }
    for (int i = 0; i < cfg->n_enc_hidden; ++i)
        if (cfg->enc_hidden[i] <= 0) { set_error("encoder hidden width %d <= 0", cfg->enc_hidden[i]); return VAEK_ERR_INVALID; }
    for (int i = 0; i < cfg->n_dec_hidden; ++i)
        if (cfg->dec_hidden[i] <= 0) { set_error("decoder hidden width %d <= 0", cfg->dec_hidden[i]); return VAEK_ERR_INVALID; }
    if (cfg->latent_dim > 250) { set_error("latent_dim %d > 250 unsupported", cfg->latent_dim); return VAEK_ERR_INVALID; }
    if (cfg->dtype != VAEK_F32 && cfg->dtype != VAEK_BF16) { set_error("unknown dtype %d", cfg->dtype); return VAEK_ERR_INVALID; }

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        set_error("no HIP device visible: libvaek.so has no CPU fallback");
        return VAEK_ERR_NO_DEVICE;
    }
    if (cfg->device < 0 || cfg->device >= ndev) { set_error("device %d out of range (%d visible)", cfg->device, ndev); return VAEK_ERR_INVALID; }
    hipDeviceProp_t prop;
    VAEK_HIP_CHECK(hipGetDeviceProperties(&prop, cfg->device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("device %d is %s; this library is built for gfx950 (MI355X) only", cfg->device, prop.gcnArchName);
        return VAEK_ERR_NO_DEVICE;
    }

    vaek_ctx* c = new (std::nothrow) vaek_ctx();
    if (!c) { set_error("out of host memory"); return VAEK_ERR_INVALID; }
    c->cfg = *cfg;
    c->B = cfg->batch; c->D = cfg->data_dim; c->L = cfg->latent_dim;
    c->Bt = cfg->global_batch > 0 ? cfg->global_batch : (int64_t)cfg->batch * cfg->world;
    c->P = 0; c->max_width = std::max(c->D, c->L);
    c->n_cu = prop.multiProcessorCount;
    add_net(c, c->enc, "Encoder", c->D, cfg->enc_hidden, cfg->n_enc_hidden, c->L);
    add_net(c, c->dec, "Decoder", c->L, cfg->dec_hidden, cfg->n_dec_hidden, c->D);
    if (cfg->sigmoid_decoder) add_net(c, c->sig, "SigDecoder", c->L, cfg->dec_hidden, cfg->n_dec_hidden, c->D);
    c->off_epsp = c->P;
    c->leaves.push_back({"epsilon_p", c->P, 1, c->L});
    c->P += c->L;
    c->off_eps = -1;
    if (cfg->tunable_eps) {
        c->off_eps = c->P;
        c->leaves.push_back({"epsilon", c->P, 1, 1});
        c->P += 1;
    }
    // per layer: its kind, the batch split of its dW|db launch and the place of its bf16 kernel copies
    int64_t wb_elems = 0, sk_elems = 0; size_t sk_part = 0;
    for (Net* net : {&c->enc, &c->dec, &c->sig}) {
        const bool b16 = net_is_b16(cfg->dtype, *net);
        for (size_t i = 0; i < net->layers.size(); ++i) {
            Layer& l = net->layers[i];
            l.kind = dense_kind(cfg->dtype, b16, i == 0 ? Pos::FIRST : i + 1 < net->layers.size() ? Pos::HIDDEN : Pos::LAST, l.n_in, l.n_out);
            plan_split(l, c->B);
            if (l.kind == Kind::HIDDEN16) { l.w16_off = wb_elems; wb_elems += 2 * (int64_t)l.n_in * l.n_out; }
            if (is_sk(l.kind)) {
                l.w16_off = sk_elems; sk_elems += 32ll * sk_H(l);
                sk_part = std::max(sk_part, sk_partial_bytes(sk_d(l), sk_H(l), l.S));
            }
        }
    }
    // wide linear decoder (BASELINE config 4): one fused kernel for its forward, the ELBO pass and both backward products; its
    // [kernel | bias] gradient comes in one slab per ROW BLOCK of that kernel's grid.  Its one layer would run gemm_f32.hip.
    c->lwd = !cfg->force_generic && !cfg->sigmoid_decoder && cfg->n_dec_hidden == 0 && c->dec.layers.back().kind == Kind::F32 &&
             lwd_supported(c->B, c->D, c->L);
    if (c->lwd) {
        Layer& l = c->dec.layers.back();
        c->lwd_rb = lwd_row_block(c->B, c->D, c->n_cu);
        l.rows_per_split = c->lwd_rb; l.S = (c->B + c->lwd_rb - 1) / c->lwd_rb;
    }
    // the slab area holds the largest split of any layer; elementwise partials one per <= 1024 row-blocks
    c->S = 1; c->rows_per_split = c->B;
    for (const Net* net : {&c->enc, &c->dec, &c->sig})
        for (const auto& l : net->layers) if (l.S > c->S) { c->S = l.S; c->rows_per_split = l.rows_per_split; }
    if (c->enc.layers.size() + c->dec.layers.size() + c->sig.layers.size() > 32) {
        set_error("too many layers"); delete c; return VAEK_ERR_INVALID;
    }
    c->rows_per_esplit = std::max(128, (int)align_up((size_t)(c->B + 1023) / 1024, 128));      // whole 64- and 128-row GEMM tiles
    c->Se = (c->B + c->rows_per_esplit - 1) / c->rows_per_esplit;

    size_t off = 0;
    off = carve_acts(c, c->enc, off);
    c->ws_samples = off; off = align_up(off + (size_t)c->B * c->L * sizeof(float), 256);
    off = carve_acts(c, c->dec, off);
    off = carve_acts(c, c->sig, off);
    c->ws_dsamp = off; off = align_up(off + (size_t)c->B * c->L * sizeof(float), 256);
    c->ws_gbuf0 = off; off = align_up(off + (size_t)c->B * c->max_width * sizeof(float), 256);
    c->ws_gbuf1 = off; off = align_up(off + (size_t)c->B * c->max_width * sizeof(float), 256);
    c->ws_slabs = off; off = align_up(off + (size_t)c->S * slab_stride(c) * sizeof(float), 256);
    c->ws_epart = off; off = align_up(off + (size_t)c->Se * 4 * sizeof(float), 256);
    c->ws_epart_blk = off; off = align_up(off + (size_t)kElboBlockSplits * 4 * sizeof(float), 256);      // vaek_elbo_fwd_bwd's own, finer splits
    c->ws_rpart = off; off = align_up(off + (size_t)c->Se * c->L * sizeof(float), 256);
    // {mse, d eps} per output tile of the decoder's last GEMM: at most (B/64) x (D/32) tiles in any of its tile shapes
    c->ws_eblk = off; off = align_up(off + (size_t)((c->B + 63) / 64) * ((c->D + 31) / 32) * 2 * sizeof(float), 256);
    // the train step's form, chosen here once (vaek_train_step_path names it): a whole-network path -- the linear / one-hidden-layer
    // kernels behind fused_train_step, or fused_mlp3.hip's -- else the layer-by-layer kernels
    c->mlp3 = !cfg->force_generic && mlp3_supported(c);
    c->fused = !cfg->force_generic && (fused_supported(c) || c->mlp3);
    c->ws_fused = off; off = align_up(off + fused_workspace_bytes(c), 256);
    c->ws_mlp3 = off; off = align_up(off + (c->mlp3 ? mlp3_workspace_bytes(c) : 0), 256);
    c->ws_wb16 = off; off = align_up(off + (size_t)wb_elems * sizeof(__bf16), 256);
    c->ws_sk16 = off; off = align_up(off + (size_t)sk_elems * sizeof(__bf16), 256);
    c->ws_skpart = off; off = align_up(off + sk_part, 256);
    c->lin = lin_plan(c);
    c->ws_lin = off; off = align_up(off + c->lin.ws_bytes, 256);
    c->ws_lwd = off; off = align_up(off + (c->lwd ? lwd_gpart_bytes(c->B, c->D, c->L) : 0), 256);
    c->resident = resident_supported(c);
    c->mlp3_loglik = mlp3_loglik_supported(c);
    c->ws_resident = off; off = align_up(off + resident_workspace_bytes(c), 256);
    c->ws_total = off;
    *out = c;
    return VAEK_OK;
}

int vaek_ctx_destroy(vaek_ctx* ctx) {
    if (!ctx) return VAEK_OK;
    vaek_comm_destroy(ctx);
    for (auto e : ctx->prof.ev) (void)hipEventDestroy(e);
    delete ctx;
    return VAEK_OK;
}

int vaek_param_count(const vaek_ctx* ctx, int64_t* P) {
    if (!ctx || !P) { set_error("null argument"); return VAEK_ERR_INVALID; }
    *P = ctx->P;
    return VAEK_OK;
}
int vaek_grad_len(const vaek_ctx* ctx, int64_t* n) {
    if (!ctx || !n) { set_error("null argument"); return VAEK_ERR_INVALID; }
    *n = ctx->P + kExtra;
    return VAEK_OK;
}
int vaek_leaf_count(const vaek_ctx* ctx, int32_t* n) {
    if (!ctx || !n) { set_error("null argument"); return VAEK_ERR_INVALID; }
    *n = (int32_t)ctx->leaves.size();
    return VAEK_OK;
}
int vaek_leaf_info(const vaek_ctx* ctx, int32_t leaf, char* name, int32_t name_cap, int64_t* offset, int32_t* rows,
                   int32_t* cols) {
    if (!ctx || leaf < 0 || leaf >= (int32_t)ctx->leaves.size()) { set_error("leaf index out of range"); return VAEK_ERR_INVALID; }
    const Leaf& l = ctx->leaves[leaf];
    if (name && name_cap > 0) { strncpy(name, l.name.c_str(), name_cap - 1); name[name_cap - 1] = 0; }
    if (offset) *offset = l.offset;
    if (rows) *rows = l.rows;
    if (cols) *cols = l.cols;
    return VAEK_OK;
}
int vaek_workspace_bytes(const vaek_ctx* ctx, size_t* bytes) {
    if (!ctx || !bytes) { set_error("null argument"); return VAEK_ERR_INVALID; }
    *bytes = ctx->ws_total;
    return VAEK_OK;
}
int vaek_uses_fused_path(const vaek_ctx* ctx, int32_t* fused) {
    if (!ctx || !fused) { set_error("null argument"); return VAEK_ERR_INVALID; }
    *fused = ctx->fused ? 1 : 0;
    return VAEK_OK;
}
int vaek_train_step_path(const vaek_ctx* ctx, char* name, int32_t cap) {
    if (!ctx || !name || cap <= 0) { set_error("vaek_train_step_path: invalid argument"); return VAEK_ERR_INVALID; }
    const char* p = ctx->mlp3 ? "mlp3" : ctx->fused ? (mlp1_supported(ctx) ? "mlp1" : "linear") : ctx->lwd ? "linear_wide" : "layers";
    if ((size_t)cap <= strlen(p)) { set_error("vaek_train_step_path: buffer too small"); return VAEK_ERR_INVALID; }
    strcpy(name, p);
    return VAEK_OK;
}

// ---- building blocks ------------------------------------------------------------------------
int vaek_dense_fwd(vaek_ctx* ctx, const float* x, const float* w, const float* b, float* y, int32_t rows,
                   int32_t n_in, int32_t n_out, int32_t act, void* stream) {
    if (!ctx || !x || !w || !y || rows <= 0 || n_in <= 0 || n_out <= 0 || (act != VAEK_ACT_NONE && act != VAEK_ACT_RELU)) {
        set_error("vaek_dense_fwd: invalid argument");
        return VAEK_ERR_INVALID;
    }
    return launch_dense_fwd(x, w, b, y, rows, n_in, n_out, act == VAEK_ACT_RELU, (hipStream_t)stream);
}

int vaek_dense_fwd_reparam(vaek_ctx* ctx, const float* x, const float* w, const float* b, float* mu, float* samples, const float* z1,
                           const float* logvar_e, int32_t rows, int32_t n_in, int32_t n_out, void* stream) {
    if (!ctx || !x || !w || !mu || !samples || !z1 || !logvar_e || rows <= 0 || n_in <= 0 || n_out <= 0) {
        set_error("vaek_dense_fwd_reparam: invalid argument");
        return VAEK_ERR_INVALID;
    }
    return launch_dense_fwd_reparam(x, w, b, mu, samples, z1, logvar_e, rows, n_in, n_out, (hipStream_t)stream);
}

// d logvar_e from the per-split sums of d_samples * z1 (fixed order) and the closed-form KL part
__global__ void reparam_finish_kernel(const float* partial, int S, int L, const float* lv, float rows_over_bt, float* out) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= L) return;
    float acc = 0.f;
    for (int s2 = 0; s2 < S; ++s2) acc += partial[(long long)s2 * L + l];
    const float v = lv[l];
    out[l] = 0.5f * expf(0.5f * v) * acc - 0.5f * (1.f - expf(v)) * rows_over_bt;
}

int vaek_reparam_bwd(vaek_ctx* ctx, float* d_samples, const float* mu, const float* z1, const float* logvar_e, float* d_logvar_e,
                     int32_t rows, int32_t latent_dim, int64_t batch_total, void* workspace, void* stream) {
    if (!ctx || !d_samples || !mu || !z1 || !logvar_e || !d_logvar_e || rows <= 0 || latent_dim <= 0 || latent_dim > 256) {
        set_error("vaek_reparam_bwd: invalid argument");
        return VAEK_ERR_INVALID;
    }
    int rc = check_ws(ctx, workspace);
    if (rc) return rc;
    const double bt = batch_total > 0 ? (double)batch_total : (double)rows;
    const int S = std::max(1, std::min(ctx->Se, (int)(((size_t)ctx->Se * ctx->L) / latent_dim)));     // what the context's partial area holds
    const int rps = (rows + S - 1) / S;
    const int Su = (rows + rps - 1) / rps;
    float* part = at<float>(workspace, ctx->ws_rpart);
    hipStream_t st = (hipStream_t)stream;
    if ((rc = launch_reparam_bwd(d_samples, mu, z1, part, rows, latent_dim, Su, rps, (float)(1.0 / bt), st))) return rc;
    hipLaunchKernelGGL(reparam_finish_kernel, dim3((latent_dim + 63) / 64), dim3(64), 0, st, (const float*)part, Su, (int)latent_dim, logvar_e,
                       (float)((double)rows / bt), d_logvar_e);
    VAEK_HIP_CHECK(hipGetLastError());
    return VAEK_OK;
}

int vaek_dense_bwd_dx(vaek_ctx* ctx, const float* dy, const float* w, const float* x_post, float* dx, int32_t rows,
                      int32_t n_in, int32_t n_out, int32_t act, int32_t accumulate, void* stream) {
    if (!ctx || !dy || !w || !dx || rows <= 0 || n_in <= 0 || n_out <= 0 || (act == VAEK_ACT_RELU && !x_post) ||
        (act != VAEK_ACT_NONE && act != VAEK_ACT_RELU)) {
        set_error("vaek_dense_bwd_dx: invalid argument");
        return VAEK_ERR_INVALID;
    }
    return launch_dense_bwd_dx(dy, w, x_post, dx, rows, n_in, n_out, act == VAEK_ACT_RELU, accumulate != 0,
                               (hipStream_t)stream);
}

int vaek_dense_bwd_dw(vaek_ctx* ctx, const float* x, const float* dy, float* dwb, int32_t rows, int32_t n_in,
                      int32_t n_out, void* workspace, void* stream) {
    if (!ctx || !x || !dy || !dwb || rows <= 0 || n_in <= 0 || n_out <= 0) {
        set_error("vaek_dense_bwd_dw: invalid argument");
        return VAEK_ERR_INVALID;
    }
    int rc = check_ws(ctx, workspace);
    if (rc) return rc;
    const int64_t n = (int64_t)(n_in + 1) * n_out;
    const int rps = std::max(64, (int)align_up((size_t)(rows + ctx->S - 1) / ctx->S, 64));
    const int S = (rows + rps - 1) / rps;
    if ((size_t)S * n * sizeof(float) > (size_t)ctx->S * ctx->P * sizeof(float)) {
        set_error("vaek_dense_bwd_dw: layer (%d+1)x%d does not fit this context's slab workspace", n_in, n_out);
        return VAEK_ERR_WORKSPACE;
    }
    float* slabs = at<float>(workspace, ctx->ws_slabs);
    if ((rc = launch_dense_bwd_dw(x, dy, slabs, n, S, rps, rows, n_in, n_out, (hipStream_t)stream))) return rc;
    return launch_sum_slabs(slabs, n, S, dwb, n, (hipStream_t)stream);
}

static int elbo_fwd_bwd_impl(vaek_ctx* ctx, const float* x, const float* x_hat_lin, const float* x_hat_sig, const float* z2,
                             const float* mu, const float* logvar_e, const float* eps_param, float eps, float* d_lin, float* d_sig, float* out4,
                             int32_t rows, int32_t data_dim, int32_t latent_dim, int64_t batch_total, void* workspace,
                             void* stream) {
    if (!ctx || !x || !x_hat_lin || !z2 || !mu || !logvar_e || !out4 || rows <= 0 || data_dim <= 0 || latent_dim <= 0 ||
        (d_lin && x_hat_sig && !d_sig)) {
        set_error("vaek_elbo_fwd_bwd: invalid argument");
        return VAEK_ERR_INVALID;
    }
    int rc = check_ws(ctx, workspace);
    if (rc) return rc;
    // the block entry point splits the rows finely (its own partial area): the train step's splits are whole GEMM tiles of >= 128 rows,
    // which at a few thousand rows of a wide model is a few dozen workgroups (the conv VAE's 4 096 x 4 096 ELBO: 32 workgroups, 0.32 ms)
    if (rows > ctx->B) { set_error("vaek_elbo_fwd_bwd: rows %d exceed this context's batch %d", rows, ctx->B); return VAEK_ERR_WORKSPACE; }
    const int rpe = std::max(1, (rows + kElboBlockSplits - 1) / kElboBlockSplits);
    const int Se = (rows + rpe - 1) / rpe;
    const int64_t bt = batch_total > 0 ? batch_total : rows;
    ElboArgs e{};
    e.x = x; e.y_lin = x_hat_lin; e.y_sig = x_hat_sig; e.z2 = z2; e.mu = mu;
    e.eps_param = eps_param; e.eps_cli = eps; e.d_lin = d_lin; e.d_sig = d_sig;
    e.partial = at<float>(workspace, ctx->ws_epart_blk);
    e.rows = rows; e.D = data_dim; e.L = latent_dim; e.S = Se; e.rows_per_split = rpe;
    e.inv_bt = (float)(1.0 / (double)bt); e.step_dev = nullptr;
    if ((rc = launch_elbo(e, (hipStream_t)stream))) return rc;
    return launch_elbo_out4(e.partial, Se, logvar_e, latent_dim, data_dim, eps_param, eps, (float)rows, e.inv_bt, out4,
                            (hipStream_t)stream);
}

int vaek_elbo_fwd_bwd(vaek_ctx* ctx, const float* x, const float* x_hat_lin, const float* x_hat_sig, const float* z2,
                      const float* mu, const float* logvar_e, float eps, float* d_lin, float* d_sig, float* out4,
                      int32_t rows, int32_t data_dim, int32_t latent_dim, int64_t batch_total, void* workspace,
                      void* stream) {
    return elbo_fwd_bwd_impl(ctx, x, x_hat_lin, x_hat_sig, z2, mu, logvar_e, nullptr, eps, d_lin, d_sig, out4, rows, data_dim, latent_dim,
                             batch_total, workspace, stream);
}

int vaek_elbo_fwd_bwd_dev(vaek_ctx* ctx, const float* x, const float* x_hat_lin, const float* x_hat_sig, const float* z2,
                          const float* mu, const float* logvar_e, const float* eps_param_dev, float eps_scale, float* d_lin, float* d_sig,
                          float* out4, int32_t rows, int32_t data_dim, int32_t latent_dim, int64_t batch_total, void* workspace,
                          void* stream) {
    if (!eps_param_dev) { set_error("vaek_elbo_fwd_bwd_dev: invalid argument"); return VAEK_ERR_INVALID; }
    return elbo_fwd_bwd_impl(ctx, x, x_hat_lin, x_hat_sig, z2, mu, logvar_e, eps_param_dev, eps_scale, d_lin, d_sig, out4, rows, data_dim,
                             latent_dim, batch_total, workspace, stream);
}

int vaek_adam_step(vaek_ctx* ctx, float* params, const float* grads, float* m, float* v, int64_t n, float lr,
                   int32_t step, const int32_t* step_dev, float grad_scale, void* stream) {
    if (!ctx || !params || !grads || !m || !v || n < 0 || (!step_dev && step < 1)) {
        set_error("vaek_adam_step: invalid argument");
        return VAEK_ERR_INVALID;
    }
    return launch_adam(params, grads, m, v, n, lr, step, step_dev, grad_scale, (hipStream_t)stream);
}

// ---- the hot path ----------------------------------------------------------------------------
int vaek_train_step_grads_only(vaek_ctx* ctx, const float* params, float* grads, int32_t* step_dev, const float* x,
                               const float* z1, const float* z2, void* workspace, void* stream) {
    ProfBind pb(ctx);
    int rc = check_train_state("vaek_train_step_grads_only", ctx, params, grads, nullptr, nullptr, step_dev, 0, false);
    if (rc || (rc = check_given("vaek_train_step_grads_only", "x", x, "z1", z1, "z2", z2)) || (rc = check_ws(ctx, workspace))) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (ctx->fused)
        return whole_step(ctx, const_cast<float*>(params), grads, nullptr, nullptr, step_dev, x, z1, z2, 0.f, false,
                          false, workspace, st);
    if ((rc = generic_grads(ctx, params, step_dev, x, z1, z2, workspace, st))) return rc;
    return generic_finalize(ctx, params, grads, nullptr, nullptr, nullptr, nullptr, 0.f, workspace, st);
}

int vaek_train_step_apply(vaek_ctx* ctx, float* params, const float* grads, float* m, float* v,
                          const int32_t* step_dev, float lr, void* stream) {
    ProfBind pb(ctx);
    if (int rc = check_train_state("vaek_train_step_apply", ctx, params, grads, m, v, step_dev)) return rc;
    return launch_adam(params, grads, m, v, ctx->P, lr, 0, step_dev, 1.f, (hipStream_t)stream);
}

int vaek_train_step(vaek_ctx* ctx, float* params, float* grads, float* m, float* v, int32_t* step_dev, const float* x,
                    const float* z1, const float* z2, float lr, void* workspace, void* stream) {
    ProfBind pb(ctx);
    int rc = check_train_state("vaek_train_step", ctx, params, grads, m, v, step_dev);
    if (rc || (rc = check_given("vaek_train_step", "x", x, "z1", z1, "z2", z2)) || (rc = check_ws(ctx, workspace))) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (ctx->cfg.world > 1) {
        if (!ctx->comm.ready) {
            set_error("vaek_train_step: world=%d but no communicator; call vaek_comm_init or use "
                      "vaek_train_step_grads_only + all-reduce + vaek_train_step_apply", ctx->cfg.world);
            return VAEK_ERR_COMM;
        }
        // fused path: the exchange happens inside the finalize kernel (the step stays two launches); fused_mlp3.hip has no
        // exchange and takes the three calls below
        if (ctx->fused && !ctx->mlp3) return whole_step(ctx, params, grads, m, v, step_dev, x, z1, z2, lr, true, true, workspace, st);
        if ((rc = vaek_train_step_grads_only(ctx, params, grads, step_dev, x, z1, z2, workspace, stream))) return rc;
        if ((rc = vaek_comm_allreduce(ctx, grads, ctx->P + kExtra, stream))) return rc;
        return vaek_train_step_apply(ctx, params, grads, m, v, step_dev, lr, stream);
    }
    if (ctx->fused) return whole_step(ctx, params, grads, m, v, step_dev, x, z1, z2, lr, true, false, workspace, st);
    if ((rc = generic_grads(ctx, params, step_dev, x, z1, z2, workspace, st))) return rc;
    return generic_finalize(ctx, params, grads, params, m, v, step_dev, lr, workspace, st);
}

// Train on the batch (x, z1, z2) AND draw the next one (x_next, z1_next, z2_next; none may alias the current batch)
// from the self-advancing generator counter: see include/vaek.h.
int vaek_train_step_gen(vaek_ctx* ctx, float* params, float* grads, float* m, float* v, int32_t* step_dev, const float* x,
                        const float* z1, const float* z2, float lr, void* workspace, int32_t kind, const float* A, int32_t dd,
                        int32_t did, int32_t pad, float var_added, float* x_next, float* z1_next, float* z2_next, int64_t row0,
                        uint64_t seed, int32_t* counter, int32_t which, uint32_t tag, void* stream) {
    ProfBind pb(ctx);
    const char* const who = "vaek_train_step_gen";
    int rc = check_train_state(who, ctx, params, grads, m, v, step_dev);
    if (rc || (rc = check_given(who, "x", x, "z1", z1, "z2", z2, "x_next", x_next, "z1_next", z1_next, "z2_next", z2_next, "counter", counter))) return rc;
    if (x_next == x || z1_next == z1 || z2_next == z2) {
        set_error("%s: the next batch must not alias the current one", who);
        return VAEK_ERR_INVALID;
    }
    BatchArgs gen;      // a draw to memory: vaek_make_batch_next's check, under its name
    if ((rc = make_batch_args(ctx, kind, A, dd, did, pad, var_added, x_next, z1_next, z2_next, ctx->B, row0, seed, nullptr, 0, counter, which, tag, &gen)) ||
        (rc = check_ws(ctx, workspace)))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    const bool comm_ok = ctx->cfg.world == 1 || (ctx->comm.ready && !ctx->mlp3);
    if (ctx->fused && comm_ok)
        return whole_step(ctx, params, grads, m, v, step_dev, x, z1, z2, lr, true, ctx->cfg.world > 1, workspace, st, &gen);
    // layer-by-layer path: the same two operations as separate launches on the one stream
    if ((rc = make_batch_launch(ctx, gen, st))) return rc;
    return vaek_train_step(ctx, params, grads, m, v, step_dev, x, z1, z2, lr, workspace, stream);
}

int vaek_supports_train_steps(const vaek_ctx* ctx, int32_t* yes) {
    if (!ctx || !yes) { set_error("null argument"); return VAEK_ERR_INVALID; }
    *yes = lin_steps_supported(ctx) ? 1 : 0;
    return VAEK_OK;
}

int vaek_train_steps(vaek_ctx* ctx, float* params, float* grads, float* m, float* v, int32_t* step_dev, const float* const* xs,
                     const float* const* z1s, const float* const* z2s, int32_t n_steps, float lr, void* workspace, void* stream) {
    ProfBind pb(ctx);
    int rc = check_train_state("vaek_train_steps", ctx, params, grads, m, v, step_dev, n_steps);
    if (rc || (rc = check_given("vaek_train_steps", "xs", xs, "z1s", z1s, "z2s", z2s))) return rc;
    if (!lin_steps_supported(ctx)) {
        set_error("vaek_train_steps: this context is not a single-GPU float32 linear VAE with L + 2 D + 1 <= 64 (use vaek_train_step)");
        return VAEK_ERR_INVALID;
    }
    if ((rc = check_ws(ctx, workspace))) return rc;
    for (int i = 0; i < n_steps; ++i)
        if (!xs[i] || !z1s[i] || !z2s[i] || ((reinterpret_cast<uintptr_t>(xs[i]) | reinterpret_cast<uintptr_t>(z1s[i]) | reinterpret_cast<uintptr_t>(z2s[i])) & 15)) {
            set_error("vaek_train_steps: batch %d has a null or not 16-byte aligned pointer", i);
            return VAEK_ERR_INVALID;
        }
    if (n_steps == 0) return VAEK_OK;
    return lin_train_steps(ctx, params, grads, m, v, step_dev, xs, z1s, z2s, n_steps, lr, workspace, (hipStream_t)stream);
}

int vaek_supports_train_steps_gen(const vaek_ctx* ctx, int32_t kind, int32_t* yes) {
    if (!ctx || !yes) { set_error("null argument"); return VAEK_ERR_INVALID; }
    *yes = lin_steps_gen_supported(ctx, kind) ? 1 : 0;
    return VAEK_OK;
}

int vaek_train_steps_gen(vaek_ctx* ctx, float* params, float* grads, float* m, float* v, int32_t* step_dev, int32_t kind, const float* A,
                         int32_t dd, int32_t did, int32_t pad, float var_added, int64_t row0, uint64_t seed, uint32_t tag, int32_t n_steps,
                         float lr, void* workspace, void* stream) {
    ProfBind pb(ctx);
    int rc = check_train_state("vaek_train_steps_gen", ctx, params, grads, m, v, step_dev, n_steps);
    if (rc) return rc;
    if (!lin_steps_gen_supported(ctx, kind)) {
        set_error("vaek_train_steps_gen: needs a context vaek_train_steps' persistent form covers and dataset kind 0 or 2 (use vaek_train_step_gen)");
        return VAEK_ERR_INVALID;
    }
    BatchArgs gen;
    if ((rc = check_train_draw("vaek_train_steps_gen", ctx, kind, A, dd, did, pad, var_added, row0, seed, step_dev, tag, &gen)) ||
        (rc = check_ws(ctx, workspace)))
        return rc;
    if (n_steps == 0) return VAEK_OK;
    return lin_train_steps_gen(ctx, params, grads, m, v, step_dev, gen, n_steps, lr, workspace, (hipStream_t)stream);
}

int vaek_supports_train_loop_gen(const vaek_ctx* ctx, int32_t kind, int32_t* yes) {
    if (!ctx || !yes) { set_error("null argument"); return VAEK_ERR_INVALID; }
    *yes = ctx->resident && kind >= 0 && kind <= 2 ? 1 : 0;
    return VAEK_OK;
}

int vaek_train_loop_steps_per_launch(void) { return resident_steps_per_launch(); }

int vaek_train_loop_max_replicas(void) { return resident_max_replicas(); }

int vaek_train_loop_replicas_workspace_bytes(const vaek_ctx* ctx, int32_t n, size_t* bytes) {
    if (!ctx || !bytes || n < 1 || n > resident_max_replicas()) {
        set_error("vaek_train_loop_replicas_workspace_bytes: null argument, or n outside 1 .. %d", resident_max_replicas());
        return VAEK_ERR_INVALID;
    }
    *bytes = ctx->resident ? resident_replicas_workspace_bytes(ctx, n) : 0;
    return VAEK_OK;
}

// ---- the trajectory ring of the resident loop: vaek_train_loop_gen_traj, vaek_train_loop_gen_replicas_traj ---------------------------
int vaek_trajectory_record_len(const vaek_ctx* ctx, int64_t* floats) {
    if (!ctx || !floats) { set_error("vaek_trajectory_record_len: null argument"); return VAEK_ERR_INVALID; }
    *floats = 2 * (int64_t)ctx->P + kExtra;
    return VAEK_OK;
}

static const char* const kLoopNeeds = "needs a single-GPU float32 linear VAE (no hidden layers, one or two decoders) with D, L <= 32 and "
                                      "1 <= batch <= 256 (see vaek_supports_train_loop_gen; else vaek_train_step_gen)";

// A vaek_trajectory checked against the context (`replicas`: the replica form, where replica_stride counts) and turned into the
// kernel's TrajArgs: after it every store of the launch lands inside the caller's ring.  Needs a non-null context; its struct_size
// was checked before the context (eval_check.h).
static int check_trajectory(const char* who, const vaek_ctx* ctx, const vaek_trajectory* traj, bool replicas, TrajArgs* out) {
    const int64_t len = 2 * (int64_t)ctx->P + kExtra;
    if (traj->every < 1) { set_error("%s: trajectory every = %d, need >= 1", who, traj->every); return VAEK_ERR_INVALID; }
    if (traj->cap < 1) { set_error("%s: trajectory cap = %lld, need >= 1", who, (long long)traj->cap); return VAEK_ERR_INVALID; }
    if (!traj->buf) { set_error("%s: trajectory buf is NULL", who); return VAEK_ERR_INVALID; }
    if (traj->record_stride < len) {
        set_error("%s: trajectory record_stride %lld < record length %lld (vaek_trajectory_record_len)", who, (long long)traj->record_stride,
                  (long long)len);
        return VAEK_ERR_INVALID;
    }
    if (traj->cap > INT64_MAX / traj->record_stride) {
        set_error("%s: trajectory cap %lld * record_stride %lld overflows", who, (long long)traj->cap, (long long)traj->record_stride);
        return VAEK_ERR_INVALID;
    }
    if (replicas && traj->replica_stride < traj->cap * traj->record_stride) {
        set_error("%s: trajectory replica_stride %lld < cap * record_stride = %lld", who, (long long)traj->replica_stride,
                  (long long)(traj->cap * traj->record_stride));
        return VAEK_ERR_INVALID;
    }
    out->buf = traj->buf; out->every = traj->every; out->cap = traj->cap; out->record_stride = traj->record_stride;
    out->replica_stride = replicas ? traj->replica_stride : 0;
    return VAEK_OK;
}

// The two loop pairs: the traced entry is the implementation, and traj == nullptr the untraced one, answering in its own name
int vaek_train_loop_gen_replicas_traj(vaek_ctx* ctx, float* params, float* grads, float* m, float* v, int32_t* step_dev,
                                      const vaek_replicas* rep, int32_t kind, const float* A, int32_t dd, int32_t did, int32_t pad,
                                      float var_added, int64_t row0, uint32_t tag, int32_t n_steps, float lr, void* workspace, void* stream,
                                      const vaek_trajectory* traj) {
    ProfBind pb(ctx);
    const char* const who = traj ? "vaek_train_loop_gen_replicas_traj" : "vaek_train_loop_gen_replicas";
    const ReplicaRules rules{ctx && ctx->resident, kLoopNeeds, resident_max_replicas(), "vaek_train_loop_max_replicas", false, true};
    int rc = check_replicas(who, ctx, params, grads, m, v, step_dev, n_steps, rep, traj, rules);
    TrajArgs tj{};
    BatchArgs gen;      // (the kernel puts seeds[r] in place of the seed)
    if (rc || (traj && (rc = check_trajectory(who, ctx, traj, true, &tj))) ||
        (rc = check_train_draw(who, ctx, kind, A, dd, did, pad, var_added, row0, 0, step_dev, tag, &gen)))
        return rc;
    const size_t ws_bytes = resident_replicas_workspace_bytes(ctx, rep->n);
    if (ws_bytes && (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15))) {
        set_error("%s: this context stages its batches in memory: workspace must be a 16-byte aligned device "
                  "pointer of vaek_train_loop_replicas_workspace_bytes() = %zu bytes", who, ws_bytes);
        return VAEK_ERR_INVALID;
    }
    if (n_steps == 0) return VAEK_OK;
    return resident_train_loop(ctx, params, grads, m, v, step_dev, gen, n_steps, lr, workspace, (hipStream_t)stream, rep, traj ? &tj : nullptr);
}

int vaek_train_loop_gen_replicas(vaek_ctx* ctx, float* params, float* grads, float* m, float* v, int32_t* step_dev,
                                 const vaek_replicas* rep, int32_t kind, const float* A, int32_t dd, int32_t did, int32_t pad,
                                 float var_added, int64_t row0, uint32_t tag, int32_t n_steps, float lr, void* workspace, void* stream) {
    return vaek_train_loop_gen_replicas_traj(ctx, params, grads, m, v, step_dev, rep, kind, A, dd, did, pad, var_added, row0, tag, n_steps, lr,
                                             workspace, stream, nullptr);
}

int vaek_train_loop_gen_traj(vaek_ctx* ctx, float* params, float* grads, float* m, float* v, int32_t* step_dev, int32_t kind, const float* A,
                             int32_t dd, int32_t did, int32_t pad, float var_added, int64_t row0, uint64_t seed, uint32_t tag, int32_t n_steps,
                             float lr, void* workspace, void* stream, const vaek_trajectory* traj) {
    ProfBind pb(ctx);
    const char* const who = traj ? "vaek_train_loop_gen_traj" : "vaek_train_loop_gen";
    int rc = traj ? check_struct_size(who, "vaek_trajectory", traj->struct_size, sizeof(vaek_trajectory)) : VAEK_OK;
    if (rc || (rc = check_train_state(who, ctx, params, grads, m, v, step_dev, n_steps))) return rc;
    if (!ctx->resident) { set_error("%s: %s", who, kLoopNeeds); return VAEK_ERR_INVALID; }
    TrajArgs tj{};
    BatchArgs gen;
    if ((traj && (rc = check_trajectory(who, ctx, traj, false, &tj))) ||
        (rc = check_train_draw(who, ctx, kind, A, dd, did, pad, var_added, row0, seed, step_dev, tag, &gen)) || (rc = check_ws(ctx, workspace)))
        return rc;
    if (n_steps == 0) return VAEK_OK;
    return resident_train_loop(ctx, params, grads, m, v, step_dev, gen, n_steps, lr, workspace, (hipStream_t)stream, nullptr, traj ? &tj : nullptr);
}

int vaek_train_loop_gen(vaek_ctx* ctx, float* params, float* grads, float* m, float* v, int32_t* step_dev, int32_t kind, const float* A,
                        int32_t dd, int32_t did, int32_t pad, float var_added, int64_t row0, uint64_t seed, uint32_t tag, int32_t n_steps,
                        float lr, void* workspace, void* stream) {
    return vaek_train_loop_gen_traj(ctx, params, grads, m, v, step_dev, kind, A, dd, did, pad, var_added, row0, seed, tag, n_steps, lr, workspace,
                                    stream, nullptr);
}

// ---- the replica form of the mlp3 step (fused_mlp3.hip): n models of one shape per step, blockIdx.y = replica ----------------------
int vaek_supports_train_step_replicas(const vaek_ctx* ctx, int32_t* yes) {
    if (!ctx || !yes) { set_error("null argument"); return VAEK_ERR_INVALID; }
    *yes = ctx->mlp3 && ctx->cfg.world == 1 ? 1 : 0;
    return VAEK_OK;
}

int vaek_train_step_max_replicas(void) { return mlp3_max_replicas(); }

int vaek_train_step_replicas_workspace_bytes(const vaek_ctx* ctx, int32_t n, size_t* bytes) {
    if (!ctx || !bytes || n < 1 || n > mlp3_max_replicas()) {
        set_error("vaek_train_step_replicas_workspace_bytes: null argument, or n outside 1 .. %d", mlp3_max_replicas());
        return VAEK_ERR_INVALID;
    }
    *bytes = ctx->mlp3 && ctx->cfg.world == 1 ? mlp3_replicas_workspace_bytes(ctx, n) : 0;
    return VAEK_OK;
}

int vaek_train_step_gen_replicas(vaek_ctx* ctx, float* params, float* grads, float* m, float* v, int32_t* step_dev,
                                 const vaek_replicas* rep, const float* x, const float* z1, const float* z2, float lr, void* workspace,
                                 int32_t kind, const float* A, int32_t dd, int32_t did, int32_t pad, float var_added, float* x_next,
                                 float* z1_next, float* z2_next, int64_t row0, int32_t* counter, int32_t which, uint32_t tag, void* stream) {
    ProfBind pb(ctx);
    const char* const fn = "vaek_train_step_gen_replicas";
    const int n_next = (x_next ? 1 : 0) + (z1_next ? 1 : 0) + (z2_next ? 1 : 0);      // 3: the drawing form, which reads seeds and counter
    const ReplicaRules rules{ctx && ctx->mlp3 && ctx->cfg.world == 1,
                             "needs a single-GPU context whose train step path is \"mlp3\" (see vaek_supports_train_step_replicas)",
                             mlp3_max_replicas(), "vaek_train_step_max_replicas", true, n_next == 3};
    int rc = check_replicas(fn, ctx, params, grads, m, v, step_dev, 0, rep, nullptr, rules);
    if (rc || (rc = check_given(fn, "x", x, "z1", z1, "z2", z2))) return rc;
    if (n_next != 0 && n_next != 3) {
        set_error("%s: x_next, z1_next and z2_next must be all NULL (no draw) or all given", fn);
        return VAEK_ERR_INVALID;
    }
    if (n_next && (rc = check_given(fn, "counter", counter))) return rc;
    if (n_next && (x_next == x || z1_next == z1 || z2_next == z2)) {
        set_error("%s: the next batch must not alias the current one", fn);
        return VAEK_ERR_INVALID;
    }
    if (dd > 16 || did > 16) { set_error("%s: dd %d or did %d > 16", fn, dd, did); return VAEK_ERR_INVALID; }
    BatchArgs gen;      // a draw to memory: vaek_make_batch_next's check, under its name (the kernel puts seeds[r] in place of the seed)
    if (n_next && (rc = make_batch_args(ctx, kind, A, dd, did, pad, var_added, x_next, z1_next, z2_next, ctx->B, row0, 0, nullptr, 0, counter, which, tag, &gen)))
        return rc;
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15)) {
        set_error("%s: workspace must be a 16-byte aligned device pointer of vaek_train_step_replicas_workspace_bytes() = %zu bytes", fn,
                  mlp3_replicas_workspace_bytes(ctx, rep->n));
        return VAEK_ERR_INVALID;
    }
    return mlp3_train_step_replicas(ctx, params, grads, m, v, step_dev, x, z1, z2, lr, workspace, (hipStream_t)stream, n_next ? &gen : nullptr, *rep);
}

int vaek_train_steps_moment_len(const vaek_ctx* ctx, int64_t* len) {
    if (!ctx || !len) { set_error("null argument"); return VAEK_ERR_INVALID; }
    *len = ctx->lin.NO;
    return VAEK_OK;
}

int vaek_train_steps_moments(vaek_ctx* ctx, const float* x, const float* z1, const float* z2, double* M, void* workspace, void* stream) {
    ProfBind pb(ctx);
    if (!ctx || !x || !z1 || !z2 || !M) { set_error("vaek_train_steps_moments: null argument"); return VAEK_ERR_INVALID; }
    if (!ctx->lin.ok) { set_error("vaek_train_steps_moments: not a float32 linear VAE with L + 2 D + 1 <= 64"); return VAEK_ERR_INVALID; }
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(z1) | reinterpret_cast<uintptr_t>(z2)) & 15) {
        set_error("vaek_train_steps_moments: batch pointers must be 16-byte aligned");
        return VAEK_ERR_INVALID;
    }
    int rc = check_ws(ctx, workspace);
    if (rc) return rc;
    return lin_moments(ctx, x, z1, z2, M, workspace, (hipStream_t)stream);
}

int vaek_train_steps_update(vaek_ctx* ctx, float* params, float* grads, float* m, float* v, int32_t* step_dev, const double* M, float lr,
                            void* workspace, void* stream) {
    ProfBind pb(ctx);
    if (!ctx || !params || !grads || !m || !v || !step_dev || !M) { set_error("vaek_train_steps_update: null argument"); return VAEK_ERR_INVALID; }
    if (!ctx->lin.ok) { set_error("vaek_train_steps_update: not a float32 linear VAE with L + 2 D + 1 <= 64"); return VAEK_ERR_INVALID; }
    int rc = check_ws(ctx, workspace);
    if (rc) return rc;
    return lin_update(ctx, params, grads, m, v, step_dev, M, lr, (hipStream_t)stream);
}

int vaek_train_steps_status(vaek_ctx* ctx, void* workspace, int32_t* gave_up) {
    if (!ctx || !workspace || !gave_up) { set_error("null argument"); return VAEK_ERR_INVALID; }
    int g = 0;
    const int rc = lin_steps_status(ctx, workspace, &g);
    *gave_up = g;
    return rc;
}

// buckets in the order the backward pass completes them: Decoder (last layer first), SigDecoder, Encoder, tail
static void bucket_list(const vaek_ctx* c, std::vector<std::pair<int64_t, int64_t>>& out) {
    out.clear();
    if (c->fused) { out.push_back({0, c->P + kExtra}); return; }
    for (const Net* net : {&c->dec, &c->sig, &c->enc})
        for (int i = (int)net->layers.size() - 1; i >= 0; --i) {
            const auto& l = net->layers[i];
            out.push_back({l.w_off, (int64_t)(l.n_in + 1) * l.n_out});
        }
    out.push_back({c->off_epsp, c->P + kExtra - c->off_epsp});
}

int vaek_bucket_count(const vaek_ctx* ctx, int32_t* n) {
    if (!ctx || !n) { set_error("null argument"); return VAEK_ERR_INVALID; }
    std::vector<std::pair<int64_t, int64_t>> b;
    bucket_list(ctx, b);
    *n = (int32_t)b.size();
    return VAEK_OK;
}

int vaek_bucket_info(const vaek_ctx* ctx, int32_t i, int64_t* offset, int64_t* count) {
    if (!ctx || !offset || !count) { set_error("null argument"); return VAEK_ERR_INVALID; }
    std::vector<std::pair<int64_t, int64_t>> b;
    bucket_list(ctx, b);
    if (i < 0 || i >= (int32_t)b.size()) { set_error("bucket index out of range"); return VAEK_ERR_INVALID; }
    *offset = b[i].first; *count = b[i].second;
    return VAEK_OK;
}

int vaek_train_step_grads_bucketed(vaek_ctx* ctx, const float* params, float* grads, int32_t* step_dev, const float* x,
                                   const float* z1, const float* z2, void* const* ready_events, void* workspace, void* stream) {
    ProfBind pb(ctx);
    if (!ctx || !params || !grads || !step_dev || !x || !z1 || !z2 || !ready_events) { set_error("vaek_train_step_grads_bucketed: null argument"); return VAEK_ERR_INVALID; }
    int rc = check_ws(ctx, workspace);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (ctx->fused) {
        if ((rc = whole_step(ctx, const_cast<float*>(params), grads, nullptr, nullptr, step_dev, x, z1, z2, 0.f, false, false,
                             workspace, st)))
            return rc;
        VAEK_HIP_CHECK(hipEventRecord((hipEvent_t)ready_events[0], st));
        return VAEK_OK;
    }
    BucketSink sink{grads, ready_events, 0};
    if ((rc = generic_grads(ctx, params, step_dev, x, z1, z2, workspace, st, &sink))) return rc;
    // tail: epsilon_p, epsilon and the loss slots (everything the layer buckets did not cover)
    if ((rc = generic_finalize(ctx, params, grads, nullptr, nullptr, nullptr, nullptr, 0.f, workspace, st, ctx->off_epsp))) return rc;
    VAEK_HIP_CHECK(hipEventRecord((hipEvent_t)ready_events[sink.next], st));
    return VAEK_OK;
}

int vaek_loss_eval(vaek_ctx* ctx, const float* params, const float* x, const float* z1, const float* z2, float* out4,
                   void* workspace, void* stream) {
    ProfBind pb(ctx);
    if (!ctx || !params || !x || !z1 || !z2 || !out4) { set_error("vaek_loss_eval: null argument"); return VAEK_ERR_INVALID; }
    int rc = check_ws(ctx, workspace);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    vaek_ctx* c = ctx;
    const bool sig = c->cfg.sigmoid_decoder != 0;
    if ((rc = convert_weights(c, params, workspace, st))) return rc;
    if ((rc = net_forward(c, c->enc, params, x, workspace, c->B, true, z1, st))) return rc;
    const float* samples = at<float>(workspace, c->ws_samples);
    if ((rc = net_forward(c, c->dec, params, samples, workspace, c->B, false, nullptr, st))) return rc;
    if (sig && (rc = net_forward(c, c->sig, params, samples, workspace, c->B, false, nullptr, st))) return rc;
    ElboArgs e{};
    e.x = x; e.y_lin = at<float>(workspace, c->dec.act_off.back());
    e.y_sig = sig ? at<float>(workspace, c->sig.act_off.back()) : nullptr;
    e.z2 = z2; e.mu = at<float>(workspace, c->enc.act_off.back());
    e.eps_param = c->off_eps >= 0 ? params + c->off_eps : nullptr; e.eps_cli = c->cfg.eps_cli;
    e.partial = at<float>(workspace, c->ws_epart);
    e.rows = c->B; e.D = c->D; e.L = c->L; e.S = c->Se; e.rows_per_split = c->rows_per_esplit;
    e.inv_bt = (float)(1.0 / (double)c->B);     // VAE.loss is a plain mean over the eval batch
    if ((rc = launch_elbo(e, st))) return rc;
    return launch_eval_out4(e.partial, c->Se, params, c->off_epsp, c->off_eps, c->L, c->D, c->cfg.eps_cli, (float)c->B,
                            e.inv_bt, out4, st);
}

int vaek_forward(vaek_ctx* ctx, const float* params, const float* x, const float* z1, const float* z2,
                 int32_t sampling, float eps, float* x_hat, float* mu_out, int32_t rows, void* workspace, void* stream) {
    ProfBind pb(ctx);
    if (!ctx || !params || !z1 || !z2 || !x_hat || (!sampling && !x) || rows <= 0) { set_error("vaek_forward: invalid argument"); return VAEK_ERR_INVALID; }
    if (rows > ctx->B) { set_error("vaek_forward: rows %d exceed this context's batch %d", rows, ctx->B); return VAEK_ERR_WORKSPACE; }
    int rc = check_ws(ctx, workspace);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    vaek_ctx* c = ctx;
    const bool sig = c->cfg.sigmoid_decoder != 0;
    const float* samples = z1;                      // sampling: mu = 0, logvar_e = 0 -> samples = z1
    if ((rc = convert_weights(c, params, workspace, st))) return rc;
    if (!sampling) {
        if ((rc = net_forward(c, c->enc, params, x, workspace, rows, true, z1, st))) return rc;
        samples = at<float>(workspace, c->ws_samples);
        if (mu_out)
            VAEK_HIP_CHECK(hipMemcpyAsync(mu_out, at<float>(workspace, c->enc.act_off.back()),
                                          (size_t)rows * c->L * sizeof(float), hipMemcpyDeviceToDevice, st));
    } else if (mu_out) {
        VAEK_HIP_CHECK(hipMemsetAsync(mu_out, 0, (size_t)rows * c->L * sizeof(float), st));
    }
    if ((rc = net_forward(c, c->dec, params, samples, workspace, rows, false, nullptr, st))) return rc;
    if (sig && (rc = net_forward(c, c->sig, params, samples, workspace, rows, false, nullptr, st))) return rc;
    const float* eps_param = (!sampling && c->off_eps >= 0) ? params + c->off_eps : nullptr;
    const float eps_val = sampling ? eps : c->cfg.eps_cli;
    return launch_add_noise(at<float>(workspace, c->dec.act_off.back()),
                            sig ? at<float>(workspace, c->sig.act_off.back()) : nullptr, z2, eps_param, eps_val, x_hat,
                            (int64_t)rows * c->D, st);
}

// Diagnostic hook (not part of include/vaek.h): device buffer for the in-kernel s_memtime stamps of
// a -DVAEK_STAMPS build (tools/stamps.sh).  No effect in the shipped build.
int vaek_debug_set_stamps(vaek_ctx* ctx, unsigned long long* buf) {
    if (!ctx) return VAEK_ERR_INVALID;
    ctx->dbg_stamps = buf;
    return VAEK_OK;
}

int vaek_profile_begin(vaek_ctx* ctx, int32_t max_records) {
    if (!ctx || max_records <= 0) { set_error("vaek_profile_begin: invalid argument"); return VAEK_ERR_INVALID; }
    Profiler& p = ctx->prof;
    while ((int)p.ev.size() < 2 * max_records) {
        hipEvent_t e;
        VAEK_HIP_CHECK(hipEventCreate(&e));
        p.ev.push_back(e);
    }
    p.label.assign(max_records, nullptr);
    p.cap = max_records; p.n = 0; p.on = true;
    return VAEK_OK;
}

int vaek_profile_report(vaek_ctx* ctx, char* buf, size_t cap) {
    if (!ctx || !buf || cap < 8) { set_error("vaek_profile_report: invalid argument"); return VAEK_ERR_INVALID; }
    Profiler& p = ctx->prof;
    p.on = false;
    std::vector<std::string> names;
    std::vector<double> total;
    std::vector<int> count;
    for (int i = 0; i < p.n; ++i) {
        VAEK_HIP_CHECK(hipEventSynchronize(p.ev[2 * i + 1]));
        float ms = 0.f;
        VAEK_HIP_CHECK(hipEventElapsedTime(&ms, p.ev[2 * i], p.ev[2 * i + 1]));
        size_t k = 0;
        for (; k < names.size(); ++k) if (names[k] == p.label[i]) break;
        if (k == names.size()) { names.push_back(p.label[i]); total.push_back(0); count.push_back(0); }
        total[k] += ms; count[k] += 1;
    }
    std::string js = "{";
    for (size_t k = 0; k < names.size(); ++k) {
        char tmp[160];
        snprintf(tmp, sizeof(tmp), "%s\"%s\": {\"count\": %d, \"total_ms\": %.6f}", k ? ", " : "", names[k].c_str(), count[k], total[k]);
        js += tmp;
    }
    js += "}";
    if (js.size() + 1 > cap) { set_error("vaek_profile_report: buffer too small"); return VAEK_ERR_INVALID; }
    memcpy(buf, js.c_str(), js.size() + 1);
    p.n = 0;
    return VAEK_OK;
}

}  // extern "C"
