// Internal declarations shared by the translation units of libvaek.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

#include "../../include/vaek.h"

namespace vaek {

constexpr int kExtra = 4;          // grads[P..P+3] = loss, mean Dkl, mean mse, 0
constexpr float kLog2Pi = 1.8378770664093453f;
constexpr float kAdamB1 = 0.9f, kAdamB2 = 0.999f, kAdamEps = 1e-8f;

void set_error(const char* fmt, ...);
#define VAEK_HIP_CHECK(expr)                                                              \
    do {                                                                                  \
        hipError_t _e = (expr);                                                           \
        if (_e != hipSuccess) {                                                           \
            vaek::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return VAEK_ERR_HIP;                                                          \
        }                                                                                 \
    } while (0)

struct Leaf {
    std::string name;
    int64_t offset;
    int rows, cols;   // bias / epsilon_p / epsilon: rows == 1
};

// Which kernels one Dense layer of the layer-by-layer step runs (dense_kind, once per layer in vaek_ctx_create).  A stack in
// bf16-STORAGE mode (net_is_b16: dtype = VAEK_BF16, >= 2 hidden layers, every hidden width b16_width) keeps its hidden
// activations and gradients as bf16; its first and last layers have one bf16-stored side.
enum class Kind : uint8_t {
    F32,          // gemm_f32.hip
    BF16,         // gemm_bf16.hip: bf16 arithmetic on f32 storage (dtype = VAEK_BF16, both widths >= 64, not a b16 stack)
    FIRST_SK,     // first layer of a b16 stack, d -> H with sk_supported(d, H): gemm_skinny16.hip
    FIRST16,      // ... otherwise: gemm_f32.hip's *_out16 / dw_dy16 / dx_in16 forms
    HIDDEN16,     // hidden -> hidden layer of a b16 stack: gemm_bf16s.hip
    LAST_SK,      // last layer of a b16 stack, H -> d with sk_supported(d, H): gemm_skinny16.hip
    LAST16,       // ... otherwise: gemm_f32.hip's *_in16 / dx_out16 / dw_x16 forms
};
enum class Pos : uint8_t { FIRST, HIDDEN, LAST };

struct Layer {
    int n_in, n_out;
    int64_t w_off;    // kernel offset in the flat buffers; bias follows at w_off + n_in*n_out
    bool relu;        // relu after this layer (every layer but the last, networks.py:35-39)
    Kind kind = Kind::F32;
    int S, rows_per_split;   // batch split of this layer's dW|db launch (one rule per kind)
    int64_t w16_off = 0;     // element offset of its bf16 kernel copies: HIDDEN16 W, then W^T in ws_wb16; *_SK the padded copy in ws_sk16
};

struct Net {
    std::vector<Layer> layers;
    // workspace byte offsets of each layer's OUTPUT activation [B, n_out] (float32; bf16 for the hidden layers of a b16 net)
    std::vector<size_t> act_off;
};

// Event-pair pool for vaek_profile_*: one pair per kernel launch while enabled.
struct Profiler {
    bool on = false;
    std::vector<hipEvent_t> ev;          // 2 * max_records
    std::vector<const char*> label;      // per record
    int n = 0, cap = 0;
};
extern thread_local Profiler* g_prof;    // set by the C entry points for the duration of a call
// One launch = one event pair, handed to hipExtLaunchKernelGGL so the timestamps are the kernel's own
// begin/end (what rocprofv3 reports), not host-side record times (which would count submission gaps
// into the ~5-10 us kernels of the metric workload).
struct ProfScope {
    int idx = -1;
    ProfScope(const char* label, hipStream_t) {
        Profiler* p = g_prof;
        if (p && p->on && p->n < p->cap) { idx = p->n++; p->label[idx] = label; }
    }
    hipEvent_t start() const { return g_prof->ev[2 * idx]; }
    hipEvent_t stop() const { return g_prof->ev[2 * idx + 1]; }
};
}  // namespace vaek
#include <hip/hip_ext.h>
namespace vaek {
template <typename K, typename... Args>
inline void launch_k(const ProfScope& ps, K kernel, dim3 grid, dim3 block, size_t shmem, hipStream_t st, Args... args) {
    if (ps.idx >= 0) hipExtLaunchKernelGGL(kernel, grid, block, shmem, st, ps.start(), ps.stop(), 0, args...);
    else hipLaunchKernelGGL(kernel, grid, block, shmem, st, args...);
}

struct Comm {
    bool ready = false;
    void* local = nullptr;      // uncached granule buffer of this rank (hipExtMallocWithFlags)
    size_t bytes = 0;
    int ng = 0;                 // granules per (bank, source rank)
    std::vector<void*> peers;   // world entries; peers[rank] == local, others IPC-mapped
    uint32_t epoch = 0;         // stand-alone all-reduce epochs (region 1)
    size_t lin_off = 0, lin_bytes = 0;   // the moment-exchange region of vaek_train_steps (linear_moments.hip), behind the status line
};

// How vaek_train_steps runs this context (linear_moments.hip: lin_plan, once in vaek_ctx_create).  All zero unless ok.
struct LinPlan {
    bool ok = false;                  // the moment form covers the model: float32 linear VAE, L + 2 D + 1 <= 64, B min(D, L) >= 8
    int NB = 0, NO = 0;               // 16-feature blocks of the instantiation (3 or 4); doubles in a moment image
    int T = 0, ntiles = 0;            // samples per tile, tiles per batch
    bool persist = false;             // the persistent form applies
    int n_stream = 0, n_reduce = 0;   // its streamer / reducer workgroups
    size_t lds_persist = 0, lds_step = 0;      // dynamic LDS of the persistent / launch-per-step form
    int which_persist = 0, which_step = 0;     // instantiation: 0 / 2 the metric's D = 12, L = 20 at compile time, else run-time (step: NB - 3;
                                               // persistent: 1 three blocks, 2 four blocks, 3 M20's D = 20, L = 20 at compile time)
    size_t M_off = 0, partial_off = 0, ws_bytes = 0;   // within the context's workspace region at ws_lin
    size_t comm_bytes = 0;            // the moment-exchange region of the P2P communicator's buffer (world > 1, persistent form)
};

}  // namespace vaek

struct vaek_ctx {
    vaek_config cfg;
    int B, D, L;
    int64_t Bt;                      // global batch (divisor of the mean)
    int64_t P;                       // trainable floats
    std::vector<vaek::Leaf> leaves;
    vaek::Net enc, dec, sig;         // sig empty unless cfg.sigmoid_decoder
    int64_t off_epsp, off_eps;       // flat offsets; off_eps = -1 without -tdv
    // batch split of the deterministic reductions: S slabs for the dW|db GEMMs, Se for elementwise
    int S, rows_per_split, Se, rows_per_esplit;
    bool fused;                      // a whole-network path is available and selected (fused_small / fused_mfma / fused_mlp1 / fused_mlp3)
    bool mlp3 = false;               // ... and it is fused_mlp3.hip's (three hidden layers both ways, small batch)
    bool resident = false;           // vaek_train_loop_gen covers this context (linear_resident.hip: resident_supported)
    bool mlp3_loglik = false;        // vaek_mlp3_log_likelihood_replicas covers this context (mlp3_loglik.hip: mlp3_loglik_supported)
    // workspace layout (bytes)
    size_t ws_samples, ws_dsamp, ws_gbuf0, ws_gbuf1, ws_slabs, ws_epart, ws_epart_blk, ws_rpart, ws_eblk, ws_fused, ws_mlp3, ws_wb16, ws_sk16, ws_skpart, ws_lin, ws_lwd, ws_resident, ws_total;
    bool lwd = false; int lwd_rb = 0;           // wide linear decoder: fused forward / ELBO / backward (linear_wide.hip), rows per row block
    int max_width;
    int n_cu;
    vaek::Comm comm;
    vaek::Profiler prof;
    unsigned long long* dbg_stamps = nullptr;   // diagnostic builds (-DVAEK_STAMPS) only
    float* loss_hist = nullptr;                 // optional device ring: loss of Adam step t -> [(t-1) % cap]
    int64_t loss_hist_cap = 0;
    vaek::LinPlan lin;
    void* lin_ws_issued = nullptr;              // workspace for which an init of vaek_train_steps' arrival counters was launched or captured
    void* lin_ws_ready = nullptr;               // ... and has run in stream order; cleared when the counters are in doubt (linear_moments.hip)
};

namespace vaek {

struct ProfBind {   // entry points bind the context's profiler for the duration of the call
    explicit ProfBind(vaek_ctx* c) { g_prof = c ? &c->prof : nullptr; }
    ~ProfBind() { g_prof = nullptr; }
};

// ---- gemm_f32.hip -------------------------------------------------------------------------
int launch_dense_fwd(const float* x, const float* w, const float* b, float* y, int rows, int n_in,
                     int n_out, bool relu, hipStream_t st);
// y = mu (stored), samples = mu + exp(lv/2) * z1
int launch_dense_fwd_reparam(const float* x, const float* w, const float* b, float* mu, float* samples,
                             const float* z1, const float* lv, int rows, int n_in, int n_out, hipStream_t st);
int launch_dense_bwd_dx(const float* dy, const float* w, const float* x_post, float* dx, int rows,
                        int n_in, int n_out, bool relu, bool accumulate, hipStream_t st);
// writes S slabs: slab[s][row*n_out + col], row in [0, n_in] (row n_in = bias), stride in floats
int launch_dense_bwd_dw(const float* x, const float* dy, float* slab0, int64_t slab_stride, int S,
                        int rows_per_split, int rows, int n_in, int n_out, hipStream_t st);

// ---- gemm_bf16.hip: the same four launchers with bf16 matrix-core arithmetic (f32 storage) -----------
int launch_dense_fwd_bf16(const float* x, const float* w, const float* b, float* y, int rows, int n_in, int n_out,
                          bool relu, hipStream_t st);
int launch_dense_fwd_reparam_bf16(const float* x, const float* w, const float* b, float* mu, float* samples,
                                  const float* z1, const float* lv, int rows, int n_in, int n_out, hipStream_t st);
int launch_dense_bwd_dx_bf16(const float* dy, const float* w, const float* x_post, float* dx, int rows, int n_in,
                             int n_out, bool relu, bool accumulate, hipStream_t st);
int launch_dense_bwd_dw_bf16(const float* x, const float* dy, float* slab0, int64_t slab_stride, int S, int rows_per_split,
                             int rows, int n_in, int n_out, hipStream_t st);

// ---- bf16-STORAGE mode (hidden activations / gradients kept as bf16 in HBM) ------------------------------------------
// gemm_f32.hip: the skinny first / last layer of a stack on the exact f32 kernel, hidden-side operand stored as bf16
int launch_dense_fwd_out16(const float* x, const float* w, const float* b, __bf16* y, int rows, int n_in, int n_out, bool relu,
                           hipStream_t st);
int launch_dense_fwd_in16(const __bf16* x, const float* w, const float* b, float* y, int rows, int n_in, int n_out, hipStream_t st);
int launch_dense_fwd_reparam_in16(const __bf16* x, const float* w, const float* b, float* mu, float* samples, const float* z1,
                                  const float* lv, int rows, int n_in, int n_out, hipStream_t st);
int launch_dense_fwd_elbo_in16(const __bf16* h, const float* w, const float* b, float* d_out, const float* x, const float* z2,
                               const float* eps_param, float eps_cli, float inv_bt, float* part, int rows, int n_in, int n_out,
                               int* bm, int* nbx, hipStream_t st);
int launch_dense_bwd_dx_out16(const float* dy, const float* w, const __bf16* x_post, __bf16* dx, int rows, int n_in, int n_out,
                              bool accumulate, hipStream_t st);
int launch_dense_bwd_dw_x16(const __bf16* x, const float* dy, float* slab0, int64_t slab_stride, int S, int rows_per_split,
                            int rows, int n_in, int n_out, hipStream_t st);
int launch_dense_bwd_dw_dy16(const float* x, const __bf16* dy, float* slab0, int64_t slab_stride, int S, int rows_per_split,
                             int rows, int n_in, int n_out, hipStream_t st);
int launch_dense_bwd_dx_in16(const __bf16* dy, const float* w, float* dx, int rows, int n_in, int n_out, bool accumulate,
                             hipStream_t st);
// gemm_bf16s.hip: the wide hidden -> hidden layers, bf16 in / bf16 out on v_mfma_f32_32x32x16_bf16
int launch_hs_fwd(const __bf16* x, const __bf16* wT, const float* b, __bf16* y, int rows, int n_in, int n_out, bool relu,
                  hipStream_t st);
int launch_hs_dx(const __bf16* dy, const __bf16* w16, const __bf16* x_post, __bf16* dx, int rows, int n_in, int n_out,
                 hipStream_t st);
int launch_hs_dw(const __bf16* x, const __bf16* dy, float* slab0, int64_t slab_stride, int S, int rows_per_split, int rows,
                 int n_in, int n_out, hipStream_t st);
int launch_cvt_weights(const float* params, __bf16* out, const int* K, const int* N, const int64_t* w_off, const int64_t* out_off,
                       int n, hipStream_t st);

// gemm_skinny16.hip: first (d -> H) / last (H -> d) layer of a bf16-storage stack, d <= 16: one HBM pass per big tensor
bool sk_supported(int d, int H);
inline bool is_sk(Kind k) { return k == Kind::FIRST_SK || k == Kind::LAST_SK; }
inline int sk_d(const Layer& l) { return l.kind == Kind::FIRST_SK ? l.n_in : l.n_out; }      // a skinny layer's d
inline int sk_H(const Layer& l) { return l.kind == Kind::FIRST_SK ? l.n_out : l.n_in; }      // ... and its H
bool sk_bwd_mfma_form(int rows, int H, int d, int S);      // which form launch_sk_last_bwd / launch_sk_first_bwd run
size_t sk_partial_bytes(int d, int H, int S);
int launch_sk_first_fwd(const float* x, const float* w, const float* b, __bf16* y, int rows, int d, int H, bool relu, hipStream_t st);
int launch_sk_last_fwd(const __bf16* h, const __bf16* wp, const float* b, float* y, int rows, int H, int d, hipStream_t st);
int launch_sk_last_fwd_reparam(const __bf16* h, const __bf16* wp, const float* b, float* mu, float* samples, const float* z1,
                               const float* lv, int rows, int H, int d, hipStream_t st);
int launch_sk_last_fwd_elbo(const __bf16* h, const __bf16* wp, const float* b, float* d_out, const float* x, const float* z2,
                            const float* eps_param, float eps_cli, float inv_bt, float* part, int rows, int H, int d, int* bm,
                            int* nbx, hipStream_t st);
int launch_sk_first_dx(const __bf16* dy, const __bf16* wp, float* dx, int rows, int H, int d, bool accumulate, hipStream_t st);
int launch_sk_last_bwd(const __bf16* h, const float* dy, const float* w, __bf16* dh, float* partial, float* slab0, int64_t slab_stride,
                       int S, int rows, int H, int d, hipStream_t st);
int launch_sk_first_bwd(const float* x, const __bf16* dy, float* partial, float* slab0, int64_t slab_stride, int S, int rows, int H,
                        int d, hipStream_t st);
int launch_sk_prep(const float* params, __bf16* out, const int* H, const int* d, const int* transposed, const int64_t* w_off,
                   const int64_t* out_off, int n, hipStream_t st);

// ---- api.hip: a Dense layer's kernels by kind -- the step's and vaek_debug_dense16's only route to the launchers above ----------
inline bool b16_width(int n) { return n % 64 == 0; }      // a hidden width a bf16-storage stack can hold
Kind dense_kind(int dtype, bool b16, Pos pos, int n_in, int n_out);      // pure: no context, no HIP call
struct DenseW {             // a layer's parameters as its kind reads them
    const float* w; const float* b;      // f32 kernel [n_in, n_out] and bias
    const __bf16* w16;                   // HIDDEN16: bf16 W, then W^T (launch_cvt_weights); *_SK: the 32-row padded copy (launch_sk_prep)
};
// the last layer's fused epilogue: the reparameterisation samples = y + exp(lv / 2) z1 (networks.py:73-74), or the decoder's ELBO
// pass (y becomes dL/dx_hat; {mse, d eps} per output tile into part, and the tile map out)
enum class Epi : uint8_t { NONE, REPARAM, ELBO };
struct Epilogue {
    Epi kind;
    float* samples; const float* z1; const float* lv;
    const float* x; const float* z2; const float* eps_param; float eps_cli, inv_bt; float* part; int bm, nbx;
};
// bf16 copies (DenseW::w16) of the HIDDEN16 and *_SK layers among ls[0..n), from params + w_off to wb16 / sk16 + w16_off
int prep_weights(const float* params, const Layer* const* ls, int n, __bf16* wb16, __bf16* sk16, hipStream_t st);
// y = act(x W + b), the epilogue e (nullptr: none) on a last layer
int dense_fwd(const Layer& l, const DenseW& p, const void* x, void* y, int rows, Epilogue* e, hipStream_t st);
// dX = dy W^T, masked where x_post (relu: the f32-storage kinds' switch) is zero, written or added (accumulate)
int dense_dx(const Layer& l, const DenseW& p, const void* dy, const void* x_post, void* dx, int rows, bool relu, bool accumulate,
             hipStream_t st);
// dW|db into l.S slabs (skpart: the skinny kinds' partials); LAST_SK writes its dX too, from the same pass
int dense_dw(const Layer& l, const DenseW& p, const void* x, const void* dy, void* dx, float* slab0, int64_t slab_stride, float* skpart,
             int rows, hipStream_t st);

// ---- elbo.hip -----------------------------------------------------------------------------
struct ElboArgs {
    const float* x; const float* y_lin; const float* y_sig; const float* z2; const float* mu;
    const float* eps_param;   // device (1,) or nullptr
    float eps_cli;            // eps = eps_param ? *eps_param * eps_cli : eps_cli
    float* d_lin; float* d_sig;   // nullptr -> no gradients (eval)
    float* partial;           // [S][4]: +0 = sum mse terms (variable part), +1 = sum mu^2, +2 = d eps sum (variable part)
    int rows, D, L, S, rows_per_split;
    float inv_bt;
    int32_t* step_dev;        // incremented by block 0 (may be nullptr)
};
int launch_elbo(const ElboArgs& a, hipStream_t st);
int launch_elbo_reduce(const float* part, int bm, int nbx, const float* mu, float* partial, int rows, int L, int S,
                       int rows_per_split, int32_t* step_dev, hipStream_t st);
int launch_dense_fwd_elbo(const float* h, const float* w, const float* b, float* d_out, const float* x, const float* z2,
                          const float* eps_param, float eps_cli, float inv_bt, float* part, int rows, int n_in, int n_out,
                          int* bm, int* nbx, hipStream_t st);
// dmu = dsamp + mu * inv_bt (in place on dsamp); partial[s][l] = sum_rows dsamp * z1
int launch_reparam_bwd(float* dsamp, const float* mu, const float* z1, float* partial,
                       int rows, int L, int S, int rows_per_split, float inv_bt, hipStream_t st);
struct FinalizeArgs {
    const float* slabs; int64_t slab_stride; int S;   // dW|db partials in flat-gradient layout (S = max over layers)
    int nseg; int seg_end[32]; int seg_S[32];          // per layer: flat index one past its [kernel|bias], its slab count
    const float* epart; const float* rpart; int Se;   // elbo partials [Se][4], reparam partials [Se][L]
    int64_t P, off_epsp, off_eps; int L, D;
    const float* params;      // for logvar_e / epsilon
    float eps_cli; float rows_over_bt; float inv_bt; float rows;
    float* grads;             // P + 4
    // optional fused Adam (world == 1): params_rw != nullptr
    float* params_rw; float* m; float* v; const int32_t* step_dev; float lr;
    float* loss_hist; long long loss_hist_cap;    // optional: loss of Adam step t -> loss_hist[(t-1) % cap]
    long long lo;             // outputs below lo are left alone (bucketed mode finalises the tail only)
};
int launch_finalize(const FinalizeArgs& a, hipStream_t st);
// streaming slab sum (+ Adam) of the outputs [0, hi); pair with launch_finalize(lo = hi) for the tail
int launch_bulk_finalize(const FinalizeArgs& a, int64_t hi, hipStream_t st);
// api.hip: bulk_finalize over [0, hi) (hi = 0: none), finalize above it (else from a.lo), Adam fused or as its own launch
int finalize_launches(const FinalizeArgs& a, int64_t hi, bool fuse, hipStream_t st);
int launch_adam(float* params, const float* grads, float* m, float* v, int64_t n, float lr, int step,
                const int32_t* step_dev, float grad_scale, hipStream_t st);
// x_hat = y_lin (+ sigmoid(y_sig)) + z2 * exp(eps/2)
int launch_add_noise(const float* y_lin, const float* y_sig, const float* z2, const float* eps_param,
                     float eps_cli, float* x_hat, int64_t n, hipStream_t st);
// stand-alone ELBO finalisation for vaek_elbo_fwd_bwd: out4 = {loss, dkl, mse, d eps}
int launch_elbo_out4(const float* partial, int S, const float* lv, int L, int D, const float* eps_param,
                     float eps, float rows, float inv_bt, float* out4, hipStream_t st);   // eps = eps_param ? eps_param[0] * eps : eps
// eval: out4 = {loss, dkl, mse, eps} from slabs
int launch_eval_out4(const float* partial, int S, const float* params, int64_t off_epsp,
                     int64_t off_eps, int L, int D, float eps_cli, float rows, float inv_bt, float* out4,
                     hipStream_t st);
int launch_sum_slabs(const float* slabs, int64_t stride, int S, float* out, int64_t n, hipStream_t st);
int launch_sum_slabs_inplace(float* slabs, int64_t stride, int S, float* out, int64_t n, hipStream_t st);   // many slabs, few outputs; clobbers the slabs
#ifdef __HIPCC__
int launch_cvt_bf16(const float* src, __bf16* dst, int64_t n, __bf16* zero8, hipStream_t st);
int launch_cvt_bf16_t(const float* src, __bf16* dst, int K, int N, __bf16* zero8, hipStream_t st);
// "Has this been set up on the CURRENT device?" -- hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per device, and a per-thread
// flag skipped it for the second device a thread drives (launches needing > 64 KB of LDS then fail with an invalid value).
struct PerDeviceOnce {
    unsigned long long mask[2] = {0ull, 0ull};          // devices 0 .. 127
    static int slot() { int dev = 0; return hipGetDevice(&dev) == hipSuccess ? (dev & 127) : 0; }
    bool need() const { const int d = slot(); return !(mask[d >> 6] >> (d & 63) & 1ull); }
    void mark() { const int d = slot(); mask[d >> 6] |= 1ull << (d & 63); }
};
// Its use: raise a kernel's dynamic-LDS limit on the current device, the first time `once` sees that device.
template <class Kernel> inline hipError_t set_max_dynamic_lds(PerDeviceOnce& once, Kernel fn, size_t bytes) {
    if (!once.need()) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) once.mark();
    return e;
}
int launch_hs_conv(int mode, const __bf16* x, const __bf16* wb, const __bf16* zeros, const float* bias, const float* mask, const __bf16* mask16,
                   float* out, __bf16* out16, int batch, int H, int W, int Cin, int Cout, bool relu, hipStream_t st);      // mode 0: forward, 1: transposed
int launch_hs_conv_dw(const __bf16* x, const __bf16* dy, const __bf16* zeros, float* slab0, int64_t slab_stride, int S, int rows_per_split,
                      int batch, int H, int W, int Cin, int Cout, hipStream_t st);
#endif

// ---- comm.hip -------------------------------------------------------------------------------
struct CommDev;
CommDev comm_dev(const vaek_ctx* c, int region);

#ifdef __HIPCC__
// flax.optim.Adam.apply_gradient (networks.py:100) for one parameter; (1 - beta) formed in double, as the oracle does
__device__ __forceinline__ void adam_apply_f(float& p, float g, float& m, float& v, float lr, float bc1, float bc2) {
    m = kAdamB1 * m + (float)(1.0 - 0.9) * g;
    v = kAdamB2 * v + (float)(1.0 - 0.999) * g * g;
    p = p - lr * (m / bc1) / (sqrtf(v / bc2) + kAdamEps);
}
#endif

// ---- fused_small.hip / fused_mfma.hip: arguments of the fused linear-VAE kernels ----------------
struct BatchArgs {
    int kind;                   // 0 linear_gaussian, 1 sigmoid, 2 sphere
    const float* A;             // linear: [dd][did] row-major; sigmoid: [dd]; sphere: unused
    int dd, did, pad; float noise_std;
    float* x; float* z1; float* z2;
    int rows; long long row0; int D, L;
    unsigned long long seed; const int32_t* step_dev; unsigned step_host, tag;
    int32_t* counter; int which; // make_batch_next: step = counter[which]; the launch stores counter[which ^ 1] = step + 1
};

struct FusedArgs {
    const float* x; const float* z1; const float* z2;
    float* partials; int pstride;      // [grid][pstride]
    int B, D, L, ntiles;
    float inv_bt, eps_cli;
    int off_be, off_wd, off_bd, off_ws, off_bs, off_epsp, off_eps, P;
    int32_t* step_dev;
    unsigned long long* stamps;        // diagnostic builds only (-DVAEK_STAMPS): [block][wave][8] s_memtime
    // single-launch step (fused_mfma.hip): the batch fits ONE workgroup, so there is nothing to reduce across workgroups
    // and workgroup 0 finalizes itself -- closed-form terms, loss, Adam, step counter; workgroups 1.. (if any) draw the
    // next batch (vaek_train_step_gen): the reference's loop body at its own batch size is one launch
    int single;
    float* grads; float* params_rw; float* m; float* v; float lr, rows_over_bt, rows;
    float* loss_hist; long long loss_hist_cap;
    int has_gen; BatchArgs gen;
};
bool fused_mfma_supported(const vaek_ctx* c);
int fused_mfma_launch(const vaek_ctx* c, const float* params, const void* fused_args, int grid, hipStream_t st);

// ---- linear_moments.hip: N pipelined steps of a linear VAE through the batch's second-moment matrix --------------------
LinPlan lin_plan(const vaek_ctx* c);
bool lin_steps_supported(const vaek_ctx* c);
int lin_train_steps(vaek_ctx* c, float* params, float* grads, float* m, float* v, int32_t* step_dev, const float* const* xs,
                    const float* const* z1s, const float* const* z2s, int n_steps, float lr, void* ws, hipStream_t st);
int lin_steps_status(vaek_ctx* c, void* ws, int* gave_up);
bool lin_steps_gen_supported(const vaek_ctx* c, int kind);
// ---- linear_wide.hip: fused forward / ELBO / backward of a wide linear decoder (BASELINE config 4) ---------------------------
bool lwd_supported(int B, int D, int L);
int lwd_row_block(int B, int D, int n_cu);
size_t lwd_gpart_bytes(int B, int D, int L);
int launch_lwd(const float* samples, const float* Wd, const float* bd, const float* x, const float* z2, const float* eps_param, float eps_cli,
               float inv_bt, float* gpart, float* slab0, int64_t slab_stride, float* part, int B, int D, int L, int RB, hipStream_t st);
int launch_lwd_second(const float* gpart, int ncb, float* dsamp, const float* mu, const float* z1, float* partial, int rows, int L, int S,
                      int rows_per_split, float inv_bt, const float* part, int nblk, float* epartial, int32_t* step_dev, hipStream_t st);
int lin_moments(vaek_ctx* c, const float* x, const float* z1, const float* z2, double* M_out, void* ws, hipStream_t st);
int lin_update(vaek_ctx* c, float* params, float* grads, float* m, float* v, int32_t* step_dev, const double* M_in, float lr, hipStream_t st);
struct BatchArgs;
int lin_train_steps_gen(vaek_ctx* c, float* params, float* grads, float* m, float* v, int32_t* step_dev, const BatchArgs& gen, int n_steps,
                        float lr, void* ws, hipStream_t st);

// ---- linear_resident.hip: N steps of a small-batch linear VAE (one or two decoders) as a loop inside one workgroup -------------
bool resident_supported(const vaek_ctx* c);       // float32, no hidden layers, D, L <= 32, world 1, 1 <= batch <= 256, not force_generic
size_t resident_workspace_bytes(const vaek_ctx* c);   // the region at ws_resident: a batch image where LDS has no room for it
int resident_steps_per_launch();
// The trajectory ring of vaek_train_loop_gen*_traj (a checked vaek_trajectory): the record of Adam step t, t % every == 0, goes to
// buf (+ r * replica_stride) + ((t / every - 1) % cap) * record_stride.  `traj` == nullptr below: the untraced kernels, as before.
struct TrajArgs {
    float* buf;
    int every;
    long long cap, record_stride, replica_stride;
};
// rep != nullptr (a checked vaek_replicas): the same loop for rep->n independent models of the context's shape, one workgroup each
// (vaek_train_loop_gen_replicas); `ws` is then the call's own workspace of resident_replicas_workspace_bytes(c, n) bytes, not the
// context's, and the rings are the caller's
int resident_max_replicas();
size_t resident_replicas_workspace_bytes(const vaek_ctx* c, int n);
int resident_train_loop(vaek_ctx* c, float* params, float* grads, float* m, float* v, int32_t* step_dev, const BatchArgs& gen, int n_steps,
                        float lr, void* ws, hipStream_t st, const vaek_replicas* rep, const TrajArgs* traj);

// ---- rng.hip ------------------------------------------------------------------------------
// validates the arguments of vaek_make_batch* and fills `out`
int make_batch_args(vaek_ctx* ctx, int32_t kind, const float* A, int32_t dd, int32_t did, int32_t pad, float var_added,
                    float* x, float* z1, float* z2, int32_t rows, int64_t row0, uint64_t seed, const int32_t* step_dev,
                    uint32_t step_host, int32_t* counter, int32_t which, uint32_t tag, BatchArgs* out);
int make_batch_launch(vaek_ctx* ctx, const BatchArgs& a, hipStream_t st);

// ---- fused_small.hip ----------------------------------------------------------------------
bool mlp1_supported(const vaek_ctx* c);          // fused_mlp1.hip: whole-network kernel for one-hidden-layer MLPs (<= 256 units)
int mlp1_grid(const vaek_ctx* c);
int mlp1_launch(vaek_ctx* c, const float* params, const float* x, const float* z1, const float* z2, float* partials, int pstride,
                int32_t* step_dev, hipStream_t st);
bool fused_supported(const vaek_ctx* c);
size_t fused_workspace_bytes(const vaek_ctx* c);
// gen != nullptr: the finalize launch carries extra blocks that draw the NEXT step's batch (vaek_train_step_gen)
int fused_train_step(vaek_ctx* c, float* params, float* grads, float* m, float* v, int32_t* step_dev,
                     const float* x, const float* z1, const float* z2, float lr, bool apply_adam, bool exchange,
                     void* ws, hipStream_t st, const BatchArgs* gen = nullptr);

// ---- fused_mlp3.hip: whole-network step for three-hidden-layer MLP VAEs (64 .. 256 units, D, L <= 32) at small batch ----------
bool mlp3_supported(const vaek_ctx* c);
size_t mlp3_workspace_bytes(const vaek_ctx* c);   // the region at ws_mlp3: stored activations / gradients and the partial rows
// two launches (chain; gradients + tail + Adam); gen != nullptr: the second carries workgroups that draw the NEXT step's batch
int mlp3_train_step(vaek_ctx* c, float* params, float* grads, float* m, float* v, int32_t* step_dev, const float* x, const float* z1,
                    const float* z2, float lr, bool apply_adam, void* ws, hipStream_t st, const BatchArgs* gen = nullptr);
// the same train step for n independent models of the context's shape, blockIdx.y = replica (vaek_train_step_gen_replicas): two
// launches whatever n is; `ws` is the call's own workspace of mlp3_replicas_workspace_bytes(c, n) bytes, not the context's; x / z1 /
// z2 and the generator's outputs are [n][B][..] stacks; state_stride % 4 == 0 (every replica then takes the base's dX load form)
int mlp3_max_replicas();
size_t mlp3_replica_region_floats(const vaek_ctx* c);
size_t mlp3_replicas_workspace_bytes(const vaek_ctx* c, int n);
int mlp3_train_step_replicas(vaek_ctx* c, float* params, float* grads, float* m, float* v, int32_t* step_dev, const float* x,
                             const float* z1, const float* z2, float lr, void* ws, hipStream_t st, const BatchArgs* gen, const vaek_replicas& rep);

// ---- what the two log-likelihood calls share (linear_loglik.hip); the checks of the evaluation calls are eval_check.h's ----------
// the last launch of both calls under the profile label `label`: n workgroups add the tile partials part[n][tiles][4] in tile order
// and store the records
int loglik_finalize(const char* label, const vaek_ctx* ctx, const float* params, const vaek_log_likelihood* ll, const double* part,
                    hipStream_t st);

// ---- mlp3_loglik.hip: importance-weighted log-likelihood of three-hidden-layer MLP VAEs; whatever the batch, world or force_generic
bool mlp3_loglik_supported(const vaek_ctx* c);
// ---- mlp3_jacobian.hip: decoder Jacobian spectra of the same contexts (vaek_ctx::mlp3_loglik is its predicate too: the call draws no
// data rows, so there is no kind)

}  // namespace vaek
