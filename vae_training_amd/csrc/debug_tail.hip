// Diagnostic entry (not part of include/vaek.h; tests/test_gpu_elbo_tail.py, tests/test_elbo_tail_ref.py): run ONE launcher of the
// step's tail (elbo.hip) -- the elementwise ELBO pass, the tile-pair reduction behind the decoder GEMM's ELBO epilogue, the
// reparameterisation backward, the finalisation (bulk_finalize, finalize, adam: finalize_launches of api.hip, the sequence the step
// itself runs), the two out4 forms, add_noise and the two slab sums -- on caller tensors through the step's own code.  As in
// debug_dense16.hip everything is checked on the host before the first launch (error -1, the reason in vaek_last_error), the
// scratch is the caller's (scratch == null: the bytes needed are written to scratch_bytes and nothing is launched) and the
// context's profiler is bound, so every launch shows under its label.  vaek_adam_step already reaches launch_adam directly.
#include "vaek_internal.h"

enum {
    VAEK_TAIL_ELBO = 0, VAEK_TAIL_ELBO_REDUCE, VAEK_TAIL_REPARAM_BWD, VAEK_TAIL_FINALIZE, VAEK_TAIL_OUT4, VAEK_TAIL_ADD_NOISE,
    VAEK_TAIL_SUM_SLABS_INPLACE, VAEK_TAIL_SUM_SLABS, VAEK_TAIL_COUNT
};

// Tensors are float32, row-major and contiguous, at any float offset (the kernels pick their 16-byte paths themselves).
struct vaek_tail_args {
    int32_t rows, D, L;
    int32_t S, rows_per_split;           // elbo / elbo_reduce / reparam_bwd: the row splits, S == ceil(rows / rows_per_split);
                                         // out4: the partial rows; finalize and sum_slabs_inplace: the slab count
    int32_t bm, nbx;                     // elbo_reduce: rows of a tile row, tiles in it
    int32_t want_deps;                   // out4: 1 = launch_elbo_out4 (lv given, out4[3] = d eps), 0 = launch_eval_out4 (params, offsets)
    int32_t Se;                          // finalize: rows of epart / rpart
    int32_t fuse;                        // finalize: Adam inside finalize_kernel (L + 5 <= 64) rather than a separate adam launch
    int32_t nseg, reserved;
    int32_t seg_end[32], seg_S[32];      // finalize: per layer the flat index one past its [kernel | bias], its slab count
    int64_t P, off_epsp, off_eps;        // finalize / out4 (eval form): the flat layout; off_eps = -1 without the epsilon leaf
    int64_t hi, lo;                      // finalize: outputs [0, hi) by bulk_finalize (0: none); outputs below lo left alone
    int64_t slab_stride, n;              // finalize / sum_slabs_inplace: floats between slabs; add_noise / sum_slabs_inplace: outputs
    int64_t loss_hist_cap;
    float eps_cli, inv_bt, rows_over_bt, rows_f, lr, reserved_f;      // rows_f: finalize / out4's row count as they take it
    const float* x; const float* y_lin; const float* y_sig; const float* z2; const float* mu; const float* eps_param;
    float* d_lin; float* d_sig;          // elbo: null = no gradients; may equal y_lin / y_sig (the step writes in place)
    float* partial;                      // elbo / elbo_reduce: [S][4]; reparam_bwd: [S][L]; out4: the [S][4] it reads
    int32_t* step_dev;                   // elbo / elbo_reduce: incremented by split 0 (may be null); finalize: read
    const float* part;                   // elbo_reduce: the {mse, d eps} tile pairs
    float* dsamp; const float* z1;       // reparam_bwd (dsamp updated in place)
    float* slabs;                        // finalize (read) / sum_slabs_inplace (clobbered)
    const float* epart; const float* rpart; const float* params;      // finalize; out4 eval form: params
    float* grads; float* params_rw; float* m; float* v; float* loss_hist;      // finalize; params_rw: null or == params
    const float* lv;                     // out4, want_deps = 1
    float* out;                          // out4: the four floats; add_noise: x_hat [n]; sum_slabs_inplace: the sums [n]
    void* scratch; int64_t scratch_bytes;
};

namespace vaek {
namespace {

bool splits_ok(int rows, int S, int rps) {
    return rps > 0 && S > 0 && (int64_t)S * rps >= rows && (int64_t)(S - 1) * rps < rows;
}

int validate(int op, const vaek_tail_args& a) {
    auto bad = [](const char* why) { set_error("vaek_debug_tail: %s", why); return VAEK_ERR_INVALID; };
    switch (op) {
    case VAEK_TAIL_ELBO:
        if (a.rows <= 0 || a.D <= 0 || a.L <= 0) return bad("rows, D and L must be positive");
        if (!a.x || !a.y_lin || !a.z2 || !a.mu || !a.partial) return bad("x, y_lin, z2, mu and partial are required");
        if (!splits_ok(a.rows, a.S, a.rows_per_split)) return bad("S must be ceil(rows / rows_per_split)");
        if (a.d_sig && (!a.d_lin || !a.y_sig)) return bad("d_sig needs d_lin and y_sig");
        if (a.d_lin && a.y_sig && !a.d_sig) return bad("gradients of a sigmoid decoder need d_sig");
        return VAEK_OK;
    case VAEK_TAIL_ELBO_REDUCE:
        if (a.rows <= 0 || a.L <= 0) return bad("rows and L must be positive");
        if (!a.part || !a.mu || !a.partial) return bad("part, mu and partial are required");
        if (a.bm <= 0 || a.nbx <= 0) return bad("bm and nbx must be positive");
        if (!splits_ok(a.rows, a.S, a.rows_per_split)) return bad("S must be ceil(rows / rows_per_split)");
        if (a.rows_per_split % a.bm) return bad("a split must start on a tile row (rows_per_split % bm == 0)");
        return VAEK_OK;
    case VAEK_TAIL_REPARAM_BWD:
        if (a.rows <= 0 || a.L <= 0) return bad("rows and L must be positive");
        if (a.L > 256) return bad("L <= 256");
        if (!a.dsamp || !a.mu || !a.z1 || !a.partial) return bad("dsamp, mu, z1 and partial are required");
        if (!splits_ok(a.rows, a.S, a.rows_per_split)) return bad("S must be ceil(rows / rows_per_split)");
        return VAEK_OK;
    case VAEK_TAIL_FINALIZE: {
        if (a.L <= 0 || a.D <= 0 || a.S <= 0 || a.Se <= 0) return bad("L, D, S and Se must be positive");
        if (!a.slabs || !a.epart || !a.rpart || !a.params || !a.grads) return bad("slabs, epart, rpart, params and grads are required");
        if (a.nseg < 0 || a.nseg > 32) return bad("nseg <= 32");
        if (a.off_epsp <= 0 || a.off_epsp > INT32_MAX) return bad("off_epsp must be positive");
        int64_t prev = 0;
        for (int k = 0; k < a.nseg; ++k) {
            if (a.seg_end[k] <= prev) return bad("segment ends must ascend");
            if (a.seg_S[k] <= 0) return bad("a segment's slab count must be positive");
            prev = a.seg_end[k];
        }
        if (prev > a.off_epsp) return bad("the last segment ends beyond off_epsp");
        if (a.off_eps != -1 && a.off_eps != a.off_epsp + a.L) return bad("off_eps is -1 or off_epsp + L");
        if (a.off_epsp + a.L + (a.off_eps >= 0 ? 1 : 0) != a.P) return bad("off_epsp + L (+ 1 with epsilon) must be P");
        if (a.slab_stride < a.off_epsp) return bad("slab_stride must cover the weights and biases");
        if (a.hi != 0 && a.hi != a.off_epsp) return bad("hi is 0 or off_epsp");
        if (a.lo != 0 && a.lo != a.off_epsp) return bad("lo is 0 or off_epsp");
        if (a.hi && a.lo) return bad("the bulk pass sets the floor itself: lo must be 0 with hi");
        if (a.params_rw && (!a.m || !a.v || !a.step_dev)) return bad("Adam needs m, v and step_dev");
        if (a.params_rw && a.params_rw != a.params) return bad("params_rw is null or params");
        if (a.fuse && !a.params_rw) return bad("fuse without Adam");
        if (a.fuse && a.L + 5 > 64) return bad("fuse needs L + 5 <= 64");
        if (a.loss_hist && a.loss_hist_cap <= 0) return bad("loss_hist_cap must be positive");
        return VAEK_OK;
    }
    case VAEK_TAIL_OUT4:
        if (a.S <= 0 || a.L <= 0 || a.D <= 0) return bad("S, L and D must be positive");
        if (!a.partial || !a.out) return bad("partial and out are required");
        if (a.want_deps ? !a.lv : !a.params) return bad("lv (want_deps) or params is required");
        if (!a.want_deps && (a.off_epsp < 0 || a.off_eps < -1)) return bad("bad offsets");
        return VAEK_OK;
    case VAEK_TAIL_ADD_NOISE:
        if (a.n <= 0) return bad("n must be positive");
        if (!a.y_lin || !a.z2 || !a.out) return bad("y_lin, z2 and out are required");
        return VAEK_OK;
    case VAEK_TAIL_SUM_SLABS_INPLACE:
    case VAEK_TAIL_SUM_SLABS:
        if (a.n <= 0 || a.S <= 0) return bad("n and S must be positive");
        if (a.slab_stride < a.n) return bad("slab_stride < n");
        if (!a.slabs || !a.out) return bad("slabs and out are required");
        return VAEK_OK;
    default:
        return bad("unknown op");
    }
}

}  // namespace
}  // namespace vaek

extern "C" int vaek_debug_tail(vaek_ctx* ctx, int32_t op, vaek_tail_args* args, void* stream) {
    using namespace vaek;
    if (!args) { set_error("vaek_debug_tail: null args"); return VAEK_ERR_INVALID; }
    vaek_tail_args& a = *args;
    int rc = validate(op, a);
    if (rc) return rc;
    constexpr int64_t need = 0;        // every tensor of these launchers is the caller's own
    if (!a.scratch) { a.scratch_bytes = need; return VAEK_OK; }
    if (a.scratch_bytes < need || (reinterpret_cast<uintptr_t>(a.scratch) & 255)) {
        set_error("vaek_debug_tail: scratch must be 256-byte aligned and hold %lld bytes", (long long)need);
        return VAEK_ERR_WORKSPACE;
    }
    if (!ctx) { set_error("vaek_debug_tail: null context"); return VAEK_ERR_INVALID; }
    ProfBind pb(ctx);
    hipStream_t st = (hipStream_t)stream;
    switch (op) {
    case VAEK_TAIL_ELBO: {
        ElboArgs e{};
        e.x = a.x; e.y_lin = a.y_lin; e.y_sig = a.y_sig; e.z2 = a.z2; e.mu = a.mu;
        e.eps_param = a.eps_param; e.eps_cli = a.eps_cli; e.d_lin = a.d_lin; e.d_sig = a.d_sig; e.partial = a.partial;
        e.rows = a.rows; e.D = a.D; e.L = a.L; e.S = a.S; e.rows_per_split = a.rows_per_split;
        e.inv_bt = a.inv_bt; e.step_dev = a.step_dev;
        return launch_elbo(e, st);
    }
    case VAEK_TAIL_ELBO_REDUCE:
        return launch_elbo_reduce(a.part, a.bm, a.nbx, a.mu, a.partial, a.rows, a.L, a.S, a.rows_per_split, a.step_dev, st);
    case VAEK_TAIL_REPARAM_BWD:
        return launch_reparam_bwd(a.dsamp, a.mu, a.z1, a.partial, a.rows, a.L, a.S, a.rows_per_split, a.inv_bt, st);
    case VAEK_TAIL_FINALIZE: {
        FinalizeArgs f{};
        f.slabs = a.slabs; f.slab_stride = a.slab_stride; f.S = a.S;
        f.nseg = a.nseg;
        for (int k = 0; k < a.nseg; ++k) { f.seg_end[k] = a.seg_end[k]; f.seg_S[k] = a.seg_S[k]; }
        f.epart = a.epart; f.rpart = a.rpart; f.Se = a.Se;
        f.P = a.P; f.off_epsp = a.off_epsp; f.off_eps = a.off_eps; f.L = a.L; f.D = a.D;
        f.params = a.params; f.eps_cli = a.eps_cli; f.rows_over_bt = a.rows_over_bt; f.inv_bt = a.inv_bt; f.rows = a.rows_f;
        f.grads = a.grads; f.params_rw = a.params_rw; f.m = a.m; f.v = a.v; f.step_dev = a.step_dev; f.lr = a.lr;
        f.loss_hist = a.step_dev ? a.loss_hist : nullptr; f.loss_hist_cap = a.loss_hist_cap;
        f.lo = a.lo;
        return finalize_launches(f, a.hi, a.fuse != 0, st);
    }
    case VAEK_TAIL_OUT4:
        if (a.want_deps)
            return launch_elbo_out4(a.partial, a.S, a.lv, a.L, a.D, a.eps_param, a.eps_cli, a.rows_f, a.inv_bt, a.out, st);
        return launch_eval_out4(a.partial, a.S, a.params, a.off_epsp, a.off_eps, a.L, a.D, a.eps_cli, a.rows_f, a.inv_bt, a.out, st);
    case VAEK_TAIL_ADD_NOISE:
        return launch_add_noise(a.y_lin, a.y_sig, a.z2, a.eps_param, a.eps_cli, a.out, a.n, st);
    case VAEK_TAIL_SUM_SLABS_INPLACE:
        return launch_sum_slabs_inplace(a.slabs, a.slab_stride, a.S, a.out, a.n, st);
    default:      // the plain slab sum the in-place form is compared with (and ends in)
        return launch_sum_slabs(a.slabs, a.slab_stride, a.S, a.out, a.n, st);
    }
}
