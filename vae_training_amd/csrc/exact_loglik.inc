// Exact log-likelihood, exact ELBO and posterior gap of one-decoder linear VAEs (vaek_exact_log_likelihood_replicas).
// Model r is a linear-Gaussian latent-variable model: p(x) = N(b_d, K^T K + e^{eps} I).  ONE workgroup per model: the parameter image,
// G = K^T K (element (i, j) one chain over l of exact float64 products of two float32 values, i <= j, mirrored) into Jacobi buffer 0,
// V = I, jacobi_solve<true> (the covariance solve's own text, eigen_dev.h), then 1 / s_i, logdet, T and the encoder's constant published
// in LDS and the rows walked in tiles of 256, thread t taking row 256 j + t through produce_row (the bits vaek_make_batch writes, or the
// caller's).  Per row, float64 VALU fmas over broadcast LDS reads (V^T c, x E, mu K: at most 3 * 32^2 per row -- the matrix cores
// would need the rows staged as operands and the three products are chained per row, so a row per thread keeps every chain in
// registers).  A thread keeps three private running sums over its rows in tile order; one fixed binary tree per sum adds them.
//
// The kernel reads rows / parameters and stores only the records, with per-lane vector stores; it reads nothing back.
//
// NOT a translation unit: cov_spectrum.hip includes this file at its end.  Compiled as a unit of its own, exact_loglik_kernel<32, 32>
// comes out with another instruction text than it has behind the covariance kernels (DESIGN 3.19), so the text is split and the
// unit is not.  eigen_dev.h and mfma_geom.h are the including file's.

namespace vaek {

constexpr int kExactHead = 10;               // doubles of the record in front of the eigenvalues
constexpr double kLog2PiD = 1.8378770664093454835606594728112;

struct ExactLogLikArgs {
    const float* params; long long state_stride;
    const unsigned long long* x_seeds; const unsigned* x_steps;      // [n]: the rows' Philox key and step (drawing mode)
    long long a_stride;
    const float* x; long long x_stride;                              // explicit rows [rows][D] per replica, or NULL: drawing mode
    double* out; long long out_stride;
    double* row_out; long long row_stride;                           // [rows][2] per replica, or NULL
    int rows, D, L, off_epsp, off_eps;
    float eps_cli;
    BatchArgs gen;                 // kind, A, dd, did, pad, noise_std, tag = x_tag, D, L; seed / step / pointers are not used
};

template <int DP, int LP>
__global__ __launch_bounds__(256) void exact_loglik_kernel(const ExactLogLikArgs a) {
    using G = ParamImage<DP, LP, false>;
    static_assert(DP <= kSpectrumMaxDim && LP <= kSpectrumMaxDim, "the Jacobi buffers and the tables hold 32");
    __shared__ __attribute__((aligned(16))) float W[G::N];
    __shared__ __attribute__((aligned(16))) double mat[2 * kMatDoubles], vec[2 * kMatDoubles];
    __shared__ double red[3][256];
    __shared__ __attribute__((aligned(16))) double sinv[kSpectrumMaxDim];
    __shared__ double rot_c[kSpectrumMaxDim], rot_s[kSpectrumMaxDim], eig[kSpectrumMaxDim], lgs[kSpectrumMaxDim];
    __shared__ double tl[kSpectrumMaxDim], kl[kSpectrumMaxDim], pub[4];
    __shared__ int rot_mate[kSpectrumMaxDim];

    const int t = threadIdx.x;
    const long long r = blockIdx.x;
    const int D = a.D, L = a.L, rows = a.rows;
    const float* const p = a.params + r * a.state_stride;
    double* const out = a.out + r * a.out_stride;

    G::fill(W, p, D, L, a.off_epsp, t);                                 // the parameter image: zero outside [D] x [L]
    __syncthreads();

    const float eps32 = a.off_eps >= 0 ? p[a.off_eps] * a.eps_cli : a.eps_cli;     // linear_loglik.hip's eps, then widened
    const double eps = (double)eps32;
    const double evar = exp(eps), einv = exp(-eps);

    // ---- G = K^T K (i <= j, mirrored) into buffer 0, V = I into both vector buffers, the per-latent terms of T and of the KL constant ----
    double sq = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int idx = t + 256 * k, i = idx >> 5, j = idx & 31;
        if (i <= j) {
            double v = 0.0;
            if (j < D)
                for (int l = 0; l < L; ++l) v = fma((double)W[G::WD + l * DP + i], (double)W[G::WD + l * DP + j], v);
            mat[i * kMatStride + j] = v;
            mat[j * kMatStride + i] = v;
            sq += i == j ? v * v : 2.0 * v * v;
        }
        const double id = i == j ? 1.0 : 0.0;
        vec[i * kMatStride + j] = id;                                   // the solve may end in either buffer: both are I outside De x De
        vec[kMatDoubles + i * kMatStride + j] = id;
    }
    if (t < kSpectrumMaxDim) {
        double tv = 0.0, kv = 0.0;
        if (t < L) {
            double k2 = 0.0;
            for (int d = 0; d < D; ++d) { const double w = (double)W[G::WD + t * DP + d]; k2 = fma(w, w, k2); }
            const double lv = (double)W[G::LV + t], ev = exp(lv);
            tv = ev * k2;
            kv = ev - 1.0 - lv;
        }
        tl[t] = tv;
        kl[t] = kv;
    }
    const double norm_g = sqrt(block_sum256(sq, red[0], t));           // its barriers also publish G, V and the tables

    const int De = D + (D & 1);
    int cur, sweeps;
    double off_f;
    jacobi_solve<true>(mat, vec, De, norm_g, red[0], rot_c, rot_s, rot_mate, t, cur, sweeps, off_f);

    // ---- 1 / s_i, log s_i; then logdet, T and the KL constant, each one serial chain in index order ------------------------------------
    const double* const A = mat + cur * kMatDoubles;
    if (t < kSpectrumMaxDim) {
        const double e = t < D ? A[t * kMatStride + t] : 0.0;
        const double s = fmax(e, 0.0) + evar;
        eig[t] = e;
        sinv[t] = t < D ? 1.0 / s : 0.0;
        lgs[t] = t < D ? log(s) : 0.0;
    }
    __syncthreads();
    if (t < 3) {
        const double* const src = t == 0 ? lgs : (t == 1 ? tl : kl);
        double s = 0.0;
        for (int i = 0; i < kSpectrumMaxDim; ++i) s += src[i];
        pub[t] = s;
    }
    __syncthreads();
    const double logdet = pub[0], T = pub[1], klc = pub[2];
    if (t < D) {
        const double e = eig[t];
        int rank = 0;
        for (int j = 0; j < D; ++j) {
            const double o = eig[j];
            rank += (o < e || (o == e && j < t)) ? 1 : 0;
        }
        out[kExactHead + rank] = e;
    }

    // ---- the rows: thread t takes row 256 j + t, j in order ------------------------------------------------------------------------------
    RowCtx rc{};
    rc.D = D; rc.L = L; rc.W = W;
    rc.g = a.gen;
    const bool explicit_rows = a.x != nullptr;
    if (explicit_rows) {
        rc.xr = a.x + r * a.x_stride;
    } else {
        if (rc.g.A) rc.g.A += r * a.a_stride;
        rc.key = philox_key(a.x_seeds[r]);
        rc.step = a.x_steps[r];
    }
    const double* const V = vec + cur * kMatDoubles;
    const double cst_lp = logdet + (double)D * kLog2PiD;
    const double cst_el = (double)D * (eps + kLog2PiD);
    double* const rout = a.row_out ? a.row_out + r * a.row_stride : nullptr;
    double sum_lp = 0.0, sum_el = 0.0, sum_gap = 0.0;
    for (int base = 0; base < rows; base += 256) {
        const int row = base + t;
        if (row < rows) {
            // V and the image are loop-invariant: a compiler that knows it lifts them out of the tile loop and spills them
            asm volatile("" ::: "memory");
            float x[kSpectrumMaxDim];
            if (explicit_rows) produce_row<SRC_EXPLICIT, DP, LP, false>(rc, row, x);
            else produce_row<SRC_REAL, DP, LP, false>(rc, row, x);
            // ---- log p(x): y = V^T (x - b_d), quad = sum y_i^2 / s_i ------------------------------------------------------------------
            double y[DP];
#pragma unroll
            for (int j = 0; j < DP; ++j) y[j] = 0.0;
#pragma unroll
            for (int i = 0; i < DP; ++i) {                                            // rows >= D of V are rows of I and meet c = 0
                const double c = (double)x[i] - (double)W[G::BD + i];
#pragma unroll
                for (int j = 0; j < DP; ++j) y[j] = fma(V[i * kMatStride + j], c, y[j]);
            }
            double quad = 0.0;
#pragma unroll
            for (int j = 0; j < DP; ++j) quad = fma(y[j] * y[j], sinv[j], quad);       // 1 / s is 0 at j >= D
            const double lp = -0.5 * (quad + cst_lp);
            // ---- ELBO(x): mu = x E + b_e, r = mu K + b_d - x ----------------------------------------------------------------------------
            double mu[LP];
#pragma unroll
            for (int l = 0; l < LP; ++l) mu[l] = (double)W[G::BE + l];
#pragma unroll
            for (int d = 0; d < DP; ++d) {                                            // a padded row of the image adds 0
                const double xd = (double)x[d];
#pragma unroll
                for (int l = 0; l < LP; ++l) mu[l] = fma(xd, (double)W[G::WE + d * LP + l], mu[l]);
            }
            double musq = 0.0;
#pragma unroll
            for (int l = 0; l < LP; ++l) musq = fma(mu[l], mu[l], musq);                // mu is 0 at l >= L
            double rr[DP];
#pragma unroll
            for (int d = 0; d < DP; ++d) rr[d] = (double)W[G::BD + d] - (double)x[d];
#pragma unroll
            for (int l = 0; l < LP; ++l) {
#pragma unroll
                for (int d = 0; d < DP; ++d) rr[d] = fma(mu[l], (double)W[G::WD + l * DP + d], rr[d]);
            }
            double rsq = 0.0;
#pragma unroll
            for (int d = 0; d < DP; ++d) rsq = fma(rr[d], rr[d], rsq);                  // columns >= D are 0 - 0
            const double el = -0.5 * (einv * (rsq + T) + cst_el) - 0.5 * (klc + musq);
            sum_lp += lp;
            sum_el += el;
            sum_gap += lp - el;
            if (rout) {
                rout[2 * (long long)row] = lp;
                rout[2 * (long long)row + 1] = el;
            }
        }
    }

    // ---- the three sums: one fixed binary tree each over the 256 threads; the record, lane t storing double t ----------------------------
    red[0][t] = sum_lp;
    red[1][t] = sum_el;
    red[2][t] = sum_gap;
    tree_sum256(red, t);
    if (t < kExactHead) {
        const double n = (double)rows;
        double v;
        switch (t) {
            case 0: v = red[0][0] / n; break;
            case 1: v = red[1][0] / n; break;
            case 2: v = red[2][0] / n; break;
            case 3: v = eps; break;
            case 4: v = logdet; break;
            case 5: v = (double)sweeps; break;
            case 6: v = off_f; break;
            case 7: v = norm_g; break;
            case 8: v = (off_f + 64.0 * (double)D * 0x1p-53 * norm_g) * einv; break;
            default: v = n; break;
        }
        out[t] = v;
    }
}

// ---- variant table: the one-decoder padded shapes of mfma_geom.h, each side rounded up to 4; a two-decoder row holds no kernel -------
typedef void (*ExactLogLikKernel)(const ExactLogLikArgs);
struct ExactLogLikVariant { int dp, lp, sig; ExactLogLikKernel fn; };
template <int DP, int LP, int SIG> struct ExactLogLikPick { static constexpr ExactLogLikKernel fn = exact_loglik_kernel<DP, LP>; };
template <int DP, int LP> struct ExactLogLikPick<DP, LP, 1> { static constexpr ExactLogLikKernel fn = nullptr; };
#define VAEK_EXACT_ROW(DP, LP, SIG, EXACT) {up4(DP), up4(LP), SIG, ExactLogLikPick<up4(DP), up4(LP), SIG>::fn},
static const ExactLogLikVariant kExactLogLikVariants[] = {VAEK_EVAL_SHAPES(VAEK_EXACT_ROW)};
#undef VAEK_EXACT_ROW

// vaek_supports_log_likelihood's predicate AND one decoder: the sigmoid second decoder has no closed form
static const ExactLogLikVariant* pick_exact_loglik(const vaek_ctx* c) {
    const vaek_config& cfg = c->cfg;
    if (cfg.dtype != VAEK_F32 || cfg.n_enc_hidden != 0 || cfg.n_dec_hidden != 0 || cfg.sigmoid_decoder) return nullptr;
    return pick_smallest_shape(kExactLogLikVariants, c->D, c->L, false);
}

static int64_t exact_loglik_record_len(const vaek_ctx* c) { return kExactHead + (int64_t)c->D; }

}  // namespace vaek

using namespace vaek;

extern "C" {

int vaek_supports_exact_log_likelihood(const vaek_ctx* ctx, int32_t kind, int32_t* yes) {
    if (!ctx || !yes) { set_error("vaek_supports_exact_log_likelihood: null argument"); return VAEK_ERR_INVALID; }
    *yes = kind >= 0 && kind <= 2 && pick_exact_loglik(ctx) ? 1 : 0;
    return VAEK_OK;
}

int vaek_exact_log_likelihood_record_len(const vaek_ctx* ctx, int64_t* doubles) {
    if (!ctx || !doubles) { set_error("vaek_exact_log_likelihood_record_len: null argument"); return VAEK_ERR_INVALID; }
    *doubles = exact_loglik_record_len(ctx);
    return VAEK_OK;
}

int vaek_exact_log_likelihood_replicas(vaek_ctx* ctx, const float* params, const vaek_exact_log_likelihood* ll, int32_t kind,
                                       const float* A, int32_t dd, int32_t did, int32_t pad, float var_added, uint32_t x_tag,
                                       void* stream) {
    const char* who = "vaek_exact_log_likelihood_replicas";
    ProfBind pb(ctx);
    const ExactLogLikVariant* var = ctx ? pick_exact_loglik(ctx) : nullptr;
    const EvalDesc d = describe(ll);
    EvalRules r{};
    r.covered = var != nullptr;
    r.needs = "needs a float32 linear VAE (no hidden layers) with ONE decoder and D, L <= 32: the sigmoid second decoder has no closed form (see "
              "vaek_supports_exact_log_likelihood)";
    r.rows_min = 1; r.rows_cap = kLogLikMaxRows; r.rows_query = "vaek_log_likelihood_max_rows";
    r.records = 1; r.record_len = ctx ? exact_loglik_record_len(ctx) : 0; r.record_query = "vaek_exact_log_likelihood_record_len";
    r.draws = true; r.kind = kind; r.A = A; r.dd = dd; r.did = did; r.pad = pad; r.x_tag = x_tag;
    if (int rc = check_eval(who, ctx, params, d, r)) return rc;
    if (int rc = check_aligned8(who, "row_out", (uintptr_t)ll->row_out)) return rc;
    if (ll->row_out && (ll->row_stride < 0 || (ll->row_stride < 2 * (int64_t)ll->rows && (ll->row_stride > 0 || ll->n > 1)))) {
        set_error("%s: row_stride %lld: need >= 2 * rows = %lld (0 with one replica)", who, (long long)ll->row_stride, 2 * (long long)ll->rows);
        return VAEK_ERR_INVALID;
    }
    ExactLogLikArgs a{};
    a.params = params; a.state_stride = ll->state_stride;
    a.x_seeds = reinterpret_cast<const unsigned long long*>(ll->x_seeds); a.x_steps = ll->x_steps;
    a.x = ll->x; a.x_stride = ll->x_stride;
    a.out = ll->out; a.out_stride = ll->out_stride; a.row_out = ll->row_out; a.row_stride = ll->row_stride;
    a.rows = ll->rows; a.D = ctx->D; a.L = ctx->L; a.off_epsp = (int)ctx->off_epsp; a.off_eps = (int)ctx->off_eps;
    a.eps_cli = ctx->cfg.eps_cli;
    fill_rows_source(&a.gen, &a.a_stride, ctx, ll->rows, d.explicit_rows(), kind, A, dd, did, pad, var_added, x_tag, ll->a_stride);
    hipStream_t st = (hipStream_t)stream;
    {
        ProfScope ps("exact_loglik_replicas", st);
        launch_k(ps, var->fn, dim3((unsigned)ll->n), dim3(256), 0, st, a);
    }
    VAEK_HIP_CHECK(hipGetLastError());
    return VAEK_OK;
}

}  // extern "C"
