// Importance-weighted log-likelihood of N small linear VAEs of one shape (vaek_log_likelihood_replicas): for every data row x, K
// samples z_k = mu(x) + exp(epsilon_p / 2) xi_k of the encoder's posterior and their log weights
//   log w_k = log p(x | z_k) + log p(z_k) - log q(z_k | x)
//           = -1/2 [ |dec(z_k) - x|^2 e^{-eps} + D (eps + log 2 pi) ] + 1/2 sum_l ( xi_kl^2 - z_kl^2 + epsilon_p[l] ),
// reduced per row to the IWAE-K bound logsumexp_k(log w_k) - log K, the K-sample ELBO estimate mean_k log w_k and the normalised
// effective sample size (sum w)^2 / (K sum w^2), and averaged over the rows.  There is no decoder-noise draw: this is the likelihood
// the reference reserves `Average Log Likelihood` for and never fills, not the noisy VAE Loss.
//
// The kernel is linear_stats.hip's with a sample loop inside the row:
//   - grid (ceil(rows / 256), n), 256 threads: a thread owns ONE row of one model.  It reads the row (explicit mode) or draws it with
//     the functions of rng_dev.h (the bits vaek_make_batch writes), encodes it once and then walks k = 0 .. K - 1 serially: sample k
//     takes its L normals from Philox blocks k ceil(L / 4) + j of the row's latent stream, so sample 0 is vaek_make_batch's z1.  An
//     online log-sum-exp carries a running max, sum e^{lw - m}, sum e^{2 (lw - m)} and sum lw in float32, in k order.  Nothing of a
//     row, a sample or a weight ever exists in HBM;
//   - the parameters live in the zero-padded LDS image of linear_stats.hip (ParamImage of eval_dev.h, one text for both; that file's
//     header says why: broadcast reads, 16 bytes at a time, static register indices, a padded row or column adds 0).  The products
//     are VALU fmas: with a row per thread the chain stays in registers;
//   - the image is loop-invariant, and a compiler that knows it lifts the weights out of the sample loop and spills them: the
//     compiler barrier at the top of the loop makes every sample read them again;
//   - the three row sums are float64: a fixed binary tree across the workgroup, then one 4-double partial per (replica, tile) in
//     the call's workspace.  A SECOND launch of n workgroups adds the tiles in tile order and stores the 4-float record with per-lane
//     vector stores.  The partials cross a launch boundary: nothing stored in a launch is read back in it, and there is no atomic,
//     counter or wait.  A record therefore depends on neither n, nor the replica index, nor the run.
#include "eval_dev.h"
#include "mfma_geom.h"
#include "eval_check.h"

namespace vaek {

struct LogLikArgs {
    const float* params; long long state_stride;
    const unsigned long long* x_seeds; const unsigned* x_steps;      // [n]: the rows' Philox key and step (drawing mode)
    const unsigned long long* z_seeds; const unsigned* z_steps;      // [n]: the samples'
    long long a_stride;
    const float* x; long long x_stride;                              // explicit rows [rows][D] per replica, or NULL: drawing mode
    double* part;                                                    // [n][tiles][4]
    int rows, samples, D, L, off_epsp, off_eps;
    float eps_cli;
    unsigned z_tag;
    BatchArgs gen;                 // kind, A, dd, did, pad, noise_std, tag = x_tag, D, L; seed / step / pointers are not used
};

// the finalize launch of this call and of vaek_mlp3_log_likelihood_replicas (loglik_finalize)
struct LogLikFinalArgs {
    const float* params; long long state_stride;
    const double* part;
    float* out; long long out_stride;
    int rows, tiles, off_eps;
    float eps_cli;
};

template <int DP, int LP, bool SIG>
__global__ __launch_bounds__(256) void linear_loglik_kernel(const LogLikArgs a) {
    using G = ParamImage<DP, LP, SIG>;
    __shared__ __attribute__((aligned(16))) float W[G::N];
    __shared__ double red[kLogLikSums][256];
    const int t = threadIdx.x;
    const int tile = blockIdx.x;
    const long long r = blockIdx.y;
    const int D = a.D, L = a.L;
    const float* const p = a.params + r * a.state_stride;

    G::fill(W, p, D, L, a.off_epsp, t);                                 // the parameter image: zero outside [D] x [L]
    __syncthreads();

    const float eps = a.off_eps >= 0 ? p[a.off_eps] * a.eps_cli : a.eps_cli;
    const float inv_var = expf(-eps);
    const int row = tile * 256 + t;
    float res[kLogLikSums] = {0.f, 0.f, 0.f};

    if (row < a.rows) {
        // ---- the row: the caller's, or vaek_make_batch's work item for (row, c0), all c0.  The draw and the encoder product below are
        // linear_stats.hip's text too: keep the two in step (eval_dev.h says why they are not shared) -------------------------------
        float x[DP];
        if (a.x) {
            const float* const xr = a.x + r * a.x_stride + (long long)row * D;
#pragma unroll
            for (int d = 0; d < DP; ++d) x[d] = d < D ? xr[d] : 0.f;
        } else {
            BatchArgs gx = a.gen;
            if (gx.A) gx.A += r * a.a_stride;
            const uint2 xkey = philox_key(a.x_seeds[r]);
            const unsigned xstep = a.x_steps[r];
            float nrm[16];
            dataset_normals(gx, xstep, row, xkey, nrm);
#pragma unroll
            for (int c0 = 0; c0 < DP; c0 += 4) {
                float o[4] = {0.f, 0.f, 0.f, 0.f};
                if (c0 < D) dataset_cols4(gx, xstep, row, xkey, nrm, c0, o);
#pragma unroll
                for (int c = 0; c < 4; ++c) x[c0 + c] = c0 + c < D ? o[c] : 0.f;
            }
        }
        // ---- mu = Encoder(x), once; mu[l >= L] = 0 and the constant of log w --------------------------------------------------
        float mu[LP];
        float lvsum = 0.f;
#pragma unroll
        for (int l = 0; l < LP; ++l) { mu[l] = W[G::BE + l]; lvsum += W[G::LV + l]; }
#pragma unroll
        for (int d = 0; d < DP; ++d) {
            if (d < D) {
#pragma unroll
                for (int l = 0; l < LP; ++l) mu[l] = fmaf(x[d], W[G::WE + d * LP + l], mu[l]);
            }
        }
        const float c0 = 0.5f * lvsum - 0.5f * (float)D * (eps + kLog2Pi);

        BatchArgs gz = a.gen;
        gz.tag = a.z_tag;
        const uint2 zkey = philox_key(a.z_seeds[r]);
        const unsigned zstep = a.z_steps[r];
        const int nlb = (L + 3) >> 2;                                      // Philox blocks of one sample

        OnlineLogSumExp lse;                                               // in k order
        for (int k = 0; k < a.samples; ++k) {
            // the image is loop-invariant, and a compiler that knows it lifts thousands of weights out of the loop and spills them:
            // every sample reads them again (broadcast LDS reads, 16 bytes each)
            asm volatile("" ::: "memory");
            // ---- z = mu + e^{lv/2} xi; qs = sum_l xi^2 - z^2.  Elements >= L of the last block are not part of the sample ----------
            float z[LP];
            float qs = 0.f;
#pragma unroll
            for (int q = 0; q < LP / 4; ++q) {
                float n4[4] = {0.f, 0.f, 0.f, 0.f};
                if (4 * q < L) latent_block(gz, zstep, row, zkey, k * nlb + q, n4);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int l = 4 * q + c;
                    const float xi = l < L ? n4[c] : 0.f;
                    z[l] = fmaf(W[G::SD + l], xi, mu[l]);                  // e^{lv/2} of the image is 0 at l >= L
                    qs = fmaf(xi, xi, qs);
                    qs = fmaf(-z[l], z[l], qs);
                }
            }
            // ---- dec(z) = Decoder(z) [+ sigmoid(SigDecoder(z))] and the residual ----------------------------------------------------
            float y[DP], ys[SIG ? DP : 1];
#pragma unroll
            for (int d = 0; d < DP; ++d) {
                y[d] = W[G::BD + d];
                if (SIG) ys[d] = W[G::BS + d];
            }
#pragma unroll
            for (int l = 0; l < LP; ++l) {
                if (l < L) {
#pragma unroll
                    for (int d = 0; d < DP; ++d) {
                        y[d] = fmaf(z[l], W[G::WD + l * DP + d], y[d]);
                        if (SIG) ys[d] = fmaf(z[l], W[G::WS + l * DP + d], ys[d]);
                    }
                }
            }
            float rsq = 0.f;
#pragma unroll
            for (int d = 0; d < DP; ++d) {
                float xh = y[d];
                if (SIG) xh += 1.f / (1.f + expf(-ys[d]));
                const float rr = d < D ? xh - x[d] : 0.f;
                rsq = fmaf(rr, rr, rsq);
            }
            lse.push(c0 + 0.5f * (qs - rsq * inv_var));
        }
        lse.finish(a.samples, res);
    }

    // ---- the tile's sums: a fixed binary tree over the 256 threads, float64 ------------------------------------------
#pragma unroll
    for (int j = 0; j < kLogLikSums; ++j) red[j][t] = (double)res[j];
    tree_sum256(red, t);
    store_tile_partial(a.part, r, tile, t, red);
}

// one workgroup per replica: the tiles' partials in tile order, then the record, lane t storing float t
__global__ __launch_bounds__(64) void loglik_finalize_kernel(const LogLikFinalArgs a) {
    const int t = threadIdx.x;
    const long long r = blockIdx.x;
    if (t >= kLogLikRecord) return;
    float v;
    if (t < kLogLikSums) {
        double s = 0.0;
        for (int tile = 0; tile < a.tiles; ++tile) s += a.part[(r * a.tiles + tile) * 4 + t];
        v = (float)(s / (double)a.rows);
    } else {
        v = a.off_eps >= 0 ? a.params[r * a.state_stride + a.off_eps] * a.eps_cli : a.eps_cli;
    }
    a.out[r * a.out_stride + t] = v;
}

// ---- variant table: the padded shapes of the resident loop (mfma_geom.h), each side rounded up to a multiple of 4; a context
// takes the smallest that holds it (an EXACT shape of that table is one more padded shape here) ---------------------------------
typedef void (*LogLikKernel)(const LogLikArgs);
struct LogLikVariant { int dp, lp, sig; LogLikKernel fn; };
#define VAEK_LOGLIK_ROW(DP, LP, SIG, EXACT) {up4(DP), up4(LP), SIG, linear_loglik_kernel<up4(DP), up4(LP), (SIG) != 0>},
static const LogLikVariant kLogLikVariants[] = {VAEK_EVAL_SHAPES(VAEK_LOGLIK_ROW)};
#undef VAEK_LOGLIK_ROW

// float32, no hidden layers, one or two decoders, a padded shape holds (D, L); two decoders: D <= 28, the bound of every other
// two-decoder path of the library.  Nothing about the batch or the world: the call reads parameters only
static const LogLikVariant* pick_loglik(const vaek_ctx* c) {
    const vaek_config& cfg = c->cfg;
    if (cfg.dtype != VAEK_F32 || cfg.n_enc_hidden != 0 || cfg.n_dec_hidden != 0) return nullptr;
    if (cfg.sigmoid_decoder && c->D > 28) return nullptr;
    return pick_smallest_shape(kLogLikVariants, c->D, c->L, cfg.sigmoid_decoder != 0);
}

static size_t loglik_workspace_bytes(int n, int rows) { return sizeof(double) * 4 * (size_t)n * (size_t)((rows + 255) / 256); }

int loglik_finalize(const char* label, const vaek_ctx* ctx, const float* params, const vaek_log_likelihood* ll, const double* part, hipStream_t st) {
    LogLikFinalArgs f{};
    f.params = params; f.state_stride = ll->state_stride; f.part = part; f.out = ll->out; f.out_stride = ll->out_stride;
    f.rows = ll->rows; f.tiles = (ll->rows + 255) / 256; f.off_eps = (int)ctx->off_eps; f.eps_cli = ctx->cfg.eps_cli;
    {
        ProfScope ps(label, st);
        launch_k(ps, loglik_finalize_kernel, dim3((unsigned)ll->n), dim3(64), 0, st, f);
    }
    VAEK_HIP_CHECK(hipGetLastError());
    return VAEK_OK;
}

}  // namespace vaek

using namespace vaek;

extern "C" {

int vaek_supports_log_likelihood(const vaek_ctx* ctx, int32_t kind, int32_t* yes) {
    if (!ctx || !yes) { set_error("vaek_supports_log_likelihood: null argument"); return VAEK_ERR_INVALID; }
    *yes = kind >= 0 && kind <= 2 && pick_loglik(ctx) ? 1 : 0;
    return VAEK_OK;
}

int vaek_log_likelihood_record_len(void) { return kLogLikRecord; }
int vaek_log_likelihood_max_rows(void) { return kLogLikMaxRows; }
int vaek_log_likelihood_max_samples(void) { return kLogLikMaxSamples; }

int vaek_log_likelihood_workspace_bytes(const vaek_ctx* ctx, int32_t n, int32_t rows, size_t* bytes) {
    const char* who = "vaek_log_likelihood_workspace_bytes";
    if (!ctx || !bytes) { set_error("%s: null argument", who); return VAEK_ERR_INVALID; }
    if (int rc = check_replica_count(who, n)) return rc;
    if (int rc = check_row_count(who, rows, 1, kLogLikMaxRows, "vaek_log_likelihood_max_rows")) return rc;
    *bytes = loglik_workspace_bytes(n, rows);
    return VAEK_OK;
}

int vaek_log_likelihood_replicas(vaek_ctx* ctx, const float* params, const vaek_log_likelihood* ll, int32_t kind, const float* A, int32_t dd,
                                 int32_t did, int32_t pad, float var_added, uint32_t x_tag, uint32_t z_tag, void* workspace, void* stream) {
    const char* who = "vaek_log_likelihood_replicas";
    ProfBind pb(ctx);
    const LogLikVariant* var = ctx ? pick_loglik(ctx) : nullptr;
    const EvalDesc d = describe(ll);
    EvalRules r{};
    r.covered = var != nullptr;
    r.needs = "needs a float32 linear VAE (no hidden layers) with D, L <= 32, D <= 28 with two decoders (see vaek_supports_log_likelihood)";
    r.rows_min = 1; r.rows_cap = kLogLikMaxRows; r.rows_query = "vaek_log_likelihood_max_rows";
    r.records = 1; r.record_len = kLogLikRecord; r.record_query = "vaek_log_likelihood_record_len";
    r.draws = true; r.kind = kind; r.A = A; r.dd = dd; r.did = did; r.pad = pad; r.x_tag = x_tag;
    r.has_z_tag = true; r.z_tag = z_tag;
    r.workspace = workspace; r.ws_align = 8; r.ws_query = "vaek_log_likelihood_workspace_bytes";
    if (int rc = check_eval(who, ctx, params, d, r)) return rc;
    if (int rc = check_sample_count(who, ll->samples)) return rc;
    const int tiles = (ll->rows + 255) / 256;
    LogLikArgs a{};
    a.params = params; a.state_stride = ll->state_stride;
    a.x_seeds = reinterpret_cast<const unsigned long long*>(ll->x_seeds); a.x_steps = ll->x_steps;
    a.z_seeds = reinterpret_cast<const unsigned long long*>(ll->z_seeds); a.z_steps = ll->z_steps;
    a.x = ll->x; a.x_stride = ll->x_stride;
    a.part = static_cast<double*>(workspace);
    a.rows = ll->rows; a.samples = ll->samples; a.D = ctx->D; a.L = ctx->L; a.off_epsp = (int)ctx->off_epsp; a.off_eps = (int)ctx->off_eps;
    a.eps_cli = ctx->cfg.eps_cli; a.z_tag = z_tag;
    fill_rows_source(&a.gen, &a.a_stride, ctx, ll->rows, d.explicit_rows(), kind, A, dd, did, pad, var_added, x_tag, ll->a_stride);
    hipStream_t st = (hipStream_t)stream;
    {
        ProfScope ps("linear_loglik_replicas", st);
        launch_k(ps, var->fn, dim3((unsigned)tiles, (unsigned)ll->n), dim3(256), 0, st, a);
    }
    VAEK_HIP_CHECK(hipGetLastError());
    return loglik_finalize("linear_loglik_finalize", ctx, params, ll, a.part, st);
}

}  // extern "C"
