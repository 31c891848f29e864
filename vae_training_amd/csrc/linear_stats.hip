// The stats event of a replica sweep (vaek_stats_event_replicas): what the reference's compute_stats() does for ONE model at every
// n_print step (model.py:153-168) -- draw 1000 real rows and 1000 latent rows, VAE.loss on them (networks.py:103-113), sample a fake
// batch from the SAME latents (networks.py:62-65, vae.py:191-201), score it (datasets.py score_batch) -- for N models of one shape
// in ONE launch: workgroup r evaluates model r and stores one record of 8 + L floats.
//
// The shape of the launch is linear_resident.hip's replica form: no cross-workgroup state, no counter, no wait, no atomic.  It is
// simpler than that kernel in every other respect, because nothing is trained:
//
//   - a thread owns a ROW.  It draws the row's dataset values and latents with the functions of rng_dev.h (the ones
//     vaek_make_batch's kernel runs: the same bits), evaluates encoder, decoder(s), residual and score for that row in registers and
//     adds the row's sums to float64 accumulators of its own; its next row is 256 further on.  No batch, no activation and no
//     partial sum ever exists in HBM, and the row loop has no barrier;
//   - the <= 3.2 K parameter floats live in a zero-padded LDS image [DP][LP] / [LP][DP].  Every lane of a wave reads the SAME weight
//     at the same time, which LDS serves as a broadcast (one access, no bank conflict), 16 bytes at a time because DP and LP are
//     multiples of 4.  The zero padding is what lets the loops run to the compile-time DP, LP with static register indices (a
//     per-thread array indexed at run time would live in scratch memory: see rng_dev.h): a padded weight row or column adds 0;
//   - the products are VALU fmas, not matrix-core blocks: with one row per thread the whole chain of a row stays in that thread's
//     registers and needs no operand image, no transposes and no barrier -- an event is 1000 rows x (3 or 5) skinny products per
//     model, microseconds either way, against two dozen launches and five host synchronisations per model on the host path;
//   - per-element arithmetic is float32; every sum over ROWS is float64: per thread over its rows in row order, then across the
//     workgroup by a fixed binary tree in LDS.  A record therefore depends on neither n, nor the replica index, nor the run.
//
// The kernel reads params, A and the per-replica tables and stores only the records, with per-lane vector stores; it reads nothing
// back.
#include "eval_dev.h"
#include "mfma_geom.h"
#include "eval_check.h"

namespace vaek {

constexpr int kStatsMaxRows = 4096;          // rows per event: bounds one launch on a shared machine -- a cap, not a tuned value
constexpr int kStatsHead = 8;                // floats of a record in front of the epsilon_p copy
constexpr int kStatsSums = 7;                // float64 row sums: mse part, |mu|^2, five score sums

struct StatsArgs {
    const float* params; long long state_stride;
    const unsigned long long* x_seeds; const unsigned* x_steps;      // [n]: the real batch's Philox key and step
    const unsigned long long* z_seeds; const unsigned* z_steps;      // [n]: the latents'
    const float* sample_eps;                                         // [n]: eps of the sampling pass
    long long a_stride;
    float* out; long long out_stride;
    int rows, D, L, off_epsp, off_eps;
    float eps_cli;
    unsigned z_tag;
    BatchArgs gen;                 // kind, A, dd, did, pad, noise_std, tag = x_tag, D, L; seed / step / pointers are not used
};

template <int DP, int LP, bool SIG>
__global__ __launch_bounds__(256) void linear_stats_kernel(const StatsArgs a) {
    using G = ParamImage<DP, LP, SIG>;
    __shared__ __attribute__((aligned(16))) float W[G::N];
    __shared__ double red[kStatsSums][256];
    const int t = threadIdx.x;
    const long long r = blockIdx.x;
    const int D = a.D, L = a.L;
    const float* const p = a.params + r * a.state_stride;

    G::fill(W, p, D, L, a.off_epsp, t);                                 // the parameter image: zero outside [D] x [L]
    __syncthreads();

    BatchArgs gx = a.gen;
    if (gx.A) gx.A += r * a.a_stride;
    BatchArgs gz = gx;
    gz.tag = a.z_tag;
    const uint2 xkey = philox_key(a.x_seeds[r]), zkey = philox_key(a.z_seeds[r]);
    const unsigned xstep = a.x_steps[r], zstep = a.z_steps[r];
    const float eps = a.off_eps >= 0 ? p[a.off_eps] * a.eps_cli : a.eps_cli;
    const float inv_var = expf(-eps), sigma = expf(0.5f * eps), ssigma = expf(0.5f * a.sample_eps[r]);
    const int kind = gx.kind, dd = gx.dd;
    const int zq0 = L >> 2, zsh = L & 3, nzb = (L + D + 3) / 4;       // z2 starts at element zsh of latent block zq0

    // ya = a W + b and yb = b W + b over the image in ONE pass over the weights (and the sigmoid head's pre-activations): rows
    // l >= L of the image are zero, so whatever the inputs hold there adds nothing
    auto decode2 = [&](const float (&ina)[LP], const float (&inb)[LP], float (&ya)[DP], float (&ysa)[SIG ? DP : 1], float (&yb)[DP],
                       float (&ysb)[SIG ? DP : 1]) {
#pragma unroll
        for (int d = 0; d < DP; ++d) {
            ya[d] = yb[d] = W[G::BD + d];
            if (SIG) ysa[d] = ysb[d] = W[G::BS + d];
        }
#pragma unroll
        for (int l = 0; l < LP; ++l) {
            if (l < L) {
#pragma unroll
                for (int d = 0; d < DP; ++d) {
                    const float w = W[G::WD + l * DP + d];
                    ya[d] = fmaf(ina[l], w, ya[d]);
                    yb[d] = fmaf(inb[l], w, yb[d]);
                    if (SIG) {
                        const float ws = W[G::WS + l * DP + d];
                        ysa[d] = fmaf(ina[l], ws, ysa[d]);
                        ysb[d] = fmaf(inb[l], ws, ysb[d]);
                    }
                }
            }
        }
    };

    double acc[kStatsSums];
#pragma unroll
    for (int k = 0; k < kStatsSums; ++k) acc[k] = 0.0;

    for (int row = t; row < a.rows; row += 256) {
        // the image is loop-invariant, and a compiler that knows it lifts thousands of weights out of the loop and spills them: every
        // row reads them again (broadcast LDS reads, 16 bytes each)
        asm volatile("" ::: "memory");
        // ---- the real row: vaek_make_batch's work item for (row, c0), all c0 (columns >= D of the last piece are not part of it).  This
        // and the encoder product below are linear_loglik.hip's text too: keep the two in step (eval_dev.h says why they are not shared)
        float x[DP];
        {
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
        // ---- the latent row: normal n is element n & 3 of block n >> 2; [0, L) is z1, [L, L + D) z2 ------------------------------
        float z1[LP], z2[DP];
#pragma unroll
        for (int q = 0; q < LP / 4; ++q) {
            float n4[4] = {0.f, 0.f, 0.f, 0.f};
            if (4 * q < L) latent_block(gz, zstep, row, zkey, q, n4);
#pragma unroll
            for (int c = 0; c < 4; ++c) z1[4 * q + c] = n4[c];            // elements >= L of the last block belong to z2: unused here
        }
        {
            // z2[4 j + k] is element zsh + k of the eight normals of blocks zq0 + j and zq0 + j + 1: zsh is uniform, every index static
            float cat[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            {
                float n4[4];
                latent_block(gz, zstep, row, zkey, zq0, n4);
                cat[4] = n4[0]; cat[5] = n4[1]; cat[6] = n4[2]; cat[7] = n4[3];
            }
#pragma unroll
            for (int j = 0; j < DP / 4; ++j) {
                if (4 * j < D) {
                    float n4[4] = {0.f, 0.f, 0.f, 0.f};
                    if (zq0 + j + 1 < nzb) latent_block(gz, zstep, row, zkey, zq0 + j + 1, n4);
#pragma unroll
                    for (int c = 0; c < 4; ++c) { cat[c] = cat[4 + c]; cat[4 + c] = n4[c]; }
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        z2[4 * j + k] = zsh == 0 ? cat[k] : (zsh == 1 ? cat[k + 1] : (zsh == 2 ? cat[k + 2] : cat[k + 3]));
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) z2[4 * j + k] = 0.f;
                }
            }
        }

        // ---- VAE.loss on (x, z1, z2): mu = Encoder(x), samples = mu + e^{lv/2} z1, x_hat = Decoder(samples) [+ sigmoid] + sigma z2 ----
        float smp[LP];
        float musq = 0.f;
        {
            float mu[LP];
#pragma unroll
            for (int l = 0; l < LP; ++l) mu[l] = W[G::BE + l];
#pragma unroll
            for (int d = 0; d < DP; ++d) {
                if (d < D) {
#pragma unroll
                    for (int l = 0; l < LP; ++l) mu[l] = fmaf(x[d], W[G::WE + d * LP + l], mu[l]);
                }
            }
#pragma unroll
            for (int l = 0; l < LP; ++l) {
                musq = fmaf(mu[l], mu[l], musq);                          // mu[l >= L] = 0
                smp[l] = fmaf(W[G::SD + l], z1[l], mu[l]);                // e^{lv/2} of the image is 0 at l >= L
            }
        }
        // the fake row comes from the SAME latents (mu = 0, logvar_e = 0 -> samples = z1): both decoder passes share one read of the weights
        float y[DP], ys[SIG ? DP : 1], yf[DP], ysf[SIG ? DP : 1];
        decode2(smp, z1, y, ys, yf, ysf);
        float rsq = 0.f;
#pragma unroll
        for (int d = 0; d < DP; ++d) {
            float xh = fmaf(sigma, z2[d], y[d]);
            if (SIG) xh += 1.f / (1.f + expf(-ys[d]));
            const float rr = d < D ? xh - x[d] : 0.f;
            rsq = fmaf(rr, rr, rsq);
        }
        acc[0] += (double)(0.5f * rsq * inv_var);
        acc[1] += (double)musq;

        // ---- the fake row and its score; eps = the caller's current_epsilon -----------------------------------------------
        float lo = 0.f, hi = 0.f, atdd = 0.f, dot = 0.f;      // sum of squares of columns < dd and > dd, column dd, fake[:dd] . A
#pragma unroll
        for (int d = 0; d < DP; ++d) {
            float f = fmaf(ssigma, z2[d], yf[d]);
            if (SIG) f += 1.f / (1.f + expf(-ysf[d]));
            if (d < dd) {
                lo = fmaf(f, f, lo);
                if (kind == 1) dot = fmaf(f, gx.A[d], dot);
            } else if (d < D) {
                if (d == dd) atdd = f; else hi = fmaf(f, f, hi);
            }
        }
        if (kind == 1) {                 // datasets.py:179-183: columns > dd, and the four sums of the all-pairs manifold error
            const double yv = (double)atdd, cv = (double)dot;
            acc[2] += (double)hi;
            acc[3] += yv; acc[4] += yv * yv; acc[5] += cv; acc[6] += cv * cv;
        } else {                         // :138 columns >= dd;  :95-97 (|fake[:dd]| - 1)^2 and columns >= dd
            acc[2] += (double)fmaf(atdd, atdd, hi);
            if (kind == 2) { const float e = sqrtf(lo) - 1.f; acc[3] += (double)(e * e); }
        }
    }

    // ---- the workgroup's sums: a fixed binary tree over the 256 threads ---------------------------------------------
#pragma unroll
    for (int k = 0; k < kStatsSums; ++k) red[k][t] = acc[k];
    tree_sum256(red, t);

    // ---- the record: lane t stores float t ------------------------------------------------------------------
    if (t < kStatsHead + L) {
        const double n = (double)a.rows;
        float v = 0.f;
        if (t < 3) {
            double klc = 0.0;
            for (int l = 0; l < L; ++l) { const float lv = W[G::LV + l]; klc += (double)(1.f + lv - expf(lv)); }
            const double dkl = 0.5 * red[1][0] / n - 0.5 * klc;                                   // networks.py:94
            const double mse = red[0][0] / n + 0.5 * (double)D * ((double)kLog2Pi + (double)eps);      // :95-96
            v = (float)(t == 0 ? dkl + mse : (t == 1 ? dkl : mse));
        } else if (t == 3) {
            v = eps;
        } else if (t == 4) {
            v = (float)((kind == 2 ? red[3][0] : red[2][0]) / n);
        } else if (t == 5) {
            if (kind == 1) {
                // mean over ALL pairs (i, j) of (y_j - c_i)^2, the reference's (B,) against (B, 1) broadcast
                const double my = red[3][0] / n, mc = red[5][0] / n;
                v = (float)(red[4][0] / n - 2.0 * my * mc + red[6][0] / n);
            } else if (kind == 2) {
                v = (float)(red[2][0] / n);
            }
        } else if (t >= kStatsHead) {
            v = W[G::LV + t - kStatsHead];
        }
        a.out[r * a.out_stride + t] = v;
    }
}

// ---- variant table: the padded shapes of the resident loop (mfma_geom.h), each side rounded up to a multiple of 4; a context
// takes the smallest that holds it (an EXACT shape of that table is one more padded shape here) ---------------------------------
typedef void (*StatsKernel)(const StatsArgs);
struct StatsVariant { int dp, lp, sig; StatsKernel fn; };
#define VAEK_STATS_ROW(DP, LP, SIG, EXACT) {up4(DP), up4(LP), SIG, linear_stats_kernel<up4(DP), up4(LP), (SIG) != 0>},
static const StatsVariant kStatsVariants[] = {VAEK_EVAL_SHAPES(VAEK_STATS_ROW)};
#undef VAEK_STATS_ROW

static const StatsVariant* pick_stats(const vaek_ctx* c) { return pick_smallest_shape(kStatsVariants, c->D, c->L, c->cfg.sigmoid_decoder != 0); }

}  // namespace vaek

using namespace vaek;

extern "C" {

int vaek_supports_stats_event(const vaek_ctx* ctx, int32_t kind, int32_t* yes) {
    if (!ctx || !yes) { set_error("vaek_supports_stats_event: null argument"); return VAEK_ERR_INVALID; }
    *yes = ctx->resident && kind >= 0 && kind <= 2 && pick_stats(ctx) ? 1 : 0;
    return VAEK_OK;
}

int vaek_stats_record_len(const vaek_ctx* ctx, int64_t* floats) {
    if (!ctx || !floats) { set_error("vaek_stats_record_len: null argument"); return VAEK_ERR_INVALID; }
    *floats = kStatsHead + (int64_t)ctx->L;
    return VAEK_OK;
}

int vaek_stats_event_max_rows(void) { return kStatsMaxRows; }

int vaek_stats_event_replicas(vaek_ctx* ctx, const float* params, const vaek_stats_event* ev, int32_t kind, const float* A, int32_t dd,
                              int32_t did, int32_t pad, float var_added, uint32_t x_tag, uint32_t z_tag, void* stream) {
    const char* who = "vaek_stats_event_replicas";
    ProfBind pb(ctx);
    const StatsVariant* var = ctx && ctx->resident ? pick_stats(ctx) : nullptr;
    const EvalDesc d = describe(ev);
    EvalRules r{};
    r.covered = var != nullptr; r.needs = "needs a context vaek_train_loop_gen covers (see vaek_supports_stats_event)";
    r.rows_min = 1; r.rows_cap = kStatsMaxRows; r.rows_query = "vaek_stats_event_max_rows";
    r.records = 1; r.record_len = ctx ? kStatsHead + (int64_t)ctx->L : 0; r.record_query = "vaek_stats_record_len";
    r.draws = true; r.kind = kind; r.A = A; r.dd = dd; r.did = did; r.pad = pad; r.x_tag = x_tag;
    r.has_z_tag = true; r.z_tag = z_tag;
    if (int rc = check_eval(who, ctx, params, d, r)) return rc;
    StatsArgs a{};
    a.params = params; a.state_stride = ev->state_stride;
    a.x_seeds = reinterpret_cast<const unsigned long long*>(ev->x_seeds); a.x_steps = ev->x_steps;
    a.z_seeds = reinterpret_cast<const unsigned long long*>(ev->z_seeds); a.z_steps = ev->z_steps;
    a.sample_eps = ev->sample_eps; a.a_stride = ev->a_stride;
    a.out = ev->out; a.out_stride = ev->out_stride;
    a.rows = ev->rows; a.D = ctx->D; a.L = ctx->L; a.off_epsp = (int)ctx->off_epsp; a.off_eps = (int)ctx->off_eps;
    a.eps_cli = ctx->cfg.eps_cli; a.z_tag = z_tag;
    fill_draw_args(&a.gen, ctx, ev->rows, kind, A, dd, did, pad, var_added, x_tag);
    hipStream_t st = (hipStream_t)stream;
    {
        ProfScope ps("linear_stats_replicas", st);
        launch_k(ps, var->fn, dim3((unsigned)ev->n), dim3(256), 0, st, a);
    }
    VAEK_HIP_CHECK(hipGetLastError());
    return VAEK_OK;
}

}  // extern "C"
