// Importance-weighted log-likelihood of N three-hidden-layer MLP VAEs of one shape (vaek_mlp3_log_likelihood_replicas): the
// estimator, the record, the block rule of the samples and the two row modes of linear_loglik.hip (vaek_log_likelihood_replicas),
// with Encoder and Decoder the four-Dense relu stacks of networks.py:26-44:
//   mu      = Encoder(x)
//   z_k     = mu + exp(epsilon_p / 2) xi_k
//   log w_k = -1/2 [ |Decoder(z_k) - x|^2 e^{-eps} + D (eps + log 2 pi) ] + 1/2 sum_l ( xi_kl^2 - z_kl^2 + epsilon_p[l] ).
// A decoder pass per SAMPLE is ~85 000 weights at 200|200|200, so unlike the linear call nothing fits a thread: every product is
// v_mfma_f32_16x16x4_f32 (exact f32), units on the rows and rows / samples on the columns: the Dense chain of mlp3_dev.h (ml_dense,
// ml_stack; one text with mlp3_stats.hip), the operand scheme of fused_mlp3.hip's m3_dense restated forward-only with TWO changes: a
// fetched weight operand feeds CB column blocks of 16, so a workgroup streams the weights once per 16 CB columns instead of once per
// 16; and a k-step wholly past K is skipped.
//
// FOUR launches per call whatever n is, ordered by the stream alone; nothing stored in a launch is read back inside it, and there
// is no atomic, counter, wait or status word:
//   1. mlp3_loglik_encode   grid (ceil(rows / 16), n): columns are data rows.  Reads the caller's rows or draws them with the functions
//      of rng_dev.h (the bits vaek_make_batch writes) and stores them in the workspace; runs the encoder; stores mu[n][rows][L].
//   2. mlp3_loglik_sample   grid (ceil(rows K / NC), n): columns of replica r are the flattened pairs j = row K + k.  A workgroup takes
//      NC contiguous columns -- many rows at small K, part of one row at large K --, builds z as a [unit][column] LDS image (sample k
//      of a row from Philox blocks k ceil(L / 4) + q of the row's latent stream), runs the four decoder products between two
//      ping-pong images, reduces |dec - x|^2 and the sum over l per column and stores log w into lw[n][rows][K].  Columns past rows K
//      are computed on clamped indices and not stored.  A column's arithmetic does not depend on its place in the tile or on its
//      neighbours: MFMA columns are independent, and every per-column reduction is one thread walking that column in a fixed order.
//   3. mlp3_loglik_rows     grid (ceil(rows / 256), n): a thread owns a row; the online log-sum-exp of linear_loglik.hip (eval_dev.h:
//      one text) over k in k order (float32, branch-free), the three row values to float64, a fixed binary tree over the tile, one
//      4-double partial.
//   4. mlp3_loglik_finalize n workgroups: the tiles in tile order, then the record, lane t storing float t (linear_loglik.hip's
//      loglik_finalize: one kernel for both calls).
// mlp3_dev.h describes the LDS images and the weight reads (no stride rule).
#include "mlp3_dev.h"
#include "eval_check.h"

namespace vaek {

constexpr int kMl3MaxColumns = 1 << 22;      // n * rows * samples: bounds the workspace and the length of a call -- a cap, not a tuned value
constexpr int ML_QB = ML_F / 4;              // Philox blocks of one sample, at most
constexpr int ML_ENC_NC = 16;                // columns of an encode tile
#ifndef VAEK_ML3_NC
#define VAEK_ML3_NC 64                       // columns of a sample tile: 64 or 32 (DESIGN 3.14 has the timing of both)
#endif
constexpr int ML_NC = VAEK_ML3_NC;
static_assert(ML_NC == 32 || ML_NC == 64, "a sample tile is two or four 16-column blocks");

struct Ml3Args {
    const float* params; long long state_stride;
    const unsigned long long* x_seeds; const unsigned* x_steps;      // [n]: the rows' Philox key and step (drawing mode)
    const unsigned long long* z_seeds; const unsigned* z_steps;      // [n]: the samples'
    long long a_stride;
    const float* x; long long x_stride;      // the rows a launch READS: the caller's, or (sample launch, drawing mode) the workspace's
    float* x_out;                            // encode launch, drawing mode: where the drawn rows go, [n][rows][D]; else NULL
    float* mu;                               // [n][rows][L]: written by the encode launch, read by the sample launch
    float* lw;                               // [n][rows][K]: written by the sample launch
    int rows, samples, D, L, off_epsp, off_eps;
    float eps_cli;
    unsigned z_tag;
    Ml3Net net;                              // the encoder's layers (encode launch) or the decoder's (sample launch)
    BatchArgs gen;                           // kind, A, dd, did, pad, noise_std, tag = x_tag, D, L
};

struct Ml3RowsArgs { const float* lw; double* part; int rows, samples; };

// ---- launch 1: rows -> mu ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ML_NT) void mlp3_loglik_encode_kernel(const Ml3Args a) {
    constexpr int NC = ML_ENC_NC;
    extern __shared__ __attribute__((aligned(16))) char ml_smem[];
    float* const img0 = reinterpret_cast<float*>(ml_smem);
    float* const img1 = img0 + ML_W * NC;
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const long long r = blockIdx.y;
    const int row0 = blockIdx.x * NC;
    const int D = a.D, L = a.L;
    const float* const P = a.params + r * a.state_stride;

    if (a.x) {                                   // the caller's rows
        const float* const xr = a.x + r * a.x_stride;
        for (int e = t; e < D * NC; e += ML_NT) {
            const int c = e & (NC - 1), d = e / NC;
            img0[ml_at<NC>(d, c)] = xr[(long long)min(row0 + c, a.rows - 1) * D + d];
        }
    } else if (t < NC * ML_QB) {                 // vaek_make_batch's work item for (row, c0): four columns of one row
        const int c = t & (NC - 1), c0 = 4 * (t / NC);
        if (c0 < D) {
            BatchArgs gx = a.gen;
            if (gx.A) gx.A += r * a.a_stride;
            const uint2 xkey = philox_key(a.x_seeds[r]);
            const unsigned xstep = a.x_steps[r];
            const int row = min(row0 + c, a.rows - 1);
            float nrm[16], o[4];
            dataset_normals(gx, xstep, row, xkey, nrm);
            dataset_cols4(gx, xstep, row, xkey, nrm, c0, o);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (c0 + i < D) {
                    img0[ml_at<NC>(c0 + i, c)] = o[i];
                    if (row0 + c < a.rows) a.x_out[(r * a.rows + row) * D + c0 + i] = o[i];
                }
            }
        }
    }
    __syncthreads();
    ml_stack<NC>(P, a.net, img0, img1, wave, lane);
    for (int e = t; e < L * NC; e += ML_NT) {    // mu is img0's rows [0, L)
        const int c = e / L, l = e - c * L;
        if (row0 + c < a.rows) a.mu[(r * a.rows + row0 + c) * L + l] = img0[ml_at<NC>(l, c)];
    }
}

// ---- launch 2: (row, k) -> log w -----------------------------------------------------------------------------------------------------
// (32 columns: 64 KB of images, so two workgroups fit a CU if the registers do -- the second bound asks for that)
__global__ __launch_bounds__(ML_NT, ML_NC == 32 ? 2 : 1) void mlp3_loglik_sample_kernel(const Ml3Args a) {
    constexpr int NC = ML_NC;
    extern __shared__ __attribute__((aligned(16))) char ml_smem[];
    float* const img0 = reinterpret_cast<float*>(ml_smem);
    float* const img1 = img0 + ML_W * NC;
    __shared__ float qsp[ML_QB][NC];             // per Philox block of a column: sum of xi^2 - z^2 over its (up to) four elements
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const long long r = blockIdx.y;
    const int D = a.D, L = a.L, K = a.samples;
    const int total = a.rows * K;                // <= 2^22
    const int col0 = blockIdx.x * NC;
    const float* const P = a.params + r * a.state_stride;
    const int nlb = (L + 3) >> 2;

    // ---- z = mu + e^{lv/2} xi as rows [0, L) of img0; thread (column c, block q) draws one Philox block -----------------------------
    {
        BatchArgs gz = a.gen;
        gz.tag = a.z_tag;
        const uint2 zkey = philox_key(a.z_seeds[r]);
        const unsigned zstep = a.z_steps[r];
        const float* const mu = a.mu + r * a.rows * L;
        for (int e = t; e < NC * nlb; e += ML_NT) {
            const int c = e & (NC - 1), q = e / NC;
            const int j = min(col0 + c, total - 1);
            const int row = j / K, k = j - row * K;
            float n4[4];
            latent_block(gz, zstep, row, zkey, k * nlb + q, n4);
            float qs = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int l = 4 * q + i;
                if (l < L) {                     // elements >= L of the last block are not part of the sample
                    const float z = fmaf(expf(0.5f * P[a.off_epsp + l]), n4[i], mu[(long long)row * L + l]);      // e^{lv/2}, networks.py:73
                    qs = fmaf(n4[i], n4[i], qs);
                    qs = fmaf(-z, z, qs);
                    img0[ml_at<NC>(l, c)] = z;
                }
            }
            qsp[q][c] = qs;
        }
    }
    __syncthreads();
    ml_stack<NC>(P, a.net, img0, img1, wave, lane);      // Decoder(z) is img0's rows [0, D)

    // ---- log w: thread c walks its column, d and q in order ---------------------------------------------------------------------------
    if (t < NC) {
        const int c = t;
        const int j = min(col0 + c, total - 1);
        const int row = j / K;
        const float* const xr = a.x + r * a.x_stride + (long long)row * D;
        const float eps = a.off_eps >= 0 ? P[a.off_eps] * a.eps_cli : a.eps_cli;
        float rsq = 0.f, qs = 0.f, lvsum = 0.f;
        for (int d = 0; d < D; ++d) {
            const float rr = img0[ml_at<NC>(d, c)] - xr[d];
            rsq = fmaf(rr, rr, rsq);
        }
        for (int q = 0; q < nlb; ++q) qs += qsp[q][c];
        for (int l = 0; l < L; ++l) lvsum += P[a.off_epsp + l];
        const float c0 = 0.5f * lvsum - 0.5f * (float)D * (eps + kLog2Pi);
        const float lw = c0 + 0.5f * (qs - rsq * expf(-eps));
        if (col0 + c < total) a.lw[r * total + j] = lw;
    }
}

// ---- launch 3: per row the online log-sum-exp over k, per tile of 256 rows the float64 sums -----------------------------------------
__global__ __launch_bounds__(256) void mlp3_loglik_rows_kernel(const Ml3RowsArgs a) {
    __shared__ double red[kLogLikSums][256];
    const int t = threadIdx.x;
    const int tile = blockIdx.x;
    const long long r = blockIdx.y;
    const int row = tile * 256 + t;
    const int K = a.samples;
    float res[kLogLikSums] = {0.f, 0.f, 0.f};
    if (row < a.rows) {
        const float* const lwr = a.lw + (r * a.rows + row) * K;
        OnlineLogSumExp lse;
        for (int k0 = 0; k0 < K; k0 += 8) {
            float v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = lwr[min(k0 + i, K - 1)];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (k0 + i < K) lse.push(v[i]);
            }
        }
        lse.finish(K, res);
    }
#pragma unroll
    for (int j = 0; j < kLogLikSums; ++j) red[j][t] = (double)res[j];
    tree_sum256(red, t);
    store_tile_partial(a.part, r, tile, t, red);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
// float32, one decoder, exactly three hidden layers of 64 .. 256 units both ways (any mix of widths), D, L <= 32.  Nothing about the
// batch, the world or force_generic: the call reads parameters only
bool mlp3_loglik_supported(const vaek_ctx* c) {
    const vaek_config& f = c->cfg;
    if (f.dtype != VAEK_F32 || f.sigmoid_decoder || f.n_enc_hidden != 3 || f.n_dec_hidden != 3) return false;
    for (int i = 0; i < 3; ++i)
        if (f.enc_hidden[i] < 64 || f.enc_hidden[i] > ML_W || f.dec_hidden[i] < 64 || f.dec_hidden[i] > ML_W) return false;
    return c->D <= ML_F && c->L <= ML_F && c->enc.layers.size() == 4 && c->dec.layers.size() == 4;
}

static int ml3_tiles(int rows) { return (rows + 255) / 256; }
static size_t ml3_up16(size_t b) { return (b + 15) & ~(size_t)15; }
// the workspace: tile partials [n][tiles][4] doubles, then x [n][rows][D], mu [n][rows][L], lw [n][rows][K] floats, each 16-byte aligned
struct Ml3Ws { size_t x, mu, lw, total; };
static Ml3Ws ml3_workspace(const vaek_ctx* c, int n, int rows, int samples) {
    Ml3Ws w;
    w.x = ml3_up16(sizeof(double) * 4 * (size_t)n * ml3_tiles(rows));
    w.mu = w.x + ml3_up16(sizeof(float) * (size_t)n * rows * c->D);
    w.lw = w.mu + ml3_up16(sizeof(float) * (size_t)n * rows * c->L);
    w.total = w.lw + ml3_up16(sizeof(float) * (size_t)n * rows * samples);
    return w;
}

}  // namespace vaek

using namespace vaek;

extern "C" {

int vaek_supports_mlp3_log_likelihood(const vaek_ctx* ctx, int32_t kind, int32_t* yes) {
    if (!ctx || !yes) { set_error("vaek_supports_mlp3_log_likelihood: null argument"); return VAEK_ERR_INVALID; }
    *yes = kind >= 0 && kind <= 2 && ctx->mlp3_loglik ? 1 : 0;
    return VAEK_OK;
}

int vaek_mlp3_log_likelihood_max_columns(void) { return kMl3MaxColumns; }

int vaek_mlp3_log_likelihood_workspace_bytes(const vaek_ctx* ctx, int32_t n, int32_t rows, int32_t samples, size_t* bytes) {
    const char* who = "vaek_mlp3_log_likelihood_workspace_bytes";
    if (!ctx || !bytes) { set_error("%s: null argument", who); return VAEK_ERR_INVALID; }
    if (int rc = check_replica_count(who, n)) return rc;
    if (int rc = check_row_count(who, rows, 1, kLogLikMaxRows, "vaek_log_likelihood_max_rows")) return rc;
    if (int rc = check_sample_count(who, samples)) return rc;
    if (int rc = check_column_count(who, n, rows, samples, "samples", kMl3MaxColumns, "vaek_mlp3_log_likelihood_max_columns")) return rc;
    *bytes = ml3_workspace(ctx, n, rows, samples).total;
    return VAEK_OK;
}

int vaek_mlp3_log_likelihood_replicas(vaek_ctx* ctx, const float* params, const vaek_log_likelihood* ll, int32_t kind, const float* A, int32_t dd,
                                      int32_t did, int32_t pad, float var_added, uint32_t x_tag, uint32_t z_tag, void* workspace, void* stream) {
    const char* who = "vaek_mlp3_log_likelihood_replicas";
    ProfBind pb(ctx);
    char needs[256];
    snprintf(needs, sizeof(needs), "needs a float32 VAE with one decoder and three hidden layers of 64 .. %d units both ways, D, L <= %d (see "
             "vaek_supports_mlp3_log_likelihood)", ML_W, ML_F);
    const EvalDesc d = describe(ll);
    EvalRules r{};
    r.covered = ctx && ctx->mlp3_loglik; r.needs = needs;
    r.rows_min = 1; r.rows_cap = kLogLikMaxRows; r.rows_query = "vaek_log_likelihood_max_rows";
    r.records = 1; r.record_len = kLogLikRecord; r.record_query = "vaek_log_likelihood_record_len";
    r.draws = true; r.kind = kind; r.A = A; r.dd = dd; r.did = did; r.pad = pad; r.x_tag = x_tag;
    r.has_z_tag = true; r.z_tag = z_tag;
    r.workspace = workspace; r.ws_align = 16; r.ws_query = "vaek_mlp3_log_likelihood_workspace_bytes";
    if (int rc = check_eval(who, ctx, params, d, r)) return rc;
    if (int rc = check_sample_count(who, ll->samples)) return rc;
    if (int rc = check_column_count(who, ll->n, ll->rows, ll->samples, "samples", kMl3MaxColumns, "vaek_mlp3_log_likelihood_max_columns")) return rc;
    const bool explicit_rows = d.explicit_rows();
    const int n = ll->n, rows = ll->rows, K = ll->samples, tiles = ml3_tiles(rows);
    const Ml3Ws w = ml3_workspace(ctx, n, rows, K);
    char* const ws = static_cast<char*>(workspace);
    Ml3Args a{};
    a.params = params; a.state_stride = ll->state_stride;
    a.x_seeds = reinterpret_cast<const unsigned long long*>(ll->x_seeds); a.x_steps = ll->x_steps;
    a.z_seeds = reinterpret_cast<const unsigned long long*>(ll->z_seeds); a.z_steps = ll->z_steps;
    a.x = ll->x; a.x_stride = ll->x_stride;
    a.x_out = explicit_rows ? nullptr : reinterpret_cast<float*>(ws + w.x);
    a.mu = reinterpret_cast<float*>(ws + w.mu);
    a.lw = reinterpret_cast<float*>(ws + w.lw);
    a.rows = rows; a.samples = K; a.D = ctx->D; a.L = ctx->L; a.off_epsp = (int)ctx->off_epsp; a.off_eps = (int)ctx->off_eps;
    a.eps_cli = ctx->cfg.eps_cli; a.z_tag = z_tag;
    fill_rows_source(&a.gen, &a.a_stride, ctx, rows, explicit_rows, kind, A, dd, did, pad, var_added, x_tag, ll->a_stride);
    ml3_net(ctx->enc, &a.net);
    Ml3Args s = a;                               // the sample launch reads the rows the encode launch read or drew
    if (!explicit_rows) { s.x = a.x_out; s.x_stride = (long long)rows * ctx->D; }
    s.x_out = nullptr;
    ml3_net(ctx->dec, &s.net);
    Ml3RowsArgs ra{};
    ra.lw = a.lw; ra.part = reinterpret_cast<double*>(ws); ra.rows = rows; ra.samples = K;

    constexpr size_t lds_enc = sizeof(float) * 2 * ML_W * ML_ENC_NC, lds_smp = sizeof(float) * 2 * ML_W * ML_NC;
    static thread_local PerDeviceOnce attr_set;
    VAEK_HIP_CHECK(set_max_dynamic_lds(attr_set, mlp3_loglik_sample_kernel, lds_smp));
    hipStream_t st = (hipStream_t)stream;
    {
        ProfScope ps("mlp3_loglik_encode", st);
        launch_k(ps, mlp3_loglik_encode_kernel, dim3((unsigned)((rows + ML_ENC_NC - 1) / ML_ENC_NC), (unsigned)n), dim3(ML_NT), lds_enc, st, a);
    }
    VAEK_HIP_CHECK(hipGetLastError());
    {
        ProfScope ps("mlp3_loglik_sample", st);
        launch_k(ps, mlp3_loglik_sample_kernel, dim3((unsigned)((rows * K + ML_NC - 1) / ML_NC), (unsigned)n), dim3(ML_NT), lds_smp, st, s);
    }
    VAEK_HIP_CHECK(hipGetLastError());
    {
        ProfScope ps("mlp3_loglik_rows", st);
        launch_k(ps, mlp3_loglik_rows_kernel, dim3((unsigned)tiles, (unsigned)n), dim3(256), 0, st, ra);
    }
    VAEK_HIP_CHECK(hipGetLastError());
    return loglik_finalize("mlp3_loglik_finalize", ctx, params, ll, ra.part, st);
}

}  // extern "C"
