// The stats event of a sweep of three-hidden-layer MLP VAEs (vaek_mlp3_stats_event_replicas): what linear_stats.hip's launch does for
// linear models -- per model a batch of real rows, a batch of latents, VAE.loss on them, a fake batch sampled from the SAME latents,
// its score, one record of 8 + L floats -- with Encoder and Decoder the four-Dense relu stacks of networks.py:26-44.  A stack is
// ~85 000 weights at 200|200|200, so a row does not fit a thread: the products are the matrix-core Dense chain of mlp3_dev.h (one
// text with mlp3_loglik.hip), rows on the columns of a [unit][column] LDS image.
//
// TWO launches per call whatever n is, ordered by the stream alone; nothing stored in a launch is read back inside it, and there is
// no atomic, counter, wait or status word:
//   1. mlp3_stats_tile      grid (ceil(rows / 32), n), 256 threads: a workgroup evaluates a tile of TR = 32 rows of replica blockIdx.y.
//      It draws the rows' x, z1, z2 with the functions of rng_dev.h (the bits vaek_make_batch writes), runs the encoder on 32
//      columns, then the decoder ONCE on 64: column c carries samples = mu + e^{lv/2} z1 of row c and column 32 + c carries z1 of
//      row c (the sampling pass: mu = 0, logvar_e = 0), so the decoder's weights are streamed once for both, as linear_stats.hip's
//      decode2 shares one read.  Then one thread per row walks its columns in index order (float32), the seven row values go to
//      float64 through a fixed binary tree over the tile, and one partial of 8 doubles is stored per (replica, tile).  Rows past
//      `rows` are computed on clamped indices and contribute 0.0.  A column's arithmetic does not depend on its place in the tile.
//   2. mlp3_stats_finalize  n workgroups: the tile partials in tile order, then linear_stats.hip's record, lane t storing float t.
//
// LDS of the tile launch: two [256][64] images = 128 KB (the encoder's [256][32] pair lives in the same bytes; the float64 tree
// takes the first 14 KB of the second image once the decoder is through), x [32][32], the latents [64][32] and mu [32][32] = 16 KB:
// 144 KB of the CU's 160, one workgroup per CU.  x has an array of its own because the chain overwrites its input image; the
// latents live in LDS because z1 / z2 start at run-time offsets of the row's normals (a per-thread array indexed at run time would
// live in scratch memory: see rng_dev.h).
#include "mlp3_dev.h"
#include "eval_check.h"

namespace vaek {

constexpr int MS_TR = 32;                    // rows of a tile = columns of the encoder pass
constexpr int MS_NC = 2 * MS_TR;             // columns of the decoder pass: samples | z1
constexpr int kMs3Head = 8;                  // floats of a record in front of the epsilon_p copy (vaek_stats_record_len = 8 + L)
constexpr int kMs3Sums = 7;                  // float64 row sums, linear_stats.hip's: mse part, |mu|^2, five score sums
constexpr int kMs3Part = 8;                  // doubles of a tile partial: the sums and a zero

struct Ms3Args {
    const float* params; long long state_stride;
    const unsigned long long* x_seeds; const unsigned* x_steps;      // [n]: the real batch's Philox key and step
    const unsigned long long* z_seeds; const unsigned* z_steps;      // [n]: the latents'
    const float* sample_eps;                                         // [n]: eps of the sampling pass
    long long a_stride;
    double* part;                                                    // [n][tiles][8]
    int rows, D, L, off_epsp, off_eps;
    float eps_cli;
    unsigned z_tag;
    Ml3Net enc, dec;
    BatchArgs gen;                 // kind, A, dd, did, pad, noise_std, tag = x_tag, D, L; seed / step / pointers are not used
};

struct Ms3FinalArgs {
    const float* params; long long state_stride;
    const double* part;
    float* out; long long out_stride;
    int rows, tiles, D, L, off_epsp, off_eps, kind;
    float eps_cli;
};

// ---- launch 1: a tile of rows -> one partial of the seven sums --------------------------------------------------------------------
__global__ __launch_bounds__(ML_NT) void mlp3_stats_tile_kernel(const Ms3Args a) {
    constexpr int TR = MS_TR, NC = MS_NC;
    extern __shared__ __attribute__((aligned(16))) char ms_smem[];
    float* const img0 = reinterpret_cast<float*>(ms_smem);
    __shared__ float xs[ML_F][TR];               // x[d][row of the tile]
    __shared__ float lat[2 * ML_F][TR];          // the row's latent normals: [0, L) z1, [L, L + D) z2
    __shared__ float mus[ML_F][TR];
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int tile = blockIdx.x;
    const long long r = blockIdx.y;
    const int row0 = tile * TR;
    const int D = a.D, L = a.L;
    const float* const P = a.params + r * a.state_stride;
    BatchArgs gx = a.gen;
    if (gx.A) gx.A += r * a.a_stride;

    // ---- the draws: thread (column c, piece c0) is vaek_make_batch's work item for four columns of a real row; thread (column c,
    // block q) draws block q of the row's latent stream: normal n is element n & 3 of block n >> 2 ------------------------------------
    {
        float* const img = img0;                 // the encoder's input image, [unit][32]
        const int c = t & (TR - 1), c0 = 4 * (t / TR);
        const int row = min(row0 + c, a.rows - 1);
        if (c0 < D) {
            const uint2 xkey = philox_key(a.x_seeds[r]);
            const unsigned xstep = a.x_steps[r];
            float nrm[16], o[4];
            dataset_normals(gx, xstep, row, xkey, nrm);
            dataset_cols4(gx, xstep, row, xkey, nrm, c0, o);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (c0 + i < D) {
                    xs[c0 + i][c] = o[i];
                    img[ml_at<TR>(c0 + i, c)] = o[i];
                }
            }
        }
        BatchArgs gz = a.gen;
        gz.tag = a.z_tag;
        const uint2 zkey = philox_key(a.z_seeds[r]);
        const unsigned zstep = a.z_steps[r];
        const int nzb = (L + D + 3) >> 2;        // <= 16: blocks 4 q + i < 64 stay inside lat
        for (int q = t / TR; q < nzb; q += ML_NT / TR) {
            float n4[4];
            latent_block(gz, zstep, row, zkey, q, n4);
#pragma unroll
            for (int i = 0; i < 4; ++i) lat[4 * q + i][c] = n4[i];
        }
    }
    __syncthreads();

    // ---- mu = Encoder(x): rows [0, L) of the 32-column image; kept aside before the images are rebuilt ------------------------------
    ml_stack<TR>(P, a.enc, img0, img0 + ML_W * TR, wave, lane);
    for (int e = t; e < L * TR; e += ML_NT) {
        const int c = e & (TR - 1), l = e / TR;
        mus[l][c] = img0[ml_at<TR>(l, c)];
    }
    __syncthreads();

    // ---- the decoder's input, [unit][64]: samples = mu + e^{lv/2} z1 (networks.py:73) | z1 ------------------------------------------------
    float* const img1 = img0 + ML_W * NC;
    for (int e = t; e < L * NC; e += ML_NT) {
        const int c = e & (NC - 1), l = e / NC;
        const int cc = c & (TR - 1);
        const float z1 = lat[l][cc];
        img0[ml_at<NC>(l, c)] = c < TR ? fmaf(expf(0.5f * P[a.off_epsp + l]), z1, mus[l][cc]) : z1;
    }
    __syncthreads();
    ml_stack<NC>(P, a.dec, img0, img1, wave, lane);      // Decoder(samples) | Decoder(z1): rows [0, D) of img0

    // ---- per row: thread c walks its two columns, d in index order; the terms are linear_stats.hip's ---------------------------------
    double v[kMs3Sums];
#pragma unroll
    for (int k = 0; k < kMs3Sums; ++k) v[k] = 0.0;
    if (t < TR && row0 + t < a.rows) {
        const int c = t;
        const float eps = a.off_eps >= 0 ? P[a.off_eps] * a.eps_cli : a.eps_cli;
        const float inv_var = expf(-eps), sigma = expf(0.5f * eps), ssigma = expf(0.5f * a.sample_eps[r]);
        const int kind = gx.kind, dd = gx.dd;
        float rsq = 0.f, musq = 0.f;
        float lo = 0.f, hi = 0.f, atdd = 0.f, dot = 0.f;      // sum of squares of columns < dd and > dd, column dd, fake[:dd] . A
        for (int d = 0; d < D; ++d) {
            const float z2 = lat[L + d][c];
            const float rr = fmaf(sigma, z2, img0[ml_at<NC>(d, c)]) - xs[d][c];
            rsq = fmaf(rr, rr, rsq);
            const float f = fmaf(ssigma, z2, img0[ml_at<NC>(d, TR + c)]);
            if (d < dd) {
                lo = fmaf(f, f, lo);
                if (kind == 1) dot = fmaf(f, gx.A[d], dot);
            } else {
                if (d == dd) atdd = f; else hi = fmaf(f, f, hi);
            }
        }
        for (int l = 0; l < L; ++l) musq = fmaf(mus[l][c], mus[l][c], musq);
        v[0] = (double)(0.5f * rsq * inv_var);
        v[1] = (double)musq;
        if (kind == 1) {                 // datasets.py:179-183: columns > dd, and the four sums of the all-pairs manifold error
            const double yv = (double)atdd, cv = (double)dot;
            v[2] = (double)hi;
            v[3] = yv; v[4] = yv * yv; v[5] = cv; v[6] = cv * cv;
        } else {                         // :138 columns >= dd;  :95-97 (|fake[:dd]| - 1)^2 and columns >= dd
            v[2] = (double)fmaf(atdd, atdd, hi);
            if (kind == 2) { const float e = sqrtf(lo) - 1.f; v[3] = (double)(e * e); }
        }
    }
    // ---- the tile's sums: the tree of eval_dev.h in the second image (the chain ended behind a barrier and nothing reads img1 again)
    double (&red)[kMs3Sums][256] = *reinterpret_cast<double (*)[kMs3Sums][256]>(img1);
#pragma unroll
    for (int k = 0; k < kMs3Sums; ++k) red[k][t] = v[k];
    tree_sum256(red, t);
    if (t < kMs3Part) a.part[(r * gridDim.x + tile) * kMs3Part + t] = t < kMs3Sums ? red[t][0] : 0.0;
}

// ---- launch 2: the tiles in tile order, then the record: lane t stores float t (linear_stats.hip's formulas) --------------------------
__global__ __launch_bounds__(64) void mlp3_stats_finalize_kernel(const Ms3FinalArgs a) {
    __shared__ double sum[kMs3Part];
    const int t = threadIdx.x;
    const long long r = blockIdx.x;
    const int L = a.L, kind = a.kind;
    const float* const p = a.params + r * a.state_stride;
    if (t < kMs3Part) {
        const double* const pr = a.part + r * a.tiles * kMs3Part + t;
        double s = 0.0;
        for (int i = 0; i < a.tiles; ++i) s += pr[(long long)i * kMs3Part];
        sum[t] = s;
    }
    __syncthreads();
    if (t < kMs3Head + L) {
        const float eps = a.off_eps >= 0 ? p[a.off_eps] * a.eps_cli : a.eps_cli;
        const double n = (double)a.rows;
        float v = 0.f;
        if (t < 3) {
            double klc = 0.0;
            for (int l = 0; l < L; ++l) { const float lv = p[a.off_epsp + l]; klc += (double)(1.f + lv - expf(lv)); }
            const double dkl = 0.5 * sum[1] / n - 0.5 * klc;                                      // networks.py:94
            const double mse = sum[0] / n + 0.5 * (double)a.D * ((double)kLog2Pi + (double)eps);      // :95-96
            v = (float)(t == 0 ? dkl + mse : (t == 1 ? dkl : mse));
        } else if (t == 3) {
            v = eps;
        } else if (t == 4) {
            v = (float)((kind == 2 ? sum[3] : sum[2]) / n);
        } else if (t == 5) {
            if (kind == 1) {
                // mean over ALL pairs (i, j) of (y_j - c_i)^2, the reference's (B,) against (B, 1) broadcast
                const double my = sum[3] / n, mc = sum[5] / n;
                v = (float)(sum[4] / n - 2.0 * my * mc + sum[6] / n);
            } else if (kind == 2) {
                v = (float)(sum[2] / n);
            }
        } else if (t >= kMs3Head) {
            v = p[a.off_epsp + t - kMs3Head];
        }
        a.out[r * a.out_stride + t] = v;
    }
}

static int ms3_tiles(int rows) { return (rows + MS_TR - 1) / MS_TR; }
// the workspace: the tile partials [n][tiles][8] doubles
static size_t ms3_workspace(int n, int rows) { return (sizeof(double) * kMs3Part * (size_t)n * ms3_tiles(rows) + 15) & ~(size_t)15; }

}  // namespace vaek

using namespace vaek;

extern "C" {

int vaek_supports_mlp3_stats_event(const vaek_ctx* ctx, int32_t kind, int32_t* yes) {
    if (!ctx || !yes) { set_error("vaek_supports_mlp3_stats_event: null argument"); return VAEK_ERR_INVALID; }
    *yes = kind >= 0 && kind <= 2 && ctx->mlp3_loglik ? 1 : 0;      // the shapes of mlp3_loglik_supported: the same chain
    return VAEK_OK;
}

int vaek_mlp3_stats_event_workspace_bytes(const vaek_ctx* ctx, int32_t n, int32_t rows, size_t* bytes) {
    const char* who = "vaek_mlp3_stats_event_workspace_bytes";
    if (!bytes) { set_error("%s: null argument", who); return VAEK_ERR_INVALID; }
    if (n < 1 || n > resident_max_replicas() || rows < 1 || rows > vaek_stats_event_max_rows()) {      // the ranges are no context's
        set_error("%s: %d replicas of %d rows, need 1 .. %d replicas (vaek_train_loop_max_replicas) and 1 .. %d rows (vaek_stats_event_max_rows)",
                  who, n, rows, resident_max_replicas(), vaek_stats_event_max_rows());
        return VAEK_ERR_INVALID;
    }
    if (!ctx) { set_error("%s: null argument", who); return VAEK_ERR_INVALID; }
    *bytes = ms3_workspace(n, rows);
    return VAEK_OK;
}

int vaek_mlp3_stats_event_replicas(vaek_ctx* ctx, const float* params, const vaek_stats_event* ev, int32_t kind, const float* A, int32_t dd,
                                   int32_t did, int32_t pad, float var_added, uint32_t x_tag, uint32_t z_tag, void* workspace, void* stream) {
    const char* who = "vaek_mlp3_stats_event_replicas";
    ProfBind pb(ctx);
    char needs[256];
    snprintf(needs, sizeof(needs), "needs a float32 VAE with one decoder and three hidden layers of 64 .. %d units both ways, D, L <= %d (see "
             "vaek_supports_mlp3_stats_event)", ML_W, ML_F);
    const EvalDesc d = describe(ev);
    EvalRules r{};
    r.covered = ctx && ctx->mlp3_loglik; r.needs = needs;
    r.rows_min = 1; r.rows_cap = vaek_stats_event_max_rows(); r.rows_query = "vaek_stats_event_max_rows";
    r.records = 1; r.record_len = ctx ? kMs3Head + (int64_t)ctx->L : 0; r.record_query = "vaek_stats_record_len";
    r.draws = true; r.kind = kind; r.A = A; r.dd = dd; r.did = did; r.pad = pad; r.x_tag = x_tag;
    r.has_z_tag = true; r.z_tag = z_tag;
    r.workspace = workspace; r.ws_align = 16; r.ws_query = "vaek_mlp3_stats_event_workspace_bytes";
    if (int rc = check_eval(who, ctx, params, d, r)) return rc;
    const int n = ev->n, rows = ev->rows, tiles = ms3_tiles(rows);
    Ms3Args a{};
    a.params = params; a.state_stride = ev->state_stride;
    a.x_seeds = reinterpret_cast<const unsigned long long*>(ev->x_seeds); a.x_steps = ev->x_steps;
    a.z_seeds = reinterpret_cast<const unsigned long long*>(ev->z_seeds); a.z_steps = ev->z_steps;
    a.sample_eps = ev->sample_eps; a.a_stride = ev->a_stride;
    a.part = static_cast<double*>(workspace);
    a.rows = rows; a.D = ctx->D; a.L = ctx->L; a.off_epsp = (int)ctx->off_epsp; a.off_eps = (int)ctx->off_eps;
    a.eps_cli = ctx->cfg.eps_cli; a.z_tag = z_tag;
    ml3_net(ctx->enc, &a.enc);
    ml3_net(ctx->dec, &a.dec);
    fill_draw_args(&a.gen, ctx, rows, kind, A, dd, did, pad, var_added, x_tag);
    Ms3FinalArgs f{};
    f.params = params; f.state_stride = ev->state_stride; f.part = a.part; f.out = ev->out; f.out_stride = ev->out_stride;
    f.rows = rows; f.tiles = tiles; f.D = ctx->D; f.L = ctx->L; f.off_epsp = a.off_epsp; f.off_eps = a.off_eps; f.kind = kind;
    f.eps_cli = a.eps_cli;

    constexpr size_t lds = sizeof(float) * 2 * ML_W * MS_NC;
    static thread_local PerDeviceOnce attr_set;
    VAEK_HIP_CHECK(set_max_dynamic_lds(attr_set, mlp3_stats_tile_kernel, lds));
    hipStream_t st = (hipStream_t)stream;
    {
        ProfScope ps("mlp3_stats_tile", st);
        launch_k(ps, mlp3_stats_tile_kernel, dim3((unsigned)tiles, (unsigned)n), dim3(ML_NT), lds, st, a);
    }
    VAEK_HIP_CHECK(hipGetLastError());
    {
        ProfScope ps("mlp3_stats_finalize", st);
        launch_k(ps, mlp3_stats_finalize_kernel, dim3((unsigned)n), dim3(64), 0, st, f);
    }
    VAEK_HIP_CHECK(hipGetLastError());
    return VAEK_OK;
}

}  // extern "C"
