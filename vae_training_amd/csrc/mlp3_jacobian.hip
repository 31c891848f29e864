// Decoder Jacobian spectra of N three-hidden-layer MLP VAEs of one shape (vaek_mlp3_decoder_jacobian_replicas): per latent row z the
// singular values squared of J(z) = d Decoder(z) / dz (D x L) -- how many directions of the latent space the decoder moves its output
// along at z -- and their means over the rows.  For the four-Dense relu stack of networks.py:26-44
//   J(z) = K3^T M3 K2^T M2 K1^T M1 K0^T,   M_i = diag(pre_i(z) > 0),
// the four kernels with the three 0/1 masks of the primal pass between them.  L tangent columns per row go through three layers of
// up to 256 units, so every product is v_mfma_f32_16x16x4_f32 (exact f32) through ml_dense of mlp3_dev.h, the Dense chain of the
// log-likelihood and stats kernels, and the symmetric solve is jacobi_solve of eigen_dev.h; both headers as they are.
// The bodies of the solve and finalize launches are the shared text of jacobian_dev.h, which vaek_linear_decoder_jacobian_replicas
// runs too.
//
// SCHEME (a): primal and tangents travel together.  A latent row takes L + 1 adjacent columns of a 64-column [unit][column] image: its
// primal column (z, then the activations) and its L tangent columns (e_l, then d activation / d z_l), so a tile holds 64 / (L + 1)
// rows and the same ml_dense call multiplies both.  The epilogue stores raw sums, the bias added on the primal column only; a pass
// over the output image then turns the primal column into relu(pre) and zeroes the row's tangents where pre <= 0 (a unit is live iff
// its float32 pre-activation is > 0: the derivative at exactly 0 is 0).  The masks are never stored: they are read off the primal
// column of the image that is being fixed up.  The layer-1 tangent of (row, l) is kernel row l of FC0: the product with e_l gives it
// exactly (one term, the other terms are exact zeros), so layer 1 is the same call as the other three.  DESIGN 3.20 says why this
// scheme and not the bit-mask one, and what it costs at L = 32.
//
// THREE launches per call whatever n is, ordered by the stream alone; nothing stored in a launch is read back inside it, and there is
// no atomic, counter, wait or status word:
//   1. mlp3_jacobian_tangent   grid (ceil(rows / (64 / (L + 1))), n): reads the caller's latents or draws them with latent_block of
//      rng_dev.h (the bits vaek_make_batch writes into z1), runs the four products between two ping-pong images and stores
//      J[n][rows][L][D] (float32) in the workspace.  Rows past the last compute on clamped indices and store nothing; unused columns
//      multiply zeros.  A column's arithmetic does not depend on its place in the tile or on its neighbours: MFMA columns are
//      independent and the fix-up reads the row's own primal column only.
//   2. mlp3_jacobian_solve     grid (rows, n): one workgroup per row forms G = J^T J (L x L) in float64, each entry a sum over d in d
//      order of exact products, takes |G|_F, runs jacobi_solve<false> on G padded to even order, ranks the eigenvalues by counting
//      and stores the row record (2 L + 4 doubles) into the workspace and, where given, row_out.
//   3. mlp3_jacobian_finalize  n workgroups: the rows in a fixed binary tree per 256 rows, then the tiles in order, float64; lane t
//      stores double t of the model record (2 L + 8 doubles).
#include "mlp3_dev.h"
#include "eigen_dev.h"
#include "eval_check.h"
#include "jacobian_dev.h"

namespace vaek {

constexpr int kMjMaxColumns = 1 << 20;       // n * rows * L: bounds the workspace (128 MB of J) and the length of a call -- a cap, not a tuned value
constexpr int MJ_NC = 64;                    // columns of a tangent tile: rows * (L + 1) of them are used

struct MjArgs {
    const float* params; long long state_stride;
    const unsigned long long* z_seeds; const unsigned* z_steps;      // [n]: the latents' Philox key and step (drawing mode)
    const float* z; long long z_stride;      // explicit latents [rows][L] per replica (0: shared); NULL = draw
    float* J;                                // [n][rows][L][D]
    int rows, D, L, rpt;                     // rpt: rows per tile = 64 / (L + 1)
    unsigned z_tag;
    Ml3Net net;                              // the decoder's layers
};

struct MjSolveArgs {
    const float* J;                          // [n][rows][L][D]
    double* rec;                             // [n][rows][2 L + 4]: the workspace's row records
    double* row_out; long long row_out_stride;      // the caller's copy (may be NULL), replica r at row_out + r * row_out_stride
    int rows, D, L;
    double rank_tol;
};

// ---- launch 1: latent rows -> J -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ML_NT) void mlp3_jacobian_tangent_kernel(const MjArgs a) {
    constexpr int NC = MJ_NC, CB = NC / 16;
    extern __shared__ __attribute__((aligned(16))) char mj_smem[];
    float* const img0 = reinterpret_cast<float*>(mj_smem);
    float* const img1 = img0 + ML_W * NC;
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const long long r = blockIdx.y;
    const int D = a.D, L = a.L, rpt = a.rpt, L1 = L + 1;
    const int row0 = blockIdx.x * rpt;
    const int used = rpt * L1;                   // columns that carry a row
    const float* const P = a.params + r * a.state_stride;

    // ---- the input image: rows [0, L) of img0; column g (L + 1) is z of row row0 + g, column g (L + 1) + 1 + l is e_l ----------------
    for (int e = t; e < L * NC; e += ML_NT) {
        const int c = e & (NC - 1), k = e / NC;
        const int j = c % L1;
        img0[ml_at<NC>(k, c)] = (c < used && j == k + 1) ? 1.f : 0.f;      // the primal columns are written below
    }
    __syncthreads();
    if (a.z) {                                   // the caller's latents
        const float* const zr = a.z + r * a.z_stride;
        for (int e = t; e < rpt * L; e += ML_NT) {
            const int g = e / L, l = e - g * L;
            img0[ml_at<NC>(l, g * L1)] = zr[(long long)min(row0 + g, a.rows - 1) * L + l];
        }
    } else {                                     // vaek_make_batch's z1: blocks q < ceil(L / 4) of the row's latent stream
        BatchArgs gz{};
        gz.tag = a.z_tag;
        const uint2 zkey = philox_key(a.z_seeds[r]);
        const unsigned zstep = a.z_steps[r];
        const int nlb = (L + 3) >> 2;
        for (int e = t; e < rpt * nlb; e += ML_NT) {
            const int g = e / nlb, q = e - g * nlb;
            float n4[4];
            latent_block(gz, zstep, min(row0 + g, a.rows - 1), zkey, q, n4);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int l = 4 * q + i;
                if (l < L) img0[ml_at<NC>(l, g * L1)] = n4[i];              // elements >= L of the last block belong to z2
            }
        }
    }
    __syncthreads();

    // which of this lane's CB columns are primal columns: they take the bias
    const int n16 = lane & 15;
    unsigned prim = 0u;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) prim |= ((16 * cb + n16) % L1 == 0 ? 1u : 0u) << cb;

#pragma unroll 1
    for (int li = 0; li < 4; ++li) {
        const float* const in = (li & 1) ? img1 : img0;
        float* const out = (li & 1) ? img0 : img1;
        auto epi = [&](int m, int c, float v, float b) { out[ml_at<NC>(m, c)] = ((prim >> (c >> 4)) & 1u) ? v + b : v; };
        const int n_in = a.net.n_in[li], n_out = a.net.n_out[li], w_off = a.net.w_off[li];
        if (n_out <= 64) ml_dense<1, CB>(P, w_off, n_out, n_in, in, wave, lane, epi);
        else ml_dense<4, CB>(P, w_off, n_out, n_in, in, wave, lane, epi);
        __syncthreads();
        if (li != 3) {                           // relu on the primal column, its mask on the row's tangents: item (unit m, row g)
            for (int e = t; e < n_out * rpt; e += ML_NT) {
                const int g = e % rpt, m = e / rpt;
                const int c0 = g * L1;
                const float p = out[ml_at<NC>(m, c0)];
                if (!(p > 0.f)) {
                    for (int j = 0; j <= L; ++j) out[ml_at<NC>(m, c0 + j)] = 0.f;
                }
            }
            __syncthreads();
        }
    }

    // ---- J[row][l][d] = tangent column l of the row, unit d of img0 -----------------------------------------------------------------
    float* const Jr = a.J + r * a.rows * (long long)(L * D);
    for (int e = t; e < rpt * L * D; e += ML_NT) {
        const int d = e % D, gl = e / D;
        const int g = gl / L, l = gl - g * L;
        if (row0 + g < a.rows) Jr[(long long)(row0 + g) * (L * D) + l * D + d] = img0[ml_at<NC>(d, g * L1 + 1 + l)];
    }
}

// ---- launch 2: J of one row -> its record (jacobian_solve_row of jacobian_dev.h on the float32 J) ------------------------------------------
__global__ __launch_bounds__(256) void mlp3_jacobian_solve_kernel(const MjSolveArgs a) {
    __shared__ JacobianSolveLds s;
    __shared__ float Js[kSpectrumMaxDim * kSpectrumMaxDim];
    const int t = threadIdx.x;
    const int row = blockIdx.x;
    const long long r = blockIdx.y;
    const int D = a.D, L = a.L;
    const long long rr = r * a.rows + row;
    const float* const Jg = a.J + rr * (L * D);
    for (int e = t; e < L * D; e += 256) Js[e] = Jg[e];
    __syncthreads();
    double* const rec = a.rec + rr * (2 * L + 4);
    double* const ro = a.row_out ? a.row_out + r * a.row_out_stride + (long long)row * (2 * L + 4) : nullptr;
    jacobian_solve_row<float>(Js, s, D, L, a.rank_tol, rec, ro, t);
}

// ---- launch 3: the row records of a replica -> its model record (jacobian_finalize_replica of jacobian_dev.h) --------------------------
__global__ __launch_bounds__(256) void mlp3_jacobian_finalize_kernel(const JacobianFinalArgs a) {
    __shared__ JacobianFinalLds s;
    jacobian_finalize_replica(a, s, blockIdx.x, threadIdx.x);
}

static int mj_rows_per_tile(int L) { return MJ_NC / (L + 1); }
// the workspace: J [n][rows][L][D] floats, then the row records [n][rows][2 L + 4] doubles, each 16-byte aligned
struct MjWs { size_t rec, total; };
static MjWs mj_workspace(const vaek_ctx* c, int n, int rows) {
    MjWs w;
    w.rec = jacobian_up16(sizeof(float) * (size_t)n * rows * c->L * c->D);
    w.total = w.rec + jacobian_up16(sizeof(double) * (size_t)n * rows * (size_t)jacobian_row_record_len(c));
    return w;
}
// the column product as `who` refuses it: the call's and its workspace query's
static int mj_check_columns(const char* who, const vaek_ctx* c, int32_t n, int32_t rows) {
    return check_column_count(who, n, rows, c->L, "latents", kMjMaxColumns, "vaek_mlp3_decoder_jacobian_max_columns");
}
static_assert(ML_W == 256 && ML_F == 32, "kMjNeeds states the bounds of mlp3_dev.h");
static const char kMjNeeds[] = "needs a float32 VAE with one decoder and three hidden layers of 64 .. 256 units both ways, D, L <= 32 (see "
                               "vaek_supports_mlp3_decoder_jacobian)";

}  // namespace vaek

using namespace vaek;

extern "C" {

int vaek_supports_mlp3_decoder_jacobian(const vaek_ctx* ctx, int32_t* yes) {
    if (!ctx || !yes) { set_error("vaek_supports_mlp3_decoder_jacobian: null argument"); return VAEK_ERR_INVALID; }
    *yes = ctx->mlp3_loglik ? 1 : 0;
    return VAEK_OK;
}

int vaek_decoder_jacobian_record_len(const vaek_ctx* ctx, int64_t* doubles) {
    if (!ctx || !doubles) { set_error("vaek_decoder_jacobian_record_len: null argument"); return VAEK_ERR_INVALID; }
    *doubles = jacobian_record_len(ctx);
    return VAEK_OK;
}

int vaek_decoder_jacobian_row_record_len(const vaek_ctx* ctx, int64_t* doubles) {
    if (!ctx || !doubles) { set_error("vaek_decoder_jacobian_row_record_len: null argument"); return VAEK_ERR_INVALID; }
    *doubles = jacobian_row_record_len(ctx);
    return VAEK_OK;
}

int vaek_mlp3_decoder_jacobian_max_columns(void) { return kMjMaxColumns; }

int vaek_mlp3_decoder_jacobian_workspace_bytes(const vaek_ctx* ctx, int32_t n, int32_t rows, size_t* bytes) {
    const char* who = "vaek_mlp3_decoder_jacobian_workspace_bytes";
    if (!ctx || !bytes) { set_error("%s: null argument", who); return VAEK_ERR_INVALID; }
    if (!ctx->mlp3_loglik) { set_error("%s: %s", who, kMjNeeds); return VAEK_ERR_INVALID; }
    if (int rc = check_replica_count(who, n)) return rc;
    if (int rc = check_row_count(who, rows, 1, kSpectrumMaxRows, "vaek_stats_event_max_rows")) return rc;
    if (int rc = mj_check_columns(who, ctx, n, rows)) return rc;
    *bytes = mj_workspace(ctx, n, rows).total;
    return VAEK_OK;
}

int vaek_mlp3_decoder_jacobian_replicas(vaek_ctx* ctx, const float* params, const vaek_decoder_jacobian* dj, uint32_t z_tag, void* workspace,
                                        void* stream) {
    const char* who = "vaek_mlp3_decoder_jacobian_replicas";
    ProfBind pb(ctx);
    const EvalDesc d = describe(dj);
    EvalRules r{};
    r.covered = ctx && ctx->mlp3_loglik; r.needs = kMjNeeds;
    r.rows_min = 1; r.rows_cap = kSpectrumMaxRows; r.rows_query = "vaek_stats_event_max_rows";
    r.records = 1; r.record_len = ctx ? jacobian_record_len(ctx) : 0; r.record_query = "vaek_decoder_jacobian_record_len";
    r.has_z_tag = true; r.z_tag = z_tag;                             // no dataset draw: the rows are latents
    r.workspace = workspace; r.ws_align = 16; r.ws_query = "vaek_mlp3_decoder_jacobian_workspace_bytes";
    if (int rc = check_eval(who, ctx, params, d, r)) return rc;
    if (int rc = mj_check_columns(who, ctx, dj->n, dj->rows)) return rc;
    if (int rc = check_jacobian_outputs(who, ctx, dj)) return rc;
    const int n = dj->n, rows = dj->rows, L = ctx->L, D = ctx->D;
    const MjWs w = mj_workspace(ctx, n, rows);
    char* const ws = static_cast<char*>(workspace);
    MjArgs a{};
    a.params = params; a.state_stride = dj->state_stride;
    a.z_seeds = reinterpret_cast<const unsigned long long*>(dj->z_seeds); a.z_steps = dj->z_steps;
    a.z = dj->z; a.z_stride = dj->z_stride;
    a.J = reinterpret_cast<float*>(ws);
    a.rows = rows; a.D = D; a.L = L; a.rpt = mj_rows_per_tile(L); a.z_tag = z_tag;
    ml3_net(ctx->dec, &a.net);
    MjSolveArgs s{};
    s.J = a.J; s.rec = reinterpret_cast<double*>(ws + w.rec); s.row_out = dj->row_out; s.row_out_stride = dj->row_out_stride;
    s.rows = rows; s.D = D; s.L = L; s.rank_tol = dj->rank_tol;
    JacobianFinalArgs f{};
    f.rec = s.rec; f.out = dj->out; f.out_stride = dj->out_stride; f.rows = rows; f.L = L; f.rank_tol = dj->rank_tol;

    constexpr size_t lds = sizeof(float) * 2 * ML_W * MJ_NC;
    static thread_local PerDeviceOnce attr_set;
    VAEK_HIP_CHECK(set_max_dynamic_lds(attr_set, mlp3_jacobian_tangent_kernel, lds));
    hipStream_t st = (hipStream_t)stream;
    {
        ProfScope ps("mlp3_jacobian_tangent", st);
        launch_k(ps, mlp3_jacobian_tangent_kernel, dim3((unsigned)((rows + a.rpt - 1) / a.rpt), (unsigned)n), dim3(ML_NT), lds, st, a);
    }
    VAEK_HIP_CHECK(hipGetLastError());
    {
        ProfScope ps("mlp3_jacobian_solve", st);
        launch_k(ps, mlp3_jacobian_solve_kernel, dim3((unsigned)rows, (unsigned)n), dim3(256), 0, st, s);
    }
    VAEK_HIP_CHECK(hipGetLastError());
    {
        ProfScope ps("mlp3_jacobian_finalize", st);
        launch_k(ps, mlp3_jacobian_finalize_kernel, dim3((unsigned)n), dim3(256), 0, st, f);
    }
    VAEK_HIP_CHECK(hipGetLastError());
    return VAEK_OK;
}

}  // extern "C"
