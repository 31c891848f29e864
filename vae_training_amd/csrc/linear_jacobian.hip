// Decoder Jacobian spectra of N linear VAEs of one shape, one or two decoders (vaek_linear_decoder_jacobian_replicas): per latent row z
// the singular values squared of J(z) = d x_hat / dz (D x L) and their means over the rows -- vaek_mlp3_decoder_jacobian_replicas for
// the models without hidden layers, same description struct, same two records.  For networks.py:73-83
//   x_hat(z) = z K_d + b_d [+ sigmoid(z K_s + b_s)],      J(z) = K_d^T [+ diag(sigmoid'(u(z))) K_s^T],   u = z K_s + b_s.
// With one decoder J is the decoder kernel at every z (all rows of a replica carry the same record); with two it changes from row to
// row through the D slopes sigmoid'(u_d), and the question the two-decoder experiments ask -- how many latent directions the trained
// generator moves its output along, which latents are off -- is read from its spectrum.
//
// J is L x D <= 32 x 32 and costs one exp per output column, so nothing forces the float32 J of the MLP call: everything from u onward
// is float64.  The slope is taken as
//   e = exp(-|u|),   g = e / ((1 + e) (1 + e)),
// symmetric in u, with no 1 - s cancellation, never inf or NaN for a finite u and exactly 0 for a saturated head (|u| above 745).
// The quotient is rounded essentially ONCE: 1 + e and its square are carried as a pair of doubles and the division is corrected once by
// its residual, which leaves g within a fraction of an ulp of e / (1 + e)^2 for the e that exp returns -- not a proven correctly rounded
// quotient (three roundings in plain float64 leave g up to 2 ulp off, and at L = 1, where G is the one number sum_d J_d^2, that put
// |G|_F 3 ulp from a long double evaluation; this form leaves about 1: tools/replay_linear_jacobian_slope.py).
//
// TWO launches per call whatever n is, ordered by the stream alone; nothing stored in a launch is read back inside it, and there is no
// atomic, counter, wait or status word:
//   1. linear_jacobian_rows      grid (rows, n), 256 threads: the workgroup of row i of replica r reads the caller's latent or draws it
//      with latent_block of rng_dev.h (the bits vaek_make_batch writes into z1; two decoders only: one decoder never looks at z), forms
//      u_d = b_s[d] + sum_l z_l K_s[l][d] in l order, g_d and J[l][d] = K_d[l][d] + g_d K_s[l][d] in LDS, and runs jacobian_solve_row of
//      jacobian_dev.h on it -- G = J^T J, |G|_F, jacobi_solve<false>, the counting rank: the text of the MLP call's solve launch -- which
//      stores the row record (2 L + 4 doubles) into the workspace and, where given, row_out.
//   2. linear_jacobian_finalize  n workgroups: jacobian_finalize_replica of jacobian_dev.h, the MLP call's finalize launch.
// The weights are read a dword at a time: state_stride has no alignment rule.
#include "jacobian_dev.h"

namespace vaek {

constexpr int kLjMaxRows = 1 << 20;          // n * rows, one workgroup each: bounds the length of a launch -- a cap, not a tuned value

struct LjArgs {
    const float* params; long long state_stride;
    const unsigned long long* z_seeds; const unsigned* z_steps;      // [n]: the latents' Philox key and step (drawing mode)
    const float* z; long long z_stride;      // explicit latents [rows][L] per replica (0: shared); NULL = draw
    double* rec;                             // [n][rows][2 L + 4]: the workspace's row records
    double* row_out; long long row_out_stride;      // the caller's copy (may be NULL), replica r at row_out + r * row_out_stride
    int rows, D, L, sig;                     // sig: two decoders
    unsigned z_tag;
    double rank_tol;
};

__global__ __launch_bounds__(256) void linear_jacobian_rows_kernel(const LjArgs a) {
    __shared__ JacobianSolveLds s;
    __shared__ double Js[kSpectrumMaxDim * kSpectrumMaxDim];
    __shared__ double gs[kSpectrumMaxDim];
    __shared__ float zs[kSpectrumMaxDim];
    const int t = threadIdx.x;
    const int row = blockIdx.x;
    const long long r = blockIdx.y;
    const int D = a.D, L = a.L;
    const long long rr = r * a.rows + row;
    const float* const P = a.params + r * a.state_stride;
    // the flat layout of a linear VAE (ParamImage::fill of eval_dev.h): encoder [D][L] + [L], then K_d [L][D], b_d, K_s [L][D], b_s
    const int off_wd = D * L + L, off_ws = off_wd + L * D + D, off_bs = off_ws + L * D;

    if (a.sig) {
        if (a.z) {                               // the caller's latent
            if (t < L) zs[t] = a.z[r * a.z_stride + (long long)row * L + t];
        } else {                                 // vaek_make_batch's z1: blocks q < ceil(L / 4) of the row's latent stream
            if (t < ((L + 3) >> 2)) {
                BatchArgs gz{};
                gz.tag = a.z_tag;
                float n4[4];
                latent_block(gz, a.z_steps[r], row, philox_key(a.z_seeds[r]), t, n4);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int l = 4 * t + i;
                    if (l < L) zs[l] = n4[i];    // elements >= L of the last block belong to z2
                }
            }
        }
        __syncthreads();
        if (t < D) {
            double u = (double)P[off_bs + t];
            for (int l = 0; l < L; ++l) u += (double)zs[l] * (double)P[off_ws + l * D + t];
            const double e = exp(-fabs(u));
            const double th = 1.0 + e, tl = e - (th - 1.0);                 // th + tl = 1 + e exactly (1 >= e)
            const double ph = th * th, pl = fma(th, th, -ph) + 2.0 * th * tl;   // ph + pl = (1 + e)^2 to 2^-104
            const double q = e / ph;
            gs[t] = q + (fma(-q, ph, e) - q * pl) / ph;
        }
        __syncthreads();
    }
    for (int e = t; e < L * D; e += 256) {
        double v = (double)P[off_wd + e];
        if (a.sig) v += gs[e % D] * (double)P[off_ws + e];
        Js[e] = v;
    }
    __syncthreads();
    double* const rec = a.rec + rr * (2 * L + 4);
    double* const ro = a.row_out ? a.row_out + r * a.row_out_stride + (long long)row * (2 * L + 4) : nullptr;
    jacobian_solve_row<double>(Js, s, D, L, a.rank_tol, rec, ro, t);
}

__global__ __launch_bounds__(256) void linear_jacobian_finalize_kernel(const JacobianFinalArgs a) {
    __shared__ JacobianFinalLds s;
    jacobian_finalize_replica(a, s, blockIdx.x, threadIdx.x);
}

// vaek_log_likelihood_replicas' models without the dataset kind: float32, no hidden layers, D, L <= 32, D <= 28 with two decoders.
// Nothing about the batch or the world: the call reads parameters only
static bool lj_covers(const vaek_ctx* c) {
    const vaek_config& cfg = c->cfg;
    if (cfg.dtype != VAEK_F32 || cfg.n_enc_hidden != 0 || cfg.n_dec_hidden != 0) return false;
    if (c->D < 1 || c->L < 1 || c->D > kSpectrumMaxDim || c->L > kSpectrumMaxDim) return false;
    return !(cfg.sigmoid_decoder && c->D > 28);
}
static size_t lj_workspace(const vaek_ctx* c, int n, int rows) {
    return jacobian_up16(sizeof(double) * (size_t)n * rows * (size_t)jacobian_row_record_len(c));
}
// n * rows as `who` refuses it: the call's and its workspace query's
static int lj_check_rows(const char* who, int32_t n, int32_t rows) {
    const long long total = (long long)n * rows;
    if (total > kLjMaxRows) {
        set_error("%s: %d replicas x %d rows = %lld rows, at most %d (vaek_linear_decoder_jacobian_max_rows)", who, n, rows, total, kLjMaxRows);
        return VAEK_ERR_INVALID;
    }
    return VAEK_OK;
}
static const char kLjNeeds[] = "needs a float32 linear VAE (no hidden layers) with D, L <= 32, D <= 28 with two decoders (see "
                               "vaek_supports_linear_decoder_jacobian)";

}  // namespace vaek

using namespace vaek;

extern "C" {

int vaek_supports_linear_decoder_jacobian(const vaek_ctx* ctx, int32_t* yes) {
    if (!ctx || !yes) { set_error("vaek_supports_linear_decoder_jacobian: null argument"); return VAEK_ERR_INVALID; }
    *yes = lj_covers(ctx) ? 1 : 0;
    return VAEK_OK;
}

int vaek_linear_decoder_jacobian_max_rows(void) { return kLjMaxRows; }

int vaek_linear_decoder_jacobian_workspace_bytes(const vaek_ctx* ctx, int32_t n, int32_t rows, size_t* bytes) {
    const char* who = "vaek_linear_decoder_jacobian_workspace_bytes";
    if (!ctx || !bytes) { set_error("%s: null argument", who); return VAEK_ERR_INVALID; }
    if (!lj_covers(ctx)) { set_error("%s: %s", who, kLjNeeds); return VAEK_ERR_INVALID; }
    if (int rc = check_replica_count(who, n)) return rc;
    if (int rc = check_row_count(who, rows, 1, kSpectrumMaxRows, "vaek_stats_event_max_rows")) return rc;
    if (int rc = lj_check_rows(who, n, rows)) return rc;
    *bytes = lj_workspace(ctx, n, rows);
    return VAEK_OK;
}

int vaek_linear_decoder_jacobian_replicas(vaek_ctx* ctx, const float* params, const vaek_decoder_jacobian* dj, uint32_t z_tag, void* workspace,
                                          void* stream) {
    const char* who = "vaek_linear_decoder_jacobian_replicas";
    ProfBind pb(ctx);
    const EvalDesc d = describe(dj);
    EvalRules r{};
    r.covered = ctx && lj_covers(ctx); r.needs = kLjNeeds;
    r.rows_min = 1; r.rows_cap = kSpectrumMaxRows; r.rows_query = "vaek_stats_event_max_rows";
    r.records = 1; r.record_len = ctx ? jacobian_record_len(ctx) : 0; r.record_query = "vaek_decoder_jacobian_record_len";
    r.has_z_tag = true; r.z_tag = z_tag;                             // no dataset draw: the rows are latents
    r.workspace = workspace; r.ws_align = 16; r.ws_query = "vaek_linear_decoder_jacobian_workspace_bytes";
    if (int rc = check_eval(who, ctx, params, d, r)) return rc;
    if (int rc = lj_check_rows(who, dj->n, dj->rows)) return rc;
    if (int rc = check_jacobian_outputs(who, ctx, dj)) return rc;
    const int n = dj->n, rows = dj->rows, L = ctx->L, D = ctx->D;
    LjArgs a{};
    a.params = params; a.state_stride = dj->state_stride;
    a.z_seeds = reinterpret_cast<const unsigned long long*>(dj->z_seeds); a.z_steps = dj->z_steps;
    a.z = dj->z; a.z_stride = dj->z_stride;
    a.rec = static_cast<double*>(workspace); a.row_out = dj->row_out; a.row_out_stride = dj->row_out_stride;
    a.rows = rows; a.D = D; a.L = L; a.sig = ctx->cfg.sigmoid_decoder ? 1 : 0; a.z_tag = z_tag; a.rank_tol = dj->rank_tol;
    JacobianFinalArgs f{};
    f.rec = a.rec; f.out = dj->out; f.out_stride = dj->out_stride; f.rows = rows; f.L = L; f.rank_tol = dj->rank_tol;

    hipStream_t st = (hipStream_t)stream;
    {
        ProfScope ps("linear_jacobian_rows", st);
        launch_k(ps, linear_jacobian_rows_kernel, dim3((unsigned)rows, (unsigned)n), dim3(256), 0, st, a);
    }
    VAEK_HIP_CHECK(hipGetLastError());
    {
        ProfScope ps("linear_jacobian_finalize", st);
        launch_k(ps, linear_jacobian_finalize_kernel, dim3((unsigned)n), dim3(256), 0, st, f);
    }
    VAEK_HIP_CHECK(hipGetLastError());
    return VAEK_OK;
}

}  // extern "C"
