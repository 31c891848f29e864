// Covariance spectra (vaek_cov_spectrum_rows, vaek_spectrum_event_replicas): the statistic the reference reserves as `EigenValues`
// and never fills -- cov_hat = jnp.cov(batch.T) of a generated batch and of a real batch, and eigh of each (datasets.py:113-125).
// ONE workgroup of 256 threads turns one set of `rows` float32 rows of D <= 32 columns into one float64 record: eigenvalues
// (ascending), column means, the covariance matrix, and how the solve ended.
//
//   MOMENTS.  The rows are staged 256 at a time as an LDS tile [256][kTileStride] of float32 (thread t produces row tile * 256 + t;
//     columns >= D and rows >= `rows` are zero) and summed on the float64 matrix cores: v_mfma_f64_16x16x4_f64 with k over the rows,
//     four per instruction.  The A and B operands share one map (lane (c = lane & 15, g = lane >> 4) holds x[4 s + g][16 b + c] of
//     k-step s), so a 16 x 16 block of the second-moment matrix is one instruction per k-step and the product x_i x_j is the exact
//     float64 product of two float32 values.  A wave owns whole output blocks and keeps them in registers across the tiles: wave 0
//     block (0, 0), wave 1 (0, 1), wave 2 (1, 1) of the upper triangle, wave 3 the column sums (A = ones: every output row is the
//     sum row) of both column blocks.  Every matrix element is therefore ONE accumulation chain over the rows in row order, and a
//     zero row adds +0.  One workgroup sums all <= 4096 rows: no tile partials, no workspace, no second launch, no atomic.
//   COVARIANCE.  m = S1 / rows, C = (S2 - rows m m^T) / (rows - 1) (jnp.cov's ddof = 1), float64, computed for i <= j and mirrored.
//   EIGENVALUES, EIGENVECTORS (vaek_cov_eigen_rows, vaek_eigen_event_replicas: the VEC instantiations).  eigen_dev.h's jacobi_solve
//     on C in the dead tile; that header says how the solve goes and what the three row sources are.
//   EXACT LOG-LIKELIHOOD (vaek_exact_log_likelihood_replicas): a third kernel on the same solve; its text is exact_loglik.inc,
//     included at the end of this file (one translation unit: DESIGN 3.19).
//   PRINCIPAL ANGLES (vaek_subspace_angles): a second kernel reads two eigen records an earlier launch stored, forms M = U^T W,
//     R = W - U M and G = R^T R in LDS and solves G with the same jacobi_solve: sin^2 of the principal angles between the two spans.
//
// The kernels read rows / parameters and store only the records, with per-lane vector stores; they read nothing back.
#include "eigen_dev.h"
#include "mfma_geom.h"
#include "eval_check.h"

namespace vaek {

struct SpectrumArgs {
    const float* x; long long x_stride;                              // SRC_EXPLICIT: set s reads x + s * x_stride
    double* out; long long out_stride;
    int rows, D;
    // the fused event only
    const float* params; long long state_stride;
    const unsigned long long* x_seeds; const unsigned* x_steps;      // [n]: the real rows' Philox key and step
    const unsigned long long* z_seeds; const unsigned* z_steps;      // [n]: the latents'
    const float* sample_eps;                                         // [n]: eps of the sampling pass
    long long a_stride;
    int L, off_epsp;
    unsigned z_tag;
    BatchArgs gen;                 // kind, A, dd, did, pad, noise_std, tag = x_tag, D, L; seed / step / pointers are not used
};

// The whole record of one set.  `smem`: the tile while the rows are summed, then the two Jacobi buffers and, with VEC, the two
// eigenvector buffers behind them.  src is uniform over the workgroup; an EVENT kernel carries the two drawing sources, the rows
// kernel the explicit one.  VEC appends V (row-major, column k the eigenvector of eigenvalue k, its largest component positive) to
// the record; what comes before it is the VEC = false record, bit for bit (V never feeds back into A).
template <bool EVENT, int DP, int LP, bool SIG, bool VEC>
__device__ __forceinline__ void cov_spectrum_set(const RowCtx& rc, const int src, const int rows, const int D, double* const out) {
    __shared__ __attribute__((aligned(16))) float smem[256 * kTileStride];
    __shared__ double red[256];
    __shared__ double S1[kSpectrumMaxDim], rot_c[kSpectrumMaxDim], rot_s[kSpectrumMaxDim], eig[kSpectrumMaxDim];
    __shared__ int rot_mate[kSpectrumMaxDim];
    static_assert(sizeof(float) * 256 * kTileStride >= sizeof(double) * 2 * kMatDoubles, "the Jacobi buffers reuse the tile");
    static_assert(!VEC || sizeof(float) * 256 * kTileStride >= sizeof(double) * 4 * kMatDoubles, "and so do the two eigenvector buffers");

    const int t = threadIdx.x;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int lane = t & 63, g = lane >> 4, c = lane & 15;
    const bool two = D > 16;                                           // the second 16-column block holds a column

    // ---- moments: S2 blocks and the column sums, accumulators live across the tiles --------------------------------------------
    f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    const int ia = w == 2 ? 16 : 0, jb = (w == 1 || w == 2) ? 16 : 0;
    for (int base = 0; base < rows; base += 256) {
        {
            float x[kSpectrumMaxDim];
            const int row = base + t;
            if (row < rows) {
                // a compiler that knows the parameter image is loop-invariant lifts it out of the tile loop and spills it
                asm volatile("" ::: "memory");
                if constexpr (!EVENT) produce_row<SRC_EXPLICIT, DP, LP, SIG>(rc, row, x);
                else if (src == SRC_REAL) produce_row<SRC_REAL, DP, LP, SIG>(rc, row, x);
                else produce_row<SRC_FAKE, DP, LP, SIG>(rc, row, x);
            } else {
#pragma unroll
                for (int d = 0; d < kSpectrumMaxDim; ++d) x[d] = 0.f;
            }
            float4* const dst = reinterpret_cast<float4*>(smem + t * kTileStride);
#pragma unroll
            for (int q = 0; q < kSpectrumMaxDim / 4; ++q) dst[q] = make_float4(x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]);
        }
        __syncthreads();
        const int left = rows - base;
        const int ksteps = ((left < 256 ? left : 256) + 3) >> 2;      // the k-steps that hold a row; the rest of the tile adds +0
        if (w < 3) {
            if (w == 0 || two) {
                for (int s = 0; s < ksteps; ++s) {
                    const float* const xr = smem + (4 * s + g) * kTileStride;
                    acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64((double)xr[ia + c], (double)xr[jb + c], acc0, 0, 0, 0);
                }
            }
        } else {
            for (int s = 0; s < ksteps; ++s) {
                const float* const xr = smem + (4 * s + g) * kTileStride;
                acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(1.0, (double)xr[c], acc0, 0, 0, 0);
                if (two) acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(1.0, (double)xr[16 + c], acc1, 0, 0, 0);
            }
        }
        __syncthreads();                                               // the tile is free again (and, after the last one, dead)
    }

    // ---- S2 (upper-triangle blocks) into the second Jacobi buffer; result (lane, register r) is row g + 4 r, column c of its block ----
    double* const mat = reinterpret_cast<double*>(smem);
    double* const S2 = mat + kSpectrumMaxDim * kMatStride;
    if (w < 3) {
#pragma unroll
        for (int r = 0; r < 4; ++r) S2[(ia + g + 4 * r) * kMatStride + jb + c] = acc0[r];
    } else if (g == 0) {
        S1[c] = acc0[0];
        S1[16 + c] = acc1[0];
    }
    __syncthreads();

    // ---- m, C (i <= j, mirrored) into the first buffer and the record ------------------------------------------------------------
    const int De = D + (D & 1);
    const double n = (double)rows;
    double sq = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int idx = t + 256 * k, i = idx >> 5, j = idx & 31;
        if (i <= j) {
            double v = 0.0;
            if (j < D) {
                const double mi = S1[i] / n, mj = S1[j] / n;
                v = (S2[i * kMatStride + j] - n * mi * mj) / (n - 1.0);
                out[2 * D + i * D + j] = v;
                out[2 * D + j * D + i] = v;
            }
            mat[i * kMatStride + j] = v;
            mat[j * kMatStride + i] = v;
            sq += i == j ? v * v : 2.0 * v * v;
        }
    }
    if (t < D) out[D + t] = S1[t] / n;
    double* const vec = mat + 2 * kMatDoubles;                     // behind S2: V starts as I
    if constexpr (VEC) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int idx = t + 256 * k, i = idx >> 5, j = idx & 31;
            vec[i * kMatStride + j] = i == j ? 1.0 : 0.0;
        }
    }
    const double norm_c = sqrt(block_sum256(sq, red, t));           // its barriers also publish the first buffer (and V)

    // ---- cyclic Jacobi, round-robin: index De - 1 stays, the others turn ------------------------------------------------------------
    int cur, sweeps;
    double off_f;
    jacobi_solve<VEC>(mat, vec, De, norm_c, red, rot_c, rot_s, rot_mate, t, cur, sweeps, off_f);

    // ---- eigenvalues ascending: the rank of a diagonal element is the count of those before it, ties by index ---------------------
    const double* const A = mat + cur * kMatDoubles;
    if (t < kSpectrumMaxDim) eig[t] = t < D ? A[t * kMatStride + t] : 0.0;
    __syncthreads();
    if (t < D) {
        const double e = eig[t];
        int rank = 0;
        for (int j = 0; j < D; ++j) {
            const double o = eig[j];
            rank += (o < e || (o == e && j < t)) ? 1 : 0;
        }
        out[rank] = e;
        if constexpr (VEC) {
            // column t goes to column `rank` with its component of largest magnitude positive (a tie: the lowest row).  The rotation
            // tables are dead: they carry the rank and the sign to the stores below.
            const double* const V = vec + cur * kMatDoubles;
            double big = 0.0, at = 1.0;
            for (int i = 0; i < D; ++i) {
                const double v = V[i * kMatStride + t];
                if (fabs(v) > big) { big = fabs(v); at = v; }
            }
            rot_mate[t] = rank;
            rot_s[t] = at < 0.0 ? -1.0 : 1.0;
        }
    }
    if (t < 4) {
        const double tail = t == 0 ? (double)sweeps : (t == 1 ? off_f : (t == 2 ? norm_c : n));
        out[2 * D + D * D + t] = tail;
    }
    if constexpr (VEC) {
        __syncthreads();
        const double* const V = vec + cur * kMatDoubles;
        double* const vout = out + 2 * D + D * D + 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int idx = t + 256 * k, i = idx >> 5, j = idx & 31;
            if (i < D && j < D) vout[i * D + rot_mate[j]] = rot_s[j] * V[i * kMatStride + j];
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void rows_kernel_body(const SpectrumArgs& a) {
    const long long s = blockIdx.x;
    RowCtx rc{};
    rc.xr = a.x + s * a.x_stride;
    rc.D = a.D;
    cov_spectrum_set<false, kSpectrumMaxDim, 4, false, VEC>(rc, SRC_EXPLICIT, a.rows, a.D, a.out + s * a.out_stride);
}

__global__ __launch_bounds__(256) void cov_spectrum_rows_kernel(const SpectrumArgs a) { rows_kernel_body<false>(a); }
__global__ __launch_bounds__(256) void cov_eigen_rows_kernel(const SpectrumArgs a) { rows_kernel_body<true>(a); }

// grid (n, 2): blockIdx.y = 0 the fake side, 1 the real side of replica blockIdx.x
template <int DP, int LP, bool SIG, bool VEC = false>
__global__ __launch_bounds__(256) void spectrum_event_kernel(const SpectrumArgs a) {
    using G = ParamImage<DP, LP, SIG>;
    __shared__ __attribute__((aligned(16))) float W[G::N];
    const int t = threadIdx.x;
    const long long r = blockIdx.x;
    const bool real = blockIdx.y != 0;
    const int D = a.D, L = a.L;
    RowCtx rc{};
    rc.D = D; rc.L = L; rc.W = W;
    rc.g = a.gen;
    if (real) {
        if (rc.g.A) rc.g.A += r * a.a_stride;
        rc.key = philox_key(a.x_seeds[r]);
        rc.step = a.x_steps[r];
    } else {
        G::fill(W, a.params + r * a.state_stride, D, L, a.off_epsp, t);   // the parameter image: zero outside [D] x [L]
        rc.g.tag = a.z_tag;
        rc.key = philox_key(a.z_seeds[r]);
        rc.step = a.z_steps[r];
        rc.ssigma = expf(0.5f * a.sample_eps[r]);
    }
    __syncthreads();
    const long long len = (long long)D * D * (VEC ? 2 : 1) + 2 * D + 4;
    cov_spectrum_set<true, DP, LP, SIG, VEC>(rc, real ? SRC_REAL : SRC_FAKE, a.rows, D, a.out + r * a.out_stride + (real ? len : 0));
}

// ---- variant table of the fused event: linear_stats.hip's (the padded shapes of mfma_geom.h, each side rounded up to 4) ----------
typedef void (*SpectrumKernel)(const SpectrumArgs);
struct SpectrumVariant { int dp, lp, sig; SpectrumKernel fn, fn_vec; };
#define VAEK_SPECTRUM_ROW(DP, LP, SIG, EXACT) \
    {up4(DP), up4(LP), SIG, spectrum_event_kernel<up4(DP), up4(LP), (SIG) != 0>, spectrum_event_kernel<up4(DP), up4(LP), (SIG) != 0, true>},
static const SpectrumVariant kSpectrumVariants[] = {VAEK_EVAL_SHAPES(VAEK_SPECTRUM_ROW)};
#undef VAEK_SPECTRUM_ROW

// vaek_supports_log_likelihood's predicate: float32, no hidden layers, one or two decoders, D, L <= 32, D <= 28 with two decoders
static const SpectrumVariant* pick_spectrum(const vaek_ctx* c) {
    const vaek_config& cfg = c->cfg;
    if (cfg.dtype != VAEK_F32 || cfg.n_enc_hidden != 0 || cfg.n_dec_hidden != 0) return nullptr;
    if (cfg.sigmoid_decoder && c->D > 28) return nullptr;
    return pick_smallest_shape(kSpectrumVariants, c->D, c->L, cfg.sigmoid_decoder != 0);
}

static int64_t spectrum_record_len(const vaek_ctx* c) { return (int64_t)c->D * c->D + 2 * (int64_t)c->D + 4; }
static int64_t eigen_record_len(const vaek_ctx* c) { return spectrum_record_len(c) + (int64_t)c->D * c->D; }
static int spectrum_max_sets() { return 2 * resident_max_replicas(); }
static const char* const kSpectrumRowsQuery = "vaek_stats_event_max_rows; one row has no ddof = 1 covariance";
// the rows and the pairs calls take any context whose data_dim the Jacobi buffers hold
static int check_spectrum_dim(const char* who, const vaek_ctx* ctx) {
    if (ctx->D > kSpectrumMaxDim) {
        set_error("%s: data_dim %d, need <= %d (see vaek_supports_cov_spectrum)", who, ctx->D, kSpectrumMaxDim);
        return VAEK_ERR_INVALID;
    }
    return VAEK_OK;
}

// ---- principal angles between two eigenbases (vaek_subspace_angles) ----------------------------------------------------------------
// Pair p: U = the ka eigenvectors of record a's largest eigenvalues, W = the kb of record b's (the last columns of the V blocks an
// EARLIER launch stored).  M = U^T W, R = W - U M formed explicitly (never I - M^T M, which loses small angles), G = R^T R for i <= j,
// mirrored, and G's eigenvalues -- sin^2 of the principal angles -- by jacobi_solve, the covariance solve's own text.  All float64 in LDS.
// The kernel stays in this unit: compiled in one of its own it comes out with other registers.
struct SubspaceArgs {
    const double* a; long long a_stride;
    const double* b; long long b_stride;
    double* out; long long out_stride;
    int D, ka, kb;
};

__global__ __launch_bounds__(256) void subspace_angles_kernel(const SubspaceArgs s) {
    __shared__ double mat[2 * kMatDoubles];
    __shared__ double U[kMatDoubles], W[kMatDoubles], M[kMatDoubles], R[kMatDoubles];
    __shared__ double red[256];
    __shared__ double rot_c[kSpectrumMaxDim], rot_s[kSpectrumMaxDim], eig[kSpectrumMaxDim];
    __shared__ int rot_mate[kSpectrumMaxDim];

    const int t = threadIdx.x;
    const long long p = blockIdx.x;
    const int D = s.D, ka = s.ka, kb = s.kb;
    const long long v0 = (long long)D * D + 2 * D + 4;               // V behind the spectrum record
    const double* const va = s.a + p * s.a_stride + v0;
    const double* const vb = s.b + p * s.b_stride + v0;
    double* const out = s.out + p * s.out_stride;

#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int idx = t + 256 * k, i = idx >> 5, j = idx & 31;
        U[i * kMatStride + j] = (i < D && j < ka) ? va[i * D + D - ka + j] : 0.0;
        W[i * kMatStride + j] = (i < D && j < kb) ? vb[i * D + D - kb + j] : 0.0;
    }
    __syncthreads();

    // ---- how far the two bases are from orthonormal, M = U^T W ---------------------------------------------------------------------
    double dev = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int idx = t + 256 * k, i = idx >> 5, j = idx & 31;
        if (i <= j && j < ka) {
            double uu = 0.0, ww = 0.0;
            for (int r = 0; r < D; ++r) {
                uu = fma(U[r * kMatStride + i], U[r * kMatStride + j], uu);
                ww = fma(W[r * kMatStride + i], W[r * kMatStride + j], ww);
            }
            const double id = i == j ? 1.0 : 0.0;
            dev = fmax(dev, fabs(uu - id));
            if (j < kb) dev = fmax(dev, fabs(ww - id));
        }
        double m = 0.0;
        if (i < ka && j < kb)
            for (int r = 0; r < D; ++r) m = fma(U[r * kMatStride + i], W[r * kMatStride + j], m);
        M[i * kMatStride + j] = m;
    }
    const double orth = block_max256(dev, red, t);                   // its barriers also publish M

    // ---- R = W - U M and the sum of its squares ----------------------------------------------------------------------------------------
    double rsq = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int idx = t + 256 * k, i = idx >> 5, j = idx & 31;
        double r = 0.0;
        if (i < D && j < kb) {
            double um = 0.0;
            for (int u = 0; u < ka; ++u) um = fma(U[i * kMatStride + u], M[u * kMatStride + j], um);
            r = W[i * kMatStride + j] - um;
        }
        R[i * kMatStride + j] = r;
        rsq += r * r;
    }
    const double frob2 = block_sum256(rsq, red, t);                  // its barriers also publish R

    // ---- G = R^T R (i <= j, mirrored), zero outside kb x kb ----------------------------------------------------------------------------
    double sq = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int idx = t + 256 * k, i = idx >> 5, j = idx & 31;
        if (i <= j) {
            double v = 0.0;
            if (j < kb)
                for (int r = 0; r < D; ++r) v = fma(R[r * kMatStride + i], R[r * kMatStride + j], v);
            mat[i * kMatStride + j] = v;
            mat[j * kMatStride + i] = v;
            sq += i == j ? v * v : 2.0 * v * v;
        }
    }
    const double norm_g = sqrt(block_sum256(sq, red, t));            // its barriers also publish G

    int cur, sweeps;
    double off_f;
    jacobi_solve<false>(mat, nullptr, kb + (kb & 1), norm_g, red, rot_c, rot_s, rot_mate, t, cur, sweeps, off_f);

    // ---- sin^2 ascending: counting ranks, ties by index; nothing is clamped --------------------------------------------------------------
    const double* const A = mat + cur * kMatDoubles;
    if (t < kSpectrumMaxDim) eig[t] = t < kb ? A[t * kMatStride + t] : 0.0;
    __syncthreads();
    if (t < kb) {
        const double e = eig[t];
        int rank = 0;
        for (int j = 0; j < kb; ++j) {
            const double o = eig[j];
            rank += (o < e || (o == e && j < t)) ? 1 : 0;
        }
        out[rank] = e;
    }
    if (t < 4) {
        const double tail = t == 0 ? frob2 : (t == 1 ? (double)sweeps : (t == 2 ? off_f : orth));
        out[kb + t] = tail;
    }
}

}  // namespace vaek

using namespace vaek;

extern "C" {

int vaek_supports_cov_spectrum(const vaek_ctx* ctx, int32_t* yes) {
    if (!ctx || !yes) { set_error("vaek_supports_cov_spectrum: null argument"); return VAEK_ERR_INVALID; }
    *yes = ctx->D >= 1 && ctx->D <= kSpectrumMaxDim ? 1 : 0;
    return VAEK_OK;
}

int vaek_cov_spectrum_record_len(const vaek_ctx* ctx, int64_t* doubles) {
    if (!ctx || !doubles) { set_error("vaek_cov_spectrum_record_len: null argument"); return VAEK_ERR_INVALID; }
    *doubles = spectrum_record_len(ctx);
    return VAEK_OK;
}

int vaek_cov_spectrum_max_sets(void) { return spectrum_max_sets(); }
int vaek_cov_spectrum_max_sweeps(void) { return kSpectrumMaxSweeps; }

// vaek_cov_spectrum_rows and, with `vec`, vaek_cov_eigen_rows: one refusal list, one launch
static int spectrum_rows_call(const char* who, bool vec, vaek_ctx* ctx, const float* x, int32_t n, int32_t rows, int64_t x_stride, double* out,
                              int64_t out_stride, void* stream) {
    ProfBind pb(ctx);
    if (!ctx || !x || !out) { set_error("%s: null context, x or out", who); return VAEK_ERR_INVALID; }
    if (int rc = check_spectrum_dim(who, ctx)) return rc;
    if (n < 1 || n > spectrum_max_sets()) {
        set_error("%s: %d sets, need 1 .. %d (vaek_cov_spectrum_max_sets)", who, n, spectrum_max_sets());
        return VAEK_ERR_INVALID;
    }
    if (int rc = check_row_count(who, rows, 2, kSpectrumMaxRows, kSpectrumRowsQuery)) return rc;
    if (int rc = check_x_stride(who, ctx, x_stride, rows)) return rc;
    const int64_t len = vec ? eigen_record_len(ctx) : spectrum_record_len(ctx);
    if (out_stride < len) {
        set_error("%s: out_stride %lld < record length %lld (%s)", who, (long long)out_stride, (long long)len,
                  vec ? "vaek_cov_eigen_record_len" : "vaek_cov_spectrum_record_len");
        return VAEK_ERR_INVALID;
    }
    if (int rc = check_aligned8(who, "out", (uintptr_t)out)) return rc;
    SpectrumArgs a{};
    a.x = x; a.x_stride = x_stride; a.out = out; a.out_stride = out_stride; a.rows = rows; a.D = ctx->D;
    hipStream_t st = (hipStream_t)stream;
    {
        ProfScope ps(vec ? "cov_eigen_rows" : "cov_spectrum_rows", st);
        launch_k(ps, vec ? cov_eigen_rows_kernel : cov_spectrum_rows_kernel, dim3((unsigned)n), dim3(256), 0, st, a);
    }
    VAEK_HIP_CHECK(hipGetLastError());
    return VAEK_OK;
}

int vaek_cov_spectrum_rows(vaek_ctx* ctx, const float* x, int32_t n, int32_t rows, int64_t x_stride, double* out, int64_t out_stride,
                           void* stream) {
    return spectrum_rows_call("vaek_cov_spectrum_rows", false, ctx, x, n, rows, x_stride, out, out_stride, stream);
}

int vaek_cov_eigen_rows(vaek_ctx* ctx, const float* x, int32_t n, int32_t rows, int64_t x_stride, double* out, int64_t out_stride,
                        void* stream) {
    return spectrum_rows_call("vaek_cov_eigen_rows", true, ctx, x, n, rows, x_stride, out, out_stride, stream);
}

int vaek_cov_eigen_record_len(const vaek_ctx* ctx, int64_t* doubles) {
    if (!ctx || !doubles) { set_error("vaek_cov_eigen_record_len: null argument"); return VAEK_ERR_INVALID; }
    *doubles = eigen_record_len(ctx);
    return VAEK_OK;
}

int vaek_supports_spectrum_event(const vaek_ctx* ctx, int32_t kind, int32_t* yes) {
    if (!ctx || !yes) { set_error("vaek_supports_spectrum_event: null argument"); return VAEK_ERR_INVALID; }
    *yes = kind >= 0 && kind <= 2 && pick_spectrum(ctx) ? 1 : 0;
    return VAEK_OK;
}

// vaek_spectrum_event_replicas and, with `vec`, vaek_eigen_event_replicas: one refusal list, one launch
static int spectrum_event_call(const char* who, bool vec, vaek_ctx* ctx, const float* params, const vaek_spectrum_event* ev, int32_t kind,
                               const float* A, int32_t dd, int32_t did, int32_t pad, float var_added, uint32_t x_tag, uint32_t z_tag,
                               void* stream) {
    ProfBind pb(ctx);
    const SpectrumVariant* var = ctx ? pick_spectrum(ctx) : nullptr;
    const EvalDesc d = describe(ev);
    EvalRules r{};
    r.covered = var != nullptr;
    r.needs = "needs a float32 linear VAE (no hidden layers) with D, L <= 32, D <= 28 with two decoders (see vaek_supports_spectrum_event)";
    r.rows_min = 2; r.rows_cap = kSpectrumMaxRows; r.rows_query = kSpectrumRowsQuery;
    r.records = 2; r.record_len = !ctx ? 0 : vec ? eigen_record_len(ctx) : spectrum_record_len(ctx);      // the fake record, the real one behind it
    r.record_query = vec ? "vaek_cov_eigen_record_len" : "vaek_cov_spectrum_record_len";
    r.draws = true; r.kind = kind; r.A = A; r.dd = dd; r.did = did; r.pad = pad; r.x_tag = x_tag;
    r.has_z_tag = true; r.z_tag = z_tag;
    if (int rc = check_eval(who, ctx, params, d, r)) return rc;
    SpectrumArgs a{};
    a.out = ev->out; a.out_stride = ev->out_stride; a.rows = ev->rows; a.D = ctx->D;
    a.params = params; a.state_stride = ev->state_stride;
    a.x_seeds = reinterpret_cast<const unsigned long long*>(ev->x_seeds); a.x_steps = ev->x_steps;
    a.z_seeds = reinterpret_cast<const unsigned long long*>(ev->z_seeds); a.z_steps = ev->z_steps;
    a.sample_eps = ev->sample_eps; a.a_stride = ev->a_stride;
    a.L = ctx->L; a.off_epsp = (int)ctx->off_epsp; a.z_tag = z_tag;
    fill_draw_args(&a.gen, ctx, ev->rows, kind, A, dd, did, pad, var_added, x_tag);
    hipStream_t st = (hipStream_t)stream;
    {
        ProfScope ps(vec ? "eigen_event_replicas" : "spectrum_event_replicas", st);
        launch_k(ps, vec ? var->fn_vec : var->fn, dim3((unsigned)ev->n, 2u), dim3(256), 0, st, a);
    }
    VAEK_HIP_CHECK(hipGetLastError());
    return VAEK_OK;
}

int vaek_spectrum_event_replicas(vaek_ctx* ctx, const float* params, const vaek_spectrum_event* ev, int32_t kind, const float* A, int32_t dd,
                                 int32_t did, int32_t pad, float var_added, uint32_t x_tag, uint32_t z_tag, void* stream) {
    return spectrum_event_call("vaek_spectrum_event_replicas", false, ctx, params, ev, kind, A, dd, did, pad, var_added, x_tag, z_tag, stream);
}

int vaek_eigen_event_replicas(vaek_ctx* ctx, const float* params, const vaek_spectrum_event* ev, int32_t kind, const float* A, int32_t dd,
                              int32_t did, int32_t pad, float var_added, uint32_t x_tag, uint32_t z_tag, void* stream) {
    return spectrum_event_call("vaek_eigen_event_replicas", true, ctx, params, ev, kind, A, dd, did, pad, var_added, x_tag, z_tag, stream);
}

int vaek_subspace_record_len(int32_t kb) { return kb + 4; }

int vaek_subspace_angles(vaek_ctx* ctx, const double* a, int64_t a_stride, const double* b, int64_t b_stride, int32_t n, int32_t ka,
                         int32_t kb, double* out, int64_t out_stride, void* stream) {
    const char* who = "vaek_subspace_angles";
    ProfBind pb(ctx);
    if (!ctx || !a || !b || !out) { set_error("%s: null context, a, b or out", who); return VAEK_ERR_INVALID; }
    if (int rc = check_spectrum_dim(who, ctx)) return rc;
    if (n < 1 || n > spectrum_max_sets()) {
        set_error("%s: %d pairs, need 1 .. %d (vaek_cov_spectrum_max_sets)", who, n, spectrum_max_sets());
        return VAEK_ERR_INVALID;
    }
    if (kb < 1 || kb > ka || ka > ctx->D) {
        set_error("%s: ka %d, kb %d: need 1 <= kb <= ka <= data_dim = %d", who, ka, kb, ctx->D);
        return VAEK_ERR_INVALID;
    }
    const int64_t len = eigen_record_len(ctx);
    if (a_stride < len || b_stride < len) {
        set_error("%s: a_stride %lld or b_stride %lld < record length %lld (vaek_cov_eigen_record_len)", who, (long long)a_stride,
                  (long long)b_stride, (long long)len);
        return VAEK_ERR_INVALID;
    }
    if (out_stride < kb + 4) {
        set_error("%s: out_stride %lld < record length %d (vaek_subspace_record_len)", who, (long long)out_stride, kb + 4);
        return VAEK_ERR_INVALID;
    }
    if (int rc = check_aligned8(who, "a, b or out", (uintptr_t)a | (uintptr_t)b | (uintptr_t)out)) return rc;
    SubspaceArgs s{};
    s.a = a; s.a_stride = a_stride; s.b = b; s.b_stride = b_stride; s.out = out; s.out_stride = out_stride;
    s.D = ctx->D; s.ka = ka; s.kb = kb;
    hipStream_t st = (hipStream_t)stream;
    {
        ProfScope ps("subspace_angles", st);
        launch_k(ps, subspace_angles_kernel, dim3((unsigned)n), dim3(256), 0, st, s);
    }
    VAEK_HIP_CHECK(hipGetLastError());
    return VAEK_OK;
}

}  // extern "C"

#include "exact_loglik.inc"      // vaek_exact_log_likelihood_replicas: its kernel, variant table and entry points
