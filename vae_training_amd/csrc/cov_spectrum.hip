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
//   EIGENVALUES.  Cyclic Jacobi in float64 on C in LDS, D padded to even, round-robin ordering: D / 2 disjoint rotations per round,
//     D - 1 rounds per sweep.  A round is "angles from the current matrix, barrier, A <- J^T A J into the other buffer, barrier";
//     each new element comes from its four sources, for i <= j, mirrored.  A rotation is skipped where a_pq == 0 and takes
//     t = 1 / (2 theta) where theta = (a_qq - a_pp) / (2 a_pq) is too large to square (both happen on the exactly-zero padding
//     columns of real rows).  The off-diagonal norm is the sum of the off-diagonal squares themselves (never |A|^2 - sum a_ii^2,
//     which stalls at 1e-8 |C|_F); the solve stops when off_F <= 2^-43 |C|_F or after kSpectrumMaxSweeps sweeps, a decision every
//     thread reads from LDS.  Ranks come from counting, ties break by index; nothing is clamped.
//   EIGENVECTORS (vaek_cov_eigen_rows, vaek_eigen_event_replicas: the VEC instantiations).  The solve is one routine, jacobi_solve;
//     with VEC a round also forms V <- V J between its two barriers into two more buffers of the dead tile, and the record gains V
//     behind the spectrum record, columns in the eigenvalues' order, the largest component of each positive.  V never feeds back, so
//     the spectrum part is bitwise the VEC = false record.
//   PRINCIPAL ANGLES (vaek_subspace_angles): a second kernel reads two eigen records an earlier launch stored, forms M = U^T W,
//     R = W - U M and G = R^T R in LDS and solves G with the same jacobi_solve: sin^2 of the principal angles between the two spans.
//   EXACT LOG-LIKELIHOOD (vaek_exact_log_likelihood_replicas): a third kernel, one workgroup per one-decoder linear VAE, solves
//     G = K^T K of the decoder kernel with jacobi_solve<true> and evaluates log N(x; b_d, G + e^{eps} I), the closed-form ELBO and
//     their gap on rows from produce_row (explicit or drawn), float64 throughout; its own header comment is above the kernel.
//
// Three row sources feed that one text through the same row -> tile-slot assignment, so a record depends on the rows' bits only:
// SRC_EXPLICIT reads [rows][D] from HBM, SRC_REAL draws row i as vaek_make_batch writes x, SRC_FAKE draws latent row i as
// vaek_make_batch writes z1 / z2 and decodes fake = Decoder(z1) [+ sigmoid(SigDecoder(z1))] + z2 exp(sample_eps / 2) in float32 from
// the zero-padded ParamImage (eval_dev.h), linear_stats.hip's fake row with a one-input decode.
//
// The kernels read rows / parameters and store only the records, with per-lane vector stores; they read nothing back.
#include "eval_dev.h"
#include "mfma_geom.h"

namespace vaek {

constexpr int kSpectrumMaxSweeps = 32;       // bounds one launch -- a cap, not a tuned value
constexpr int kSpectrumMaxDim = 32;
constexpr int kSpectrumMaxRows = 4096;       // = vaek_stats_event_max_rows()
constexpr int kTileStride = 36;              // floats between two rows of the LDS tile: 16-byte aligned, 16 distinct banks per 4 rows
constexpr int kMatStride = 32;               // doubles between two rows of the Jacobi buffers
constexpr double kSpectrumTol = 0x1p-43;

enum { SRC_EXPLICIT = 0, SRC_REAL = 1, SRC_FAKE = 2 };

using f64x4 = __attribute__((ext_vector_type(4))) double;

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

// what a row source needs besides the row index
struct RowCtx {
    const float* xr;               // SRC_EXPLICIT: the set's rows
    const float* W;                // SRC_FAKE: the parameter image
    BatchArgs g;                   // SRC_REAL: the dataset draw; SRC_FAKE: its tag is z_tag
    uint2 key; unsigned step;
    int D, L;
    float ssigma;                  // SRC_FAKE: exp(sample_eps / 2)
};

// row `row` of the set as 32 floats, columns >= D zero
template <int SRC, int DP, int LP, bool SIG>
__device__ __forceinline__ void produce_row(const RowCtx& c, int row, float (&x)[kSpectrumMaxDim]) {
    const int D = c.D;
#pragma unroll
    for (int d = DP; d < kSpectrumMaxDim; ++d) x[d] = 0.f;
    if constexpr (SRC == SRC_EXPLICIT) {
        const float* const xr = c.xr + (long long)row * D;
#pragma unroll
        for (int d = 0; d < DP; ++d) x[d] = d < D ? xr[d] : 0.f;
    } else if constexpr (SRC == SRC_REAL) {
        // vaek_make_batch's work item for (row, c0), all c0: linear_stats.hip's text
        float nrm[16];
        dataset_normals(c.g, c.step, row, c.key, nrm);
#pragma unroll
        for (int c0 = 0; c0 < DP; c0 += 4) {
            float o[4] = {0.f, 0.f, 0.f, 0.f};
            if (c0 < D) dataset_cols4(c.g, c.step, row, c.key, nrm, c0, o);
#pragma unroll
            for (int k = 0; k < 4; ++k) x[c0 + k] = c0 + k < D ? o[k] : 0.f;
        }
    } else {
        using G = ParamImage<DP, LP, SIG>;
        const int L = c.L;
        const float* const W = c.W;
        const int zq0 = L >> 2, zsh = L & 3, nzb = (L + D + 3) / 4;       // z2 starts at element zsh of latent block zq0
        // the latent row: normal n is element n & 3 of block n >> 2; [0, L) is z1, [L, L + D) z2 (linear_stats.hip's text)
        float z1[LP], z2[DP];
#pragma unroll
        for (int q = 0; q < LP / 4; ++q) {
            float n4[4] = {0.f, 0.f, 0.f, 0.f};
            if (4 * q < L) latent_block(c.g, c.step, row, c.key, q, n4);
#pragma unroll
            for (int k = 0; k < 4; ++k) z1[4 * q + k] = n4[k];            // elements >= L of the last block belong to z2: rows l >= L of the image are 0
        }
        {
            float cat[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            {
                float n4[4];
                latent_block(c.g, c.step, row, c.key, zq0, n4);
                cat[4] = n4[0]; cat[5] = n4[1]; cat[6] = n4[2]; cat[7] = n4[3];
            }
#pragma unroll
            for (int j = 0; j < DP / 4; ++j) {
                if (4 * j < D) {
                    float n4[4] = {0.f, 0.f, 0.f, 0.f};
                    if (zq0 + j + 1 < nzb) latent_block(c.g, c.step, row, c.key, zq0 + j + 1, n4);
#pragma unroll
                    for (int k = 0; k < 4; ++k) { cat[k] = cat[4 + k]; cat[4 + k] = n4[k]; }
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        z2[4 * j + k] = zsh == 0 ? cat[k] : (zsh == 1 ? cat[k + 1] : (zsh == 2 ? cat[k + 2] : cat[k + 3]));
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) z2[4 * j + k] = 0.f;
                }
            }
        }
        // fake = Decoder(z1) [+ sigmoid(SigDecoder(z1))] + z2 exp(sample_eps / 2): the one-input form of linear_stats.hip's decode2
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
                    y[d] = fmaf(z1[l], W[G::WD + l * DP + d], y[d]);
                    if (SIG) ys[d] = fmaf(z1[l], W[G::WS + l * DP + d], ys[d]);
                }
            }
        }
#pragma unroll
        for (int d = 0; d < DP; ++d) {
            float f = fmaf(c.ssigma, z2[d], y[d]);
            if (SIG) f += 1.f / (1.f + expf(-ys[d]));
            x[d] = d < D ? f : 0.f;
        }
    }
}

// the sum of v over the 256 threads, the same value in every thread: a fixed binary tree in LDS
__device__ __forceinline__ double block_sum256(double v, double* red, int t) {
    red[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// the largest v over the 256 threads, the same value in every thread (v >= 0)
__device__ __forceinline__ double block_max256(double v, double* red, int t) {
    red[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] = fmax(red[t], red[t + s]);
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

constexpr int kMatDoubles = kSpectrumMaxDim * kMatStride;     // one Jacobi buffer

// Cyclic Jacobi, round-robin, on the symmetric De x De matrix in buffer 0 of `mat` (two buffers of kMatDoubles; De even, index
// De - 1 stays, the others turn), published by a barrier before the call.  Leaves the diagonalised matrix in buffer `cur` and returns
// (cur, sweeps, off_F), the same in every thread.  VEC: buffer 0 of `vec` (two more buffers) starts as I, also published, and every
// round forms V <- V J between the round's own two barriers: new column i = c_i V[:, i] + s_i V[:, mate(i)]; V ends in buffer `cur`
// of `vec` with C V = V diag(A).
template <bool VEC>
__device__ __forceinline__ void jacobi_solve(double* const mat, double* const vec, const int De, const double norm_c, double* const red,
                                             double* const rot_c, double* const rot_s, int* const rot_mate, const int t, int& cur_out,
                                             int& sweeps_out, double& off_out) {
    int cur = 0, sweeps = 0;
    double off_f;
    for (;;) {
        const double* const A = mat + cur * kMatDoubles;
        double osq = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int idx = t + 256 * k, i = idx >> 5, j = idx & 31;
            if (i < j && j < De) { const double v = A[i * kMatStride + j]; osq += 2.0 * v * v; }
        }
        off_f = sqrt(block_sum256(osq, red, t));                     // the same value in every thread: the decision is uniform
        if (off_f <= kSpectrumTol * norm_c || sweeps == kSpectrumMaxSweeps) break;
        const int n1 = De - 1;
        for (int round = 0; round < n1; ++round) {
            const double* const Ac = mat + cur * kMatDoubles;
            double* const An = mat + (cur ^ 1) * kMatDoubles;
            if (t < De / 2) {
                const int p = t == 0 ? round : (round + t) % n1;
                const int q = t == 0 ? n1 : (round - t + n1) % n1;
                const double apq = Ac[p * kMatStride + q];
                double cs = 1.0, sn = 0.0;
                if (apq != 0.0) {
                    const double theta = (Ac[q * kMatStride + q] - Ac[p * kMatStride + p]) / (2.0 * apq);
                    const double ath = fabs(theta);
                    const double tt = ath > 1e150 ? 0.5 / theta : copysign(1.0, theta) / (ath + sqrt(theta * theta + 1.0));
                    cs = 1.0 / sqrt(tt * tt + 1.0);
                    sn = tt * cs;
                }
                rot_c[p] = cs; rot_c[q] = cs;
                rot_s[p] = -sn; rot_s[q] = sn;                       // new column i = c col_i + s_i col_mate(i)
                rot_mate[p] = q; rot_mate[q] = p;
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int idx = t + 256 * k, i = idx >> 5, j = idx & 31;
                if (i <= j && j < De) {
                    const int mi = rot_mate[i], mj = rot_mate[j];
                    const double ci = rot_c[i], si = rot_s[i], cj = rot_c[j], sj = rot_s[j];
                    const double v = ci * (cj * Ac[i * kMatStride + j] + sj * Ac[i * kMatStride + mj]) +
                                     si * (cj * Ac[mi * kMatStride + j] + sj * Ac[mi * kMatStride + mj]);
                    An[i * kMatStride + j] = v;
                    An[j * kMatStride + i] = v;
                }
            }
            if constexpr (VEC) {
                const double* const Vc = vec + cur * kMatDoubles;
                double* const Vn = vec + (cur ^ 1) * kMatDoubles;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int idx = t + 256 * k, i = idx >> 5, j = idx & 31;
                    if (i < De && j < De) Vn[i * kMatStride + j] = rot_c[j] * Vc[i * kMatStride + j] + rot_s[j] * Vc[i * kMatStride + rot_mate[j]];
                }
            }
            __syncthreads();
            cur ^= 1;
        }
        ++sweeps;
    }
    cur_out = cur; sweeps_out = sweeps; off_out = off_f;
}

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
static const SpectrumVariant kSpectrumVariants[] = {VAEK_MFMA_SHAPES(VAEK_SPECTRUM_ROW)};
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

// ---- principal angles between two eigenbases (vaek_subspace_angles) ----------------------------------------------------------------
// Pair p: U = the ka eigenvectors of record a's largest eigenvalues, W = the kb of record b's (the last columns of the V blocks an
// EARLIER launch stored).  M = U^T W, R = W - U M formed explicitly (never I - M^T M, which loses small angles), G = R^T R for i <= j,
// mirrored, and G's eigenvalues -- sin^2 of the principal angles -- by jacobi_solve, the covariance solve's own text.  All float64 in LDS.
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

// ---- exact log-likelihood, exact ELBO and posterior gap of one-decoder linear VAEs (vaek_exact_log_likelihood_replicas) ------------
// Model r is a linear-Gaussian latent-variable model: p(x) = N(b_d, K^T K + e^{eps} I).  ONE workgroup per model: the parameter image,
// G = K^T K (element (i, j) one chain over l of exact float64 products of two float32 values, i <= j, mirrored) into Jacobi buffer 0,
// V = I, jacobi_solve<true> (the covariance solve's own text), then 1 / s_i, logdet, T and the encoder's constant published in LDS
// and the rows walked in tiles of 256, thread t taking row 256 j + t through produce_row (the bits vaek_make_batch writes, or the
// caller's).  Per row, float64 VALU fmas over broadcast LDS reads (V^T c, x E, mu K: at most 3 * 32^2 per row -- the matrix cores
// would need the rows staged as operands and the three products are chained per row, so a row per thread keeps every chain in
// registers).  A thread keeps three private running sums over its rows in tile order; one fixed binary tree per sum adds them.
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
static const ExactLogLikVariant kExactLogLikVariants[] = {VAEK_MFMA_SHAPES(VAEK_EXACT_ROW)};
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
    if (ctx->D > kSpectrumMaxDim) {
        set_error("%s: data_dim %d, need <= %d (see vaek_supports_cov_spectrum)", who, ctx->D, kSpectrumMaxDim);
        return VAEK_ERR_INVALID;
    }
    if (n < 1 || n > spectrum_max_sets()) {
        set_error("%s: %d sets, need 1 .. %d (vaek_cov_spectrum_max_sets)", who, n, spectrum_max_sets());
        return VAEK_ERR_INVALID;
    }
    if (rows < 2 || rows > kSpectrumMaxRows) {
        set_error("%s: %d rows, need 2 .. %d (vaek_stats_event_max_rows; one row has no ddof = 1 covariance)", who, rows, kSpectrumMaxRows);
        return VAEK_ERR_INVALID;
    }
    if (x_stride < 0 || (x_stride > 0 && x_stride < (int64_t)rows * ctx->D)) {
        set_error("%s: x_stride %lld: need 0 (shared rows) or >= rows * D = %lld", who, (long long)x_stride, (long long)rows * ctx->D);
        return VAEK_ERR_INVALID;
    }
    const int64_t len = vec ? eigen_record_len(ctx) : spectrum_record_len(ctx);
    if (out_stride < len) {
        set_error("%s: out_stride %lld < record length %lld (%s)", who, (long long)out_stride, (long long)len,
                  vec ? "vaek_cov_eigen_record_len" : "vaek_cov_spectrum_record_len");
        return VAEK_ERR_INVALID;
    }
    if (((uintptr_t)out & 7u) != 0) { set_error("%s: out is not 8-byte aligned", who); return VAEK_ERR_INVALID; }
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
    if (!ctx || !params || !ev) { set_error("%s: null context, params or event", who); return VAEK_ERR_INVALID; }
    if (ev->struct_size != (int32_t)sizeof(vaek_spectrum_event)) {
        set_error("%s: vaek_spectrum_event.struct_size %d != %d (header / library mismatch)", who, ev->struct_size, (int)sizeof(vaek_spectrum_event));
        return VAEK_ERR_INVALID;
    }
    const SpectrumVariant* var = pick_spectrum(ctx);
    if (!var) {
        set_error("%s: needs a float32 linear VAE (no hidden layers) with D, L <= 32, D <= 28 with two decoders (see "
                  "vaek_supports_spectrum_event)", who);
        return VAEK_ERR_INVALID;
    }
    if (ev->n < 1 || ev->n > resident_max_replicas()) {
        set_error("%s: %d replicas, need 1 .. %d (vaek_train_loop_max_replicas)", who, ev->n, resident_max_replicas());
        return VAEK_ERR_INVALID;
    }
    if (ev->rows < 2 || ev->rows > kSpectrumMaxRows) {
        set_error("%s: %d rows, need 2 .. %d (vaek_stats_event_max_rows; one row has no ddof = 1 covariance)", who, ev->rows, kSpectrumMaxRows);
        return VAEK_ERR_INVALID;
    }
    if (!ev->x_seeds || !ev->x_steps || !ev->z_seeds || !ev->z_steps || !ev->sample_eps || !ev->out) {
        set_error("%s: x_seeds, x_steps, z_seeds, z_steps, sample_eps or out is NULL", who);
        return VAEK_ERR_INVALID;
    }
    const int64_t len = vec ? eigen_record_len(ctx) : spectrum_record_len(ctx);
    if (ev->state_stride < ctx->P || ev->out_stride < 2 * len) {
        set_error("%s: state_stride %lld < P = %lld or out_stride %lld < two records of %lld (%s)", who, (long long)ev->state_stride,
                  (long long)ctx->P, (long long)ev->out_stride, (long long)len, vec ? "vaek_cov_eigen_record_len" : "vaek_cov_spectrum_record_len");
        return VAEK_ERR_INVALID;
    }
    if (((uintptr_t)ev->out & 7u) != 0) { set_error("%s: out is not 8-byte aligned", who); return VAEK_ERR_INVALID; }
    if (int rc = check_dataset_draw(who, ctx, kind, A, dd, did, pad, ev->a_stride, x_tag)) return rc;
    if (z_tag >= 0x40000000u) { set_error("%s: a tag >= 2^30", who); return VAEK_ERR_INVALID; }
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
    if (ctx->D > kSpectrumMaxDim) {
        set_error("%s: data_dim %d, need <= %d (see vaek_supports_cov_spectrum)", who, ctx->D, kSpectrumMaxDim);
        return VAEK_ERR_INVALID;
    }
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
    if ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 7u) != 0) { set_error("%s: a, b or out is not 8-byte aligned", who); return VAEK_ERR_INVALID; }
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
    if (!ctx || !params || !ll) { set_error("%s: null context, params or description", who); return VAEK_ERR_INVALID; }
    if (ll->struct_size != (int32_t)sizeof(vaek_exact_log_likelihood)) {
        set_error("%s: vaek_exact_log_likelihood.struct_size %d != %d (header / library mismatch)", who, ll->struct_size,
                  (int)sizeof(vaek_exact_log_likelihood));
        return VAEK_ERR_INVALID;
    }
    const ExactLogLikVariant* var = pick_exact_loglik(ctx);
    if (!var) {
        set_error("%s: needs a float32 linear VAE (no hidden layers) with ONE decoder and D, L <= 32: the sigmoid second decoder has no "
                  "closed form (see vaek_supports_exact_log_likelihood)", who);
        return VAEK_ERR_INVALID;
    }
    if (ll->n < 1 || ll->n > resident_max_replicas()) {
        set_error("%s: %d replicas, need 1 .. %d (vaek_train_loop_max_replicas)", who, ll->n, resident_max_replicas());
        return VAEK_ERR_INVALID;
    }
    if (ll->rows < 1 || ll->rows > kLogLikMaxRows) {
        set_error("%s: %d rows, need 1 .. %d (vaek_log_likelihood_max_rows)", who, ll->rows, kLogLikMaxRows);
        return VAEK_ERR_INVALID;
    }
    const bool explicit_rows = ll->x != nullptr;
    if (!ll->out || (!explicit_rows && (!ll->x_seeds || !ll->x_steps))) {
        set_error("%s: x_seeds, x_steps (drawing mode) or out is NULL", who);
        return VAEK_ERR_INVALID;
    }
    const int64_t len = exact_loglik_record_len(ctx);
    if (ll->state_stride < ctx->P || ll->out_stride < len) {
        set_error("%s: state_stride %lld < P = %lld or out_stride %lld < record length %lld (vaek_exact_log_likelihood_record_len)", who,
                  (long long)ll->state_stride, (long long)ctx->P, (long long)ll->out_stride, (long long)len);
        return VAEK_ERR_INVALID;
    }
    if ((((uintptr_t)ll->out | (uintptr_t)ll->row_out) & 7u) != 0) { set_error("%s: out or row_out is not 8-byte aligned", who); return VAEK_ERR_INVALID; }
    if (ll->row_out && (ll->row_stride < 0 || (ll->row_stride < 2 * (int64_t)ll->rows && (ll->row_stride > 0 || ll->n > 1)))) {
        set_error("%s: row_stride %lld: need >= 2 * rows = %lld (0 with one replica)", who, (long long)ll->row_stride, 2 * (long long)ll->rows);
        return VAEK_ERR_INVALID;
    }
    if (explicit_rows) {
        if (ll->x_stride < 0 || (ll->x_stride > 0 && ll->x_stride < (int64_t)ll->rows * ctx->D)) {
            set_error("%s: x_stride %lld: need 0 (shared rows) or >= rows * D = %lld", who, (long long)ll->x_stride, (long long)ll->rows * ctx->D);
            return VAEK_ERR_INVALID;
        }
    } else if (int rc = check_dataset_draw(who, ctx, kind, A, dd, did, pad, ll->a_stride, x_tag)) {
        return rc;
    }
    ExactLogLikArgs a{};
    a.params = params; a.state_stride = ll->state_stride;
    a.x_seeds = reinterpret_cast<const unsigned long long*>(ll->x_seeds); a.x_steps = ll->x_steps;
    a.x = ll->x; a.x_stride = ll->x_stride;
    a.out = ll->out; a.out_stride = ll->out_stride; a.row_out = ll->row_out; a.row_stride = ll->row_stride;
    a.rows = ll->rows; a.D = ctx->D; a.L = ctx->L; a.off_epsp = (int)ctx->off_epsp; a.off_eps = (int)ctx->off_eps;
    a.eps_cli = ctx->cfg.eps_cli;
    if (explicit_rows) {
        fill_draw_args(&a.gen, ctx, ll->rows, 2, nullptr, 0, 0, 0, 0.f, 0);      // nothing is drawn: the sphere's kind, which has no matrix
    } else {
        a.a_stride = ll->a_stride;
        fill_draw_args(&a.gen, ctx, ll->rows, kind, A, dd, did, pad, var_added, x_tag);
    }
    hipStream_t st = (hipStream_t)stream;
    {
        ProfScope ps("exact_loglik_replicas", st);
        launch_k(ps, var->fn, dim3((unsigned)ll->n), dim3(256), 0, st, a);
    }
    VAEK_HIP_CHECK(hipGetLastError());
    return VAEK_OK;
}
}  // extern "C"
