// What the covariance / eigen kernels share (cov_spectrum.hip with the principal angles, exact_loglik.hip): the float64 Jacobi solve of a
// symmetric matrix of at most 32 x 32 in LDS, the two 256-thread reductions it decides with, and the row sources that feed the
// covariance moments and the exact log-likelihood.  Each is ONE text.  (The counting-rank store of the eigenvalues is NOT here: as a
// shared function it changed the instruction text of the kernels that called it, so each kernel keeps its eight lines)
//
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
//
// Three row sources feed that one text through the same row -> tile-slot assignment, so a record depends on the rows' bits only:
// SRC_EXPLICIT reads [rows][D] from HBM, SRC_REAL draws row i as vaek_make_batch writes x, SRC_FAKE draws latent row i as
// vaek_make_batch writes z1 / z2 and decodes fake = Decoder(z1) [+ sigmoid(SigDecoder(z1))] + z2 exp(sample_eps / 2) in float32 from
// the zero-padded ParamImage (eval_dev.h), linear_stats.hip's fake row with a one-input decode.  produce_row lives here and not in
// eval_dev.h: linear_stats.hip and linear_loglik.hip keep their own row text and include only that header.
#pragma once
#include "eval_dev.h"

namespace vaek {

constexpr int kSpectrumMaxSweeps = 32;       // bounds one launch -- a cap, not a tuned value
constexpr int kSpectrumMaxDim = 32;
constexpr int kSpectrumMaxRows = 4096;       // = vaek_stats_event_max_rows()
constexpr int kTileStride = 36;              // floats between two rows of the LDS tile: 16-byte aligned, 16 distinct banks per 4 rows
constexpr int kMatStride = 32;               // doubles between two rows of the Jacobi buffers
constexpr double kSpectrumTol = 0x1p-43;

enum { SRC_EXPLICIT = 0, SRC_REAL = 1, SRC_FAKE = 2 };

using f64x4 = __attribute__((ext_vector_type(4))) double;

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

}  // namespace vaek
