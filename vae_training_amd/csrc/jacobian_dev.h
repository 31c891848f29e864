// What the decoder-Jacobian calls share (mlp3_jacobian.hip, linear_jacobian.hip): the row solve -- J of one latent row in LDS -> its
// row record -- and the finalize launch -- the row records of a replica -> its model record.  Each is ONE text; a .hip file keeps the
// thin __global__ wrappers and whatever produces J.  The solve is templated on J's element type: float for the MLP call, whose J is the
// float32 image of four matrix-core products (the products of two floats are exact in float64), double for the linear call, whose J is
// cheap enough to form in float64.  Neither instantiation knows where J came from.
//   ROW RECORD (2 L + 4 doubles): [0, L) lambda descending, [L, 2 L) diag G, [2 L] rank, [2 L + 1] sweeps, [2 L + 2] off_F, [2 L + 3] |G|_F
//   MODEL RECORD (2 L + 8 doubles): include/vaek.h
#pragma once
#include "eigen_dev.h"
#include "eval_check.h"

namespace vaek {

constexpr int MJ_QS = 8;                     // sums one tree pass of the finalize launch carries

// the LDS of a row solve besides J itself
struct JacobianSolveLds {
    double mat[2 * kMatDoubles];
    double red[256];
    double rot_c[kSpectrumMaxDim], rot_s[kSpectrumMaxDim], eig[kSpectrumMaxDim], dg[kSpectrumMaxDim];
    int rot_mate[kSpectrumMaxDim];
};

// Js: J[l][d] of the row (L x D, row stride D) in LDS, published by a barrier before the call.  Forms G = J^T J for i <= j, mirrored,
// zero outside [L] x [L], each entry a sum over d in d order; |G|_F; jacobi_solve<false> on G padded to even order; the eigenvalues
// ranked descending by counting, ties by index; diag G, the rank under rank_tol, sweeps and off_F.  Stores the record at rec and, where
// given, at ro.  256 threads.
template <typename T>
__device__ __forceinline__ void jacobian_solve_row(const T* const Js, JacobianSolveLds& s, const int D, const int L, const double rank_tol,
                                                   double* const rec, double* const ro, const int t) {
    double* const mat = s.mat;
    double sq = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int idx = t + 256 * k, i = idx >> 5, j = idx & 31;
        if (i <= j) {
            double v = 0.0;
            if (j < L) {
                for (int d = 0; d < D; ++d) v += (double)Js[i * D + d] * (double)Js[j * D + d];
            }
            mat[i * kMatStride + j] = v;
            mat[j * kMatStride + i] = v;
            if (i == j) s.dg[i] = v;
            sq += i == j ? v * v : 2.0 * v * v;
        }
    }
    const double norm_g = sqrt(block_sum256(sq, s.red, t));          // its barriers also publish the first buffer

    int cur, sweeps;
    double off_f;
    jacobi_solve<false>(mat, nullptr, L + (L & 1), norm_g, s.red, s.rot_c, s.rot_s, s.rot_mate, t, cur, sweeps, off_f);

    // ---- eigenvalues descending: the rank of a diagonal element is the count of those before it, ties by index -----------------------
    const double* const A = mat + cur * kMatDoubles;
    if (t < kSpectrumMaxDim) s.eig[t] = t < L ? A[t * kMatStride + t] : 0.0;
    __syncthreads();
    if (t < L) {
        const double e = s.eig[t];
        int rank = 0;
        for (int j = 0; j < L; ++j) {
            const double o = s.eig[j];
            rank += (o > e || (o == e && j < t)) ? 1 : 0;
        }
        rec[rank] = e;
        rec[L + t] = s.dg[t];
        if (ro) { ro[rank] = e; ro[L + t] = s.dg[t]; }
    }
    if (t >= 64 && t < 68) {
        const int q = t - 64;
        double tail;
        if (q == 0) {                            // the numerical rank: #{k : lambda_k > rank_tol lambda_1}, 0 where lambda_1 = 0
            double top = 0.0;
            for (int j = 0; j < L; ++j) top = fmax(top, s.eig[j]);
            int cnt = 0;
            for (int j = 0; j < L; ++j) cnt += (top > 0.0 && s.eig[j] > rank_tol * top) ? 1 : 0;
            tail = (double)cnt;
        } else {
            tail = q == 1 ? (double)sweeps : (q == 2 ? off_f : norm_g);
        }
        rec[2 * L + q] = tail;
        if (ro) ro[2 * L + q] = tail;
    }
}

struct JacobianFinalArgs {
    const double* rec;                       // [n][rows][2 L + 4]
    double* out; long long out_stride;
    int rows, L;
    double rank_tol;
};

// the LDS of the finalize launch
struct JacobianFinalLds {
    double red[MJ_QS][256];
    double mred[256];
    double res[2 * kSpectrumMaxDim + 8];
};

// the row records of replica r -> its model record: the rows in a fixed binary tree per 256 rows, then the tiles in order, float64;
// lane t stores double t of the record.  256 threads.
__device__ __forceinline__ void jacobian_finalize_replica(const JacobianFinalArgs& a, JacobianFinalLds& s, const long long r, const int t) {
    const int L = a.L, rows = a.rows, len = 2 * L + 4;
    const double* const rec = a.rec + r * rows * (long long)len;
    const int tiles = (rows + 255) / 256;
    const int nq = 2 * L + 2;                    // sums: lambda_k (L), diag (L), rank, |J|_F^2 = the diagonal added in l order

    for (int q0 = 0; q0 < nq; q0 += MJ_QS) {
        double acc[MJ_QS];
#pragma unroll
        for (int k = 0; k < MJ_QS; ++k) acc[k] = 0.0;
        for (int tile = 0; tile < tiles; ++tile) {
            const int row = tile * 256 + t;
            const double* const rw = rec + (long long)min(row, rows - 1) * len;
#pragma unroll
            for (int k = 0; k < MJ_QS; ++k) {
                const int q = q0 + k;
                double v = 0.0;
                if (row < rows && q < nq) {
                    if (q <= 2 * L) {
                        v = rw[q];
                    } else {
                        for (int l = 0; l < L; ++l) v += rw[L + l];
                    }
                }
                s.red[k][t] = v;
            }
            tree_sum256(s.red, t);
#pragma unroll
            for (int k = 0; k < MJ_QS; ++k) acc[k] += s.red[k][0];       // the tiles in tile order
            __syncthreads();
        }
        if (t == 0) {
#pragma unroll
            for (int k = 0; k < MJ_QS; ++k) {
                const int q = q0 + k;
                if (q < nq) {
                    const double mean = acc[k] / (double)rows;
                    if (q < 2 * L) s.res[8 + q] = mean;
                    else if (q == 2 * L) s.res[1] = mean;
                    else s.res[4] = mean;
                }
            }
        }
    }

    // ---- the extremes: every one a maximum of values >= 0 (the smallest rank as L - the largest of L - rank) -------------------------
    double mx_rank = 0.0, mx_def = 0.0, mx_sweeps = 0.0, mx_ratio = 0.0;
    for (int tile = 0; tile < tiles; ++tile) {
        const int row = tile * 256 + t;
        double rk = (double)L, sw = 0.0, ratio = 0.0, has = 0.0;
        if (row < rows) {
            const double* const rw = rec + (long long)row * len;
            rk = rw[2 * L]; sw = rw[2 * L + 1];
            const double ng = rw[2 * L + 3];
            ratio = ng > 0.0 ? rw[2 * L + 2] / ng : 0.0;
            has = 1.0;
        }
        mx_rank = fmax(mx_rank, block_max256(has * rk, s.mred, t));
        mx_def = fmax(mx_def, block_max256((double)L - rk, s.mred, t));
        mx_sweeps = fmax(mx_sweeps, block_max256(sw, s.mred, t));
        mx_ratio = fmax(mx_ratio, block_max256(ratio, s.mred, t));
    }
    if (t == 0) {
        s.res[0] = (double)rows;
        s.res[2] = (double)L - mx_def;
        s.res[3] = mx_rank;
        s.res[5] = mx_sweeps;
        s.res[6] = mx_ratio;
        s.res[7] = a.rank_tol;
    }
    __syncthreads();
    if (t < 2 * L + 8) a.out[r * a.out_stride + t] = s.res[t];
}

// the two record lengths, and the refusals both calls make after check_eval, as `who` makes them: row_out's stride and alignment, rank_tol
static inline int64_t jacobian_record_len(const vaek_ctx* c) { return 2 * (int64_t)c->L + 8; }
static inline int64_t jacobian_row_record_len(const vaek_ctx* c) { return 2 * (int64_t)c->L + 4; }
static inline size_t jacobian_up16(size_t b) { return (b + 15) & ~(size_t)15; }
static inline int check_jacobian_outputs(const char* who, const vaek_ctx* ctx, const vaek_decoder_jacobian* dj) {
    const int64_t rlen = jacobian_row_record_len(ctx);
    if (dj->row_out && dj->row_out_stride < (int64_t)dj->rows * rlen) {
        set_error("%s: row_out_stride %lld < rows x row record length = %lld (vaek_decoder_jacobian_row_record_len)", who,
                  (long long)dj->row_out_stride, (long long)dj->rows * rlen);
        return VAEK_ERR_INVALID;
    }
    if (int rc = check_aligned8(who, "row_out", (uintptr_t)dj->row_out)) return rc;
    if (!(dj->rank_tol >= 0.0 && dj->rank_tol < 1.0)) {
        set_error("%s: rank_tol %g, need 0 <= rank_tol < 1", who, dj->rank_tol);
        return VAEK_ERR_INVALID;
    }
    return VAEK_OK;
}

}  // namespace vaek
