// The Lanczos core of the three Hessians (elbo_hessian.hip, sampled_hessian.hip, mlp3_hessian.hip), once: the constants and the record
// layout, the start rule, the one-workgroup orthogonalise-and-measure step, the breakdown rule, the Ritz tail, omega, the pair order
// and the Lanczos record's stores.  Device only; every function is called by all 256 threads of a workgroup and takes its LDS scratch as
// pointers (the exact kernel lays the Jacobi buffers over dead images of its dynamic pool, the other two hold static arrays).  What is
// NOT here, on purpose: the state-block layouts and the launch structure of the three recursions, the mlp3 unit's chunked vector
// arithmetic, and who computes omega there.  eigen_dev.h is included and not edited.
//
// The Lanczos record, kLanczosRecord doubles (the two sampled calls add [140] samples and [141] two-decoder flag on top):
//    [0] f                [4] Jacobi sweeps        [8]  eps                      [12, 44)   Ritz values, ascending, zero beyond k
//    [1] |grad f|         [5] off_F after them     [9]  theta_max  (0 at k = 0)  [44, 76)   residual bounds |beta_k V[k-1][i]|, same order
//    [2] k, steps taken   [6] |T|_F                [10] theta_min  (0 at k = 0)  [76, 108)  alpha_1 .. alpha_k, zero beyond k
//    [3] beta_k           [7] rows                 [11] omega = max |v_i . v_j|  [108, 140) beta_1 .. beta_k, zero beyond k
// The HVP record, kHvpRecord doubles: [0] f  [1] |grad f|  [2] eps  [3] rows.  Its store is one select and stays written out in the
// three units: as a helper of either shape it reorders elbo_hessian_kernel<false> (+4 % on 32 products) and mlp3_hessian_record_kernel.
#pragma once
#include "eigen_dev.h"

namespace vaek {

constexpr int kLanczosMaxSteps = 32;
static_assert(kLanczosMaxSteps == kSpectrumMaxDim, "T is solved by the Jacobi routine: its size bounds the steps");
constexpr int kLanczosHead = 12;
constexpr int kLanczosRecord = kLanczosHead + 4 * kLanczosMaxSteps;
constexpr int kHvpRecord = 4;
constexpr int kHvpMaxVectors = 64;           // bounds one call -- a cap, not a tuned value
constexpr double kLanczosBreakdown = 0x1p-40;
constexpr double kLog2PiF64 = 1.8378770664093454835606594728112;

// the LDS scratch of the Ritz tail: mat and vec two Jacobi buffers each, red of 256 doubles, the others of kSpectrumMaxDim; alpha and
// beta hold the recursion's coefficients when the tail is called
struct LanczosLds {
    double *mat, *vec, *red, *alpha, *beta, *rot_c, *rot_s, *eig;
    int* rot_mate;
};
struct RitzResult { int sweeps; double off_f, norm_t, beta_k; };

// the steps a start vector of norm n0 allows: none for v0 = 0 or not a number, else no more than the dimension
__device__ __forceinline__ int lanczos_kmax(const double n0, const int steps, const int P) {
    return n0 > 0.0 && n0 < INFINITY ? (steps < P ? steps : P) : 0;
}

// v_1 = v0 / |v0| into basis row 0 (not stored at kmax = 0); returns kmax
__device__ __forceinline__ int lanczos_start(const double* const v0, double* const basis, const int P, const int steps, double* const red,
                                             const int t) {
    double part = 0.0;
    for (int e = t; e < P; e += 256) part = fma(v0[e], v0[e], part);
    const double n0 = sqrt(block_sum256(part, red, t));
    const int kmax = lanczos_kmax(n0, steps, P);
    if (kmax > 0)
        for (int e = t; e < P; e += 256) basis[e] = v0[e] / n0;
    return kmax;
}

// w = H v_{j+1} in LDS, published: classical Gram-Schmidt, twice, against basis rows 0 .. j, every dot through block_sum256.  alpha is
// what the two passes take out along v_{j+1}, beta = |w| afterwards; both the same in every thread.
__device__ __forceinline__ void lanczos_orthogonalise(double* const wv, const double* const basis, const int P, const int j, double* const coef,
                                                      double* const red, const int t, double& alpha_out, double& beta_out) {
    double al = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
        for (int i = 0; i <= j; ++i) {
            const double* const vi = basis + (long long)i * P;
            double d = 0.0;
            for (int e = t; e < P; e += 256) d = fma(vi[e], wv[e], d);
            d = block_sum256(d, red, t);
            if (t == 0) coef[i] = d;
            if (i == j) al += d;
        }
        __syncthreads();
        for (int e = t; e < P; e += 256) {
            double s = wv[e];
            for (int i = 0; i <= j; ++i) s = fma(-coef[i], basis[(long long)i * P + e], s);
            wv[e] = s;
        }
        __syncthreads();
    }
    double part = 0.0;
    for (int e = t; e < P; e += 256) part = fma(wv[e], wv[e], part);
    alpha_out = al;
    beta_out = sqrt(block_sum256(part, red, t));
}

// THE breakdown rule, after step k: stop where beta is below kLanczosBreakdown of the largest |alpha|, beta so far, or at kmax.
// `scale` is that largest value before the step and after it.
__device__ __forceinline__ bool lanczos_stop(const double al, const double be, const int k, const int kmax, double& scale) {
    scale = fmax(scale, fabs(al));
    const bool stop = be <= kLanczosBreakdown * scale || k == kmax;
    scale = fmax(scale, be);
    return stop;
}

// ... and v_{k+1} = w / beta into basis row k where the recursion goes on.  The same values in every thread: the decision is uniform.
__device__ __forceinline__ bool lanczos_next(const double* const wv, double* const basis, const int P, const int k, const int kmax,
                                             const double al, const double be, double& scale, const int t) {
    const bool stop = lanczos_stop(al, be, k, kmax, scale);
    if (!stop) {
        double* const vn = basis + (long long)k * P;
        for (int e = t; e < P; e += 256) vn[e] = wv[e] / be;
    }
    return stop;
}

// alpha_1 .. alpha_k and beta_1 .. beta_k in s.alpha / s.beta, published: T (k x k, tridiagonal, zero outside) into Jacobi buffer 0,
// V = I, the solve, then slots 9, 10 (k > 0) and 12 .. 139 of the record
__device__ __forceinline__ RitzResult lanczos_ritz(const LanczosLds& s, const int k, double* const out, const int t) {
    double sq = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int idx = t + 256 * q, i = idx >> 5, j = idx & 31;
        double v = 0.0;
        if (i < k && j < k) {                                           // the pad row and column of an odd k are zero
            if (i == j) v = s.alpha[i];
            else if (i + 1 == j) v = s.beta[i];
            else if (j + 1 == i) v = s.beta[j];
        }
        s.mat[i * kMatStride + j] = v;
        if (i <= j) sq += i == j ? v * v : 2.0 * v * v;
        const double id = i == j ? 1.0 : 0.0;
        s.vec[i * kMatStride + j] = id;                                 // the solve may end in either buffer
        s.vec[kMatDoubles + i * kMatStride + j] = id;
    }
    RitzResult r;
    r.norm_t = sqrt(block_sum256(sq, s.red, t));                        // its barriers also publish T and V
    int cur = 0;
    r.sweeps = 0;
    r.off_f = 0.0;
    if (k > 0) jacobi_solve<true>(s.mat, s.vec, k + (k & 1), r.norm_t, s.red, s.rot_c, s.rot_s, s.rot_mate, t, cur, r.sweeps, r.off_f);
    const double* const A = s.mat + cur * kMatDoubles;
    const double* const V = s.vec + cur * kMatDoubles;
    if (t < kLanczosMaxSteps) s.eig[t] = t < k ? A[t * kMatStride + t] : 0.0;
    __syncthreads();
    r.beta_k = k > 0 ? s.beta[k - 1] : 0.0;
    // Ritz values ascending by counting ranks (the pad of an odd k is index k: not counted), residual bounds in the same order
    if (t < kLanczosMaxSteps) {
        if (t < k) {
            const double e = s.eig[t];
            int rank = 0;
            for (int j = 0; j < k; ++j) {
                const double o = s.eig[j];
                rank += (o < e || (o == e && j < t)) ? 1 : 0;
            }
            out[kLanczosHead + rank] = e;
            out[kLanczosHead + kLanczosMaxSteps + rank] = fabs(r.beta_k * V[(k - 1) * kMatStride + t]);
            if (rank == k - 1) out[9] = e;
            if (rank == 0) out[10] = e;
        } else {
            out[kLanczosHead + t] = 0.0;
            out[kLanczosHead + kLanczosMaxSteps + t] = 0.0;
        }
        out[kLanczosHead + 2 * kLanczosMaxSteps + t] = t < k ? s.alpha[t] : 0.0;
        out[kLanczosHead + 3 * kLanczosMaxSteps + t] = t < k ? s.beta[t] : 0.0;
    }
    return r;
}

// pair q of the order (0, 1), (0, 2), (1, 2), (0, 3), ..: (i, j) with i < j; the pairs below row k are the first k (k - 1) / 2
__device__ __forceinline__ void lanczos_pair(const int q, int& i_out, int& j_out) {
    int j = 1, first = 0;
    while (first + j <= q) { first += j; ++j; }
    i_out = q - first;
    j_out = j;
}

// omega = max_{i < j < k} |v_i . v_j| of a basis one workgroup can walk: a wave per pair, lanes over the elements, one fixed butterfly
__device__ __forceinline__ double lanczos_omega(const double* const basis, const int P, const int k, double* const red, const int t) {
    double wmax = 0.0;
    const int wave = t >> 6, lane = t & 63, npairs = k * (k - 1) / 2;
    for (int q = wave; q < npairs; q += 4) {
        int i, j;
        lanczos_pair(q, i, j);
        const double* const vi = basis + (long long)i * P;
        const double* const vj = basis + (long long)j * P;
        double s = 0.0;
        for (int e = lane; e < P; e += 64) s = fma(vi[e], vj[e], s);
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        wmax = fmax(wmax, fabs(s));
    }
    return block_max256(wmax, red, t);
}

// slots 0 .. 8 and 11 of the record, and zeros into 9, 10 where k = 0 (lanczos_ritz stores them otherwise)
__device__ __forceinline__ void lanczos_head_store(double* const out, const int t, const int k, const double f, const double gnorm,
                                                   const double eps, const int rows, const double omega, const RitzResult& r) {
    if (t < kLanczosHead) {
        double v;
        switch (t) {
            case 0: v = f; break;
            case 1: v = gnorm; break;
            case 2: v = (double)k; break;
            case 3: v = r.beta_k; break;
            case 4: v = (double)r.sweeps; break;
            case 5: v = r.off_f; break;
            case 6: v = r.norm_t; break;
            case 7: v = (double)rows; break;
            case 8: v = eps; break;
            case 11: v = omega; break;
            default: v = 0.0; break;                                    // theta_max, theta_min where k = 0
        }
        if (t < 9 || t == 11 || k == 0) out[t] = v;
    }
}

}  // namespace vaek
