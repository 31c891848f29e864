// The pieces the row-per-thread evaluation kernels share (linear_stats.hip, linear_loglik.hip and the row launch of mlp3_loglik.hip):
// the zero-padded parameter image of a linear VAE and its fill, the online log-sum-exp of the importance weights, the float64 tree
// over a workgroup and the tile partial the finalize launch reads.  Each is ONE text: a change to the flat parameter layout or to the
// estimator is made here and reaches every kernel.  The drawn data row and the encoder product over the image are NOT here: called
// from this header they cost linear_loglik_kernel<32, 32, true> 16 % of its device time (the allocator then settles at 256 VGPRs and
// two waves per SIMD instead of 256 + 69 AGPRs and one), so linear_stats.hip and linear_loglik.hip each keep their text.
#pragma once
#include "rng_dev.h"
#include "vaek_internal.h"

namespace vaek {

constexpr int kLogLikRecord = 4;             // IWAE-K bound, ELBO estimate, effective sample size, eps
constexpr int kLogLikSums = 3;               // float64 row sums

constexpr int up4(int n) { return (n + 3) & ~3; }

// the smallest padded shape of a variant table ({dp, lp, sig, fn} rows, built from VAEK_EVAL_SHAPES) that holds (D, L)
template <typename V, int N>
const V* pick_smallest_shape(const V (&table)[N], int D, int L, bool sig) {
    const V* best = nullptr;
    for (const auto& v : table) {
        if (v.sig != (sig ? 1 : 0) || v.dp < D || v.lp < L) continue;
        if (!best || v.dp * v.lp < best->dp * best->lp) best = &v;
    }
    return best;
}

// The <= 3.2 K parameter floats of a linear VAE as a zero-padded LDS image [DP][LP] / [LP][DP] (linear_stats.hip's header says why:
// broadcast reads, 16 bytes at a time, static register indices, a padded row or column adds 0).  The members are float offsets.
template <int DP, int LP, bool SIG>
struct ParamImage {
    static_assert(DP % 4 == 0 && LP % 4 == 0, "the image is read 16 bytes at a time");
    static constexpr int WE = 0, BE = WE + DP * LP, WD = BE + LP, BD = WD + LP * DP, WS = BD + DP, BS = WS + (SIG ? LP * DP : 0),
                         SD = BS + (SIG ? DP : 0), LV = SD + LP, N = LV + LP;      // SD: exp(epsilon_p / 2), LV: epsilon_p itself

    // thread t of 256 fills its share from the flat parameters p: zero outside [D] x [L].  The caller's barrier follows
    static __device__ __forceinline__ void fill(float* W, const float* p, int D, int L, int off_epsp, int t) {
        const int off_be = D * L, off_wd = off_be + L, off_bd = off_wd + L * D, off_ws = off_bd + D, off_bs = off_ws + L * D;
        for (int i = t; i < DP * LP; i += 256) {
            const int d = i / LP, l = i % LP;
            W[WE + i] = (d < D && l < L) ? p[d * L + l] : 0.f;
            const int l2 = i / DP, d2 = i % DP;
            const bool in = l2 < L && d2 < D;
            W[WD + i] = in ? p[off_wd + l2 * D + d2] : 0.f;
            if (SIG) W[WS + i] = in ? p[off_ws + l2 * D + d2] : 0.f;
        }
        for (int i = t; i < LP; i += 256) {
            const float lv = i < L ? p[off_epsp + i] : 0.f;
            W[BE + i] = i < L ? p[off_be + i] : 0.f;
            W[LV + i] = lv;
            W[SD + i] = i < L ? expf(0.5f * lv) : 0.f;                    // e^{lv/2}, networks.py:73
        }
        for (int i = t; i < DP; i += 256) {
            W[BD + i] = i < D ? p[off_bd + i] : 0.f;
            if (SIG) W[BS + i] = i < D ? p[off_bs + i] : 0.f;
        }
    }
};

// online log-sum-exp of a row's log weights, float32, in push order: running max, sum e^{lw - m}, sum e^{2 (lw - m)}, sum lw
struct OnlineLogSumExp {
    float m = -INFINITY, s1 = 0.f, s2 = 0.f, sl = 0.f;
    __device__ __forceinline__ void push(float lw) {
        const float mn = fmaxf(m, lw);
        const float c = expf(m - mn), e = expf(lw - mn);                   // first sample: c = e^{-inf} = 0, e = 1
        s1 = fmaf(s1, c, e);
        s2 = fmaf(s2, c * c, e * e);
        sl += lw;
        m = mn;
    }
    // the row's IWAE-K bound, K-sample ELBO estimate and normalised effective sample size
    __device__ __forceinline__ void finish(int K, float (&res)[kLogLikSums]) const {
        const float kf = (float)K;
        res[0] = m + logf(s1) - logf(kf);
        res[1] = sl / kf;
        res[2] = (s1 * s1) / (kf * s2);
    }
};

// the workgroup's NS sums: thread t has stored red[.][t]; a fixed binary tree over the 256 threads leaves them in red[.][0]
template <int NS>
__device__ __forceinline__ void tree_sum256(double (&red)[NS][256], int t) {
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int k = 0; k < NS; ++k) red[k][t] += red[k][t + s];
        }
        __syncthreads();
    }
}

// the tile's partial [4] of replica r in part[n][tiles = gridDim.x][4]: lane t stores double t; the finalize launch reads it
__device__ __forceinline__ void store_tile_partial(double* part, long long r, int tile, int t, const double (&red)[kLogLikSums][256]) {
    if (t < 4) {
        double v = 0.0;
        if (t < kLogLikSums) v = red[t][0];
        part[(r * gridDim.x + tile) * 4 + t] = v;
    }
}

}  // namespace vaek
