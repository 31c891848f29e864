// Hessian of the SAMPLE-AVERAGE ELBO of three-hidden-layer MLP VAEs (vaek_mlp3_sampled_elbo_hvp_replicas, ..._hessian_lanczos_replicas): the f_K of
// sampled_hessian.hip with the two linear maps replaced by the four-Dense relu stacks of networks.py:26-44.  Fix the rows and K latent
// samples per row; f_K(theta) is then a deterministic function, piecewise smooth (relu has no second derivative away from the kink), and
// its gradient and Hessian-vector products are exact derivatives written out by hand: forward over reverse through both stacks
// (include/vaek.h gives the formulas, DESIGN 3.24 the derivation).  Nothing is finite-differenced.  Leaves, rows, samples and directions
// are widened to float64 once and everything below is float64 on v_mfma_f64_16x16x4_f64, so a unit is live iff its FLOAT64
// pre-activation is > 0 (mlp3_jacobian.hip's float32 definition does not apply here).
//
//   CHAIN LAUNCH, grid (tiles, n).  Column q = i K + k of a replica is (row i, sample k).  A workgroup of 256 threads takes kHsCols = 8
//     columns of one replica as a 16-column [unit][column] float64 LDS image: columns 0 .. 7 primal, 8 .. 15 the same columns' tangents,
//     so W . [h | dh] is ONE product pass; dW . [0 | h] is a second pass into the same accumulators whose operand fetch reads column
//     c - 8 and zeroes c < 8.  The backward pass is the same pair on [g | dg] with the kernels read transposed.  Weights stream from L2
//     as float32, directions as float64, widened in registers.  The masks of the six hidden layers stay in LDS as bytes.  The row pitch
//     is 16 doubles: an operand read (ds_read_b64, banks modulo 64 dwords, 32-lane halves) takes two k-rows of 32 dwords each, a
//     result store (16-lane groups, banks modulo 32) one row of 32 dwords -- neither conflicts, so the image needs no swizzle.
//     Per Dense layer the workgroup stores its input image (h, or dh in a tangent launch) and its masked output gradient (g_a, or dg_a)
//     to the workspace as [unit][column pitch], and one row of per-tile partials for the terms that are sums over the columns without a
//     weight matrix (f_K's terms, the epsilon_p and epsilon leaves), one chain per element in column order.  Columns past the replica's
//     last compute on clamped indices with weight 0.
//   CONTRACTION LAUNCH, grid (tiles of every layer's [kernel | bias] + 1, n).  A workgroup owns 16 x 64 elements of one layer's
//     (n_in + 1) x n_out image (the bias is the row of a constant-1 input) and sums h^T g (gradient) or dh^T g + h^T dg (tangent) over
//     ALL the replica's columns in column order on the matrix cores; the last workgroup of a replica adds the tail partials in tile
//     order and the terms no column has.
//   RECORD LAUNCH, n workgroups: |grad f_K|_2 by one fixed tree, the gradient to the caller where asked, the 4-double record.
//
//   LANCZOS (vaek_mlp3_sampled_elbo_hessian_lanczos_replicas).  A length-P vector (P up to 296 545) does not fit a workgroup's LDS and one
//     step's Gram-Schmidt would read ~170 MB through a single CU, so every launch that touches such a vector has grid (chunks of 2048
//     elements, n); dots are per-chunk partials that cross a launch boundary and are added in chunk order by whoever needs them.  Per
//     step: chain, contraction (w = H v_j into the workspace), then four vector launches (dots; Gram-Schmidt pass 1 + the dots of pass 2;
//     pass 2 + |w|^2; alpha, beta, lanczos_dev.h's breakdown rule, v_{j+1} into the caller's basis).  A replica that is done has a flag
//     per later step in its state block and those launches return at once.  Then the chunks' partial Gram matrices of the basis (the
//     header's pair order), and n workgroups that run the header's Ritz tail and record store with omega from the Gram partials.  The
//     start rule, the record layout and the constants are the header's too; the chunked arithmetic is this unit's own.
//
// Nothing stored in a launch is read back in it; there is no atomic, counter, wait or spin.  Launches: 3 + 2 nvec (hvp call), 6 + 6 steps
// (Lanczos call).
#include "lanczos_dev.h"
#include "eval_check.h"

namespace vaek {

constexpr int kHsMaxColumns = 1 << 14;                // n * rows * samples of one call ...
constexpr int kHsReplicaColumnsLog2 = 13;             // ... and rows * samples of one replica, 2^13: caps on the launch length and the workspace
constexpr int kHsCols = 8;                            // columns of a chain tile
constexpr int kHsPitch = 16;                          // doubles between two units of the image: primal | tangent
constexpr int kHsW = 256;                             // widest layer
constexpr int kHsF = 32;                              // widest D / L
constexpr int kHsTail = 40;                           // doubles of a tile's tail partial: [0, L) the epsilon_p sums  [32] the residual sum  [33] the |mu|^2 sum
constexpr int kHsHead = 8;                            // doubles at the head of a replica's workspace block: [0] f_K
constexpr size_t kHsLds = sizeof(double) * 2 * kHsW * kHsPitch;
constexpr int kHsDepth = 8;                            // k-steps of a product whose operands are fetched together (weights come from L2)
constexpr int kHsTileK = 16, kHsTileM = 64;           // a contraction workgroup's tile of [kernel | bias]
constexpr int kHsRecord = kLanczosRecord + 2;         // the Lanczos record, then samples and the two-decoder flag (0 here)
constexpr int kHsChunk = 2048;                        // elements of a length-P vector one workgroup of a vector launch owns: 8 a thread
constexpr int kHsPairs = kLanczosMaxSteps * (kLanczosMaxSteps - 1) / 2;      // 496 pairs of basis rows
constexpr int kHsPairPitch = 512;
constexpr int kHsGramSub = 64;                        // elements of a chunk staged at a time by the Gram launch
// a replica's Lanczos state, in doubles: [1] k  [3] f_K  [4] |grad f_K|  [5] eps, then alpha, beta, and per step j the scale and the done
// flag AS THEY STAND BEFORE step j (one slot a step: a launch never reads what it stores)
constexpr int kHsState = 192, hsAlpha = 32, hsBeta = 64, hsScale = 96, hsDone = 136;

// layers 0 .. 3 the encoder's, 4 .. 7 the decoder's
struct HsNet {
    int n_in[8], n_out[8], w_off[8];
    long long h_off[8], g_off[8], dh_off[8], dg_off[8];      // doubles from the replica's workspace block; [unit][cpitch]
    int tile0[9];                                            // first contraction tile of each layer; [8]: the tail workgroup
};

struct HsArgs {
    const float* params; long long state_stride;
    const unsigned long long* x_seeds; const unsigned* x_steps;
    const unsigned long long* z_seeds; const unsigned* z_steps;
    long long a_stride;
    const float* x; long long x_stride;
    const float* xi; long long xi_stride;
    int rows, samples, D, L, P, off_p, off_c;                // off_c < 0: no epsilon leaf
    float eps_cli;
    unsigned z_tag;
    BatchArgs gen;
    HsNet net;
    double* ws; long long block;                             // replica r's block at ws + r * block
    int tiles, cpitch;                                       // chain tiles of a replica, columns between two units in the workspace
    long long gvec_off, tail_off;
    // the Lanczos call
    long long state_off, wvec_off, dotA_off, dotB_off, nrm_off, gram_off;      // doubles from the replica's block
    int chunks;
    const double* v0; long long v0_stride;
    double* basis; long long basis_stride;
    int steps, j, use_flag;                                  // use_flag: a replica whose state says done before step j is skipped
    const double* dir; long long dir_stride;                 // a tangent launch's direction, [P] per replica
    double* dst; long long dst_stride;                       // where a contraction launch puts its P doubles (NULL: the block's gvec)
    double* grad; long long grad_stride;                     // record launch: the caller's gradient buffer or NULL
    double* out; long long out_stride;
};

__device__ __forceinline__ f64x4 hs_mfma(double a, double b, f64x4 acc) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0); }

// out(m, c) = sum_k W[k][m] in(k, c)  (+ TAN: sum_k dW[k][m] in(k, c - 8) on c >= 8)  + bias: b[m] on c < 8, db[m] on c >= 8; relu
// with the mask of the primal column where RELU, the mask bytes stored by the primal lanes.  Wave w owns unit blocks w, w + 4, ..
template <bool TAN, bool RELU>
__device__ __forceinline__ void hs_forward(const float* __restrict__ W, const double* __restrict__ dW, int n_in, int n_out, const double* in,
                                           double* out, unsigned char* mask, int wave, int lane) {
    const int n = lane & 15, kq = lane >> 4;
    const int nblk = (n_out + 15) >> 4;
    for (int mb = wave; mb < nblk; mb += 4) {
        const int m = min(16 * mb + n, n_out - 1);
        f64x4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < n_in; k0 += 4 * kHsDepth) {               // kHsDepth k-steps' operands in flight; a k past n_in meets a zero
            double av[kHsDepth], bv[kHsDepth];
#pragma unroll
            for (int j = 0; j < kHsDepth; ++j) {
                const int k = k0 + 4 * j + kq;
                const int kk = min(k, n_in - 1);
                const float w = W[(long long)kk * n_out + m];
                av[j] = k < n_in ? (double)w : 0.0;
                bv[j] = in[kk * kHsPitch + n];
            }
#pragma unroll
            for (int j = 0; j < kHsDepth; ++j) acc = hs_mfma(av[j], bv[j], acc);
        }
        if (TAN) {
            for (int k0 = 0; k0 < n_in; k0 += 4 * kHsDepth) {
                double av[kHsDepth], bv[kHsDepth];
#pragma unroll
                for (int j = 0; j < kHsDepth; ++j) {
                    const int k = k0 + 4 * j + kq;
                    const int kk = min(k, n_in - 1);
                    const double w = dW[(long long)kk * n_out + m];
                    av[j] = k < n_in ? w : 0.0;
                    const double b = in[kk * kHsPitch + (n & 7)];
                    bv[j] = n >= 8 ? b : 0.0;
                }
#pragma unroll
                for (int j = 0; j < kHsDepth; ++j) acc = hs_mfma(av[j], bv[j], acc);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int mo = 16 * mb + kq + 4 * r;
            const int mc = min(mo, n_out - 1);
            const double bias = n < 8 ? (double)W[(long long)n_in * n_out + mc] : (TAN ? dW[(long long)n_in * n_out + mc] : 0.0);
            double v = acc[r] + bias;
            if (RELU) {
                const double pv = __shfl(v, lane ^ 8);                 // a tangent lane reads its primal column's pre-activation
                const bool on = (n < 8 ? v : pv) > 0.0;
                v = on ? v : 0.0;
                if (n < 8 && mo < n_out) mask[mo * kHsCols + n] = on ? 1 : 0;
            }
            if (mo < n_out) out[mo * kHsPitch + n] = v;
        }
    }
}

// out(k, c) = sum_m W[k][m] in(m, c)  (+ TAN: sum_m dW[k][m] in(m, c - 8) on c >= 8), masked by the mask of unit k where given
template <bool TAN>
__device__ __forceinline__ void hs_backward(const float* __restrict__ W, const double* __restrict__ dW, int n_in, int n_out, const double* in,
                                            double* out, const unsigned char* mask, int wave, int lane) {
    const int n = lane & 15, kq = lane >> 4;
    const int nblk = (n_in + 15) >> 4;
    for (int kb = wave; kb < nblk; kb += 4) {
        const long long row = (long long)min(16 * kb + n, n_in - 1) * n_out;
        f64x4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int m0 = 0; m0 < n_out; m0 += 4 * kHsDepth) {
            double av[kHsDepth], bv[kHsDepth];
#pragma unroll
            for (int j = 0; j < kHsDepth; ++j) {
                const int m = m0 + 4 * j + kq;
                const int mm = min(m, n_out - 1);
                const float w = W[row + mm];
                av[j] = m < n_out ? (double)w : 0.0;
                bv[j] = in[mm * kHsPitch + n];
            }
#pragma unroll
            for (int j = 0; j < kHsDepth; ++j) acc = hs_mfma(av[j], bv[j], acc);
        }
        if (TAN) {
            for (int m0 = 0; m0 < n_out; m0 += 4 * kHsDepth) {
                double av[kHsDepth], bv[kHsDepth];
#pragma unroll
                for (int j = 0; j < kHsDepth; ++j) {
                    const int m = m0 + 4 * j + kq;
                    const int mm = min(m, n_out - 1);
                    const double w = dW[row + mm];
                    av[j] = m < n_out ? w : 0.0;
                    const double b = in[mm * kHsPitch + (n & 7)];
                    bv[j] = n >= 8 ? b : 0.0;
                }
#pragma unroll
                for (int j = 0; j < kHsDepth; ++j) acc = hs_mfma(av[j], bv[j], acc);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = 16 * kb + kq + 4 * r;
            if (k < n_in) {
                const bool on = mask ? mask[k * kHsCols + (n & 7)] != 0 : true;
                out[k * kHsPitch + n] = on ? acc[r] : 0.0;
            }
        }
    }
}

// the image's primal (TAN false) or tangent (true) columns of `units` units to dst [unit][cpitch] at column col0
template <bool TAN>
__device__ __forceinline__ void hs_store(const double* img, int units, double* dst, int cpitch, int col0, int t) {
    for (int e = t; e < units * kHsCols; e += 256) {
        const int u = e >> 3, c = e & 7;
        dst[(long long)u * cpitch + col0 + c] = img[u * kHsPitch + c + (TAN ? 8 : 0)];
    }
}

// TAN false: the gradient launch (stores h, g_a and the partials of f_K); true: the tangent launch for a.dir (stores dh, dg_a)
template <bool TAN>
__global__ __launch_bounds__(256) void mlp3_hessian_chain_kernel(const HsArgs a) {
    extern __shared__ __attribute__((aligned(16))) double hs_img[];
    __shared__ unsigned char mask[6][kHsW * kHsCols];
    __shared__ float xs[kHsCols][kHsF], xis[kHsCols][kHsF];
    __shared__ double mus[kHsF][kHsPitch], cw0[kHsCols], cw1[kHsCols], red[2][kHsF];
    double* const img0 = hs_img;
    double* const img1 = hs_img + kHsW * kHsPitch;
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int tile = blockIdx.x;
    const long long r = blockIdx.y;
    const int D = a.D, L = a.L;
    const float* const p = a.params + r * a.state_stride;
    const double* const dir = TAN ? a.dir + r * a.dir_stride : nullptr;
    double* const blk = a.ws + r * a.block;
    if (a.use_flag && blk[a.state_off + hsDone + a.j] != 0.0) return;  // uniform: written by an earlier launch
    const int ncols = a.rows * a.samples;
    const int col0 = tile * kHsCols;

    const double eps_cli = (double)a.eps_cli;
    const double eps = a.off_c >= 0 ? (double)p[a.off_c] * eps_cli : eps_cli;
    const double deps = TAN && a.off_c >= 0 ? eps_cli * dir[a.off_c] : 0.0;
    const double c0 = exp(-eps) / (double)ncols, c1 = 1.0 / (double)ncols;

    // ---- the rows and the samples of the tile's columns: thread (column, part) ---------------------------------------------------------
    if (t < kHsCols * 8) {
        const int col = t >> 3, part = t & 7;
        const bool valid = col0 + col < ncols;
        const int q = valid ? col0 + col : ncols - 1;                  // a column past the last: clamped, weight 0
        const int i = q / a.samples, k = q % a.samples;
        if (part == 0) {
            RowCtx rc{};
            rc.D = D; rc.L = L; rc.g = a.gen;
            float x[kSpectrumMaxDim];
            if (a.x) {
                rc.xr = a.x + r * a.x_stride;
                produce_row<SRC_EXPLICIT, kSpectrumMaxDim, 4, false>(rc, i, x);
            } else {
                if (rc.g.A) rc.g.A += r * a.a_stride;
                rc.key = philox_key(a.x_seeds[r]);
                rc.step = a.x_steps[r];
                produce_row<SRC_REAL, kSpectrumMaxDim, 4, false>(rc, i, x);
            }
#pragma unroll
            for (int d = 0; d < kHsF; ++d) xs[col][d] = x[d];
            cw0[col] = valid ? c0 : 0.0;
            cw1[col] = valid ? c1 : 0.0;
        }
        float n4[4] = {0.f, 0.f, 0.f, 0.f};
        if (4 * part < L) {
            if (a.xi) {
                const float* const xi = a.xi + r * a.xi_stride;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (4 * part + e < L) n4[e] = xi[(long long)q * L + 4 * part + e];
            } else {
                BatchArgs gz = a.gen;
                gz.tag = a.z_tag;
                latent_block(gz, a.z_steps[r], i, philox_key(a.z_seeds[r]), k * ((L + 3) >> 2) + part, n4);
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) xis[col][4 * part + e] = 4 * part + e < L ? n4[e] : 0.f;
    }
    __syncthreads();
    for (int e = t; e < D * kHsPitch; e += 256) {
        const int d = e >> 4, c = e & 15;
        img0[e] = c < 8 ? (double)xs[c][d] : 0.0;
    }
    __syncthreads();

    // ---- the encoder, forward: img0 -> img1 -> img0 -> img1 -> img0 ---------------------------------------------------------------------
#pragma unroll 1
    for (int li = 0; li < 4; ++li) {
        const double* const in = (li & 1) ? img1 : img0;
        double* const out = (li & 1) ? img0 : img1;
        const int n_in = a.net.n_in[li], n_out = a.net.n_out[li];
        hs_store<TAN>(in, n_in, blk + (TAN ? a.net.dh_off[li] : a.net.h_off[li]), a.cpitch, col0, t);
        const float* const W = p + a.net.w_off[li];
        const double* const dW = TAN ? dir + a.net.w_off[li] : nullptr;
        if (li < 3) hs_forward<TAN, true>(W, dW, n_in, n_out, in, out, mask[li], wave, lane);
        else hs_forward<TAN, false>(W, dW, n_in, n_out, in, out, nullptr, wave, lane);
        __syncthreads();
    }
    // ---- the head: mu kept, s = mu + sd xi, ds = dmu + dp sd xi / 2 into img0 --------------------------------------------------------------
    for (int e = t; e < L * kHsPitch; e += 256) {
        const int l = e >> 4, c = e & 15;
        const double m = img0[e];
        mus[l][c] = m;
        const double sx = exp(0.5 * (double)p[a.off_p + l]) * (double)xis[c & 7][l];
        img0[e] = c < 8 ? m + sx : (TAN ? m + 0.5 * dir[a.off_p + l] * sx : 0.0);
    }
    __syncthreads();
    // ---- the decoder, forward ------------------------------------------------------------------------------------------------------------------
#pragma unroll 1
    for (int li = 4; li < 8; ++li) {
        const double* const in = (li & 1) ? img1 : img0;
        double* const out = (li & 1) ? img0 : img1;
        const int n_in = a.net.n_in[li], n_out = a.net.n_out[li];
        hs_store<TAN>(in, n_in, blk + (TAN ? a.net.dh_off[li] : a.net.h_off[li]), a.cpitch, col0, t);
        const float* const W = p + a.net.w_off[li];
        const double* const dW = TAN ? dir + a.net.w_off[li] : nullptr;
        if (li < 7) hs_forward<TAN, true>(W, dW, n_in, n_out, in, out, mask[li - 1], wave, lane);
        else hs_forward<TAN, false>(W, dW, n_in, n_out, in, out, nullptr, wave, lane);
        __syncthreads();
    }
    // ---- r = y - x, g_y = c0 r, dg_y = c0 (dy - deps r) into img0; the residual partial: thread d walks its columns in order ------------------
    if (t < D) {
        const int d = t;
        double qs = 0.0;
        for (int c = 0; c < kHsCols; ++c) {
            const double rr = img0[d * kHsPitch + c] - (double)xs[c][d];
            const double dr = TAN ? img0[d * kHsPitch + 8 + c] : 0.0;
            qs += TAN ? cw0[c] * rr * (0.5 * deps * rr - dr) : cw0[c] * rr * rr;
            img0[d * kHsPitch + c] = cw0[c] * rr;
            img0[d * kHsPitch + 8 + c] = TAN ? cw0[c] * (dr - deps * rr) : 0.0;
        }
        red[0][d] = qs;
    }
    __syncthreads();
    // ---- the decoder, backward: g_a of layer li is in the image; stored, then carried to the layer's input ------------------------------------
#pragma unroll 1
    for (int li = 7; li >= 4; --li) {
        const double* const in = (li & 1) ? img0 : img1;               // layer li's output image
        double* const out = (li & 1) ? img1 : img0;
        const int n_in = a.net.n_in[li], n_out = a.net.n_out[li];
        hs_store<TAN>(in, n_out, blk + (TAN ? a.net.dg_off[li] : a.net.g_off[li]), a.cpitch, col0, t);
        const float* const W = p + a.net.w_off[li];
        const double* const dW = TAN ? dir + a.net.w_off[li] : nullptr;
        hs_backward<TAN>(W, dW, n_in, n_out, in, out, li > 4 ? mask[li - 2] : nullptr, wave, lane);
        __syncthreads();
    }
    // ---- g_s is img0's rows [0, L): the epsilon_p partial, the |mu|^2 partial, then g_mu = g_s + c1 mu, dg_mu = dg_s + c1 dmu -------------------
    if (t < L) {
        const int l = t;
        const double sd = exp(0.5 * (double)p[a.off_p + l]);
        const double dp = TAN ? dir[a.off_p + l] : 0.0;
        double ps = 0.0, ms = 0.0;
        for (int c = 0; c < kHsCols; ++c) {
            const double hx = 0.5 * sd * (double)xis[c][l];
            const double gs = img0[l * kHsPitch + c];
            if (TAN) ps += img0[l * kHsPitch + 8 + c] * hx + gs * (0.5 * dp * hx);
            else { ps += gs * hx; ms += cw1[c] * (0.5 * mus[l][c] * mus[l][c]); }
        }
        red[1][l] = ms;
        blk[a.tail_off + (long long)tile * kHsTail + l] = ps;
    }
    __syncthreads();
    if (t == 0) {
        double qs = 0.0, ms = 0.0;
        for (int d = 0; d < D; ++d) qs += red[0][d];
        for (int l = 0; l < L; ++l) ms += red[1][l];
        blk[a.tail_off + (long long)tile * kHsTail + 32] = qs;
        blk[a.tail_off + (long long)tile * kHsTail + 33] = ms;
    }
    for (int e = t; e < L * kHsPitch; e += 256) {
        const int l = e >> 4, c = e & 15;
        if (c < 8 || TAN) img0[e] += cw1[c & 7] * mus[l][c];
    }
    __syncthreads();
    // ---- the encoder, backward; the gradient of the rows is not needed -------------------------------------------------------------------------
#pragma unroll 1
    for (int li = 3; li >= 0; --li) {
        const double* const in = (li & 1) ? img0 : img1;
        double* const out = (li & 1) ? img1 : img0;
        const int n_in = a.net.n_in[li], n_out = a.net.n_out[li];
        hs_store<TAN>(in, n_out, blk + (TAN ? a.net.dg_off[li] : a.net.g_off[li]), a.cpitch, col0, t);
        if (li == 0) break;
        const float* const W = p + a.net.w_off[li];
        const double* const dW = TAN ? dir + a.net.w_off[li] : nullptr;
        hs_backward<TAN>(W, dW, n_in, n_out, in, out, mask[li - 1], wave, lane);
        __syncthreads();
    }
}

// element e of the sum of replica block `blk`'s tail partials, tiles in tile order
__device__ __forceinline__ double hs_tail(const HsArgs& a, const double* blk, int e) {
    const double* const part = blk + a.tail_off + e;
    double s = 0.0;
    for (int tile = 0; tile < a.tiles; ++tile) s += part[(long long)tile * kHsTail];
    return s;
}

// TAN false: the gradient (and f_K into the block's head); true: H v for a.dir
template <bool TAN>
__global__ __launch_bounds__(256) void mlp3_hessian_contract_kernel(const HsArgs a) {
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const long long r = blockIdx.y;
    double* const blk = a.ws + r * a.block;
    if (a.use_flag && blk[a.state_off + hsDone + a.j] != 0.0) return;
    double* const dst = a.dst ? a.dst + r * a.dst_stride : blk + (a.use_flag ? a.wvec_off : a.gvec_off);
    const int b = blockIdx.x;
    if (b == a.net.tile0[8]) {
        // ---- the leaves no layer owns and f_K --------------------------------------------------------------------------------------------------
        const float* const p = a.params + r * a.state_stride;
        const double* const dir = TAN ? a.dir + r * a.dir_stride : nullptr;
        const double eps_cli = (double)a.eps_cli;
        if (t < a.L) {
            const double w = exp((double)p[a.off_p + t]);
            dst[a.off_p + t] = hs_tail(a, blk, t) + (TAN ? 0.5 * w * dir[a.off_p + t] : 0.5 * (w - 1.0));
        } else if (t == 32) {
            const double qs = hs_tail(a, blk, 32);
            if (a.off_c >= 0) dst[a.off_c] = TAN ? eps_cli * qs : eps_cli * (0.5 * (double)a.D - 0.5 * qs);
        } else if (t == 33 && !TAN) {
            const double eps = a.off_c >= 0 ? (double)p[a.off_c] * eps_cli : eps_cli;
            double klc = 0.0;
            for (int l = 0; l < a.L; ++l) { const double pl = (double)p[a.off_p + l]; klc += exp(pl) - 1.0 - pl; }
            blk[0] = hs_tail(a, blk, 33) + 0.5 * hs_tail(a, blk, 32) + 0.5 * klc + 0.5 * (double)a.D * (eps + kLog2PiF64);
        }
        return;
    }
    int li = 0;
    while (b >= a.net.tile0[li + 1]) ++li;                             // uniform
    const int n_in = a.net.n_in[li], n_out = a.net.n_out[li];
    const int mt = (n_out + kHsTileM - 1) / kHsTileM;
    const int local = b - a.net.tile0[li];
    const int k0 = (local / mt) * kHsTileK, m0 = (local % mt) * kHsTileM + 16 * wave;
    if (m0 >= n_out) return;                                           // a wave past the layer's last unit block
    const int n = lane & 15, kq = lane >> 4;
    const int k = k0 + n;                                              // this lane's row of [kernel | bias] as the A operand
    const bool bias_row = k == n_in;
    const int kc = min(k, n_in - 1), mc = min(m0 + n, n_out - 1);
    const double* const H = blk + a.net.h_off[li] + (long long)kc * a.cpitch + kq;
    const double* const G = blk + a.net.g_off[li] + (long long)mc * a.cpitch + kq;
    const double* const DH = blk + a.net.dh_off[li] + (long long)kc * a.cpitch + kq;
    const double* const DG = blk + a.net.dg_off[li] + (long long)mc * a.cpitch + kq;
    const int ncp = a.cpitch;                                          // every column the chain launch stored: a multiple of 8
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int q = 0; q < ncp; q += 4 * kHsDepth) {                      // kHsDepth k-steps' operands in flight; a step past the last column adds 0
        double h[kHsDepth], g[kHsDepth], dh[kHsDepth], dg[kHsDepth];
#pragma unroll
        for (int j = 0; j < kHsDepth; ++j) {
            const bool live = q + 4 * j < ncp;
            const int qq = live ? q + 4 * j : 0;
            h[j] = live ? H[qq] : 0.0; g[j] = live ? G[qq] : 0.0;
            if (TAN) { dh[j] = live ? DH[qq] : 0.0; dg[j] = live ? DG[qq] : 0.0; }
        }
#pragma unroll
        for (int j = 0; j < kHsDepth; ++j) {
            if (TAN) {
                acc = hs_mfma(bias_row ? 0.0 : dh[j], g[j], acc);
                acc = hs_mfma(bias_row ? (q + 4 * j < ncp ? 1.0 : 0.0) : h[j], dg[j], acc);
            } else {
                acc = hs_mfma(bias_row ? (q + 4 * j < ncp ? 1.0 : 0.0) : h[j], g[j], acc);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int ko = k0 + kq + 4 * q, mo = m0 + n;
        if (ko <= n_in && mo < n_out) dst[a.net.w_off[li] + (long long)ko * n_out + mo] = acc[q];
    }
}

// |grad f_K|_2 by one workgroup: thread t the elements t + 256 i in order, then the fixed tree (one text for both calls' records)
__device__ __forceinline__ double hs_grad_norm(const double* g, int P, double* red, int t) {
    double part = 0.0;
    for (int e = t; e < P; e += 256) part = fma(g[e], g[e], part);
    return sqrt(block_sum256(part, red, t));
}

// one workgroup per replica: |grad f_K|_2, the gradient to the caller where asked, the 4-double record
__global__ __launch_bounds__(256) void mlp3_hessian_record_kernel(const HsArgs a) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    const long long r = blockIdx.x;
    const double* const blk = a.ws + r * a.block;
    const double* const g = blk + a.gvec_off;
    double* const grad = a.grad ? a.grad + r * a.grad_stride : nullptr;
    if (grad)
        for (int e = t; e < a.P; e += 256) grad[e] = g[e];
    const double gnorm = hs_grad_norm(g, a.P, red, t);
    if (t < kHvpRecord) {
        const float* const p = a.params + r * a.state_stride;
        const double eps_cli = (double)a.eps_cli;
        const double eps = a.off_c >= 0 ? (double)p[a.off_c] * eps_cli : eps_cli;
        a.out[r * a.out_stride + t] = t == 0 ? blk[0] : (t == 1 ? gnorm : (t == 2 ? eps : (double)a.rows));
    }
}

// ---- Lanczos across launches, the vector work spread over P: every launch below that touches a length-P vector has grid (chunks, n), a
// workgroup owning kHsChunk elements (thread t the eight elements chunk * kHsChunk + t + 256 i).  A dot is a per-chunk partial (one fixed
// tree over the workgroup) that crosses a launch boundary and is added in chunk order by every workgroup that needs it.
__device__ __forceinline__ double hs_chunk_sum(const double* part, int chunks, int pitch) {
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += part[(long long)c * pitch];
    return s;
}

// before step 1, first launch: the chunk's partial of |v0|^2
__global__ __launch_bounds__(256) void mlp3_hessian_init_dots_kernel(const HsArgs a) {
    __shared__ double red[256];
    const int t = threadIdx.x, chunk = blockIdx.x;
    const long long r = blockIdx.y;
    double* const blk = a.ws + r * a.block;
    const double* const v0 = a.v0 + r * a.v0_stride;
    double pv = 0.0;
#pragma unroll
    for (int i = 0; i < kHsChunk / 256; ++i) {
        const int e = chunk * kHsChunk + t + 256 * i;
        if (e < a.P) pv = fma(v0[e], v0[e], pv);
    }
    pv = block_sum256(pv, red, t);
    if (t == 0) blk[a.dotA_off + chunk * kLanczosMaxSteps] = pv;
}

// second launch: v_1 = v0 / |v0| into the basis; chunk 0 writes the state block
__global__ __launch_bounds__(256) void mlp3_hessian_init_kernel(const HsArgs a) {
    __shared__ double red[256];
    const int t = threadIdx.x, chunk = blockIdx.x;
    const long long r = blockIdx.y;
    double* const blk = a.ws + r * a.block;
    double* const state = blk + a.state_off;
    const double n0 = sqrt(hs_chunk_sum(blk + a.dotA_off, a.chunks, kLanczosMaxSteps));
    const int kmax = lanczos_kmax(n0, a.steps, a.P);
    if (kmax > 0) {
        double* const basis = a.basis + r * a.basis_stride;
        const double* const v0 = a.v0 + r * a.v0_stride;
#pragma unroll
        for (int i = 0; i < kHsChunk / 256; ++i) {
            const int e = chunk * kHsChunk + t + 256 * i;
            if (e < a.P) basis[e] = v0[e] / n0;
        }
    }
    if (chunk != 0) return;                                            // uniform
    const double gnorm = hs_grad_norm(blk + a.gvec_off, a.P, red, t);
    if (t < kHsState) {
        double v = 0.0;
        if (t == 3) v = blk[0];
        else if (t == 4) v = gnorm;
        else if (t == 5) {
            const double eps_cli = (double)a.eps_cli;
            v = a.off_c >= 0 ? (double)a.params[r * a.state_stride + a.off_c] * eps_cli : eps_cli;
        } else if (t >= hsDone && t <= hsDone + kLanczosMaxSteps) v = kmax > 0 ? 0.0 : 1.0;
        state[t] = v;
    }
}

// step j + 1 of a replica that is not done, in four launches.  w = H v_{j+1} lies in the block's wvec (the contraction launch).
//   MODE 0  dotA[chunk][i] = v_i . w over the chunk, i <= j
//   MODE 1  coef_i = sum of dotA over the chunks;  w -= sum_i coef_i v_i;  dotB[chunk][i] = v_i . w          (classical Gram-Schmidt ...
//   MODE 2  coef_i = sum of dotB;  w -= sum_i coef_i v_i;  nrm[chunk] = |w|^2                                   ... twice)
//   MODE 3  alpha = coef_j of both passes, beta = |w|, the breakdown test, v_{j+2} = w / beta; chunk 0 writes the state
template <int MODE>
__global__ __launch_bounds__(256) void mlp3_hessian_lanczos_kernel(const HsArgs a) {
    __shared__ double red[256], coef[kLanczosMaxSteps];
    const int t = threadIdx.x, chunk = blockIdx.x, j = a.j;
    const long long r = blockIdx.y;
    double* const blk = a.ws + r * a.block;
    double* const state = blk + a.state_off;
    if (state[hsDone + j] != 0.0) return;                              // uniform; this launch stores hsDone + j + 1 .. only
    const int P = a.P;
    double* const basis = a.basis + r * a.basis_stride;
    double* const w = blk + a.wvec_off;
    double* const dotA = blk + a.dotA_off;
    double* const dotB = blk + a.dotB_off;
    double we[kHsChunk / 256];
    int ei[kHsChunk / 256];
#pragma unroll
    for (int i = 0; i < kHsChunk / 256; ++i) {
        const int e = chunk * kHsChunk + t + 256 * i;
        ei[i] = e < P ? e : -1;
        we[i] = e < P ? w[e] : 0.0;
    }
    if (MODE == 1 || MODE == 2) {
        if (t <= j) coef[t] = hs_chunk_sum((MODE == 1 ? dotA : dotB) + t, a.chunks, kLanczosMaxSteps);
        __syncthreads();
        for (int i = 0; i <= j; ++i) {
            const double* const vi = basis + (long long)i * P;
            const double ci = coef[i];
#pragma unroll
            for (int q = 0; q < kHsChunk / 256; ++q)
                if (ei[q] >= 0) we[q] = fma(-ci, vi[ei[q]], we[q]);
        }
#pragma unroll
        for (int q = 0; q < kHsChunk / 256; ++q)
            if (ei[q] >= 0) w[ei[q]] = we[q];
    }
    if (MODE == 0 || MODE == 1) {
        double* const out = (MODE == 0 ? dotA : dotB) + chunk * kLanczosMaxSteps;
        for (int i = 0; i <= j; ++i) {
            const double* const vi = basis + (long long)i * P;
            double d = 0.0;
#pragma unroll
            for (int q = 0; q < kHsChunk / 256; ++q)
                if (ei[q] >= 0) d = fma(vi[ei[q]], we[q], d);
            d = block_sum256(d, red, t);
            if (t == 0) out[i] = d;
        }
    }
    if (MODE == 2) {
        double d = 0.0;
#pragma unroll
        for (int q = 0; q < kHsChunk / 256; ++q) d = fma(we[q], we[q], d);
        d = block_sum256(d, red, t);
        if (t == 0) blk[a.nrm_off + chunk] = d;
    }
    if (MODE == 3) {
        const double al = hs_chunk_sum(dotA + j, a.chunks, kLanczosMaxSteps) + hs_chunk_sum(dotB + j, a.chunks, kLanczosMaxSteps);
        const double be = sqrt(hs_chunk_sum(blk + a.nrm_off, a.chunks, 1));
        const int k = j + 1, kmax = a.steps < P ? a.steps : P;
        double scale = state[hsScale + j];
        const bool stop = lanczos_stop(al, be, k, kmax, scale);        // the same values in every thread of every chunk
        if (!stop) {
            double* const vn = basis + (long long)k * P;
#pragma unroll
            for (int q = 0; q < kHsChunk / 256; ++q)
                if (ei[q] >= 0) vn[ei[q]] = we[q] / be;
        }
        if (chunk == 0) {
            if (t == 0) { state[hsAlpha + j] = al; state[hsBeta + j] = be; state[1] = (double)k; state[hsScale + k] = scale; }
            if (stop && t > j && t <= kLanczosMaxSteps) state[hsDone + t] = 1.0;
        }
    }
}

// after the last step: the chunk's partial of v_i . v_j for every pair i < j < k, kHsGramSub elements staged at a time
__global__ __launch_bounds__(256) void mlp3_hessian_gram_kernel(const HsArgs a) {
    __shared__ double tile[kLanczosMaxSteps][kHsGramSub + 1];
    const int t = threadIdx.x, chunk = blockIdx.x;
    const long long r = blockIdx.y;
    double* const blk = a.ws + r * a.block;
    const int k = (int)blk[a.state_off + 1];
    const double* const basis = a.basis + r * a.basis_stride;
    int pi[2], pj[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        lanczos_pair(t + 256 * h, pi[h], pj[h]);
    }
    double acc[2] = {0.0, 0.0};
    for (int s0 = 0; s0 < kHsChunk; s0 += kHsGramSub) {
        for (int idx = t; idx < kLanczosMaxSteps * kHsGramSub; idx += 256) {
            const int row = idx / kHsGramSub, c = idx % kHsGramSub;
            const int e = chunk * kHsChunk + s0 + c;
            tile[row][c] = row < k && e < a.P ? basis[(long long)row * a.P + e] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (pj[h] < k) {
                double s = acc[h];
                for (int c = 0; c < kHsGramSub; ++c) s = fma(tile[pi[h]][c], tile[pj[h]][c], s);
                acc[h] = s;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int h = 0; h < 2; ++h)
        if (t + 256 * h < kHsPairs) blk[a.gram_off + (long long)chunk * kHsPairPitch + t + 256 * h] = acc[h];
}

// the last launch, n workgroups: T from the state block, then lanczos_dev.h's tail with omega from the Gram partials in chunk order
__global__ __launch_bounds__(256) void mlp3_hessian_final_kernel(const HsArgs a) {
    __shared__ double mat[2 * kMatDoubles], vecs[2 * kMatDoubles];
    __shared__ double red[256], alpha[kSpectrumMaxDim], beta[kSpectrumMaxDim], rot_c[kSpectrumMaxDim], rot_s[kSpectrumMaxDim], eig[kSpectrumMaxDim];
    __shared__ int rot_mate[kSpectrumMaxDim];
    const int t = threadIdx.x;
    const long long r = blockIdx.x;
    const double* const blk = a.ws + r * a.block;
    const double* const state = blk + a.state_off;
    double* const out = a.out + r * a.out_stride;
    const int k = (int)state[1];
    if (t < k) { alpha[t] = state[hsAlpha + t]; beta[t] = state[hsBeta + t]; }
    __syncthreads();
    LanczosLds s;
    s.mat = mat; s.vec = vecs; s.red = red; s.alpha = alpha; s.beta = beta;
    s.rot_c = rot_c; s.rot_s = rot_s; s.eig = eig; s.rot_mate = rot_mate;
    const RitzResult rz = lanczos_ritz(s, k, out, t);
    // omega = max_{i < j < k} |v_i . v_j|: thread t the pairs t and t + 256 of lanczos_pair's order, the chunks' partials in chunk order
    double wmax = 0.0;
    for (int q = t; q < k * (k - 1) / 2; q += 256) wmax = fmax(wmax, fabs(hs_chunk_sum(blk + a.gram_off + q, a.chunks, kHsPairPitch)));
    const double omega = block_max256(wmax, red, t);
    lanczos_head_store(out, t, k, state[3], state[4], state[5], a.rows, omega, rz);
    if (t == 12) out[kHsRecord - 2] = (double)a.samples;
    if (t == 13) out[kHsRecord - 1] = 0.0;
}

// ---- host side --------------------------------------------------------------------------------------------------------------------------
// the leaf layout the kernels index by: the eight Dense layers in order, then epsilon_p and, under tunable_eps, epsilon
static bool hs_layout(const vaek_ctx* c) {
    if (!c->mlp3_loglik) return false;
    int64_t off = 0;
    for (int i = 0; i < 8; ++i) {
        const Layer& l = i < 4 ? c->enc.layers[i] : c->dec.layers[i - 4];
        if (l.w_off != off) return false;
        off += (int64_t)(l.n_in + 1) * l.n_out;
    }
    return c->off_epsp == off && (c->off_eps < 0 || c->off_eps == off + c->L) && c->P == off + c->L + (c->off_eps >= 0 ? 1 : 0);
}

static int hs_tiles(int rows, int samples) { return (rows * samples + kHsCols - 1) / kHsCols; }

// the workspace of one replica, in doubles: head, the gradient, the tail partials, the Lanczos state, w, the dot / norm / Gram partials
// of the chunks, then per layer h, g_a, dh, dg_a as [unit][cpitch]
static long long hs_plan(const vaek_ctx* c, int rows, int samples, HsArgs* a) {
    const int tiles = hs_tiles(rows, samples), cpitch = tiles * kHsCols;
    long long off = kHsHead;
    const long long gvec = off;
    off += (c->P + 1) & ~(int64_t)1;
    const long long tail = off;
    off += (long long)tiles * kHsTail;
    const int chunks = (int)((c->P + kHsChunk - 1) / kHsChunk);
    const long long state = off, wvec = state + kHsState, dotA = wvec + ((c->P + 1) & ~(int64_t)1), dotB = dotA + (long long)chunks * kLanczosMaxSteps,
                    nrm = dotB + (long long)chunks * kLanczosMaxSteps, gram = nrm + ((chunks + 1) & ~1);
    off = gram + (long long)chunks * kHsPairPitch;
    int tile = 0;
    for (int i = 0; i < 8; ++i) {
        const Layer& l = i < 4 ? c->enc.layers[i] : c->dec.layers[i - 4];
        if (a) {
            a->net.n_in[i] = l.n_in; a->net.n_out[i] = l.n_out; a->net.w_off[i] = (int)l.w_off;
            a->net.h_off[i] = off; a->net.g_off[i] = off + (long long)l.n_in * cpitch;
            a->net.dh_off[i] = off + (long long)(l.n_in + l.n_out) * cpitch; a->net.dg_off[i] = off + (long long)(2 * l.n_in + l.n_out) * cpitch;
            a->net.tile0[i] = tile;
        }
        tile += ((l.n_in + 1 + kHsTileK - 1) / kHsTileK) * ((l.n_out + kHsTileM - 1) / kHsTileM);
        off += 2LL * (l.n_in + l.n_out) * cpitch;
    }
    if (a) {
        a->net.tile0[8] = tile; a->tiles = tiles; a->cpitch = cpitch; a->gvec_off = gvec; a->tail_off = tail; a->block = off;
        a->state_off = state; a->wvec_off = wvec; a->dotA_off = dotA; a->dotB_off = dotB; a->nrm_off = nrm; a->gram_off = gram; a->chunks = chunks;
    }
    return off;
}

static int hs_check_size(const char* who, int32_t n, int32_t rows, int32_t samples) {
    return check_sampled_columns(who, n, rows, samples, kHsReplicaColumnsLog2, kHsMaxColumns, "vaek_mlp3_sampled_elbo_hessian_max_columns");
}

static int hs_common(const char* who, const EvalDesc& d, const SampleSource& x, int record, const char* record_query, vaek_ctx* ctx, const float* params,
                     int32_t kind, const float* A, int32_t dd, int32_t did, int32_t pad, float var_added, uint32_t x_tag, uint32_t z_tag,
                     void* workspace, HsArgs* a) {
    char needs[256];
    snprintf(needs, sizeof(needs), "needs a float32 VAE with one decoder and three hidden layers of 64 .. %d units both ways, D, L <= %d (see "
             "vaek_supports_mlp3_sampled_elbo_hessian)", kHsW, kHsF);
    EvalRules r{};
    r.covered = ctx && hs_layout(ctx); r.needs = needs;
    r.rows_min = 1; r.rows_cap = kLogLikMaxRows; r.rows_query = "vaek_log_likelihood_max_rows";
    r.records = 1; r.record_len = record; r.record_query = record_query;
    r.draws = true; r.kind = kind; r.A = A; r.dd = dd; r.did = did; r.pad = pad; r.x_tag = x_tag;
    r.has_z_tag = true; r.z_tag = z_tag;
    r.workspace = workspace; r.ws_align = 16; r.ws_query = "vaek_mlp3_sampled_elbo_hessian_workspace_bytes";
    if (int rc = check_eval(who, ctx, params, d, r)) return rc;
    if (int rc = hs_check_size(who, d.n, d.rows, x.samples)) return rc;
    if (int rc = check_sample_source(who, x, d.rows, ctx->L)) return rc;
    a->params = params; a->state_stride = d.state_stride;
    a->x_seeds = reinterpret_cast<const unsigned long long*>(d.x_seeds); a->x_steps = d.x_steps;
    a->z_seeds = reinterpret_cast<const unsigned long long*>(x.z_seeds); a->z_steps = x.z_steps;
    a->x = d.rows_ptr; a->x_stride = d.rows_stride;
    a->xi = x.xi; a->xi_stride = x.xi_stride;
    a->rows = d.rows; a->samples = x.samples; a->D = ctx->D; a->L = ctx->L; a->P = (int)ctx->P;
    a->off_p = (int)ctx->off_epsp; a->off_c = (int)ctx->off_eps;
    a->eps_cli = ctx->cfg.eps_cli; a->z_tag = z_tag;
    a->ws = static_cast<double*>(workspace);
    hs_plan(ctx, d.rows, x.samples, a);
    fill_rows_source(&a->gen, &a->a_stride, ctx, d.rows, d.explicit_rows(), kind, A, dd, did, pad, var_added, x_tag, d.a_stride);
    return VAEK_OK;
}

template <bool TAN>
static int hs_launch_pair(const char* chain_label, const char* contract_label, const HsArgs& a, int n, hipStream_t st) {
    static thread_local PerDeviceOnce attr_set;
    VAEK_HIP_CHECK(set_max_dynamic_lds(attr_set, mlp3_hessian_chain_kernel<TAN>, kHsLds));
    {
        ProfScope ps(chain_label, st);
        launch_k(ps, mlp3_hessian_chain_kernel<TAN>, dim3((unsigned)a.tiles, (unsigned)n), dim3(256), kHsLds, st, a);
    }
    VAEK_HIP_CHECK(hipGetLastError());
    {
        ProfScope ps(contract_label, st);
        launch_k(ps, mlp3_hessian_contract_kernel<TAN>, dim3((unsigned)(a.net.tile0[8] + 1), (unsigned)n), dim3(256), 0, st, a);
    }
    VAEK_HIP_CHECK(hipGetLastError());
    return VAEK_OK;
}

template <class Kernel>
static int hs_launch(hipStream_t st, const char* label, Kernel fn, dim3 grid, const HsArgs& a) {
    {
        ProfScope ps(label, st);
        launch_k(ps, fn, grid, dim3(256), 0, st, a);
    }
    VAEK_HIP_CHECK(hipGetLastError());
    return VAEK_OK;
}

}  // namespace vaek

using namespace vaek;

extern "C" {

int vaek_supports_mlp3_sampled_elbo_hessian(const vaek_ctx* ctx, int32_t kind, int32_t* yes) {
    if (!ctx || !yes) { set_error("vaek_supports_mlp3_sampled_elbo_hessian: null argument"); return VAEK_ERR_INVALID; }
    *yes = kind >= 0 && kind <= 2 && hs_layout(ctx) ? 1 : 0;
    return VAEK_OK;
}

int vaek_mlp3_sampled_elbo_hessian_max_columns(void) { return kHsMaxColumns; }

int vaek_mlp3_sampled_elbo_hessian_workspace_bytes(const vaek_ctx* ctx, int32_t n, int32_t rows, int32_t samples, size_t* bytes) {
    const char* who = "vaek_mlp3_sampled_elbo_hessian_workspace_bytes";
    if (!ctx || !bytes) { set_error("%s: null argument", who); return VAEK_ERR_INVALID; }
    if (int rc = check_replica_count(who, n)) return rc;
    if (int rc = check_row_count(who, rows, 1, kLogLikMaxRows, "vaek_log_likelihood_max_rows")) return rc;
    if (int rc = hs_check_size(who, n, rows, samples)) return rc;
    if (!hs_layout(ctx)) {
        set_error("%s: an unsupported context (see vaek_supports_mlp3_sampled_elbo_hessian)", who);
        return VAEK_ERR_INVALID;
    }
    *bytes = sizeof(double) * (size_t)n * (size_t)hs_plan(ctx, rows, samples, nullptr);
    return VAEK_OK;
}

int vaek_mlp3_sampled_elbo_hvp_replicas(vaek_ctx* ctx, const float* params, const vaek_sampled_elbo_hvp* hp, int32_t kind, const float* A,
                                        int32_t dd, int32_t did, int32_t pad, float var_added, uint32_t x_tag, uint32_t z_tag, void* workspace,
                                        void* stream) {
    const char* who = "vaek_mlp3_sampled_elbo_hvp_replicas";
    ProfBind pb(ctx);
    HsArgs a{};
    const EvalDesc d = describe(hp);
    if (int rc = hs_common(who, d, sample_source(d, hp), kHvpRecord, "vaek_elbo_hvp_record_len", ctx, params, kind, A, dd, did, pad, var_added,
                           x_tag, z_tag, workspace, &a))
        return rc;
    if (int rc = check_hvp_buffers(who, hp, ctx->P, true)) return rc;
    const int64_t P = ctx->P;
    const int n = hp->n;
    hipStream_t st = (hipStream_t)stream;
    a.out = hp->out; a.out_stride = hp->out_stride;
    a.grad = hp->grad; a.grad_stride = hp->grad_stride;
    if (int rc = hs_launch_pair<false>("mlp3_hessian_grad_chain", "mlp3_hessian_grad_contract", a, n, st)) return rc;
    if (int rc = hs_launch(st, "mlp3_hessian_record", mlp3_hessian_record_kernel, dim3((unsigned)n), a)) return rc;
    for (int i = 0; i < hp->nvec; ++i) {
        a.dir = hp->v + (int64_t)i * P; a.dir_stride = hp->v_stride;
        a.dst = hp->hv + (int64_t)i * P; a.dst_stride = hp->hv_stride;
        if (int rc = hs_launch_pair<true>("mlp3_hessian_hvp_chain", "mlp3_hessian_hvp_contract", a, n, st)) return rc;
    }
    return VAEK_OK;
}

int vaek_mlp3_sampled_elbo_hessian_lanczos_replicas(vaek_ctx* ctx, const float* params, const vaek_sampled_elbo_hessian* hs, int32_t kind,
                                                    const float* A, int32_t dd, int32_t did, int32_t pad, float var_added, uint32_t x_tag,
                                                    uint32_t z_tag, void* workspace, void* stream) {
    const char* who = "vaek_mlp3_sampled_elbo_hessian_lanczos_replicas";
    ProfBind pb(ctx);
    HsArgs a{};
    const EvalDesc d = describe(hs);
    if (int rc = hs_common(who, d, sample_source(d, hs), kHsRecord, "vaek_sampled_elbo_hessian_record_len", ctx, params, kind, A, dd, did, pad,
                           var_added, x_tag, z_tag, workspace, &a))
        return rc;
    if (int rc = check_lanczos_buffers(who, hs, ctx->P)) return rc;
    const int64_t P = ctx->P;
    const int n = hs->n;
    hipStream_t st = (hipStream_t)stream;
    a.out = hs->out; a.out_stride = hs->out_stride;
    a.v0 = hs->v0; a.v0_stride = hs->v0_stride; a.basis = hs->basis; a.basis_stride = hs->basis_stride; a.steps = hs->steps;
    const dim3 vgrid((unsigned)a.chunks, (unsigned)n);
    if (int rc = hs_launch_pair<false>("mlp3_hessian_grad_chain", "mlp3_hessian_grad_contract", a, n, st)) return rc;
    if (int rc = hs_launch(st, "mlp3_hessian_init_dots", mlp3_hessian_init_dots_kernel, vgrid, a)) return rc;
    if (int rc = hs_launch(st, "mlp3_hessian_init", mlp3_hessian_init_kernel, vgrid, a)) return rc;
    a.use_flag = 1;
    for (int j = 0; j < hs->steps; ++j) {
        a.j = j;
        a.dir = hs->basis + (int64_t)j * P; a.dir_stride = hs->basis_stride;
        if (int rc = hs_launch_pair<true>("mlp3_hessian_hvp_chain", "mlp3_hessian_hvp_contract", a, n, st)) return rc;
        if (int rc = hs_launch(st, "mlp3_hessian_lanczos_dots", mlp3_hessian_lanczos_kernel<0>, vgrid, a)) return rc;
        if (int rc = hs_launch(st, "mlp3_hessian_lanczos_gs1", mlp3_hessian_lanczos_kernel<1>, vgrid, a)) return rc;
        if (int rc = hs_launch(st, "mlp3_hessian_lanczos_gs2", mlp3_hessian_lanczos_kernel<2>, vgrid, a)) return rc;
        if (int rc = hs_launch(st, "mlp3_hessian_lanczos_next", mlp3_hessian_lanczos_kernel<3>, vgrid, a)) return rc;
    }
    if (int rc = hs_launch(st, "mlp3_hessian_gram", mlp3_hessian_gram_kernel, vgrid, a)) return rc;
    return hs_launch(st, "mlp3_hessian_final", mlp3_hessian_final_kernel, dim3((unsigned)n), a);
}

}  // extern "C"
