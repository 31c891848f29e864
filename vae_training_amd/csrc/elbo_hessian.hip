// Hessian of the exact ELBO of one-decoder linear VAEs (vaek_elbo_hvp_replicas, vaek_elbo_hessian_lanczos_replicas): Hessian-vector
// products and a Lanczos spectrum of f(theta) = -mean_x ELBO(x), the closed form vaek_exact_log_likelihood_replicas evaluates.  f
// depends on the rows through S = (1 / rows) sum [x; 1][x; 1]^T alone, so the gradient and a product H v are a handful of float64
// products of matrices of at most 33 x 32, whatever the number of rows; H never exists as a matrix.  ONE workgroup of 256 threads per
// replica, no cross-workgroup state (include/vaek.h gives the formulas; DESIGN 3.21 the derivation and the measurements).
//
//   MOMENTS.  cov_spectrum.hip's accumulation restated: the rows staged 256 at a time as an LDS tile through produce_row (SRC_EXPLICIT
//     or SRC_REAL, thread t row 256 j + t), sum x x^T and sum x on v_mfma_f64_16x16x4_f64 with k over the rows.  Every element is ONE
//     chain over the rows in row order: the record depends on the rows' bits only.
//   IMAGES.  S, U = [E; b_e], K, R = U K + C, SR = S R and a direction's dU, dK, dR, dG: float64, rows of kIm = 33 doubles (the odd
//     stride lets a wave read a column of K or dK without a bank conflict).  The "ones" row of U, R, ... is row D, not row 32.
//   HVP.  Plain float64 fmas on the 256 threads, three phases with a barrier between them; thread t owns elements t, t + 256, ... of a
//     phase's output and every sum runs in index order.  The one reduction across threads (tr(SR^T dR) for the epsilon row) is
//     block_sum256's fixed tree.
//   LANCZOS.  lanczos_dev.h's recursion, the whole of it in this launch: full reorthogonalisation (classical Gram-Schmidt twice against
//     every earlier vector, each dot through block_sum256), the breakdown rule, the Ritz tail, omega and the record.  The basis lives in
//     the caller's buffer ([steps][P] doubles per replica) and is read back by the workgroup that stored it, behind a barrier; the vector
//     being built lives in LDS.  T goes into the Jacobi buffers (over the dead direction images).
//
// The kernels read rows / parameters / directions and store only the named outputs, with per-lane vector stores.
#include "lanczos_dev.h"
#include "eval_check.h"

namespace vaek {

constexpr int kIm = 33;                      // doubles between two rows of an image
constexpr int kImg = kIm * kIm;
constexpr int kFlat = 2176;                  // >= P at D = L = 32 with epsilon: 2 * 1024 + 3 * 32 + 1 = 2145
// the pool, in doubles: five standing images, four of the direction, the flat vector being built
constexpr int oS = 0, oU = kImg, oK = 2 * kImg, oR = 3 * kImg, oSR = 4 * kImg, oDU = 5 * kImg, oDK = 6 * kImg, oDR = 7 * kImg,
              oDG = 8 * kImg, oW = 9 * kImg, kPoolDoubles = oW + kFlat;
constexpr size_t kHessLds = sizeof(double) * kPoolDoubles;
static_assert(oDK % 2 == 0, "the row tile is stored 16 bytes at a time");
static_assert(oDK * 2 + 256 * kTileStride <= kPoolDoubles * 2, "the row tile lies over the direction images and the flat vector");
static_assert(oDU + 4 * kMatDoubles <= oW, "the Jacobi buffers lie over the direction images");
static_assert(oDU + kMatDoubles <= oDK, "the second moments wait in front of the tile");

struct HessArgs {
    const float* params; long long state_stride;
    const unsigned long long* x_seeds; const unsigned* x_steps;      // [n]: the rows' Philox key and step (drawing mode)
    long long a_stride;
    const float* x; long long x_stride;                              // explicit rows [rows][D] per replica, or NULL: drawing mode
    double* out; long long out_stride;
    int rows, D, L, P, off_p, off_c;                                 // off_c < 0: no epsilon leaf
    float eps_cli;
    // vaek_elbo_hvp_replicas
    const double* v; long long v_stride;
    double* hv; long long hv_stride;
    double* grad; long long grad_stride;
    int nvec;
    // vaek_elbo_hessian_lanczos_replicas
    const double* v0; long long v0_stride;
    double* basis; long long basis_stride;
    int steps;
    BatchArgs gen;                 // kind, A, dd, did, pad, noise_std, tag = x_tag, D, L; seed / step / pointers are not used
};

// what a product H v reads besides the direction: the standing images and the per-latent tables
struct HessModel {
    double *S, *U, *K, *SR, *dU, *dK, *dR, *dG;
    double *wl, *k2, *dw, *kdk, *dbd, *red, *pub;
    int D, L, P, off_wd, off_bd, off_p, off_c;
    double a, Q, eps_cli;
};

// hout <- H vin, both flat [P] in the leaf order (global or LDS).  Called by all 256 threads; ends with a barrier.
__device__ __forceinline__ void hess_hvp(const HessModel& m, const double* const vin, double* const hout, const int t) {
    const int D = m.D, L = m.L;
    // ---- the direction into its images: dU = [dE; db_e], dK, db_d, dw = w dp, deps = eps_cli dc ----------------------------------------
    for (int e = t; e < m.P; e += 256) {
        const double x = vin[e];
        if (e < m.off_wd) m.dU[(e / L) * kIm + e % L] = x;
        else if (e < m.off_bd) { const int q = e - m.off_wd; m.dK[(q / D) * kIm + q % D] = x; }
        else if (e < m.off_p) m.dbd[e - m.off_bd] = x;
        else if (e < m.off_p + L) m.dw[e - m.off_p] = m.wl[e - m.off_p] * x;
        else m.pub[0] = m.eps_cli * x;
    }
    if (m.off_c < 0 && t == 0) m.pub[0] = 0.0;
    __syncthreads();
    const double deps = m.pub[0], a = m.a;
    // ---- dR = dU K + U dK + [0; db_d];  K_l . dK_l -----------------------------------------------------------------------------------------
    for (int idx = t; idx < (D + 1) * 32; idx += 256) {
        const int i = idx >> 5, d = idx & 31;
        if (d < D) {
            double s = i == D ? m.dbd[d] : 0.0;
            for (int l = 0; l < L; ++l) {
                s = fma(m.dU[i * kIm + l], m.K[l * kIm + d], s);
                s = fma(m.U[i * kIm + l], m.dK[l * kIm + d], s);
            }
            m.dR[i * kIm + d] = s;
        }
    }
    if (t < L) {
        double s = 0.0;
        for (int d = 0; d < D; ++d) s = fma(m.K[t * kIm + d], m.dK[t * kIm + d], s);
        m.kdk[t] = s;
    }
    __syncthreads();
    // ---- dG = a (S dR - deps SR);  tr(SR^T dR) ---------------------------------------------------------------------------------------------
    double part = 0.0;
    for (int idx = t; idx < (D + 1) * 32; idx += 256) {
        const int i = idx >> 5, d = idx & 31;
        if (d < D) {
            double s = 0.0;
            for (int k = 0; k <= D; ++k) s = fma(m.S[i * kIm + k], m.dR[k * kIm + d], s);
            const double sr = m.SR[i * kIm + d];
            m.dG[i * kIm + d] = a * (s - deps * sr);
            part = fma(sr, m.dR[i * kIm + d], part);
        }
    }
    const double tr = block_sum256(part, m.red, t);                  // its barriers also publish dG
    // ---- (Hv)_U = S dU + dG K^T + a SR dK^T ------------------------------------------------------------------------------------------------
    for (int idx = t; idx < (D + 1) * 32; idx += 256) {
        const int i = idx >> 5, l = idx & 31;
        if (l < L) {
            double s = 0.0, g = 0.0;
            for (int k = 0; k <= D; ++k) s = fma(m.S[i * kIm + k], m.dU[k * kIm + l], s);
            for (int d = 0; d < D; ++d) s = fma(m.dG[i * kIm + d], m.K[l * kIm + d], s);
            for (int d = 0; d < D; ++d) g = fma(m.SR[i * kIm + d], m.dK[l * kIm + d], g);
            hout[i * L + l] = fma(a, g, s);
        }
    }
    // ---- (Hv)_K = a dU^T SR + U^T dG + a (w dK + dw K - deps w K) ---------------------------------------------------------------------------
    for (int idx = t; idx < L * 32; idx += 256) {
        const int l = idx >> 5, d = idx & 31;
        if (d < D) {
            double s = 0.0, g = 0.0;
            for (int i = 0; i <= D; ++i) g = fma(m.dU[i * kIm + l], m.SR[i * kIm + d], g);
            for (int i = 0; i <= D; ++i) s = fma(m.U[i * kIm + l], m.dG[i * kIm + d], s);
            const double w = m.wl[l], kk = m.K[l * kIm + d];
            g += w * m.dK[l * kIm + d] + m.dw[l] * kk - deps * w * kk;
            hout[m.off_wd + l * D + d] = fma(a, g, s);
        }
    }
    if (t < D) hout[m.off_bd + t] = m.dG[D * kIm + t];
    if (t < L) {
        const double w = m.wl[t], dw = m.dw[t], k2 = m.k2[t];
        hout[m.off_p + t] = 0.5 * dw + 0.5 * a * dw * k2 + a * w * m.kdk[t] - 0.5 * deps * a * w * k2;
    }
    if (t == 0 && m.off_c >= 0) {
        double dq = 2.0 * tr;
        for (int l = 0; l < L; ++l) dq += m.dw[l] * m.k2[l] + 2.0 * m.wl[l] * m.kdk[l];
        hout[m.off_c] = m.eps_cli * (0.5 * deps * a * m.Q - 0.5 * a * dq);
    }
    __syncthreads();
}

template <bool LANCZOS>
__global__ __launch_bounds__(256) void elbo_hessian_kernel(const HessArgs a) {
    extern __shared__ __attribute__((aligned(16))) double pool[];
    __shared__ double red[256];
    __shared__ double S1[kSpectrumMaxDim], wl[kSpectrumMaxDim], pl[kSpectrumMaxDim], k2[kSpectrumMaxDim], dw[kSpectrumMaxDim];
    __shared__ double kdk[kSpectrumMaxDim], dbd[kSpectrumMaxDim], bd[kSpectrumMaxDim], coef[kSpectrumMaxDim], alpha[kSpectrumMaxDim];
    __shared__ double beta[kSpectrumMaxDim], rot_c[kSpectrumMaxDim], rot_s[kSpectrumMaxDim], eig[kSpectrumMaxDim], pub[4];
    __shared__ int rot_mate[kSpectrumMaxDim];

    const int t = threadIdx.x;
    const long long r = blockIdx.x;
    const int D = a.D, L = a.L, P = a.P, rows = a.rows;
    const int off_wd = (D + 1) * L, off_bd = off_wd + L * D;
    const float* const p = a.params + r * a.state_stride;
    double* const out = a.out + r * a.out_stride;
    double* const S = pool + oS;
    double* const U = pool + oU;
    double* const K = pool + oK;
    double* const R = pool + oR;
    double* const SR = pool + oSR;
    double* const wv = pool + oW;

    // ---- moments: cov_spectrum.hip's tile loop.  Waves 0 .. 2 own the blocks (0, 0), (0, 1), (1, 1) of sum x x^T, wave 3 the column sums --
    {
        RowCtx rc{};
        rc.D = D; rc.L = L;
        rc.g = a.gen;
        const bool explicit_rows = a.x != nullptr;
        if (explicit_rows) {
            rc.xr = a.x + r * a.x_stride;
        } else {
            if (rc.g.A) rc.g.A += r * a.a_stride;
            rc.key = philox_key(a.x_seeds[r]);
            rc.step = a.x_steps[r];
        }
        float* const smem = reinterpret_cast<float*>(pool + oDK);
        const int w = __builtin_amdgcn_readfirstlane(t >> 6);
        const int lane = t & 63, g = lane >> 4, c = lane & 15;
        const bool two = D > 16;
        f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
        const int ia = w == 2 ? 16 : 0, jb = (w == 1 || w == 2) ? 16 : 0;
        for (int base = 0; base < rows; base += 256) {
            {
                float x[kSpectrumMaxDim];
                const int row = base + t;
                if (row < rows) {
                    if (explicit_rows) produce_row<SRC_EXPLICIT, kSpectrumMaxDim, 4, false>(rc, row, x);
                    else produce_row<SRC_REAL, kSpectrumMaxDim, 4, false>(rc, row, x);
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
            const int ksteps = ((left < 256 ? left : 256) + 3) >> 2;  // the k-steps that hold a row; the rest of the tile adds +0
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
            __syncthreads();                                           // the tile is free again (and, after the last one, dead)
        }
        // result (lane, register q) is row g + 4 q, column c of its block; the upper-triangle blocks wait in front of the tile
        double* const S2 = pool + oDU;
        if (w < 3) {
#pragma unroll
            for (int q = 0; q < 4; ++q) S2[(ia + g + 4 * q) * kMatStride + jb + c] = acc0[q];
        } else if (g == 0) {
            S1[c] = acc0[0];
            S1[16 + c] = acc1[0];
        }
        __syncthreads();
        // S = (1 / rows) [sum x x^T, sum x; sum x^T, rows], the ones row and column at index D, zero outside; U and K start as zero
        const double n = (double)rows;
        for (int idx = t; idx < kImg; idx += 256) {
            const int i = idx / kIm, j = idx % kIm;
            double v = 0.0;
            if (i < D && j < D) v = (i <= j ? S2[i * kMatStride + j] : S2[j * kMatStride + i]) / n;
            else if (i == D && j < D) v = S1[j] / n;
            else if (j == D && i < D) v = S1[i] / n;
            else if (i == D && j == D) v = 1.0;
            S[idx] = v;
            U[idx] = 0.0;
            K[idx] = 0.0;
            R[idx] = 0.0;
            SR[idx] = 0.0;
        }
        __syncthreads();
    }

    // ---- the parameters, widened once: U = [E; b_e], K, b_d, p, w = e^p, eps ------------------------------------------------------------
    for (int e = t; e < off_bd; e += 256) {
        const double x = (double)p[e];
        if (e < off_wd) U[(e / L) * kIm + e % L] = x;
        else { const int q = e - off_wd; K[(q / D) * kIm + q % D] = x; }
    }
    if (t < kSpectrumMaxDim) {
        bd[t] = t < D ? (double)p[off_bd + t] : 0.0;
        const double lv = t < L ? (double)p[a.off_p + t] : 0.0;
        pl[t] = lv;
        wl[t] = t < L ? exp(lv) : 0.0;
    }
    const double eps_cli = (double)a.eps_cli;
    const double eps = a.off_c >= 0 ? (double)p[a.off_c] * eps_cli : eps_cli;
    const double ea = exp(-eps);
    __syncthreads();

    // ---- R = U K + [-I; b_d], |K_l|^2 ------------------------------------------------------------------------------------------------------
    for (int idx = t; idx < (D + 1) * 32; idx += 256) {
        const int i = idx >> 5, d = idx & 31;
        if (d < D) {
            double s = i == D ? bd[d] : (i == d ? -1.0 : 0.0);
            for (int l = 0; l < L; ++l) s = fma(U[i * kIm + l], K[l * kIm + d], s);
            R[i * kIm + d] = s;
        }
    }
    if (t < kSpectrumMaxDim) {
        double s = 0.0;
        if (t < L)
            for (int d = 0; d < D; ++d) s = fma(K[t * kIm + d], K[t * kIm + d], s);
        k2[t] = s;
    }
    __syncthreads();
    // ---- SR = S R, Q = tr(R^T S R) + sum_l w_l |K_l|^2 -------------------------------------------------------------------------------------
    double part = 0.0;
    for (int idx = t; idx < (D + 1) * 32; idx += 256) {
        const int i = idx >> 5, d = idx & 31;
        if (d < D) {
            double s = 0.0;
            for (int k = 0; k <= D; ++k) s = fma(S[i * kIm + k], R[k * kIm + d], s);
            SR[i * kIm + d] = s;
            part = fma(R[i * kIm + d], s, part);
        }
    }
    double Q = block_sum256(part, red, t);                            // its barriers also publish SR
    double klc = 0.0;
    for (int l = 0; l < L; ++l) {
        Q = fma(wl[l], k2[l], Q);
        klc += wl[l] - 1.0 - pl[l];
    }

    // ---- the gradient into the flat vector; tr(U^T S U) ------------------------------------------------------------------------------------
    part = 0.0;
    for (int idx = t; idx < (D + 1) * 32; idx += 256) {
        const int i = idx >> 5, l = idx & 31;
        if (l < L) {
            double s = 0.0, g = 0.0;
            for (int k = 0; k <= D; ++k) s = fma(S[i * kIm + k], U[k * kIm + l], s);
            for (int d = 0; d < D; ++d) g = fma(SR[i * kIm + d], K[l * kIm + d], g);
            part = fma(U[i * kIm + l], s, part);
            wv[i * L + l] = fma(ea, g, s);
        }
    }
    for (int idx = t; idx < L * 32; idx += 256) {
        const int l = idx >> 5, d = idx & 31;
        if (d < D) {
            double g = wl[l] * K[l * kIm + d];
            for (int i = 0; i <= D; ++i) g = fma(U[i * kIm + l], SR[i * kIm + d], g);
            wv[off_wd + l * D + d] = ea * g;
        }
    }
    if (t < D) wv[off_bd + t] = ea * SR[D * kIm + t];
    if (t < L) wv[a.off_p + t] = 0.5 * (wl[t] - 1.0) + 0.5 * ea * wl[t] * k2[t];
    if (t == 0 && a.off_c >= 0) wv[a.off_c] = eps_cli * (0.5 * (double)D - 0.5 * ea * Q);
    const double trusu = block_sum256(part, red, t);                  // its barriers also publish the gradient
    const double f = 0.5 * trusu + 0.5 * klc + 0.5 * ea * Q + 0.5 * (double)D * (eps + kLog2PiF64);
    part = 0.0;
    for (int e = t; e < P; e += 256) part = fma(wv[e], wv[e], part);
    const double gnorm = sqrt(block_sum256(part, red, t));

    HessModel m;
    m.S = S; m.U = U; m.K = K; m.SR = SR;
    m.dU = pool + oDU; m.dK = pool + oDK; m.dR = pool + oDR; m.dG = pool + oDG;
    m.wl = wl; m.k2 = k2; m.dw = dw; m.kdk = kdk; m.dbd = dbd; m.red = red; m.pub = pub;
    m.D = D; m.L = L; m.P = P; m.off_wd = off_wd; m.off_bd = off_bd; m.off_p = a.off_p; m.off_c = a.off_c;
    m.a = ea; m.Q = Q; m.eps_cli = a.off_c >= 0 ? eps_cli : 0.0;

    if constexpr (!LANCZOS) {
        if (a.grad) {
            double* const g = a.grad + r * a.grad_stride;
            for (int e = t; e < P; e += 256) g[e] = wv[e];
        }
        if (t < kHvpRecord) out[t] = t == 0 ? f : (t == 1 ? gnorm : (t == 2 ? eps : (double)rows));
        if (a.nvec > 0) {                                               // nvec = 0: v and hv may be NULL and are not touched
            const double* const v = a.v + r * a.v_stride;
            double* const hv = a.hv + r * a.hv_stride;
            for (int i = 0; i < a.nvec; ++i) hess_hvp(m, v + (long long)i * P, hv + (long long)i * P, t);
        }
    } else {
        double* const basis = a.basis + r * a.basis_stride;
        const double* const v0 = a.v0 + r * a.v0_stride;
        // ---- v_1 = v0 / |v0|; v0 = 0 (or not a number): k = 0 -------------------------------------------------------------------------------
        const int kmax = lanczos_start(v0, basis, P, a.steps, red, t);
        // The basis is stored to global memory and read back by other lanes of THIS workgroup (the products, the Gram-Schmidt passes,
        // omega) behind __syncthreads() alone: that relies on workgroup-scope visibility of global stores, which holds where a workgroup
        // shares one CU's vector L1 (the default mode) and would not under threadgroup-split (tgsplit) mode.
        __syncthreads();
        // T goes into the Jacobi buffers over the direction images, dead once the last product is done
        LanczosLds s;
        s.mat = pool + oDU; s.vec = s.mat + 2 * kMatDoubles; s.red = red; s.alpha = alpha; s.beta = beta;
        s.rot_c = rot_c; s.rot_s = rot_s; s.eig = eig; s.rot_mate = rot_mate;
        int k = 0;
        double scale = 0.0;
        for (int j = 0; j < kmax; ++j) {
            hess_hvp(m, basis + (long long)j * P, wv, t);
            double al, be;
            lanczos_orthogonalise(wv, basis, P, j, coef, red, t, al, be);
            if (t == 0) { alpha[j] = al; beta[j] = be; }
            k = j + 1;
            if (lanczos_next(wv, basis, P, k, kmax, al, be, scale, t)) break;
            __syncthreads();
        }
        __syncthreads();
        const RitzResult rz = lanczos_ritz(s, k, out, t);
        const double omega = lanczos_omega(basis, P, k, red, t);
        lanczos_head_store(out, t, k, f, gnorm, eps, rows, omega, rz);
    }
}

// vaek_supports_exact_log_likelihood's predicate: float32, no hidden layers, ONE decoder, D, L <= 32
static bool elbo_hessian_covered(const vaek_ctx* c) {
    const vaek_config& cfg = c->cfg;
    return cfg.dtype == VAEK_F32 && cfg.n_enc_hidden == 0 && cfg.n_dec_hidden == 0 && !cfg.sigmoid_decoder && c->D >= 1 && c->L >= 1 &&
           c->D <= kSpectrumMaxDim && c->L <= kSpectrumMaxDim;
}

// the leaf layout the kernel indexes by: E, b_e, K, b_d, epsilon_p and, under tunable_eps, epsilon
static bool elbo_hessian_layout(const vaek_ctx* c) {
    const int64_t off_p = (int64_t)(c->D + 1) * c->L + (int64_t)c->L * c->D + c->D;
    return c->off_epsp == off_p && (c->off_eps < 0 || c->off_eps == off_p + c->L) && c->P == off_p + c->L + (c->off_eps >= 0 ? 1 : 0);
}

// the description's checks (`record`: the call's record length and its query) and what the two kernels share of HessArgs
static int hessian_common(const char* who, const EvalDesc& d, int record, const char* record_query, vaek_ctx* ctx, const float* params,
                          int32_t kind, const float* A, int32_t dd, int32_t did, int32_t pad, float var_added, uint32_t x_tag, HessArgs* a) {
    EvalRules r{};
    r.covered = ctx && elbo_hessian_covered(ctx) && elbo_hessian_layout(ctx);
    r.needs = "needs a float32 linear VAE (no hidden layers) with ONE decoder and D, L <= 32: the sigmoid second decoder has no closed form (see "
              "vaek_supports_elbo_hessian)";
    r.rows_min = 1; r.rows_cap = kLogLikMaxRows; r.rows_query = "vaek_log_likelihood_max_rows";
    r.records = 1; r.record_len = record; r.record_query = record_query;
    r.draws = true; r.kind = kind; r.A = A; r.dd = dd; r.did = did; r.pad = pad; r.x_tag = x_tag;
    if (int rc = check_eval(who, ctx, params, d, r)) return rc;
    a->params = params; a->state_stride = d.state_stride;
    a->x_seeds = reinterpret_cast<const unsigned long long*>(d.x_seeds); a->x_steps = d.x_steps;
    a->x = d.rows_ptr; a->x_stride = d.rows_stride;
    a->rows = d.rows; a->D = ctx->D; a->L = ctx->L; a->P = (int)ctx->P; a->off_p = (int)ctx->off_epsp; a->off_c = (int)ctx->off_eps;
    a->eps_cli = ctx->cfg.eps_cli;
    fill_rows_source(&a->gen, &a->a_stride, ctx, d.rows, d.explicit_rows(), kind, A, dd, did, pad, var_added, x_tag, d.a_stride);
    return VAEK_OK;
}

template <bool LANCZOS>
static int hessian_launch(const char* label, const HessArgs& a, int n, hipStream_t st) {
    static thread_local PerDeviceOnce attr_set;
    VAEK_HIP_CHECK(set_max_dynamic_lds(attr_set, elbo_hessian_kernel<LANCZOS>, kHessLds));
    {
        ProfScope ps(label, st);
        launch_k(ps, elbo_hessian_kernel<LANCZOS>, dim3((unsigned)n), dim3(256), kHessLds, st, a);
    }
    VAEK_HIP_CHECK(hipGetLastError());
    return VAEK_OK;
}

}  // namespace vaek

using namespace vaek;

extern "C" {

int vaek_supports_elbo_hessian(const vaek_ctx* ctx, int32_t kind, int32_t* yes) {
    if (!ctx || !yes) { set_error("vaek_supports_elbo_hessian: null argument"); return VAEK_ERR_INVALID; }
    *yes = kind >= 0 && kind <= 2 && elbo_hessian_covered(ctx) ? 1 : 0;
    return VAEK_OK;
}

int vaek_elbo_hvp_max_vectors(void) { return kHvpMaxVectors; }
int vaek_elbo_hvp_record_len(void) { return kHvpRecord; }
int vaek_elbo_hessian_max_steps(void) { return kLanczosMaxSteps; }
int vaek_elbo_hessian_record_len(void) { return kLanczosRecord; }

int vaek_elbo_hessian_basis_doubles(const vaek_ctx* ctx, int32_t steps, int64_t* doubles) {
    if (!ctx || !doubles) { set_error("vaek_elbo_hessian_basis_doubles: null argument"); return VAEK_ERR_INVALID; }
    if (!elbo_hessian_covered(ctx) || steps < 1 || steps > kLanczosMaxSteps) {
        set_error("vaek_elbo_hessian_basis_doubles: an unsupported context (see vaek_supports_elbo_hessian) or %d steps outside 1 .. %d", steps,
                  kLanczosMaxSteps);
        return VAEK_ERR_INVALID;
    }
    *doubles = (int64_t)steps * ctx->P;
    return VAEK_OK;
}

int vaek_elbo_hvp_replicas(vaek_ctx* ctx, const float* params, const vaek_elbo_hvp* hp, int32_t kind, const float* A, int32_t dd, int32_t did,
                           int32_t pad, float var_added, uint32_t x_tag, void* stream) {
    const char* who = "vaek_elbo_hvp_replicas";
    ProfBind pb(ctx);
    HessArgs a{};
    if (int rc = hessian_common(who, describe(hp), kHvpRecord, "vaek_elbo_hvp_record_len", ctx, params, kind, A, dd, did, pad, var_added, x_tag, &a))
        return rc;
    if (int rc = check_hvp_buffers(who, hp, ctx->P, false)) return rc;      // one launch: v and hv may overlap, as they always could
    a.out = hp->out; a.out_stride = hp->out_stride;
    a.v = hp->v; a.v_stride = hp->v_stride; a.hv = hp->hv; a.hv_stride = hp->hv_stride;
    a.grad = hp->grad; a.grad_stride = hp->grad_stride; a.nvec = hp->nvec;
    return hessian_launch<false>("elbo_hvp_replicas", a, hp->n, (hipStream_t)stream);
}

int vaek_elbo_hessian_lanczos_replicas(vaek_ctx* ctx, const float* params, const vaek_elbo_hessian* hs, int32_t kind, const float* A, int32_t dd,
                                       int32_t did, int32_t pad, float var_added, uint32_t x_tag, void* stream) {
    const char* who = "vaek_elbo_hessian_lanczos_replicas";
    ProfBind pb(ctx);
    HessArgs a{};
    if (int rc = hessian_common(who, describe(hs), kLanczosRecord, "vaek_elbo_hessian_record_len", ctx, params, kind, A, dd, did, pad, var_added, x_tag, &a))
        return rc;
    if (int rc = check_lanczos_buffers(who, hs, ctx->P)) return rc;
    a.out = hs->out; a.out_stride = hs->out_stride;
    a.v0 = hs->v0; a.v0_stride = hs->v0_stride; a.basis = hs->basis; a.basis_stride = hs->basis_stride; a.steps = hs->steps;
    return hessian_launch<true>("elbo_hessian_replicas", a, hs->n, (hipStream_t)stream);
}

}  // extern "C"
