// Hessian of the SAMPLE-AVERAGE ELBO of linear VAEs with one or two decoders (vaek_sampled_elbo_hvp_replicas,
// vaek_sampled_elbo_hessian_lanczos_replicas): fix the rows and K latent samples per row, and the Monte-Carlo ELBO f_K(theta) is a smooth
// deterministic function whose gradient and Hessian-vector products are exact derivatives, written out by hand (forward over reverse;
// include/vaek.h gives the formulas, DESIGN 3.22 the derivation).  Nothing is finite-differenced.  The cost scales with rows x K, so the
// work is spread over the device and the Lanczos recursion runs across launches.
//
//   COLUMN TILES.  Column q = i K + k of a replica is the pair (row i, sample k).  A workgroup of 256 threads takes kTileCols = 256
//     columns of one replica, 32 at a time: it stages x (the row sources of eigen_dev.h) and xi (explicit, or the BLOCK RULE of
//     vaek_log_likelihood_replicas: sample k of row i is Philox blocks k ceil(L / 4) + j of the row's latent stream), runs the primal pass
//     and, for a direction, the tangent-forward, backward and tangent-backward passes, all float64 on v_mfma_f64_16x16x4_f64: columns x D
//     by D x L and back, and the contractions x^T g, s^T g over the columns, whose accumulators stay in registers across the eight
//     sub-tiles.  Every element of the tile's PARTIAL of H v (or of grad f_K and f_K) is ONE chain over the tile's columns in column order.
//   COMBINE.  One workgroup per replica adds the tiles' partials in tile order.  The partials cross a launch boundary: nothing stored in
//     a launch is read back in it, and there is no atomic, counter, wait or spin.
//   LANCZOS.  lanczos_dev.h's recursion, a launch per piece.  Per step one tile launch (H v_j) and one per-replica launch: combine, then
//     the header's step (classical Gram-Schmidt twice against v_1 .. v_j, alpha_j, beta_j, the breakdown rule, v_{j+1} into the caller's
//     basis).  A replica that is done leaves a flag in its state block of the workspace; the later launches read it and do nothing.  The
//     last launch runs the header's Ritz tail, omega and record store on the alpha and beta of the state block.
//
// The kernels read rows / samples / parameters / directions and store only the named outputs and the workspace, with per-lane vector
// stores.  Launches: 2 + 2 nvec (hvp call), 3 + 2 steps (Lanczos call).
#include "lanczos_dev.h"
#include "eval_check.h"

namespace vaek {

constexpr int kSampMaxColumns = 1 << 22;     // n * rows * samples of one call ...
constexpr int kSampReplicaColumnsLog2 = 16;  // ... and rows * samples of one replica, 2^16: caps on the length of a launch
constexpr int kSampRecord = kLanczosRecord + 2;      // the Lanczos record, then samples and the two-decoder flag

constexpr int kSub = 32;                     // columns of a sub-tile: two 16-row blocks of the matrix-core products
constexpr int kTileCols = 256;               // columns of a workgroup's tile
constexpr int kMs = 33;                      // doubles (floats, for x and xi) between two rows of an LDS matrix: odd, no bank conflict down a column
constexpr int kMat = kSub * kMs;
constexpr int kState = 128;                  // doubles of a replica's state block: [0] done  [1] k  [2] scale  [3] f  [4] |grad|  [5] eps
constexpr int sAlpha = 32, sBeta = 64;       //   [32, 64) alpha  [64, 96) beta
constexpr int kSampFlat = 2816;              // >= P: 2809 at D = 28, L = 32 with two decoders and epsilon

// the pool, in doubles: parameter and direction matrices, ten vectors of 32, ten column-tile matrices, x and xi as floats
constexpr int oE = 0, oK = kMat, oKs = 2 * kMat, oDE = 3 * kMat, oDK = 4 * kMat, oDKs = 5 * kMat, oVec = 6 * kMat;
constexpr int vBe = 0, vBd = 32, vBs = 64, vSd = 96, vEw = 128, vPl = 160, vDbe = 192, vDbd = 224, vDbs = 256, vDp = 288;
constexpr int oT = oVec + 320;
constexpr int oS = oT, oR = oT + kMat, oSP = oT + 2 * kMat, oQE = oT + 3 * kMat, oGS = oT + 4 * kMat, oDMU = oT + 5 * kMat,
              oDS = oT + 6 * kMat, oDGY = oT + 7 * kMat, oDGA = oT + 8 * kMat, oDGS = oT + 9 * kMat, oX = oT + 10 * kMat,
              kSampPool = oX + kMat;         // x and xi: kMat floats each
constexpr size_t kSampLds = sizeof(double) * kSampPool;
static_assert(kSampLds + 4096 <= 160 * 1024, "the pool and the static arrays fit one CU's LDS");

struct SampArgs {
    const float* params; long long state_stride;
    const unsigned long long* x_seeds; const unsigned* x_steps;      // [n]: the rows' Philox key and step (drawing mode)
    const unsigned long long* z_seeds; const unsigned* z_steps;      // [n]: the samples' (xi == NULL)
    long long a_stride;
    const float* x; long long x_stride;                              // explicit rows [rows][D] per replica, or NULL
    const float* xi; long long xi_stride;                            // explicit samples [rows * samples][L] per replica, or NULL
    int rows, samples, D, L, P, sig, off_p, off_c;                   // off_c < 0: no epsilon leaf
    float eps_cli;
    unsigned z_tag;
    BatchArgs gen;                 // kind, A, dd, did, pad, noise_std, tag = x_tag, D, L
    double* ws; int tiles, pstride;                                  // state blocks [n][kState], then partials [n][tiles][pstride]
    const double* dir; long long dir_stride;                         // the direction of a tangent launch, [P] per replica
    int use_flag;                                                    // Lanczos: a replica whose state says done is skipped
    // the per-replica launches
    double* dst; long long dst_stride;                               // hvp: H v or the gradient (NULL: not stored)
    double* out; long long out_stride;
    const double* v0; long long v0_stride;
    double* basis; long long basis_stride;
    int steps, j;
};

__device__ __forceinline__ double* samp_partial(const SampArgs& a, long long r, int tile, int n_replicas) {
    return a.ws + (long long)n_replicas * kState + (r * a.tiles + tile) * (long long)a.pstride;
}

// acc += A B over `ksteps` k-steps of 4: fa(i, k) is element (i, k) of the 16 x 4k A, fb(k, j) of the 4k x 16 B.  Result register q of
// lane (g = lane >> 4, c = lane & 15) is element (g + 4 q, c).
template <class FA, class FB>
__device__ __forceinline__ f64x4 mma(f64x4 acc, const int ksteps, const int g, const int c, FA fa, FB fb) {
    for (int s = 0; s < ksteps; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(fa(c, 4 * s + g), fb(4 * s + g, c), acc, 0, 0, 0);
    return acc;
}

// TAN false: the partial of grad f_K and f_K; true: of H v for the direction a.dir
template <bool TAN>
__global__ __launch_bounds__(256) void sampled_tile_kernel(const SampArgs a, const int n_replicas) {
    extern __shared__ __attribute__((aligned(16))) double pool[];
    __shared__ double cw[2 * kSub], vs[2][32];

    const int t = threadIdx.x;
    const int tile = blockIdx.x;
    const long long r = blockIdx.y;
    if (a.use_flag && a.ws[r * kState] != 0.0) return;                 // uniform: written by an earlier launch
    const int D = a.D, L = a.L, P = a.P;
    const bool sig = a.sig != 0;
    const int off_be = D * L, off_K = (D + 1) * L, off_bd = off_K + L * D, off_Ks = off_bd + D, off_bs = off_Ks + L * D;
    const float* const p = a.params + r * a.state_stride;
    const double* const dir = TAN ? a.dir + r * a.dir_stride : nullptr;
    double* const Em = pool + oE;
    double* const Km = pool + oK;
    double* const Ksm = pool + oKs;
    double* const dEm = pool + oDE;
    double* const dKm = pool + oDK;
    double* const dKsm = pool + oDKs;
    double* const vec = pool + oVec;
    double* const Sm = pool + oS;
    double* const Rm = pool + oR;
    double* const SPm = pool + oSP;
    double* const QEm = pool + oQE;
    double* const GSm = pool + oGS;
    double* const DMUm = pool + oDMU;
    double* const DSm = pool + oDS;
    double* const DGYm = pool + oDGY;
    double* const DGAm = pool + oDGA;
    double* const DGSm = pool + oDGS;
    float* const Xf = reinterpret_cast<float*>(pool + oX);
    float* const XIf = Xf + kMat;

    // ---- the pool starts as zero: every padded row and column of a matrix adds 0 ------------------------------------------------------------
    for (int idx = t; idx < kSampPool; idx += 256) pool[idx] = 0.0;
    __syncthreads();
    // ---- the parameters (and the direction), widened once -------------------------------------------------------------------------------------
    for (int e = t; e < P; e += 256) {
        const double x = (double)p[e];
        const double dx = TAN ? dir[e] : 0.0;
        if (e < off_be) { const int o = (e / L) * kMs + e % L; Em[o] = x; dEm[o] = dx; }
        else if (e < off_K) { vec[vBe + e - off_be] = x; vec[vDbe + e - off_be] = dx; }
        else if (e < off_bd) { const int q = e - off_K, o = (q / D) * kMs + q % D; Km[o] = x; dKm[o] = dx; }
        else if (e < off_Ks) { vec[vBd + e - off_bd] = x; vec[vDbd + e - off_bd] = dx; }
        else if (sig && e < off_bs) { const int q = e - off_Ks, o = (q / D) * kMs + q % D; Ksm[o] = x; dKsm[o] = dx; }
        else if (sig && e < a.off_p) { vec[vBs + e - off_bs] = x; vec[vDbs + e - off_bs] = dx; }
        else if (e < a.off_p + L) {
            const int l = e - a.off_p;
            vec[vPl + l] = x; vec[vSd + l] = exp(0.5 * x); vec[vEw + l] = exp(x); vec[vDp + l] = dx;
        }
    }
    const double eps_cli = (double)a.eps_cli;
    const double eps = a.off_c >= 0 ? (double)p[a.off_c] * eps_cli : eps_cli;
    const double ea = exp(-eps);
    const double deps = TAN && a.off_c >= 0 ? eps_cli * dir[a.off_c] : 0.0;
    const int ncols = a.rows * a.samples;
    const double c0 = ea / (double)ncols, c1 = 1.0 / (double)ncols;
    __syncthreads();

    // ---- the sources of the rows and of the samples -------------------------------------------------------------------------------------------
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
    BatchArgs gz = a.gen;
    gz.tag = a.z_tag;
    const float* const xi = a.xi ? a.xi + r * a.xi_stride : nullptr;
    const uint2 zkey = xi ? make_uint2(0u, 0u) : philox_key(a.z_seeds[r]);
    const unsigned zstep = xi ? 0u : a.z_steps[r];
    const int nlb = (L + 3) >> 2;                                      // Philox blocks of one sample

    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int lane = t & 63, g = lane >> 4, c = lane & 15;
    const int nbD = (D + 15) >> 4, nbL = (L + 15) >> 4, kD = (D + 3) >> 2, kL = (L + 3) >> 2;
    const int nE = nbD * nbL, nK = nbL * nbD, nAll = nE + nK + (sig ? nK : 0);      // the 16 x 16 blocks of dE, dK, dK_s: wave w owns w, w + 4, w + 8
    f64x4 acc[3];
#pragma unroll
    for (int b = 0; b < 3; ++b) acc[b] = f64x4{0.0, 0.0, 0.0, 0.0};
    double vsum = 0.0, vsum2 = 0.0;                                    // thread (grp, idx): a bias / epsilon_p element or a term of f, one chain over the columns
    const int grp = t >> 5, idx = t & 31;

    for (int sub = 0; sub < kTileCols / kSub; ++sub) {
        const int base = tile * kTileCols + sub * kSub;
        if (base >= ncols) break;                                       // uniform
        // ---- stage x and xi: thread (col, part) draws block `part` of its column's sample; part 0 also produces the row ---------------------
        {
            const int col = t >> 3, part = t & 7;
            const int q = base + col;
            const bool valid = q < ncols;
            const int i = valid ? q / a.samples : 0, k = valid ? q % a.samples : 0;
            if (part == 0) {
                float x[kSpectrumMaxDim];
                if (valid) {
                    if (explicit_rows) produce_row<SRC_EXPLICIT, kSpectrumMaxDim, 4, false>(rc, i, x);
                    else produce_row<SRC_REAL, kSpectrumMaxDim, 4, false>(rc, i, x);
                } else {
#pragma unroll
                    for (int d = 0; d < kSpectrumMaxDim; ++d) x[d] = 0.f;
                }
#pragma unroll
                for (int d = 0; d < kSpectrumMaxDim; ++d) Xf[col * kMs + d] = x[d];
                cw[col] = valid ? c0 : 0.0;
                cw[kSub + col] = valid ? c1 : 0.0;
            }
            float n4[4] = {0.f, 0.f, 0.f, 0.f};
            if (valid && 4 * part < L) {
                if (xi) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (4 * part + e < L) n4[e] = xi[(long long)q * L + 4 * part + e];
                } else {
                    latent_block(gz, zstep, i, zkey, k * nlb + part, n4);
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) XIf[col * kMs + 4 * part + e] = 4 * part + e < L ? n4[e] : 0.f;
        }
        __syncthreads();

        // ---- mu = x E + b_e, s = mu + e^{p/2} xi;  dmu = x dE + db_e, ds = dmu + 1/2 dp e^{p/2} xi  (32 x L, k over D) -----------------------
        for (int b = w; b < 2 * nbL; b += 4) {
            const int i0 = (b / nbL) * 16, j0 = (b % nbL) * 16;
            const f64x4 z = {0.0, 0.0, 0.0, 0.0};
            const f64x4 mu = mma(z, kD, g, c, [&](int i, int k) { return (double)Xf[(i0 + i) * kMs + k]; },
                                 [&](int k, int j) { return Em[k * kMs + j0 + j]; });
            f64x4 dmu = z;
            if (TAN)
                dmu = mma(z, kD, g, c, [&](int i, int k) { return (double)Xf[(i0 + i) * kMs + k]; },
                          [&](int k, int j) { return dEm[k * kMs + j0 + j]; });
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int col = i0 + g + 4 * q, l = j0 + c, o = col * kMs + l;
                const double sx = vec[vSd + l] * (double)XIf[o];
                const double m = mu[q] + vec[vBe + l];
                Sm[o] = m + sx;
                if (TAN) {
                    const double dm = dmu[q] + vec[vDbe + l];
                    DMUm[o] = dm;
                    DSm[o] = dm + 0.5 * vec[vDp + l] * sx;
                } else {
                    DMUm[o] = m;                                        // the gradient pass keeps mu here
                }
            }
        }
        __syncthreads();

        // ---- y = s K + b_d, u = s K_s + b_s, r = y + sigmoid(u) - x and their tangents; g_y = c0 r, g_a = g_y sigma'  (32 x D, k over L) -----
        for (int b = w; b < 2 * nbD; b += 4) {
            const int i0 = (b / nbD) * 16, j0 = (b % nbD) * 16;
            const f64x4 z = {0.0, 0.0, 0.0, 0.0};
            auto fs = [&](int i, int k) { return Sm[(i0 + i) * kMs + k]; };
            auto fds = [&](int i, int k) { return DSm[(i0 + i) * kMs + k]; };
            const f64x4 y = mma(z, kL, g, c, fs, [&](int k, int j) { return Km[k * kMs + j0 + j]; });
            f64x4 u = z, dy = z, du = z;
            if (sig) u = mma(z, kL, g, c, fs, [&](int k, int j) { return Ksm[k * kMs + j0 + j]; });
            if (TAN) {
                dy = mma(z, kL, g, c, fds, [&](int k, int j) { return Km[k * kMs + j0 + j]; });
                dy = mma(dy, kL, g, c, fs, [&](int k, int j) { return dKm[k * kMs + j0 + j]; });
                if (sig) {
                    du = mma(z, kL, g, c, fds, [&](int k, int j) { return Ksm[k * kMs + j0 + j]; });
                    du = mma(du, kL, g, c, fs, [&](int k, int j) { return dKsm[k * kMs + j0 + j]; });
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int col = i0 + g + 4 * q, d = j0 + c, o = col * kMs + d;
                double rr = 0.0, sp = 0.0, qe = 0.0, dgy = 0.0, dga = 0.0;
                if (d < D) {
                    const double w0 = cw[col];
                    double sg = 0.0, spp = 0.0;
                    if (sig) {
                        sg = 1.0 / (1.0 + exp(-(u[q] + vec[vBs + d])));
                        sp = sg * (1.0 - sg);
                        spp = sp * (1.0 - 2.0 * sg);
                    }
                    rr = y[q] + vec[vBd + d] + sg - (double)Xf[o];
                    if (TAN) {
                        const double dun = sig ? du[q] + vec[vDbs + d] : 0.0;
                        const double dr = dy[q] + vec[vDbd + d] + sp * dun;
                        dgy = w0 * (dr - deps * rr);
                        dga = dgy * sp + w0 * rr * spp * dun;
                        qe = w0 * rr * (0.5 * deps * rr - dr);
                    } else {
                        qe = w0 * rr * rr;
                    }
                }
                Rm[o] = rr; SPm[o] = sp; QEm[o] = qe;
                if (TAN) { DGYm[o] = dgy; DGAm[o] = dga; }
            }
        }
        __syncthreads();

        // ---- g_s = g_y K^T + g_a K_s^T;  dg_s = dg_y K^T + g_y dK^T + dg_a K_s^T + g_a dK_s^T  (32 x L, k over D) ---------------------------
        for (int b = w; b < 2 * nbL; b += 4) {
            const int i0 = (b / nbL) * 16, j0 = (b % nbL) * 16;
            const f64x4 z = {0.0, 0.0, 0.0, 0.0};
            auto fgy = [&](int i, int k) { return cw[i0 + i] * Rm[(i0 + i) * kMs + k]; };
            auto fga = [&](int i, int k) { return cw[i0 + i] * Rm[(i0 + i) * kMs + k] * SPm[(i0 + i) * kMs + k]; };
            f64x4 gs = mma(z, kD, g, c, fgy, [&](int k, int j) { return Km[(j0 + j) * kMs + k]; });
            if (sig) gs = mma(gs, kD, g, c, fga, [&](int k, int j) { return Ksm[(j0 + j) * kMs + k]; });
            f64x4 dgs = z;
            if (TAN) {
                dgs = mma(z, kD, g, c, [&](int i, int k) { return DGYm[(i0 + i) * kMs + k]; }, [&](int k, int j) { return Km[(j0 + j) * kMs + k]; });
                dgs = mma(dgs, kD, g, c, fgy, [&](int k, int j) { return dKm[(j0 + j) * kMs + k]; });
                if (sig) {
                    dgs = mma(dgs, kD, g, c, [&](int i, int k) { return DGAm[(i0 + i) * kMs + k]; },
                              [&](int k, int j) { return Ksm[(j0 + j) * kMs + k]; });
                    dgs = mma(dgs, kD, g, c, fga, [&](int k, int j) { return dKsm[(j0 + j) * kMs + k]; });
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int o = (i0 + g + 4 * q) * kMs + j0 + c;
                GSm[o] = gs[q];
                if (TAN) DGSm[o] = dgs[q];
            }
        }
        __syncthreads();

        // ---- the contractions over the 32 columns into the standing accumulators: dE = x^T g_mu, dK = s^T g_y, dK_s = s^T g_a and their
        // tangents x^T dg_mu, ds^T g_y + s^T dg_y, ds^T g_a + s^T dg_a;  g_mu = g_s + c1 mu ------------------------------------------------------
        auto fgy = [&](int k, int d) { return cw[k] * Rm[k * kMs + d]; };
        auto fga = [&](int k, int d) { return cw[k] * Rm[k * kMs + d] * SPm[k * kMs + d]; };
        auto gmu = [&](int k, int l) { return (TAN ? DGSm[k * kMs + l] : GSm[k * kMs + l]) + cw[kSub + k] * DMUm[k * kMs + l]; };
#pragma unroll
        for (int bi = 0; bi < 3; ++bi) {
            const int b = w + 4 * bi;
            if (b < nE) {
                const int i0 = (b / nbL) * 16, j0 = (b % nbL) * 16;
                acc[bi] = mma(acc[bi], kSub / 4, g, c, [&](int i, int k) { return (double)Xf[k * kMs + i0 + i]; },
                              [&](int k, int j) { return gmu(k, j0 + j); });
            } else if (b < nAll) {
                const bool second = b >= nE + nK;
                const int bb = b - nE - (second ? nK : 0);
                const int i0 = (bb / nbD) * 16, j0 = (bb % nbD) * 16;
                auto fs = [&](int i, int k) { return Sm[k * kMs + i0 + i]; };
                auto fds = [&](int i, int k) { return DSm[k * kMs + i0 + i]; };
                if (!second) {
                    if (TAN) {
                        acc[bi] = mma(acc[bi], kSub / 4, g, c, fds, [&](int k, int j) { return fgy(k, j0 + j); });
                        acc[bi] = mma(acc[bi], kSub / 4, g, c, fs, [&](int k, int j) { return DGYm[k * kMs + j0 + j]; });
                    } else {
                        acc[bi] = mma(acc[bi], kSub / 4, g, c, fs, [&](int k, int j) { return fgy(k, j0 + j); });
                    }
                } else {
                    if (TAN) {
                        acc[bi] = mma(acc[bi], kSub / 4, g, c, fds, [&](int k, int j) { return fga(k, j0 + j); });
                        acc[bi] = mma(acc[bi], kSub / 4, g, c, fs, [&](int k, int j) { return DGAm[k * kMs + j0 + j]; });
                    } else {
                        acc[bi] = mma(acc[bi], kSub / 4, g, c, fs, [&](int k, int j) { return fga(k, j0 + j); });
                    }
                }
            }
        }
        // ---- the bias and epsilon_p elements and the terms of f and of the epsilon element: thread (grp, idx), columns in order ------------
        for (int k = 0; k < kSub; ++k) {
            const int o = k * kMs + idx;
            if (grp == 0) vsum += gmu(k, idx);
            else if (grp == 1) vsum += TAN ? DGYm[o] : fgy(k, idx);
            else if (grp == 2) vsum += TAN ? DGAm[o] : fga(k, idx);
            else if (grp == 3) {
                const double hx = 0.5 * vec[vSd + idx] * (double)XIf[o];
                vsum += TAN ? DGSm[o] * hx + GSm[o] * (0.5 * vec[vDp + idx] * hx) : GSm[o] * hx;
            } else if (grp == 4) vsum += QEm[o];
            else if (grp == 5 && !TAN) vsum2 += cw[kSub + k] * (0.5 * DMUm[o] * DMUm[o]);
        }
        __syncthreads();                                               // the sub-tile's matrices are free again
    }

    // ---- the tile's partial.  Tile 0 also carries the terms that no column has ---------------------------------------------------------------
    double* const part = samp_partial(a, r, tile, n_replicas);
    const bool first = tile == 0;
#pragma unroll
    for (int bi = 0; bi < 3; ++bi) {
        const int b = w + 4 * bi;
        if (b < nE) {
            const int i0 = (b / nbL) * 16, j0 = (b % nbL) * 16;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int d = i0 + g + 4 * q, l = j0 + c;
                if (d < D && l < L) part[d * L + l] = acc[bi][q];
            }
        } else if (b < nAll) {
            const bool second = b >= nE + nK;
            const int bb = b - nE - (second ? nK : 0);
            const int i0 = (bb / nbD) * 16, j0 = (bb % nbD) * 16;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int l = i0 + g + 4 * q, d = j0 + c;
                if (l < L && d < D) part[(second ? off_Ks : off_K) + l * D + d] = acc[bi][q];
            }
        }
    }
    if (grp == 0 && idx < L) part[off_be + idx] = vsum;
    if (grp == 1 && idx < D) part[off_bd + idx] = vsum;
    if (grp == 2 && idx < D && sig) part[off_bs + idx] = vsum;
    if (grp == 3 && idx < L) {
        const double ew = vec[vEw + idx];
        part[a.off_p + idx] = first ? vsum + (TAN ? 0.5 * ew * vec[vDp + idx] : 0.5 * (ew - 1.0)) : vsum;
    }
    if (grp == 4) vs[0][idx] = idx < D ? vsum : 0.0;
    if (grp == 5) vs[1][idx] = idx < L ? vsum2 : 0.0;
    __syncthreads();
    if (t == 0) {
        double qs = 0.0, ms = 0.0;
        for (int d = 0; d < D; ++d) qs += vs[0][d];
        for (int l = 0; l < L; ++l) ms += vs[1][l];
        if (TAN) {
            if (a.off_c >= 0) part[a.off_c] = eps_cli * qs;            // eps_cli (1/2 deps sum c0 r^2 - sum c0 r . dr)
        } else {
            if (a.off_c >= 0) part[a.off_c] = eps_cli * ((first ? 0.5 * (double)D : 0.0) - 0.5 * qs);
            double f = ms + 0.5 * qs;
            if (first) {
                double klc = 0.0;
                for (int l = 0; l < L; ++l) klc += vec[vEw + l] - 1.0 - vec[vPl + l];
                f += 0.5 * klc + 0.5 * (double)D * (eps + kLog2PiF64);
            }
            part[P] = f;
        }
    }
}

// element e of the sum of replica r's partials, tiles in tile order
__device__ __forceinline__ double samp_combine(const SampArgs& a, long long r, int n_replicas, int e) {
    const double* const part = samp_partial(a, r, 0, n_replicas) + e;
    double s = 0.0;
    int tile = 0;
    for (; tile + 8 <= a.tiles; tile += 8) {                           // eight loads in flight, the adds in tile order
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = part[(long long)(tile + q) * a.pstride];
#pragma unroll
        for (int q = 0; q < 8; ++q) s += v[q];
    }
    for (; tile < a.tiles; ++tile) s += part[(long long)tile * a.pstride];
    return s;
}

// one workgroup per replica.  GRAD: the gradient (to a.dst where given) and the 4-double record; else H v to a.dst
template <bool GRAD>
__global__ __launch_bounds__(256) void sampled_combine_kernel(const SampArgs a, const int n_replicas) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    const long long r = blockIdx.x;
    double* const dst = a.dst ? a.dst + r * a.dst_stride : nullptr;
    double part = 0.0;
    for (int e = t; e < a.P; e += 256) {
        const double s = samp_combine(a, r, n_replicas, e);
        if (dst) dst[e] = s;
        part = fma(s, s, part);
    }
    if constexpr (GRAD) {
        const double gnorm = sqrt(block_sum256(part, red, t));
        if (t < kHvpRecord) {
            const float* const p = a.params + r * a.state_stride;
            const double eps_cli = (double)a.eps_cli;
            const double eps = a.off_c >= 0 ? (double)p[a.off_c] * eps_cli : eps_cli;
            const double f = samp_combine(a, r, n_replicas, a.P);
            a.out[r * a.out_stride + t] = t == 0 ? f : (t == 1 ? gnorm : (t == 2 ? eps : (double)a.rows));
        }
    }
}

// Lanczos, before step 1: f and |grad f_K| from the gradient partials, v_1 = v0 / |v0| into the basis, the state block
__global__ __launch_bounds__(256) void sampled_lanczos_init_kernel(const SampArgs a, const int n_replicas) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    const long long r = blockIdx.x;
    const int P = a.P;
    double* const state = a.ws + r * kState;
    double* const basis = a.basis + r * a.basis_stride;
    const double* const v0 = a.v0 + r * a.v0_stride;
    double part = 0.0;
    for (int e = t; e < P; e += 256) { const double s = samp_combine(a, r, n_replicas, e); part = fma(s, s, part); }
    const double gnorm = sqrt(block_sum256(part, red, t));
    const int kmax = lanczos_start(v0, basis, P, a.steps, red, t);
    if (t < kState) {
        double v = 0.0;
        if (t == 0) v = kmax > 0 ? 0.0 : 1.0;
        else if (t == 3) v = samp_combine(a, r, n_replicas, P);
        else if (t == 4) v = gnorm;
        else if (t == 5) {
            const double eps_cli = (double)a.eps_cli;
            v = a.off_c >= 0 ? (double)a.params[r * a.state_stride + a.off_c] * eps_cli : eps_cli;
        }
        state[t] = v;
    }
}

// Lanczos step j + 1 of a replica that is not done: w = the combined partials of H v_{j+1}, classical Gram-Schmidt twice, alpha, beta,
// the breakdown test, v_{j+2} into the basis.  The basis rows it reads were stored by earlier launches.
__global__ __launch_bounds__(256) void sampled_lanczos_step_kernel(const SampArgs a, const int n_replicas) {
    __shared__ double red[256], wv[kSampFlat], coef[kLanczosMaxSteps];
    const int t = threadIdx.x;
    const long long r = blockIdx.x;
    const int P = a.P, j = a.j;
    double* const state = a.ws + r * kState;
    const bool done = state[0] != 0.0;
    const double scale0 = state[2];
    __syncthreads();                                                   // every thread has read the state before thread 0 stores into it
    if (done) return;
    double* const basis = a.basis + r * a.basis_stride;
    for (int e = t; e < P; e += 256) wv[e] = samp_combine(a, r, n_replicas, e);
    __syncthreads();
    double al, be, scale = scale0;
    lanczos_orthogonalise(wv, basis, P, j, coef, red, t, al, be);
    const int k = j + 1;
    const bool stop = lanczos_next(wv, basis, P, k, a.steps < P ? a.steps : P, al, be, scale, t);
    if (t == 0) {
        state[sAlpha + j] = al; state[sBeta + j] = be;
        state[1] = (double)k; state[2] = scale;
        if (stop) state[0] = 1.0;
    }
}

// the last launch: T from the state block, then lanczos_dev.h's tail: the solve, the Ritz values and their bounds, omega, the record
__global__ __launch_bounds__(256) void sampled_lanczos_final_kernel(const SampArgs a) {
    __shared__ double mat[2 * kMatDoubles], vecs[2 * kMatDoubles];
    __shared__ double red[256], alpha[kSpectrumMaxDim], beta[kSpectrumMaxDim], rot_c[kSpectrumMaxDim], rot_s[kSpectrumMaxDim], eig[kSpectrumMaxDim];
    __shared__ int rot_mate[kSpectrumMaxDim];
    const int t = threadIdx.x;
    const long long r = blockIdx.x;
    const double* const state = a.ws + r * kState;
    double* const out = a.out + r * a.out_stride;
    const int k = (int)state[1];
    if (t < k) { alpha[t] = state[sAlpha + t]; beta[t] = state[sBeta + t]; }
    __syncthreads();
    LanczosLds s;
    s.mat = mat; s.vec = vecs; s.red = red; s.alpha = alpha; s.beta = beta;
    s.rot_c = rot_c; s.rot_s = rot_s; s.eig = eig; s.rot_mate = rot_mate;
    const RitzResult rz = lanczos_ritz(s, k, out, t);
    const double omega = lanczos_omega(a.basis + r * a.basis_stride, a.P, k, red, t);
    lanczos_head_store(out, t, k, state[3], state[4], state[5], a.rows, omega, rz);
    if (t == 12) out[kSampRecord - 2] = (double)a.samples;
    if (t == 13) out[kSampRecord - 1] = a.sig ? 1.0 : 0.0;
}

// vaek_supports_log_likelihood's predicate: float32, no hidden layers, one or two decoders, D, L <= 32, D <= 28 with two
static bool sampled_covered(const vaek_ctx* c) {
    const vaek_config& cfg = c->cfg;
    if (cfg.dtype != VAEK_F32 || cfg.n_enc_hidden != 0 || cfg.n_dec_hidden != 0) return false;
    if (c->D < 1 || c->L < 1 || c->D > kSpectrumMaxDim || c->L > kSpectrumMaxDim) return false;
    return !(cfg.sigmoid_decoder && c->D > 28);
}

// the leaf layout the kernels index by: E, b_e, K, b_d, [K_s, b_s,] epsilon_p and, under tunable_eps, epsilon
static bool sampled_layout(const vaek_ctx* c) {
    const int64_t dec = (int64_t)c->L * c->D + c->D;
    const int64_t off_p = (int64_t)(c->D + 1) * c->L + dec * (c->cfg.sigmoid_decoder ? 2 : 1);
    return c->off_epsp == off_p && (c->off_eps < 0 || c->off_eps == off_p + c->L) && c->P == off_p + c->L + (c->off_eps >= 0 ? 1 : 0) &&
           c->P < kSampFlat;
}

static int samp_tiles(int rows, int samples) { return (rows * samples + kTileCols - 1) / kTileCols; }
static int samp_pstride(const vaek_ctx* c) { return (int)((c->P + 2) & ~(int64_t)1); }
static size_t samp_workspace_bytes(const vaek_ctx* c, int n, int rows, int samples) {
    return sizeof(double) * ((size_t)n * kState + (size_t)n * samp_tiles(rows, samples) * samp_pstride(c));
}

// rows, samples and their products, for a call and for the workspace query alike
static int samp_check_size(const char* who, int32_t n, int32_t rows, int32_t samples) {
    return check_sampled_columns(who, n, rows, samples, kSampReplicaColumnsLog2, kSampMaxColumns, "vaek_sampled_elbo_hessian_max_columns");
}

static int sampled_common(const char* who, const EvalDesc& d, const SampleSource& x, int record, const char* record_query, vaek_ctx* ctx,
                          const float* params, int32_t kind, const float* A, int32_t dd, int32_t did, int32_t pad, float var_added, uint32_t x_tag,
                          uint32_t z_tag, void* workspace, SampArgs* a) {
    EvalRules r{};
    r.covered = ctx && sampled_covered(ctx) && sampled_layout(ctx);
    r.needs = "needs a float32 linear VAE (no hidden layers) with one or two decoders and D, L <= 32, D <= 28 with two decoders (see "
              "vaek_supports_sampled_elbo_hessian)";
    r.rows_min = 1; r.rows_cap = kLogLikMaxRows; r.rows_query = "vaek_log_likelihood_max_rows";
    r.records = 1; r.record_len = record; r.record_query = record_query;
    r.draws = true; r.kind = kind; r.A = A; r.dd = dd; r.did = did; r.pad = pad; r.x_tag = x_tag;
    r.has_z_tag = true; r.z_tag = z_tag;
    r.workspace = workspace; r.ws_align = 16; r.ws_query = "vaek_sampled_elbo_hessian_workspace_bytes";
    if (int rc = check_eval(who, ctx, params, d, r)) return rc;
    if (int rc = samp_check_size(who, d.n, d.rows, x.samples)) return rc;
    if (int rc = check_sample_source(who, x, d.rows, ctx->L)) return rc;
    a->params = params; a->state_stride = d.state_stride;
    a->x_seeds = reinterpret_cast<const unsigned long long*>(d.x_seeds); a->x_steps = d.x_steps;
    a->z_seeds = reinterpret_cast<const unsigned long long*>(x.z_seeds); a->z_steps = x.z_steps;
    a->x = d.rows_ptr; a->x_stride = d.rows_stride;
    a->xi = x.xi; a->xi_stride = x.xi_stride;
    a->rows = d.rows; a->samples = x.samples; a->D = ctx->D; a->L = ctx->L; a->P = (int)ctx->P; a->sig = ctx->cfg.sigmoid_decoder ? 1 : 0;
    a->off_p = (int)ctx->off_epsp; a->off_c = (int)ctx->off_eps;
    a->eps_cli = ctx->cfg.eps_cli; a->z_tag = z_tag;
    a->ws = static_cast<double*>(workspace); a->tiles = samp_tiles(d.rows, x.samples); a->pstride = samp_pstride(ctx);
    fill_rows_source(&a->gen, &a->a_stride, ctx, d.rows, d.explicit_rows(), kind, A, dd, did, pad, var_added, x_tag, d.a_stride);
    return VAEK_OK;
}

template <bool TAN>
static int samp_launch_tiles(const char* label, const SampArgs& a, int n, hipStream_t st) {
    static thread_local PerDeviceOnce attr_set;
    VAEK_HIP_CHECK(set_max_dynamic_lds(attr_set, sampled_tile_kernel<TAN>, kSampLds));
    {
        ProfScope ps(label, st);
        launch_k(ps, sampled_tile_kernel<TAN>, dim3((unsigned)a.tiles, (unsigned)n), dim3(256), kSampLds, st, a, n);
    }
    VAEK_HIP_CHECK(hipGetLastError());
    return VAEK_OK;
}

template <class Kernel, class... Args>
static int samp_launch_replicas(const char* label, Kernel fn, int n, hipStream_t st, Args... args) {
    {
        ProfScope ps(label, st);
        launch_k(ps, fn, dim3((unsigned)n), dim3(256), 0, st, args...);
    }
    VAEK_HIP_CHECK(hipGetLastError());
    return VAEK_OK;
}

}  // namespace vaek

using namespace vaek;

extern "C" {

int vaek_supports_sampled_elbo_hessian(const vaek_ctx* ctx, int32_t kind, int32_t* yes) {
    if (!ctx || !yes) { set_error("vaek_supports_sampled_elbo_hessian: null argument"); return VAEK_ERR_INVALID; }
    *yes = kind >= 0 && kind <= 2 && sampled_covered(ctx) && sampled_layout(ctx) ? 1 : 0;
    return VAEK_OK;
}

int vaek_sampled_elbo_hessian_max_columns(void) { return kSampMaxColumns; }
int vaek_sampled_elbo_hessian_record_len(void) { return kSampRecord; }

int vaek_sampled_elbo_hessian_workspace_bytes(const vaek_ctx* ctx, int32_t n, int32_t rows, int32_t samples, size_t* bytes) {
    const char* who = "vaek_sampled_elbo_hessian_workspace_bytes";
    if (!ctx || !bytes) { set_error("%s: null argument", who); return VAEK_ERR_INVALID; }
    if (int rc = check_replica_count(who, n)) return rc;
    if (int rc = check_row_count(who, rows, 1, kLogLikMaxRows, "vaek_log_likelihood_max_rows")) return rc;
    if (int rc = samp_check_size(who, n, rows, samples)) return rc;
    if (!sampled_covered(ctx) || !sampled_layout(ctx)) {
        set_error("%s: an unsupported context (see vaek_supports_sampled_elbo_hessian)", who);
        return VAEK_ERR_INVALID;
    }
    *bytes = samp_workspace_bytes(ctx, n, rows, samples);
    return VAEK_OK;
}

int vaek_sampled_elbo_hvp_replicas(vaek_ctx* ctx, const float* params, const vaek_sampled_elbo_hvp* hp, int32_t kind, const float* A, int32_t dd,
                                   int32_t did, int32_t pad, float var_added, uint32_t x_tag, uint32_t z_tag, void* workspace, void* stream) {
    const char* who = "vaek_sampled_elbo_hvp_replicas";
    ProfBind pb(ctx);
    SampArgs a{};
    const EvalDesc d = describe(hp);
    if (int rc = sampled_common(who, d, sample_source(d, hp), kHvpRecord, "vaek_elbo_hvp_record_len", ctx, params, kind, A, dd, did, pad, var_added,
                                x_tag, z_tag, workspace, &a))
        return rc;
    if (int rc = check_hvp_buffers(who, hp, ctx->P, true)) return rc;
    const int64_t P = ctx->P;
    const int n = hp->n;
    hipStream_t st = (hipStream_t)stream;
    a.out = hp->out; a.out_stride = hp->out_stride;
    a.dst = hp->grad; a.dst_stride = hp->grad_stride;
    if (int rc = samp_launch_tiles<false>("sampled_elbo_grad_tiles", a, n, st)) return rc;
    if (int rc = samp_launch_replicas("sampled_elbo_grad_combine", sampled_combine_kernel<true>, n, st, a, n)) return rc;
    for (int i = 0; i < hp->nvec; ++i) {
        a.dir = hp->v + (int64_t)i * P; a.dir_stride = hp->v_stride;
        a.dst = hp->hv + (int64_t)i * P; a.dst_stride = hp->hv_stride;
        if (int rc = samp_launch_tiles<true>("sampled_elbo_hvp_tiles", a, n, st)) return rc;
        if (int rc = samp_launch_replicas("sampled_elbo_hvp_combine", sampled_combine_kernel<false>, n, st, a, n)) return rc;
    }
    return VAEK_OK;
}

int vaek_sampled_elbo_hessian_lanczos_replicas(vaek_ctx* ctx, const float* params, const vaek_sampled_elbo_hessian* hs, int32_t kind,
                                               const float* A, int32_t dd, int32_t did, int32_t pad, float var_added, uint32_t x_tag,
                                               uint32_t z_tag, void* workspace, void* stream) {
    const char* who = "vaek_sampled_elbo_hessian_lanczos_replicas";
    ProfBind pb(ctx);
    SampArgs a{};
    const EvalDesc d = describe(hs);
    if (int rc = sampled_common(who, d, sample_source(d, hs), kSampRecord, "vaek_sampled_elbo_hessian_record_len", ctx, params, kind, A, dd, did, pad,
                                var_added, x_tag, z_tag, workspace, &a))
        return rc;
    if (int rc = check_lanczos_buffers(who, hs, ctx->P)) return rc;
    const int64_t P = ctx->P;
    const int n = hs->n;
    hipStream_t st = (hipStream_t)stream;
    a.out = hs->out; a.out_stride = hs->out_stride;
    a.v0 = hs->v0; a.v0_stride = hs->v0_stride; a.basis = hs->basis; a.basis_stride = hs->basis_stride; a.steps = hs->steps;
    if (int rc = samp_launch_tiles<false>("sampled_elbo_grad_tiles", a, n, st)) return rc;
    if (int rc = samp_launch_replicas("sampled_elbo_lanczos_init", sampled_lanczos_init_kernel, n, st, a, n)) return rc;
    a.use_flag = 1;
    for (int j = 0; j < hs->steps; ++j) {
        a.j = j;
        a.dir = hs->basis + (int64_t)j * P; a.dir_stride = hs->basis_stride;
        if (int rc = samp_launch_tiles<true>("sampled_elbo_hvp_tiles", a, n, st)) return rc;
        if (int rc = samp_launch_replicas("sampled_elbo_lanczos_step", sampled_lanczos_step_kernel, n, st, a, n)) return rc;
    }
    return samp_launch_replicas("sampled_elbo_lanczos_final", sampled_lanczos_final_kernel, n, st, a);
}

}  // extern "C"
