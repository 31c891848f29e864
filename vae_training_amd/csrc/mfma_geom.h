// Block geometry of the matrix-core linear-VAE kernels (fused_mfma.hip, linear_resident.hip) and the table of shapes they are
// instantiated for.
#pragma once
#include <hip/hip_runtime.h>

#include "vaek_internal.h"

namespace vaek {

using f32x4 = __attribute__((ext_vector_type(4))) float;

// ---- block geometry of a feature axis of padded length N (<= 32) ----------------------------------
template <int N>
struct Axis {
    static constexpr int NB = (N + 15) / 16;
    static constexpr bool full(int b) { return N - 16 * b >= 16; }
    static constexpr int rem(int b) { return N - 16 * b >= 16 ? 16 : N - 16 * b; }
    static constexpr int nreg(int b) { return full(b) ? 4 : (rem(b) + 3) / 4; }     // registers = k-steps used
    // feature held by lane group g, register r of block b
    static __device__ __forceinline__ constexpr int feat(int b, int g, int r) { return full(b) ? 16 * b + 4 * g + r : 16 * b + 4 * r + g; }
};

template <int DP, int LP, bool SIG>
struct MGeom {
    using AD = Axis<DP>;
    using AL = Axis<LP>;
    static constexpr int TILE = 256, NW = 4, NSUB = 4;
    static constexpr int TS = TILE + 2;
    static constexpr int NB1 = DP * (SIG ? 2 : 1);
    // A ROW OF ONES behind the samples rows / behind the x rows of the operand image, where the last 16-row block of that
    // operand has a spare row anyway (LP resp. DP not a multiple of 16): [samples | 1]^T dy and [x | 1]^T dmu then deliver
    // the bias gradients as one more output row of MFMAs that run regardless -- no per-sample column-sum adds in the
    // chain, no DPP row reductions and LDS traffic for them on the tail.
    static constexpr int ONE1 = LP % 16 != 0 ? 1 : 0, ONE2 = DP % 16 != 0 ? 1 : 0;
    static constexpr int FS = 0, FX = FS + LP + ONE1, FDY = FX + DP + ONE2, FDM = FDY + NB1, NF = FDM + LP;
    static constexpr int IB1 = (LP + 15) / 16, JB1 = (NB1 + 15) / 16, IB2 = (DP + 15) / 16, JB2 = (LP + 15) / 16;
    static constexpr int NBLK = IB1 * JB1 + IB2 * JB2;
    static constexpr int NF_PAD = FDM + JB2 * 16;
    static constexpr int T_FLOATS = NF_PAD * TS;
    // cross-wave reduction image: MFMA blocks, then column sums [dy | dys | dmu | gz], then 3 scalars
    static constexpr int NCS = NB1 + 2 * LP;
    static constexpr int R_PER_WAVE = NBLK * 256 + NCS + 4;
    static constexpr int R_FLOATS = NW * R_PER_WAVE;
    static constexpr int LDS_FLOATS = (T_FLOATS > R_FLOATS ? T_FLOATS : R_FLOATS);
    // the flat gradient of the padded shape: every parameter, then the kExtra loss slots; thread t of 256 owns t, t + 256, ...
    static constexpr int PMAX = DP * LP + LP + (SIG ? 2 : 1) * (LP * DP + DP) + LP + 1 + kExtra;
    static constexpr int NOUT = (PMAX + 255) / 256;
};

// (DP, LP, SIG, EXACT) of every instantiation; a context takes the smallest that holds it (EXACT: only its own D, L)
#ifndef VAEK_FUSED_ONLY_M
#define VAEK_MFMA_SHAPES(X)                                                                          \
    /* exact shapes of seed_linpadding_expts.sh (the metric's configuration first) */               \
    X(12, 20, 0, 1) X(20, 20, 0, 1) X(20, 10, 0, 1)                                                  \
    /* zero-padded coverage of every other D, L <= 32 */                                             \
    X(16, 16, 0, 0) X(32, 32, 0, 0) X(12, 4, 0, 0)                                                   \
    /* sigmoid dataset (two decoders): sigmoid_vae_padding_expts.sh shapes */                        \
    X(8, 8, 1, 0) X(12, 12, 1, 0) X(16, 16, 1, 0) X(20, 8, 1, 0) X(24, 16, 1, 0) X(28, 24, 1, 1)
// ... and of the evaluation kernels (linear_stats / linear_loglik / cov_spectrum / exact_loglik), which keep no MGeom image in LDS and
// so also hold the largest two-decoder shape
#define VAEK_EVAL_SHAPES(X) VAEK_MFMA_SHAPES(X) X(32, 32, 1, 0)
#else
#define VAEK_MFMA_SHAPES(X) X(12, 20, 0, 1)
#define VAEK_EVAL_SHAPES(X) VAEK_MFMA_SHAPES(X)
#endif

// The row of a variant table built from VAEK_MFMA_SHAPES (fields dp, lp, sig, exact) that a context takes: the smallest padded shape
// that holds it and whose `bytes` field fits the LDS of a CU.
constexpr size_t kLdsLimit = 160 * 1024;
template <class V, size_t N>
const V* pick_shape(const V (&table)[N], const vaek_ctx* c, size_t V::*bytes) {
    const V* best = nullptr;
    for (const V& v : table) {
        if (v.sig != (c->cfg.sigmoid_decoder ? 1 : 0) || v.dp < c->D || v.lp < c->L || v.*bytes > kLdsLimit) continue;
        if (v.exact && (v.dp != c->D || v.lp != c->L)) continue;
        if (!best || v.dp * v.lp < best->dp * best->lp) best = &v;
    }
    return best;
}
// ... and every row can be picked: MGeom<32, 32, true> needs 165,120 bytes, so the table has no such row, and a two-decoder shape with
// D > 24 or L > 16 other than 28 x 24 has no matrix-core kernel
#define VAEK_MFMA_FITS(DP, LP, SIG, EXACT) \
    static_assert(sizeof(float) * MGeom<DP, LP, (SIG) != 0>::LDS_FLOATS <= kLdsLimit, "a matrix-core shape no context can take");
VAEK_MFMA_SHAPES(VAEK_MFMA_FITS)
#undef VAEK_MFMA_FITS

}  // namespace vaek
