// The chain core of the matrix-core linear-VAE kernels: everything fused_linear_mfma_kernel (fused_mfma.hip: the multi-workgroup
// step and its self-finalizing SINGLE form) and linear_resident_kernel (linear_resident.hip: the step as the body of a loop) have
// in common, once.  The operand layout is described at the top of fused_mfma.hip, the geometry in mfma_geom.h.
//
// The core is TEXT, included into both kernels in the order they run it (the precedent is mlp3_chain_body.inc):
//
//     mfma_chain_srcoff.inc     where each flat-gradient output of a thread sits in the reduction image
//     mfma_chain_operands.inc   operand predicates, weight operands, per-lane constants (the kernel defines what a fetch is)
//     mfma_chain_zero.inc       accumulators and column sums, zeroed
//     mfma_chain_tile.inc       mu, samples, y (+ sigmoid head), residual / loss / dy, g, dmu, the T image, both reduction GEMMs
//     mfma_chain_reduce.inc     rowsum / rows4 (DPP), accumulators and sums into the R image, fetch_cs, batch_sum_k
//     mfma_chain_grad.inc       the closed-form gradient of the self-finalizing tail
//
// Text and not functions: as forced-inline members over structs of the register arrays the same lines give different device text
// in all 78 instantiations, and with it different last bits wherever the compiler pairs the fused multiply-add of an a*b + c*d
// expression differently (s_deps in the tile, v in adam_apply_f; profiles/mfma_chain.txt).  As text both kernels compile to the
// device code they had with the lines written out twice, which tools/kernel_diff.py shows against any earlier tree.
//
// What a kernel keeps to itself is WHERE its operands come from and in which order it asks for them: the fused kernel loads x, the
// weights, z1, z2 from HBM in that order, every load unconditional and the zeroing selects after the last of them; the resident
// kernel reads a staged batch and an LDS image of the parameter vector.  The rule of linear_resident.hip holds for every piece: no
// pointer to parameters is const __restrict__ (mfma_chain_grad.inc reads the other threads' parameters through the plain `pother`).
#pragma once
#include "mfma_geom.h"

// One 16-feature block `b` of axis AX of one sample's row `p` (n features wide) into dst[4], for the lane group g of the including
// kernel: a float4 when the block is full and the width a multiple of 4 (`vec`), scalars otherwise.  Every load is UNCONDITIONAL,
// from a clamped column (the kernel clamps the row): a sample past the batch end reads row B-1 again and a padded column reads
// column n-1 -- finite values whose every contribution is already masked downstream (rr, dmu, mu^2 by `valid`; padded columns by
// zero weights / zero e^{lv/2} and by rows of the gradient image nobody reads), and nothing is zeroed afterwards.  With the loads
// under `if (valid)` hipcc merged each conditionally loaded float4 into its zero-initialised registers INSIDE the branch, i.e. put
// an `s_waitcnt vmcnt` into every sub-tile's block, and a zeroing pass after the loads waits for all of them.  Now all 56 loads of a
// wave of the metric's kernel (24 parameter, 32 input) leave before the first wait.  Measured: 8.76 -> 8.64 us per launch only --
// the load phase is bandwidth-, not latency-bound, and at 260 VGPRs hipcc still copies the z1 / z2 registers away early enough
// that the first products wait for ~3/4 of the bytes.
// (_VEC and _ELT are its two halves, for a kernel that fills two arrays block by block in its own issue order.)
#define VAEK_LOAD_BLOCK_VEC(AX, dst, p, b, n)                                                                    \
    do {                                                                                                         \
        const float4 u_ = *reinterpret_cast<const float4*>((p) + min(AX::feat(b, g, 0), (n) - 4));               \
        (dst)[0] = u_.x; (dst)[1] = u_.y; (dst)[2] = u_.z; (dst)[3] = u_.w;                                      \
    } while (0)
#define VAEK_LOAD_BLOCK_ELT(AX, dst, p, b, n, r) (dst)[r] = (r) < AX::nreg(b) ? (p)[min(AX::feat(b, g, r), (n) - 1)] : 0.f
#define VAEK_LOAD_BLOCK(AX, dst, p, b, n, vec)                                                                   \
    do {                                                                                                         \
        if (AX::full(b) && (vec)) {                                                                              \
            VAEK_LOAD_BLOCK_VEC(AX, dst, p, b, n);                                                               \
        } else {                                                                                                 \
            _Pragma("unroll") for (int r_ = 0; r_ < 4; ++r_) VAEK_LOAD_BLOCK_ELT(AX, dst, p, b, n, r_);          \
        }                                                                                                        \
    } while (0)
