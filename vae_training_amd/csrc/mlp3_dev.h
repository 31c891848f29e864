// The forward-only matrix-core Dense chain of the three-hidden-layer MLP evaluation kernels (mlp3_loglik.hip, mlp3_stats.hip): the
// [unit][column] LDS image and its bank swizzle, one Dense layer over CB column blocks of 16 and the four-layer relu stack.  ONE text:
// mlp3_loglik.hip's header describes the operand scheme.
//
// LDS images for NC >= 32.  An operand read is lane (n, kq) -> element (k0 + kq, 16 cb + n), a dword read whose banks are taken
// modulo 32 within each 32-lane half (kq 0 | 1, 2 | 3); with a row pitch of NC >= 32 floats both k-rows of a half would share 16
// banks.  The epilogue's store is lane (n, kq) -> element (16 blk + 4 kq + r, 16 cb + n), the same problem.  So element (k, c) lives
// at k NC + (c ^ 16 s(k)), s(k) = (k ^ (k >> 2)) & 1: a read's two rows differ in bit 0 of k, a store's two rows in bit 2, and s
// tells both apart, so neither conflicts.  Only the place changes, never the arithmetic.
//
// The weights are read one dword per lane and product (16 lanes of a unit block read 64 contiguous bytes), any alignment: there is
// no stride rule.
#pragma once
#include "eval_dev.h"

namespace vaek {

using ml_f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int ML_NT = 256;                   // threads of the chain kernels
constexpr int ML_W = 256;                    // widest hidden layer
constexpr int ML_F = 32;                     // widest D / L

struct Ml3Net { int n_in[4], n_out[4], w_off[4]; };        // one stack's Dense layers

// float index of element (k, c) of a [unit][NC] image
template <int NC>
__device__ __forceinline__ int ml_at(int k, int c) {
    return k * NC + (NC >= 32 ? (c ^ (((k ^ (k >> 2)) & 1) << 4)) : c);
}

// out(m, column) = sum_{k < K} kernel[k][m] * in(k, column), m < M, handed to epi(m, column, sum, bias[m]); kernel = P + w_off, row
// pitch M, bias behind it.  m3_dense's forward form (fused_mlp3.hip) over CB column blocks: wave w owns the 16-unit blocks w, w + 4,
// .. (NB of them), the operands of 8 k-steps (a chunk) are fetched while the previous chunk is multiplied, every load is
// unconditional at a clamped index and k >= K is zeroed on the LDS operand, so a clamped weight meets a zero.  A unit block past M
// multiplies clamped rows and stores nothing.
template <int NB, int CB, typename Epi>
__device__ __forceinline__ void ml_dense(const float* __restrict__ P, int w_off, int M, int K, const float* in, int wave, int lane, Epi&& epi) {
    constexpr int NC = 16 * CB;
    const int n = lane & 15, kq = lane >> 4;
    const float* const bias = P + w_off + K * M;
    int wrow[NB];
    float bia[NB][4];
#pragma unroll
    for (int bi = 0; bi < NB; ++bi) {
        wrow[bi] = w_off + min(16 * (wave + 4 * bi) + n, M - 1);
#pragma unroll
        for (int r = 0; r < 4; ++r) bia[bi][r] = bias[min(16 * (wave + 4 * bi) + 4 * kq + r, M - 1)];
    }
    ml_f32x4 acc[NB][CB];
#pragma unroll
    for (int bi = 0; bi < NB; ++bi)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) acc[bi][cb] = ml_f32x4{0.f, 0.f, 0.f, 0.f};
    const int nchunks = (K + 31) / 32;
    float av0[NB][8], av1[NB][8], bv0[CB][8], bv1[CB][8];
    auto fetch = [&](float (&av)[NB][8], float (&bv)[CB][8], int c) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = min(32 * c + 4 * j + kq, K - 1);
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) bv[cb][j] = in[ml_at<NC>(k, 16 * cb + n)];
#pragma unroll
            for (int bi = 0; bi < NB; ++bi) av[bi][j] = P[wrow[bi] + k * M];
        }
    };
    auto mult = [&](float (&av)[NB][8], float (&bv)[CB][8], int c) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (32 * c + 4 * j < K) {            // wave-uniform: a k-step wholly past K would add zeros (K = 200: 6 of the last chunk's 8)
                const bool live = 32 * c + 4 * j + kq < K;
#pragma unroll
                for (int cb = 0; cb < CB; ++cb) {
                    const float b = live ? bv[cb][j] : 0.f;
#pragma unroll
                    for (int bi = 0; bi < NB; ++bi) acc[bi][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[bi][j], b, acc[bi][cb], 0, 0, 0);
                }
            }
        }
    };
    fetch(av0, bv0, 0);
    for (int c = 0; c < nchunks; c += 2) {
        fetch(av1, bv1, c + 1);                  // past the end: clamped loads, never multiplied
        __builtin_amdgcn_sched_barrier(0);
        mult(av0, bv0, c);
        __builtin_amdgcn_sched_barrier(0);
        fetch(av0, bv0, c + 2);
        __builtin_amdgcn_sched_barrier(0);
        if (c + 1 < nchunks) mult(av1, bv1, c + 1);
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int bi = 0; bi < NB; ++bi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = 16 * (wave + 4 * bi) + 4 * kq + r;
            if (m < M) {
#pragma unroll
                for (int cb = 0; cb < CB; ++cb) epi(m, 16 * cb + n, acc[bi][cb][r], bia[bi][r]);
            }
        }
}

// the four Dense layers of one stack: img0 -> img1 -> img0 -> img1 -> img0, relu after the first three; ends behind a barrier
template <int NC>
__device__ __forceinline__ void ml_stack(const float* __restrict__ P, const Ml3Net& net, float* img0, float* img1, int wave, int lane) {
    constexpr int CB = NC / 16;
#pragma unroll 1
    for (int li = 0; li < 4; ++li) {
        const float* const in = (li & 1) ? img1 : img0;
        float* const out = (li & 1) ? img0 : img1;
        const bool relu = li != 3;
        auto epi = [&](int m, int c, float v, float b) { v += b; out[ml_at<NC>(m, c)] = relu ? fmaxf(v, 0.f) : v; };
        const int n_in = net.n_in[li], n_out = net.n_out[li], w_off = net.w_off[li];
        if (n_out <= 64) ml_dense<1, CB>(P, w_off, n_out, n_in, in, wave, lane, epi);
        else ml_dense<4, CB>(P, w_off, n_out, n_in, in, wave, lane, epi);
        __syncthreads();
    }
}

// a stack's Dense layers as the kernels take them (host)
static inline void ml3_net(const Net& net, Ml3Net* out) {
    for (int i = 0; i < 4; ++i) { out->n_in[i] = net.layers[i].n_in; out->n_out[i] = net.layers[i].n_out; out->w_off[i] = (int)net.layers[i].w_off; }
}

}  // namespace vaek
