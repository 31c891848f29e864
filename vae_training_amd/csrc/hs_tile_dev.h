// Device text shared by the bf16-storage kernels (gemm_bf16s.hip, gemm_skinny16.hip, conv_bf16.hip): the vector types, the
// LDS-DMA piece, the counted waits, and the ONE tile core of the NT-shaped kernels (hs_nt_kernel, hs_nt_p_kernel,
// hs_conv_kernel): geometry, bank swizzle, staging positions, fragment addresses, k-tile product, ring step, bf16 epilogue.
// Why storage, why inline-assembly LDS-DMA and why a ring: the head of gemm_bf16s.hip.  DESIGN 3.3.
//
// A new NT-shaped kernel supplies four things around this text: its tile walk (m0, n0), the global address of each staging
// position (row, column) -- HsTile says which row and which swizzled column thread t loads in pass i and where it lands --
// the loop skeleton (prologue of NS - 1 stages; per k-tile: T::wait_tile, stage into `fill`, acc.multiply from `slot`,
// T::advance), and its epilogue.  What it must keep:
//  * P loads per k-tile and wave, all A passes then all B passes, and nothing else between a stage and its wait that the wait
//    arithmetic does not account for (older operations are harmless: vmcnt retires in issue order);
//  * the barrier of the ring step is the raw s_barrier -- __syncthreads() would put a full s_waitcnt in front of it and drain the ring;
//  * the swizzle comes from swz() alone: on the SOURCE address at staging (the LDS side of a global_load_lds is lane-linear), on
//    the read address at the fragment.
#pragma once
#include "vaek_internal.h"

namespace vaek {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using bf16x4 = __attribute__((ext_vector_type(4))) __bf16;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
typedef __attribute__((address_space(3))) void lds_void_t;
typedef const __attribute__((address_space(1))) void glb_void_t;

// 16 bytes per lane global -> LDS; the LDS side is wave-uniform base + 16 * lane.  In inline assembly: through
// __builtin_amdgcn_global_load_lds hipcc knows that LDS is being written and puts s_waitcnt vmcnt(0) in front of the next LDS
// read it cannot tell apart -- in every kernel of gemm_bf16s.hip that was the operand reads of the k-tile being multiplied, RIGHT
// BEHIND the issue of the next k-tile's loads: the ring never overlapped a load with a product (ISA: "8 x global_load_lds,
// s_waitcnt vmcnt(0), ds_read_b128 ..."; the ablation found loads and MFMAs additive and every ring depth equally fast; the
// skinny backward kernel's ring was drained four times per block, 36 us per launch).  Every wait on these loads is the kernels'
// own counted one (wait_tiles) in front of a barrier.
__device__ __forceinline__ void glds16(const void* gsrc, void* lds_wave_base) {
    const unsigned m0v = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(size_t)(lds_void_t*)lds_wave_base);
    _Pragma("clang diagnostic push") _Pragma("clang diagnostic ignored \"-Winline-asm\"")      // (M0 on the clobber list: it is what the LDS-DMA takes its LDS address from)
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(gsrc), "s"(m0v) : "memory", "m0");
    _Pragma("clang diagnostic pop")
}
__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {
    const bf16x2 v = {(__bf16)lo, (__bf16)hi};
    return __builtin_bit_cast(unsigned, v);
}
// bf16 -> f32 is a 16-bit shift: the two halves of a packed pair
__device__ __forceinline__ float bf16_lo(unsigned u) { return __builtin_bit_cast(float, u << 16); }
__device__ __forceinline__ float bf16_hi(unsigned u) { return __builtin_bit_cast(float, u & 0xffff0000u); }

// Counted waits: s_waitcnt vmcnt(N) returns once at most N of this wave's vector-memory operations are still outstanding
// (they retire in issue order), i.e. "everything up to tile kt has landed, the `newer` younger tiles may stay in flight".
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
template <int P, int MAXT> __device__ __forceinline__ void wait_tiles(int newer) {       // P loads per tile, newer in [0, MAXT]
    static_assert(P * MAXT <= 63, "vmcnt is a 6-bit counter");
    if constexpr (MAXT == 0) wait_vmcnt<0>();
    else if (newer >= MAXT) wait_vmcnt<P * MAXT>();
    else wait_tiles<P, MAXT - 1>(newer);
}

enum { HS_FWD = 0, HS_DX = 1 };
struct HsArgs {
    const __bf16* A; const __bf16* Bt; __bf16* C;   // A [M, K] (lda), Bt [N, K] (ldb), C [M, N] (ldc); K, N multiples of 64
    int M, N, K, lda, ldb, ldc;
    const float* bias; int relu;                    // FWD
    const __bf16* aux;                              // DX: relu-mask source [M, ldc] (the layer's bf16 input), or nullptr
};

// The BM x BN output tile of a workgroup of WM x WN waves, multiplied from a ring of NS stages of BK-deep k-tiles.
//
// LDS image of an R-row x BK-k operand tile (BK = 64 / 32): 128- / 64-byte rows, 16-byte chunk c of row r at chunk position
// c ^ f(r), f = (r >> 1) & 7 / (r >> 2) & 3: the 16 lanes ds_read_b128 services together (rows {0-3,12-15,20-27} /
// {4-11,16-19,28-31} of a fragment, one chunk column) then cover all 16 chunk slots of the 256-byte bank row.  A stage is the A
// image followed by the B image.
//
// Ring of NS stages: a k-tile's MFMAs take ~0.25 us per wave, an HBM / L2 round trip under load 1-3 us, so ONE tile of
// prefetch (the first version: 2.8 us per k-tile) is a latency chain; NS - 1 tiles are in flight while one is multiplied.
template <int BM, int BN, int WM, int WN, int BK, int NS>
struct HsTile {
    static constexpr int NTH = 64 * WM * WN;
    static constexpr int TM = BM / WM / 32, TN = BN / WN / 32;      // 32 x 32 fragments per wave
    static constexpr int RB = 2 * BK, CPR = BK / 8;                 // row bytes, 16-byte chunks per row
    static constexpr int A_BYTES = BM * RB, B_BYTES = BN * RB, BUF = A_BYTES + B_BYTES;
    static constexpr int A_PASSES = BM * CPR / NTH, B_PASSES = BN * CPR / NTH, P = A_PASSES + B_PASSES;      // P: loads per k-tile and wave
    static_assert(BM * CPR % NTH == 0 && BN * CPR % NTH == 0 && B_PASSES >= 1, "whole staging passes");
    static_assert(BK == 64 || BK == 32, "k-tile depth");

    static __device__ __forceinline__ int swz(int row) { return BK == 64 ? (row >> 1) & 7 : (row >> 2) & 3; }

    // staging, thread t in pass i (of either operand): the tile row it loads, the k-column (in elements) of its 16-byte chunk with
    // the swizzle applied, and where the wave's 1 KB piece lands in the operand's image
    static __device__ __forceinline__ void stage_pos(int t, int i, int& row, int& col) {
        const int p = i * NTH + t;
        row = p / CPR; col = ((p % CPR) ^ swz(row)) * 8;
    }
    static __device__ __forceinline__ int stage_dst(int wv, int i) { return (i * NTH + wv * 64) * 16; }

    // fragment addresses within a stage: lane (r = lane & 31, h = lane >> 5) reads chunk 2 s + h of its row for k-step s
    struct Frag {
        int a_lo, a_x6, b_lo, b_x6;
        __device__ __forceinline__ Frag(int wm, int wn, int lane) {
            const int r = lane & 31, h = lane >> 5;
            const int arow = wm * (BM / WM) + r, brow = wn * (BN / WN) + r;
            const int ax = swz(arow), bx = swz(brow);
            a_lo = arow * RB + ((h ^ ax) & 1) * 16; a_x6 = (ax & 6) * 16;
            b_lo = brow * RB + ((h ^ bx) & 1) * 16 + A_BYTES; b_x6 = (bx & 6) * 16;
        }
    };

    // the wave's accumulators.  Operands swapped in the MFMA: D[n][m] -- lane & 31 = output row m, registers = columns n
    struct Acc {
        f32x16 v[TM][TN];
        __device__ __forceinline__ void zero() {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int q = 0; q < 16; ++q) v[i][j][q] = 0.f;
        }
        __device__ __forceinline__ void multiply(const char* base, const Frag& f) {      // += the k-tile staged at base
#pragma unroll
            for (int s = 0; s < BK / 16; ++s) {
                bf16x8 fa[TM], fb[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) fa[i] = *reinterpret_cast<const bf16x8*>(base + f.a_lo + i * 32 * RB + ((32 * s) ^ f.a_x6));
#pragma unroll
                for (int j = 0; j < TN; ++j) fb[j] = *reinterpret_cast<const bf16x8*>(base + f.b_lo + j * 32 * RB + ((32 * s) ^ f.b_x6));
#if defined(VAEK_HS_ABLATE) && (VAEK_HS_ABLATE & 1)      // diagnostic (tools/hs_ablate.sh): no MFMAs, operands kept alive
#pragma unroll
                for (int i = 0; i < TM; ++i) asm volatile("" ::"v"(fa[i]));
#pragma unroll
                for (int j = 0; j < TN; ++j) asm volatile("" ::"v"(fb[j]));
#else
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        v[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb[j], fa[i], v[i][j], 0, 0, 0);
#endif
            }
        }
    };

    // The ring step of k-tile q: this wave's share of it has landed (`left` = how many tiles follow it in the stream; at most
    // min(NS - 2, left) of them stay in flight), then the barrier: everyone's share has, and everyone is done reading tile q - 1,
    // whose slot (`fill`) the caller now stages the tile NS - 1 ahead into.
    static __device__ __forceinline__ void wait_tile(int left) {
        wait_tiles<P, NS - 2>(min(NS - 2, left));
        __builtin_amdgcn_s_barrier();
    }
    // ring positions, two ints of the kernel: `slot` (from 0) holds the k-tile being multiplied, `fill` (from NS - 1) the one to load
    static __device__ __forceinline__ void advance(int& slot, int& fill) {
        slot = slot + 1 == NS ? 0 : slot + 1;
        fill = fill + 1 == NS ? 0 : fill + 1;
    }

    // bias of the wave's TN x 32 columns from nbase, as the epilogue's registers own them
    static __device__ __forceinline__ void load_bias(const float* bias, int nbase, int lane, float4 (&bias4)[TN][4]) {
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) bias4[j][q] = *reinterpret_cast<const float4*>(bias + nbase + j * 32 + 8 * q + 4 * (lane >> 5));
    }
};

// The bf16 epilogue of the NT kernels for the wave whose rows start at mbase and whose columns at nbase < N (N is a multiple of 64
// = the wave's column span, so the caller's test is wave-uniform): register q of tile (i, j) = C[mbase + 32 i + r][nbase + 32 j +
// (q & 3) + 8 (q >> 2) + 4 h].  FWD: + bias (bias4, T::load_bias), relu as one v_max with a uniform floor -- no branch per value;
// DX: relu' from the layer's bf16 input, prefetched by the caller (PRE: pmask[(i TN + j) 2 + u]) or loaded here.  With one
// v_permlane32_swap per dword a lane stores 16 bytes, row and wave 128 contiguous bytes.
// Args: `const HsArgs` (a copy) from a kernel that never takes its argument's address -- through a reference the stores to C may
// alias g's fields for all the compiler knows, and it forms every store address anew (hs_nt_kernel: 100-470 bytes, 1-4 us per
// launch, profiles/hs_tile_core.txt) --, `const HsArgs&` from the persistent kernel, whose lambdas hold g by reference anyway.
template <int EPI, class T, bool PRE, class Args>
__device__ __forceinline__ void hs_nt_epilogue(Args g, const typename T::Acc& acc, int mbase, int nbase, int lane,
                                               const float4 (&bias4)[T::TN][4], const uint4* pmask) {
    constexpr int TM = T::TM, TN = T::TN;
    const int r = lane & 31, h = lane >> 5;
    const float floor_v = g.relu ? 0.f : -__builtin_huge_valf();
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int m = mbase + i * 32 + r;
        const bool row_ok = m < g.M;
        const long long rowoff = (long long)(row_ok ? m : g.M - 1) * g.ldc;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int nj = nbase + j * 32;
            // after the swaps lanes 0-31 own columns [8 qq, 8 qq + 8), lanes 32-63 [8 qq + 8, 8 qq + 16), qq = 0, 2
            uint4 mask[2];
            if (EPI == HS_DX && g.aux) {
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    if constexpr (PRE) mask[u] = pmask[(i * TN + j) * 2 + u];
                    else mask[u] = *reinterpret_cast<const uint4*>(g.aux + rowoff + nj + 16 * u + 8 * h);
                }
            }
            unsigned d[4][2];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float v[4];
#pragma unroll
                for (int p = 0; p < 4; ++p) v[p] = acc.v[i][j][4 * q + p];
                if (EPI == HS_FWD) {
                    const float4 b = bias4[j][q];
#pragma unroll
                    for (int p = 0; p < 4; ++p) v[p] = fmaxf(v[p] + (p == 0 ? b.x : p == 1 ? b.y : p == 2 ? b.z : b.w), floor_v);
                }
                d[q][0] = pack_bf16(v[0], v[1]); d[q][1] = pack_bf16(v[2], v[3]);
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int qq = 2 * u;
                const auto sx = __builtin_amdgcn_permlane32_swap(d[qq][0], d[qq + 1][0], false, false);
                const auto sy = __builtin_amdgcn_permlane32_swap(d[qq][1], d[qq + 1][1], false, false);
                uint4 o = make_uint4(sx[0], sy[0], sx[1], sy[1]);
                if (EPI == HS_DX && g.aux) {
                    auto keep = [](unsigned a) {      // per bf16 half: 0xffff where the activation is > 0 (relu'), else 0
                        const unsigned lo = (int)(short)(a & 0xffffu) > 0 ? 0xffffu : 0u;
                        const unsigned hi = (int)a > 0xffff ? 0xffff0000u : 0u;
                        return lo | hi;
                    };
                    o.x &= keep(mask[u].x); o.y &= keep(mask[u].y); o.z &= keep(mask[u].z); o.w &= keep(mask[u].w);
                }
#if defined(VAEK_HS_ABLATE) && (VAEK_HS_ABLATE & 2)      // diagnostic: no output stores (values kept alive)
                asm volatile("" ::"v"(o.x), "v"(o.y), "v"(o.z), "v"(o.w));
#else
                if (row_ok) *reinterpret_cast<uint4*>(g.C + rowoff + nj + 16 * u + 8 * h) = o;
#endif
            }
        }
    }
}

}  // namespace vaek
