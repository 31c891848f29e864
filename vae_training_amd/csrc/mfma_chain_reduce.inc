// Chain piece (mfma_chain_dev.h): column sums over the 16 lanes of a row, every wave's accumulators and sums into its slice of
// the reduction image R (which reuses T, hence the barrier before), and the two readers of the image behind the barrier after.
    // all-reduce over the 16 lanes of a DPP row (= the 16 sample columns of one row group): v += ror(v, n)
    // as ONE v_add_f32 with a row_ror modifier each -- __shfl_xor would go through the LDS crossbar
    auto rowsum = [&](float v) {
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false));   // row_ror:8
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xf, 0xf, false));   // row_ror:4
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x122, 0xf, 0xf, false));   // row_ror:2
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x121, 0xf, 0xf, false));   // row_ror:1
        return v;
    };
    __syncthreads();           // every wave is done with its T columns before T is reused as R
    float* R = T + wave * G::R_PER_WAVE;
    {
        const int col = lane & 15, row0 = 4 * (lane >> 4);
        int blk = 0;
#pragma unroll
        for (int i = 0; i < G::IB1; ++i)
#pragma unroll
            for (int jj = 0; jj < G::JB1; ++jj, ++blk)
#pragma unroll
                for (int r = 0; r < 4; ++r) R[(blk * 16 + row0 + r) * 16 + col] = acc1[i][jj][r];
#pragma unroll
        for (int i = 0; i < G::IB2; ++i)
#pragma unroll
            for (int jj = 0; jj < G::JB2; ++jj, ++blk)
#pragma unroll
                for (int r = 0; r < 4; ++r) R[(blk * 16 + row0 + r) * 16 + col] = acc2[i][jj][r];
        float* CS = R + G::NBLK * 256;     // [dy (DP) | dys (DP)] [dmu (LP)] [gz (LP)]
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int r = 0; r < AD::nreg(db); ++r) {
                const int d = AD::feat(db, g, r);
                if (!G::ONE1) {
                    const float v = rowsum(cs_dy[db][r]);
                    float vs = 0.f;
                    if (SIG) vs = rowsum(cs_dys[db][r]);
                    if (j == 0 && d < DP) { CS[d] = v; if (SIG) CS[DP + d] = vs; }
                }
            }
#pragma unroll
        for (int lb = 0; lb < NLB; ++lb)
#pragma unroll
            for (int r = 0; r < AL::nreg(lb); ++r) {
                const int l = AL::feat(lb, g, r);
                const float w = rowsum(cs_gz[lb][r]);
                if (j == 0 && l < LP) CS[G::NB1 + LP + l] = w;
                if (!G::ONE2) {
                    const float v = rowsum(cs_dmu[lb][r]);
                    if (j == 0 && l < LP) CS[G::NB1 + l] = v;
                }
            }
        float m0 = rowsum(s_mse), m1 = rowsum(s_musq), m2 = rowsum(s_deps);      // 16 lanes by DPP, then the 4 rows
        // the four rows by two more DPP adds (row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3: lane 63 ends
        // up with the wave's total) -- __shfl_xor is two trips through the LDS crossbar per value
        auto rows4 = [&](float v) {
            v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x142, 0xa, 0xf, false));
            v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x143, 0xc, 0xf, false));
            return v;
        };
        m0 = rows4(m0); m1 = rows4(m1); m2 = rows4(m2);
        if (lane == 63) { CS[G::NCS + 0] = m0; CS[G::NCS + 1] = m1; CS[G::NCS + 2] = m2; }
    }
    __syncthreads();
    auto fetch_cs = [&](int k) -> float {
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < G::NW; ++w) v += T[w * G::R_PER_WAVE + G::NBLK * 256 + k];
        return v;
    };
    auto batch_sum_k = [&](int k) -> float {            // this thread's k-th output, summed over the workgroup's four waves
        const int o = src_off[k];
        const int oc = o != 0xffff ? o : 0;               // unconditional LDS reads, select afterwards
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < G::NW; ++w) v += T[w * G::R_PER_WAVE + oc];
        return o != 0xffff ? v : 0.f;
    };
