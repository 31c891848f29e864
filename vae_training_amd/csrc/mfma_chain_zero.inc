// Chain piece (mfma_chain_dev.h): the accumulators and column sums a wave carries over its tiles, zeroed.
    f32x4 acc1[G::IB1][G::JB1], acc2[G::IB2][G::JB2];
#pragma unroll
    for (int i = 0; i < G::IB1; ++i)
#pragma unroll
        for (int jj = 0; jj < G::JB1; ++jj) acc1[i][jj] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < G::IB2; ++i)
#pragma unroll
        for (int jj = 0; jj < G::JB2; ++jj) acc2[i][jj] = f32x4{0.f, 0.f, 0.f, 0.f};
    float cs_dy[NDB][4], cs_dys[SIG ? NDB : 1][4], cs_dmu[NLB][4], cs_gz[NLB][4];
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int r = 0; r < 4; ++r) { cs_dy[db][r] = 0.f; if (SIG) cs_dys[db][r] = 0.f; }
#pragma unroll
    for (int lb = 0; lb < NLB; ++lb)
#pragma unroll
        for (int r = 0; r < 4; ++r) { cs_dmu[lb][r] = 0.f; cs_gz[lb][r] = 0.f; }
    float s_mse = 0.f, s_deps = 0.f, s_musq = 0.f;
