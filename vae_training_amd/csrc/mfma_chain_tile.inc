// Chain piece (mfma_chain_dev.h): one tile of 256 samples -- forward, loss terms, backward, the feature-major image and the wave's
// share of both batch-reduction GEMMs.  VAEK_MSTAMP(2..4) mark the phases in a -DVAEK_STAMPS build of the fused kernel (a no-op
// elsewhere).  Needs the operands, the inputs (xv, z1v, z2v, valid), the zeroed sums, sigma, inv_var, dscale, a.inv_bt, T.
    // ---- mu^T = We^T x^T + be : the four 16-sample sub-tiles are independent MFMA chains ----------
    f32x4 mu[NSUB][NLB];
#pragma unroll
    for (int s = 0; s < NSUB; ++s)
#pragma unroll
        for (int lb = 0; lb < NLB; ++lb) mu[s][lb] = f32x4{c_be[lb][0], c_be[lb][1], c_be[lb][2], c_be[lb][3]};
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int k = 0; k < AD::nreg(db); ++k)
#pragma unroll
            for (int s = 0; s < NSUB; ++s)
#pragma unroll
                for (int lb = 0; lb < NLB; ++lb)
                    mu[s][lb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wmu[lb][db][k], xv[s][db][k], mu[s][lb], 0, 0, 0);
    // ---- samples = mu + e^{lv/2} z1 (networks.py:73-74), in accumulator layout ---------------------
    float sv[NSUB][NLB][4];
#pragma unroll
    for (int s = 0; s < NSUB; ++s)
#pragma unroll
        for (int lb = 0; lb < NLB; ++lb)
#pragma unroll
            for (int r = 0; r < AL::nreg(lb); ++r) {
                const float m = mu[s][lb][r];
                sv[s][lb][r] = fmaf(c_sd[lb][r], z1v[s][lb][r], m);
                s_musq = valid[s] ? fmaf(m, m, s_musq) : s_musq;
            }
    VAEK_MSTAMP(2);
    // ---- y^T = Wd^T samples^T + bd (and the sigmoid head): B operand = the registers above ----------
    f32x4 y[NSUB][NDB], ys[SIG ? NSUB : 1][NDB];
#pragma unroll
    for (int s = 0; s < NSUB; ++s)
#pragma unroll
        for (int db = 0; db < NDB; ++db) {
            y[s][db] = f32x4{c_bd[db][0], c_bd[db][1], c_bd[db][2], c_bd[db][3]};
            if (SIG) ys[s][db] = f32x4{c_bs[db][0], c_bs[db][1], c_bs[db][2], c_bs[db][3]};
        }
#pragma unroll
    for (int lb = 0; lb < NLB; ++lb)
#pragma unroll
        for (int k = 0; k < AL::nreg(lb); ++k)
#pragma unroll
            for (int s = 0; s < NSUB; ++s)
#pragma unroll
                for (int db = 0; db < NDB; ++db) {
                    y[s][db] = __builtin_amdgcn_mfma_f32_16x16x4f32(wy[db][lb][k], sv[s][lb][k], y[s][db], 0, 0, 0);
                    if (SIG) ys[s][db] = __builtin_amdgcn_mfma_f32_16x16x4f32(wys[db][lb][k], sv[s][lb][k], ys[s][db], 0, 0, 0);
                }
    // ---- residual, loss terms, dL/dx_hat (networks.py:81-83, :94-98) -------------------------------
    float dyv[NSUB][NDB][4], dysv[SIG ? NSUB : 1][NDB][4];
#pragma unroll
    for (int s = 0; s < NSUB; ++s)
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int r = 0; r < AD::nreg(db); ++r) {
                const int d = AD::feat(db, g, r);
                float xh = fmaf(sigma, z2v[s][db][r], y[s][db][r]);
                float sg = 0.f;
                if (SIG) { sg = 1.f / (1.f + expf(-ys[s][db][r])); xh += sg; }
                const float rr = (valid[s] && d < D) ? xh - xv[s][db][r] : 0.f;
                const float q = rr * rr * inv_var;
                s_mse = fmaf(0.5f, q, s_mse);
                s_deps += -0.5f * q + 0.5f * sigma * z2v[s][db][r] * rr * inv_var;
                const float dyd = rr * dscale;
                dyv[s][db][r] = dyd;
                if (!G::ONE1) cs_dy[db][r] += dyd;
                if (SIG) { const float ds = dyd * sg * (1.f - sg); dysv[s][db][r] = ds; if (!G::ONE1) cs_dys[db][r] += ds; }
            }
    VAEK_MSTAMP(3);
    // ---- g^T = Wd dy^T (+ Ws dys^T) ------------------------------------------------------------------
    f32x4 gq[NSUB][NLB];
#pragma unroll
    for (int s = 0; s < NSUB; ++s)
#pragma unroll
        for (int lb = 0; lb < NLB; ++lb) gq[s][lb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int k = 0; k < AD::nreg(db); ++k)
#pragma unroll
            for (int s = 0; s < NSUB; ++s)
#pragma unroll
                for (int lb = 0; lb < NLB; ++lb) {
                    gq[s][lb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wg[lb][db][k], dyv[s][db][k], gq[s][lb], 0, 0, 0);
                    if (SIG) gq[s][lb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wgs[lb][db][k], dysv[s][db][k], gq[s][lb], 0, 0, 0);
                }
    // ---- dmu, column sums, and the feature-major image for the batch-reduction GEMMs ------------------
#pragma unroll
    for (int s = 0; s < NSUB; ++s) {
        float* Tc = T + wave * 64 + s * 16 + j;
#pragma unroll
        for (int lb = 0; lb < NLB; ++lb)
#pragma unroll
            for (int r = 0; r < AL::nreg(lb); ++r) {
                const int l = AL::feat(lb, g, r);
                const float gl = gq[s][lb][r];
                const float dmu = valid[s] ? fmaf(mu[s][lb][r], a.inv_bt, gl) : 0.f;     // dmu = g + mu/B
                if (!G::ONE2) cs_dmu[lb][r] += dmu;
                cs_gz[lb][r] = fmaf(gl, z1v[s][lb][r], cs_gz[lb][r]);                     // reparam part of d lv
                if (l < LP) { Tc[(G::FS + l) * G::TS] = sv[s][lb][r]; Tc[(G::FDM + l) * G::TS] = dmu; }
            }
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int r = 0; r < AD::nreg(db); ++r) {
                const int d = AD::feat(db, g, r);
                if (d < DP) {
                    Tc[(G::FX + d) * G::TS] = xv[s][db][r];
                    Tc[(G::FDY + d) * G::TS] = dyv[s][db][r];
                    if (SIG) Tc[(G::FDY + DP + d) * G::TS] = dysv[s][db][r];
                }
            }
    }
    // each wave reads back only its own 64 columns: wave-level ordering is enough (no s_barrier)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    VAEK_MSTAMP(4);
    // ---- dWd (+dWs) = samples^T [dy|dys],  dWe = x^T dmu : K = the wave's 64 samples ------------------
    {
        const float* Tk = T + wave * 64 + (lane >> 4) + (lane & 15) * G::TS;
        constexpr int NOP = G::IB1 + G::JB1 + G::IB2 + G::JB2;
        // Operand prefetch runs ONE group of GS k-steps ahead: lgkmcnt is a 4-bit counter, so the wait
        // in front of a group's MFMAs can only be exact while <= 15 younger reads are in flight.
        constexpr int GS = (2 * NOP <= 15) ? 2 : 1, NG = 16 / GS;
        float op[2][GS][NOP];
        auto load_group = [&](int gi, int which) {
#pragma unroll
            for (int u = 0; u < GS; ++u) {
                const int s4 = 4 * (gi * GS + u);
                int n = 0;
#pragma unroll
                for (int i = 0; i < G::IB1; ++i) op[which][u][n++] = Tk[(G::FS + 16 * i) * G::TS + s4];
#pragma unroll
                for (int jj = 0; jj < G::JB1; ++jj) op[which][u][n++] = Tk[(G::FDY + 16 * jj) * G::TS + s4];
#pragma unroll
                for (int i = 0; i < G::IB2; ++i) op[which][u][n++] = Tk[(G::FX + 16 * i) * G::TS + s4];
#pragma unroll
                for (int jj = 0; jj < G::JB2; ++jj) op[which][u][n++] = Tk[(G::FDM + 16 * jj) * G::TS + s4];
            }
        };
        load_group(0, 0);
#pragma unroll
        for (int gi = 0; gi < NG; ++gi) {
            if (gi + 1 < NG) load_group(gi + 1, (gi + 1) & 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < GS; ++u) {
                const float* o = op[gi & 1][u];
#pragma unroll
                for (int i = 0; i < G::IB1; ++i)
#pragma unroll
                    for (int jj = 0; jj < G::JB1; ++jj)
                        acc1[i][jj] = __builtin_amdgcn_mfma_f32_16x16x4f32(o[i], o[G::IB1 + jj], acc1[i][jj], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < G::IB2; ++i)
#pragma unroll
                    for (int jj = 0; jj < G::JB2; ++jj)
                        acc2[i][jj] = __builtin_amdgcn_mfma_f32_16x16x4f32(o[G::IB1 + G::JB1 + i], o[G::IB1 + G::JB1 + G::IB2 + jj],
                                                                           acc2[i][jj], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
