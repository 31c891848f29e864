// Chain piece (mfma_chain_dev.h): the operand predicates, the weights as MFMA A operands (lane = output row ai, k group akg)
// and the per-lane constants, zero outside [D, L].  The including kernel says what fetching an operand is:
//   VAEK_W(dst, idx, ok)     dst <- parameter idx of the flat vector, valid where ok
//   VAEK_WSD(dst, idx, ok)   the same for c_sd, whose parameter is logvar_e and whose value is e^{lv/2}
// Needs ai, akg, g, D, L, off_*.
    // row ai of a block <-> (g', r') = (ai >> 2, ai & 3)
    auto latrow = [&](int lb) { return AL::feat(lb, ai >> 2, ai & 3); };
    auto datrow = [&](int db) { return AD::feat(db, ai >> 2, ai & 3); };
    float wmu[NLB][NDB][4], wy[NDB][NLB][4], wg[NLB][NDB][4], wys[SIG ? NDB : 1][NLB][4], wgs[SIG ? NLB : 1][NDB][4];
    auto w_ok1 = [&](int lb, int db, int s) { return s < AD::nreg(db) && (ai & 3) < AL::nreg(lb) && latrow(lb) < L && AD::feat(db, akg, s) < D; };
    auto w_ok2 = [&](int db, int lb, int s) { return s < AL::nreg(lb) && (ai & 3) < AD::nreg(db) && datrow(db) < D && AL::feat(lb, akg, s) < L; };
#pragma unroll
    for (int lb = 0; lb < NLB; ++lb)
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                // mu: out row = latent latrow(lb), k = data dim feat(db, akg, s);  g: same roles, weights Wd
                const int lo = latrow(lb), dk = AD::feat(db, akg, s);
                const bool ok = w_ok1(lb, db, s);
                VAEK_W(wmu[lb][db][s], dk * L + lo, ok);
                VAEK_W(wg[lb][db][s], off_wd + lo * D + dk, ok);
                if (SIG) VAEK_W(wgs[lb][db][s], off_ws + lo * D + dk, ok);
                // y: out row = data dim datrow(db), k = latent feat(lb, akg, s)
                const int dout = datrow(db), lk = AL::feat(lb, akg, s);
                const bool ok2 = w_ok2(db, lb, s);
                VAEK_W(wy[db][lb][s], off_wd + lk * D + dout, ok2);
                if (SIG) VAEK_W(wys[db][lb][s], off_ws + lk * D + dout, ok2);
            }
    // per-lane constants in accumulator layout (group g, register r)
    float c_be[NLB][4], c_sd[NLB][4], c_bd[NDB][4], c_bs[SIG ? NDB : 1][4];
#pragma unroll
    for (int lb = 0; lb < NLB; ++lb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int l = AL::feat(lb, g, r);
            const bool ok = r < AL::nreg(lb) && l < L;
            VAEK_W(c_be[lb][r], off_be + l, ok);
            VAEK_WSD(c_sd[lb][r], off_epsp + l, ok);
        }
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int d = AD::feat(db, g, r);
            const bool ok = r < AD::nreg(db) && d < D;
            VAEK_W(c_bd[db][r], off_bd + d, ok);
            if (SIG) VAEK_W(c_bs[db][r], off_bs + d, ok);
        }
