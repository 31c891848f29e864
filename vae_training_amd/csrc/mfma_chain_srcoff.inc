// Chain piece (mfma_chain_dev.h): the src_off table.  Needs t, D, L, off_*, a.P, G, NOUT.
    // Where each of this thread's outputs (flat-gradient index t, t + 256, ...) will sit in the cross-wave reduction image
    // of the epilogue -- worked out NOW, under the input loads' latency, instead of as ~40 VALU + divergent branches per
    // output on the kernel's tail.  0xffff = an output this kernel leaves zero.
    unsigned short src_off[NOUT];
    {
        auto blk_off = [&](int gemm, int i, int jj) {
            const int blk = gemm == 1 ? (i >> 4) * G::JB1 + (jj >> 4) : G::IB1 * G::JB1 + (i >> 4) * G::JB2 + (jj >> 4);
            return (blk * 16 + (i & 15)) * 16 + (jj & 15);
        };
#pragma unroll
        for (int k = 0; k < NOUT; ++k) {
            const int idx = t + 256 * k;
            int o = 0xffff;
            if (idx < off_be) o = blk_off(2, idx / L, idx % L);                                   // dWe = x^T dmu
            else if (idx < off_wd) o = G::ONE2 ? blk_off(2, DP, idx - off_be) : G::NBLK * 256 + G::NB1 + idx - off_be;   // dbe = 1^T dmu
            else if (idx < off_bd) { const int kk = idx - off_wd; o = blk_off(1, kk / D, kk % D); }   // dWd = samples^T dy
            else if (idx < off_bd + D) o = G::ONE1 ? blk_off(1, LP, idx - off_bd) : G::NBLK * 256 + idx - off_bd;        // dbd = 1^T dy
            else if (SIG && idx < off_bs) { const int kk = idx - off_ws; o = blk_off(1, kk / D, DP + kk % D); }
            else if (SIG && idx < off_bs + D) o = G::ONE1 ? blk_off(1, LP, DP + idx - off_bs) : G::NBLK * 256 + DP + idx - off_bs;
            else if (idx >= off_epsp && idx < off_epsp + L) o = G::NBLK * 256 + G::NB1 + LP + idx - off_epsp;   // sum g*z1
            else if (idx >= a.P && idx < a.P + 3) o = G::NBLK * 256 + G::NCS + idx - a.P;
            src_off[k] = (unsigned short)o;
        }
    }
