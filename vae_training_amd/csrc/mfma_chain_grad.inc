// Chain piece (mfma_chain_dev.h): the self-finalizing tail's closed forms.  One workgroup holds the whole batch, so its sums ARE
// the batch sums; this turns gq_, output idx's batch sum, into its gradient: the KL part of a log-variance (pk[k] is the thread's
// own parameter), the decoder noise, the three loss slots.  `pother` is where the OTHER threads' parameters are read -- a plain
// pointer, never const __restrict__ (linear_resident.hip says why): params_rw in the single-step kernel, the LDS image in the
// resident one.
        if (idx >= off_epsp && idx < off_epsp + L) {
            const float lv = pk[k];
            gq_ = 0.5f * expf(0.5f * lv) * gq_ - 0.5f * (1.f - expf(lv)) * a.rows_over_bt;
        } else if (idx == a.off_eps) {
            gq_ = a.eps_cli * (s_deps_t + 0.5f * a.rows * (float)D) * a.inv_bt;
        } else if (idx >= a.P) {
            if (idx < a.P + 3) {
                float klc = 0.f;
                for (int l = 0; l < L; ++l) { const float lv = pother[off_epsp + l]; klc += 1.f + lv - expf(lv); }
                const float eps_s = a.off_eps >= 0 ? pother[a.off_eps] * a.eps_cli : a.eps_cli;
                const float dkl = (0.5f * s_musq_t - 0.5f * a.rows * klc) * a.inv_bt;
                const float mse = (s_mse_t + 0.5f * a.rows * (float)D * (kLog2Pi + eps_s)) * a.inv_bt;
                gq_ = idx == a.P ? dkl + mse : (idx == a.P + 1 ? dkl : mse);
            } else {
                gq_ = 0.f;
            }
        }
