// The body of mlp3_chain_kernel and mlp3_chain_replicas_kernel (fused_mlp3.hip includes it into both): `a` is the launch's
// Mlp3ChainArgs, or replica blockIdx.y's Mlp3ChainSlice of them.
    extern __shared__ __attribute__((aligned(16))) char m3_smem[];
    Mlp3Lds& s = *reinterpret_cast<Mlp3Lds*>(m3_smem);
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int D = a.D, L = a.L, Bs = a.Bs;
    const int row0 = blockIdx.x * M3_R, valid = min(M3_R, a.B - row0);
    const float* const P = a.params;
    if (blockIdx.x == 0 && t == 0 && a.step_dev) a.step_dev[0] += 1;
    M3_STAMP(0);
    // ---- inputs as [feature][sample] images, zero-padded; loads unconditional at clamped indices, selects at the LDS store
    float shl[2];
    {
        float xv[2], z1v[2], z2v[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e = t + i * M3_NT, c = e >> 4, sm = e & 15;
            const long long row = row0 + min(sm, valid - 1);
            xv[i] = a.x[row * D + min(c, D - 1)]; z1v[i] = a.z1[row * L + min(c, L - 1)]; z2v[i] = a.z2[row * D + min(c, D - 1)];
            shl[i] = P[a.off_epsp + min(c, L - 1)];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e = t + i * M3_NT, c = e >> 4;
            (&s.X[0][0])[e] = c < D ? xv[i] : 0.f; (&s.Z1[0][0])[e] = c < L ? z1v[i] : 0.f; (&s.Z2[0][0])[e] = c < D ? z2v[i] : 0.f;
            shl[i] = expf(0.5f * shl[i]);
        }
    }
    const float eps_ld = P[a.off_eps >= 0 ? a.off_eps : 0];
    const float eps = a.off_eps >= 0 ? eps_ld * a.eps_cli : a.eps_cli;
    const float sigma = expf(0.5f * eps), inv_var = expf(-eps);
    float p_mse = 0.f, p_musq = 0.f, p_deps = 0.f;
    __syncthreads();
    M3_STAMP(1);

    // ---- forward: encoder 0 .. 3, reparameterisation, decoder 4 .. 7, ELBO
    for (int li = 0; li < M3_NL; ++li) {
        const int n_in = a.ly.n_in[li], n_out = a.ly.n_out[li];
        const int w_off = a.ly.w_off[li];
        const M3Img in = m3_in_img(s, li), out = m3_out_img(s, li);
        m3_store_img(a.acts + a.ly.a_off[li], in, n_in, Bs, row0, t);
        const bool relu = li != 3 && li != 7;
        auto epi = [&](int m, int n, float v, float b) { v += b; out[m][n] = relu ? fmaxf(v, 0.f) : v; };
        const float* const bias = P + w_off + n_in * n_out;
        if (n_out <= 64) m3_dense<1, false>(P, w_off, bias, n_out, n_in, n_out, true, 0, a.e_max, in, wave, lane, epi);
        else m3_dense<4, false>(P, w_off, bias, n_out, n_in, n_out, true, 0, a.e_max, in, wave, lane, epi);
        __syncthreads();
        if (li == 3) {               // samples = mu + e^{lv/2} z1
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int e = t + i * M3_NT, c = e >> 4, sm = e & 15;
                if (c < L) {
                    const float mu = (&s.MU[0][0])[e];
                    (&s.SMP[0][0])[e] = fmaf(shl[i], (&s.Z1[0][0])[e], mu);
                    if (sm < valid) p_musq = fmaf(mu, mu, p_musq);
                }
            }
            __syncthreads();
        }
        M3_STAMP(2 + li);
    }
    // ---- ELBO, elementwise over [feature][sample]: decoder noise, residual, dL/dx_hat (zero for rows past the batch), scalar sums
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int e = t + i * M3_NT, c = e >> 4, sm = e & 15;
        const bool in = sm < valid && c < D;
        const float z2v = (&s.Z2[0][0])[e];
        const float res = (&s.XH[0][0])[e] + z2v * sigma - (&s.X[0][0])[e];
        (&s.XH[0][0])[e] = in ? res * inv_var * a.inv_bt : 0.f;
        if (in) {
            const float q = 0.5f * res * res * inv_var;
            p_mse += q;
            p_deps += -q + 0.5f * sigma * z2v * res * inv_var;
        }
    }
    __syncthreads();
    M3_STAMP(10);
    m3_store_img(a.acts + a.ly.g_off[7], s.XH, D, Bs, row0, t);

    // ---- backward: dX of layer li from the gradient image of its output, through the relu of the layer below, in place
    for (int li = M3_NL - 1; li >= 1; --li) {
        const int n_in = a.ly.n_in[li], n_out = a.ly.n_out[li];
        const int w_off = a.ly.w_off[li], sh = a.ly.shift[li];
        const M3Img dy = m3_out_img(s, li);
        const M3Img dst = li == 4 ? s.DS : m3_out_img(s, li - 1);
        const bool mask = li != 4;
        auto epi = [&](int m, int n, float v, float) { dst[m][n] = (!mask || dst[m][n] > 0.f) ? v : 0.f; };
        if (sh >= 0 && n_in <= 64) m3_dense<1, true>(P, w_off, P, n_in, n_out, n_out, false, sh, a.e_max, dy, wave, lane, epi);
        else if (sh >= 0) m3_dense<4, true>(P, w_off, P, n_in, n_out, n_out, false, sh, a.e_max, dy, wave, lane, epi);
        else if (n_in <= 64) m3_dense<1, false>(P, w_off, P, n_in, n_out, n_out, false, 0, a.e_max, dy, wave, lane, epi);
        else m3_dense<4, false>(P, w_off, P, n_in, n_out, n_out, false, 0, a.e_max, dy, wave, lane, epi);
        __syncthreads();
        if (li == 4) {               // d mu = d samples + mu / Bt (zero for rows past the batch); DS becomes d samples * z1
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int e = t + i * M3_NT, c = e >> 4, sm = e & 15;
                if (c < L) {
                    const float ds = (&s.DS[0][0])[e];
                    (&s.MU[0][0])[e] = sm < valid ? fmaf((&s.MU[0][0])[e], a.inv_bt, ds) : 0.f;
                    (&s.DS[0][0])[e] = sm < valid ? ds * (&s.Z1[0][0])[e] : 0.f;
                }
            }
            __syncthreads();
        }
        m3_store_img(a.acts + a.ly.g_off[li - 1], m3_out_img(s, li - 1), a.ly.n_out[li - 1], Bs, row0, t);
        M3_STAMP(10 + (M3_NL - li));
    }

    // ---- this workgroup's partial row: the three scalar sums (lanes by xor-shuffle, the four waves in order), epsilon_p's sums
    float* const row = a.part + (long long)blockIdx.x * M3_PS;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        p_mse += __shfl_xor(p_mse, o, 64); p_musq += __shfl_xor(p_musq, o, 64); p_deps += __shfl_xor(p_deps, o, 64);
    }
    if (lane == 0) { s.RED[wave][0] = p_mse; s.RED[wave][1] = p_musq; s.RED[wave][2] = p_deps; }
    __syncthreads();
    if (t < 3) row[t] = (s.RED[0][t] + s.RED[1][t]) + (s.RED[2][t] + s.RED[3][t]);
    if (t == 3) row[3] = 0.f;
    if (t < L) {
        float g = 0.f;
#pragma unroll
        for (int r = 0; r < M3_R; ++r) g += s.DS[t][r];
        row[4 + t] = g;
    }
    M3_STAMP(18);
