// The body of mlp3_grad_kernel and mlp3_grad_replicas_kernel (fused_mlp3.hip includes it into both): `a` is the launch's
// Mlp3GradArgs and `b` its generator arguments, or replica blockIdx.y's slices of them.
    __shared__ float As[M3_TK][M3_TB];           // [kernel row | bias][batch row]
    __shared__ float Gs[M3_TB][M3_TJ + 1];       // [batch row][column]
    const int t = threadIdx.x, lane = t & 63, kq = __builtin_amdgcn_readfirstlane(t >> 6);
    const int bid = blockIdx.x, ntiles = a.tile0[M3_NL];
    if (bid > ntiles) {              // vaek_train_step_gen: the next step's batch does not depend on the weights
        const unsigned step = make_batch_step(b);
        make_batch_items(b, step, (long long)(bid - ntiles - 1) * M3_NT + t);
        make_batch_advance(b, step, bid == ntiles + 1 && t == 0);
        return;
    }
    if (bid == ntiles) { m3_tail(a); return; }
    int li = 0;
#pragma unroll
    for (int i = 1; i < M3_NL; ++i) li = bid >= a.tile0[i] ? i : li;
    const int n_in = a.ly.n_in[li], n_out = a.ly.n_out[li], Bs = a.Bs;
    const int tiles_j = (n_out + M3_TJ - 1) / M3_TJ, rel = bid - a.tile0[li];
    const int k0 = M3_TK * (rel / tiles_j), j0 = M3_TJ * (rel % tiles_j);
    const float* const ap = a.acts + a.ly.a_off[li];
    const float* const gp = a.acts + a.ly.g_off[li];
    // this thread's four outputs: rows k0 + 4 kq + i (row n_in is the bias), column j0 + lane; Adam state loaded up front
    const int j = j0 + lane;
    int idx[4]; bool ok[4];
    float p_old[4], m_old[4], v_old[4];
    const float* const ps = a.params_rw ? a.params_rw : a.params;
    const float* const ms = a.m ? a.m : a.params;
    const float* const vs = a.v ? a.v : a.params;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = k0 + 4 * kq + i;
        ok[i] = k <= n_in && j < n_out;
        idx[i] = a.ly.w_off[li] + (ok[i] ? k * n_out + j : 0);
        p_old[i] = ps[idx[i]]; m_old[i] = ms[idx[i]]; v_old[i] = vs[idx[i]];
    }
    const int tstep = a.step_dev ? a.step_dev[0] : 0;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < Bs; c0 += M3_TB) {
        const bool in = c0 + lane < Bs;
        const int bc = min(c0 + lane, Bs - 1);
        float gv[16], av[4];
#pragma unroll
        for (int r = 0; r < 16; ++r) gv[r] = gp[(long long)min(j0 + 16 * kq + r, n_out - 1) * Bs + bc];
#pragma unroll
        for (int r = 0; r < 4; ++r) av[r] = ap[(long long)min(k0 + 4 * kq + r, n_in - 1) * Bs + bc];
        __syncthreads();             // the previous chunk is no longer read
#pragma unroll
        for (int r = 0; r < 16; ++r) Gs[lane][16 * kq + r] = in ? gv[r] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) As[4 * kq + r][lane] = !in ? 0.f : (k0 + 4 * kq + r == n_in ? 1.f : av[r]);
        __syncthreads();
#pragma unroll 16
        for (int r = 0; r < M3_TB; ++r) {
            const float g = Gs[r][lane];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = fmaf(As[4 * kq + i][r], g, acc[i]);
        }
    }
    const float bc1 = -expm1f((float)tstep * -0.10536051565782628f);
    const float bc2 = -expm1f((float)tstep * -0.0010005003335835335f);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (ok[i]) {
            a.grads[idx[i]] = acc[i];
            if (a.params_rw) {
                adam_apply_f(p_old[i], acc[i], m_old[i], v_old[i], a.lr, bc1, bc2);
                a.params_rw[idx[i]] = p_old[i]; a.m[idx[i]] = m_old[i]; a.v[idx[i]] = v_old[i];
            }
        }
    }
