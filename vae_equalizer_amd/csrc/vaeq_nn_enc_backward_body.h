// vaeq_nn_enc_backward_body.h -- the body of nn_enc_backward_kernel and nn_enc_backward_x_kernel (vaeq_nn_ops.hip), included inside each of them.
// The including kernel defines `constexpr bool GX` (true: also the input gradient, written to its parameter `gx`); everything else is the kernels'
// common parameter list.  No include guard: it is meant to be included once per kernel.  Textual inclusion, not a shared device function: handing the pointers through a call changes the register allocation of
// nn_enc_backward_kernel, whose instruction stream is held fixed.
    extern __shared__ float4 smem4[];
    float *sm = reinterpret_cast<float *>(smem4);
    constexpr int C = 2 * NLEV, CQ = C / 4, NWV = NT / 64;
    constexpr bool MF = nn_mf(NLEV), BN = MODE != 0;
    constexpr int CP = nn_cp(NLEV);
    const int tid = threadIdx.x, run = blockIdx.x, lane = tid & 63, wv = tid >> 6;
    const NNLayout l = nn_enc_layout(L, sps, NLEV, k1, k2, BN, true);
    const int N = (L + sps - 1) / sps, NP = l.NP, AS = l.AS, Lx = l.Lx, Lz = l.Lz, p1 = l.p1, p2 = l.p2;
    float *xs = sm + l.xs, *z1 = sm + l.z1, *zb = sm + l.zb, *bnst = sm + l.bnst, *a2 = sm + l.a2 + l.A0, *scr = sm + l.mu;
    float *th = sm + l.th, *gr = sm + l.gr, *w1t = sm + l.w1t, *w2t = sm + l.w2t, *w2u = sm + l.w2u;
    for (int i = tid; i < l.total; i += NT) sm[i] = 0.f;       // halos, guard columns, padding rows and every cell an operand tile may read past its rows
    __syncthreads();
    for (int i = tid; i < NP; i += NT) th[i] = theta[(size_t)run * NP + i];
    const float *xr = x + (size_t)run * 2 * (size_t)L;
    for (int i = tid; i < 2 * L; i += NT) {
        const int row = i / L, c = i - row * L;
        xs[row * Lx + p1 + c] = xr[i];
    }
    if constexpr (MF) {                                        // the rows of ones: the bias columns of the weight-gradient GEMMs (mfma_wgrad16, ROW1)
        for (int i = tid; i < Lx; i += NT) xs[2 * Lx + i] = 1.0f;
        for (int i = tid; i < Lz; i += NT) zb[CP * Lz + i] = 1.0f;
    }
    if (BN && tid < C) {
        const float s0 = stats[(size_t)run * 2 * C + tid], s1 = stats[(size_t)run * 2 * C + C + tid];
        bnst[tid] = s0;
        bnst[C + tid] = MODE == 1 ? s1 : 1.0f / sqrtf(s1 + 1e-5f);
    }
    __syncthreads();
    nn_transpose_weights<NT, NLEV>(l, k1, k2, th, w1t, w2t, w2u);
    __syncthreads();
    // ---- ELU(fc1(x)) again (not saved by the forward), then the normalisation with the statistics the forward used
    nn_fc1_elu<NT, NLEV>(l, k1, xs, th, w1t, z1, L, 0, L);
    __syncthreads();
    if constexpr (BN) {
        nn_enc_batchnorm<NT, NLEV, false>(l, th, z1, zb, bnst, [](int, float, float, float) {});
        __syncthreads();
    }
    // ---- softmax backward per axis: dL/dlogit_i = q_i (dL/dq_i - sum_j q_j dL/dq_j); item = (axis, n)
    for (int it = tid; it < 2 * N; it += NT) {
        const int axq = it / N, n = it - axq * N;
        float qv[NLEV], gv[NLEV], dot = 0.f;
#pragma unroll
        for (int i = 0; i < NLEV; i++) {
            const size_t ix = ((size_t)run * C + axq * NLEV + i) * N + n;
            qv[i] = q[ix]; gv[i] = gq[ix];
        }
#pragma unroll
        for (int i = 0; i < NLEV; i++) dot = fmaf(qv[i], gv[i], dot);
#pragma unroll
        for (int i = 0; i < NLEV; i++) a2[(axq * NLEV + i) * AS + n] = qv[i] * (gv[i] - dot);
    }
    __syncthreads();
    // ---- fc2 weight / bias gradients: gw2[c][cc][k] = sum_n g2[c][n] zb[cc][n sps + k]
    if constexpr (MF) {
        mfma_wgrad16<NT, true>(a2, AS, N, zb, sps, C * k2, k2, Lz, scr, 4 * N, [&](int c0, int j, f32x4 acc) {
            const float av_[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
            for (int t = 0; t < 4; t++) {
                if (c0 + t >= C) continue;                     // (16-QAM on the 16-row path: rows 8 .. 15 are padding)
                if (j == C * k2) gr[l.oB2 + c0 + t] = av_[t];
                else gr[l.oW2 + (c0 + t) * C * k2 + j] = av_[t];
            }
        }, AS - l.A0 - N, CP);
    } else {
        const int nkq = (k2 + 3) / 4, ngrp = C * nkq;
        for (int grp = wv; grp <= ngrp; grp += NWV) {
            const bool bias = grp == ngrp;
            const int cc = bias ? 0 : grp / nkq, k0 = bias ? 0 : (grp - cc * nkq) * 4;
            nn_tapgroup_grad<C>(N, zb + cc * Lz + k0, sps, a2, AS, bias, lane, [&](int t, int c, float sum) {
                if (bias) { if (t == 0) gr[l.oB2 + c] = sum; }
                else if (k0 + t < k2) gr[l.oW2 + (c * C + cc) * k2 + k0 + t] = sum;
            });
        }
    }
    __syncthreads();
    // ---- back through fc2 (transposed strided convolution); Net: times ELU' in place of z1, Net_BN: dL/d(BatchNorm output) in place of zb
    if constexpr (MF) {
        mfma_convT16<NT, 3>(w2u, k2, p2, sps, a2, AS, L,
            [&](int cc, int sx) { return BN ? 0.f : z1[cc * Lz + p2 + sx]; },
            [&](int cc, int sx, float g, float z) {
                const int ix = cc * Lz + p2 + sx;
                if (BN) zb[ix] = g;
                else z1[ix] = g * (z > 0.f ? 1.0f : z + 1.0f);
            });
    } else
    for (int it = tid; it < CQ * L; it += NT) {
        const int ccq = it / L, sx = it - ccq * L;
        float g0 = 0.f, g1 = 0.f, g2 = 0.f, g3 = 0.f;
        for (int k = 0; k < k2; k++) {
            const int t = sx + p2 - k;
            if (t < 0 || t % sps) continue;
            const int n = t / sps;
            if (n >= N) continue;
            const float4 *w = reinterpret_cast<const float4 *>(w2u + (k * C) * C + 4 * ccq);
#pragma unroll
            for (int c = 0; c < C; c++) {
                const float av_ = a2[c * AS + n];
                const float4 w4 = w[c * CQ];
                g0 = fmaf(w4.x, av_, g0); g1 = fmaf(w4.y, av_, g1); g2 = fmaf(w4.z, av_, g2); g3 = fmaf(w4.w, av_, g3);
            }
        }
        const float gg[4] = {g0, g1, g2, g3};
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int ix = (4 * ccq + u) * Lz + p2 + sx;
            if (BN) zb[ix] = gg[u];
            else {
                const float z = z1[ix];
                z1[ix] = gg[u] * (z > 0.f ? 1.0f : z + 1.0f);                             // ELU' = 1 or exp(a1) = z1 + 1
            }
        }
    }
    __syncthreads();
    if constexpr (BN) {                                        // BatchNorm backward, then ELU'; one wave per channel
        for (int c = wv; c < C; c += NWV) {
            float *zr = z1 + c * Lz + p2;
            const float *gp = zb + c * Lz + p2;
            float s1 = 0.f, s2 = 0.f;
            for (int sx = lane; sx < L; sx += 64) { s1 += gp[sx]; s2 = fmaf(gp[sx], zr[sx], s2); }
            s1 = wave_sum_fast(s1);
            s2 = wave_sum_fast(s2);
            if (lane == 0) { gr[l.oG + c] = s2; gr[l.oBt + c] = s1; }
            const float mean = bnst[c], rstd = bnst[C + c], gs = th[l.oG + c] * rstd;
            // training mode: the mean and the variance depend on every sample of the row; eval mode: they are constants
            const float m1 = MODE == 1 ? s1 / (float)L : 0.f, m2 = MODE == 1 ? s2 / (float)L : 0.f;
            for (int sx = lane; sx < L; sx += 64) {
                const float zh = zr[sx];
                const float gz = gs * (gp[sx] - m1 - zh * m2);
                const float z = zh / rstd + mean;              // ELU output before the normalisation
                zr[sx] = gz * (z > 0.f ? 1.0f : z + 1.0f);
            }
        }
        __syncthreads();
    }
    // ---- input gradient, back through fc1 (2 output rows: vector-ALU work): gx[i][s] = sum_c sum_k fc1.weight[c][i][k] gz[c][s - k + p1], one thread
    // per (row, sample), c then k ascending.  Every lane walks all k1 taps (a uniform trip count: no exec-masked loop); a tap that falls outside
    // [0, L) -- zero padding in the reference, at the first and last p1 samples only -- reads the clamped cell and contributes an exact 0.
    // The weight is a broadcast read of th, gz consecutive lanes on consecutive cells.
    if constexpr (GX) {
        float *gxr = gx + (size_t)run * 2 * (size_t)L;
        for (int it = tid; it < 2 * L; it += NT) {
            const int i = it / L, s = it - i * L;
            float acc = 0.f;
            for (int c = 0; c < C; c++) {
                const float *w = th + l.oW1 + (c * 2 + i) * k1, *gz = z1 + c * Lz + p2;
                for (int k = 0; k < k1; k++) {
                    const int sy = s + p1 - k, sc = min(max(sy, 0), L - 1);
                    const float g = ldsv(gz + sc);
                    acc = fmaf(w[k], sy == sc ? g : 0.f, acc);
                }
            }
            gxr[it] = acc;
        }
    }
    // ---- fc1 weight / bias gradients: gw1[c][i][k] = sum_s gz[c][s] x[i][s + k]
    if constexpr (MF) {
        mfma_wgrad16<NT, true>(z1 + p2, Lz, L, xs, 1, 2 * k1, k1, Lx, scr, 4 * N, [&](int c0, int j, f32x4 acc) {
            const float av_[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
            for (int t = 0; t < 4; t++) {
                if (c0 + t >= C) continue;
                if (j == 2 * k1) gr[l.oB1 + c0 + t] = av_[t];
                else gr[l.oW1 + (c0 + t) * 2 * k1 + j] = av_[t];
            }
        }, Lz - p2 - L);
    } else {
        const int nkq = (k1 + 3) / 4, ngrp = 2 * nkq;
        for (int grp = wv; grp <= ngrp; grp += NWV) {
            const bool bias = grp == ngrp;
            const int i = bias ? 0 : grp / nkq, k0 = bias ? 0 : (grp - i * nkq) * 4;
            nn_tapgroup_grad<C>(L, xs + i * Lx + k0, 1, z1 + p2, Lz, bias, lane, [&](int t, int c, float sum) {
                if (bias) { if (t == 0) gr[l.oB1 + c] = sum; }
                else if (k0 + t < k1) gr[l.oW1 + (c * 2 + i) * k1 + k0 + t] = sum;
            });
        }
    }
    __syncthreads();
    for (int i = tid; i < NP; i += NT) g_out[(size_t)run * NP + i] = gr[i];
