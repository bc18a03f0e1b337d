// vaeq_awgn_info.hip -- information-rate figures of one AWGN validation frame on the device: achievable rate of symbol-wise mismatched decoding
// (AIR), generalised mutual information of the bit-wise decoder (GMI) and the pre-FEC bit error rate, per run, over exactly the symbols the SER_q
// of the fused validation passes keeps (validate_tail, vaeq_validate.h: q[:, 11+sh : -11] against data[:, 11 : -11-sh]).  The reference has no such
// metric; the definitions are closed-form (include/vaeq.h, DESIGN.md section 5, tests/_ref_awgn_info.py).
//
// One 256-thread workgroup per run.  q-mode reads the stored posteriors q[2 n_lev][N] (the VAE-NN encoder's output); y-mode recomputes the VAE-LE
// demapper's posteriors in the log domain from the un-normalised equaliser output y[2][N] the validation kernels leave behind
// (func_VAELE_MQAM_shaping.py:228-229: yhat_c = y_c / mean_n|y_c| * amp_mean over the WHOLE row, q = softmax_i(-(yhat_c - a_i)^2 / var)), after a
// first pass that forms the two means.  Every kept symbol is then read ONCE and all four rotation hypotheses of SER_q (:97-123) are accumulated in
// that pass; the winner -- fewest symbol errors of argmax(q), ties to the smallest h -- is picked at the end.  As in vaeq_epilogue_info.hip a
// rotation only exchanges the axes and reverses the level order, and g(n-1-i) = g(i) ^ n/2, so per axis the 2 log2(n_lev) bit-wise sums are formed
// once and every hypothesis is a selection among (axis, level in {t_I, n-1-t_I, t_Q, n-1-t_Q}).
// Integer counts are exact; float sums run per thread in symbol order, then over the wave's lanes (DPP, fixed order), then over the four waves in
// order: no atomics, two calls give identical bits.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "vaeq.h"
#include "vaeq_awgn_eval.h"
#include "vaeq_info.h"
#include "vaeq_launch.h"
#include "vaeq_wave.h"

namespace vaeq {

constexpr int AINFO_NT = 256, AINFO_WAVES = AINFO_NT / 64, AINFO_EDGE = 11;

struct AwgnInfoShared {
    float red[AINFO_WAVES];                   // eval_block_sum's scratch (y-mode: the two sums of |y_c|)
    float f[AINFO_WAVES][8];                  // [wave][2 h + (0: AIR terms, 1: GMI terms)]
    int c[AINFO_WAVES][8];                    // [wave][h: symbol errors | 4 + h: bit errors]
};

template <int NL, bool YMODE>
__global__ __launch_bounds__(AINFO_NT) void awgn_info_kernel(int N, const float *__restrict__ q, const float *__restrict__ y,
                                                             const __half *__restrict__ txg, const float *__restrict__ amp_g,
                                                             const float *__restrict__ Pg, const float *__restrict__ amp_mean,
                                                             const float *__restrict__ var, const int32_t *__restrict__ shift,
                                                             float *__restrict__ info, int32_t *__restrict__ counts)
{
    constexpr int S = NL - 1, NB = NL == 2 ? 1 : (NL == 4 ? 2 : 3);
    constexpr float LOG2E = 1.4426950408889634f;
    __shared__ AwgnInfoShared sh;
    const int run = blockIdx.x, tid = threadIdx.x;
    float *o = info + (size_t)run * 3;
    int32_t *cn = counts + (size_t)run * 4;
    // the window of validate_tail: kept symbol j < len pairs sample 11 + sft + j with TX symbol 11 + j; where it is not empty -10 <= sft <= N - 23,
    // so both stay inside [11, N - 11).  (64-bit: N - 22 - sft leaves int32 for a shift nobody can find but anybody can pass)
    const int sft = shift[run];
    const long long len64 = (long long)N - 2 * AINFO_EDGE - (long long)sft;
    bool empty = (long long)AINFO_EDGE + sft <= 0 || len64 <= 0;
    const int len = empty ? 0 : (int)len64;

    const float *src = YMODE ? y + (size_t)run * 2 * N : q + (size_t)run * 2 * NL * N;
    float amp[NL], sc[2] = {0.f, 0.f}, ivl = 0.f;
    if constexpr (YMODE) {
        // m_c = sum_n |y_c[n]| / N over the whole row: per thread in index order, over the wave's lanes, over the waves in order
        float sa0 = 0.f, sa1 = 0.f;
        if (!empty) {                                          // (uniform: every thread of the workgroup takes the same side)
#pragma unroll 4
            for (int n = tid; n < N; n += AINFO_NT) { sa0 += fabsf(src[n]); sa1 += fabsf(src[(size_t)N + n]); }
        }
        sa0 = eval_block_sum<AINFO_NT>(sa0, sh.red, tid);
        sa1 = eval_block_sum<AINFO_NT>(sa1, sh.red, tid);
        const float m0 = sa0 / (float)N, m1 = sa1 / (float)N, A = amp_mean[run];
        if (m0 == 0.f || m1 == 0.f) empty = true;              // a component that is zero throughout has no normalisation: no measurement
        sc[0] = A / m0; sc[1] = A / m1;
        ivl = LOG2E / var[run];
#pragma unroll
        for (int i = 0; i < NL; i++) amp[i] = amp_g[i];
    }
    if (empty) {                                               // nothing kept is no measurement (the NaN of the validation's SER)
        if (tid == 0) {
            o[0] = o[1] = o[2] = NAN;
            cn[0] = cn[1] = cn[2] = cn[3] = 0;
        }
        return;
    }

    const __half *txI = txg + (size_t)run * 2 * N, *txQ = txI + N;
    const float scale = 0.5f * S;
    float fs[8];
    int se[4], be[4];
#pragma unroll
    for (int i = 0; i < 8; i++) fs[i] = 0.f;
#pragma unroll
    for (int i = 0; i < 4; i++) se[i] = be[i] = 0;

    for (int j = tid; j < len; j += AINFO_NT) {
        const int m = AINFO_EDGE + sft + j, n = AINFO_EDGE + j;
        const int tI = min(max((int)rintf(scale * __half2float(txI[n]) + scale), 0), S);
        const int tQ = min(max((int)rintf(scale * __half2float(txQ[n]) + scale), 0), S);
        // v[c][i]: q-mode the posterior q, y-mode its unnormalised log2
        float v[2][NL];
        int d[2];
#pragma unroll
        for (int c = 0; c < 2; c++) {
            if constexpr (YMODE) {
                const float yv = src[(size_t)c * N + m] * sc[c];
#pragma unroll
                for (int i = 0; i < NL; i++) {
                    const float dd = yv - amp[i];
                    v[c][i] = -(dd * dd) * ivl;
                }
            } else {
#pragma unroll
                for (int i = 0; i < NL; i++) v[c][i] = src[(size_t)(c * NL + i) * N + m];
            }
            float best = v[c][0];
            int bi = 0;
#pragma unroll
            for (int i = 1; i < NL; i++)
                if (v[c][i] > best) { best = v[c][i]; bi = i; }                                  // first maximum, as argmax
            d[c] = bi;
        }
        // L[c][k][b]: log2 of the posterior mass of the levels whose label bit k is b; lse[c]: y-mode's log2 of the normaliser
        float L[2][NB][2], lse[2] = {0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 2; c++)
#pragma unroll
            for (int k = 0; k < NB; k++) {
                if constexpr (YMODE) {                         // log-sum-exp around each set's OWN maximum: no set underflows
                    float mx[2] = {-INFINITY, -INFINITY}, sm[2] = {0.f, 0.f};
#pragma unroll
                    for (int i = 0; i < NL; i++) { const int b = (info_gray(i) >> k) & 1; mx[b] = fmaxf(mx[b], v[c][i]); }
#pragma unroll
                    for (int i = 0; i < NL; i++) { const int b = (info_gray(i) >> k) & 1; sm[b] += __builtin_amdgcn_exp2f(v[c][i] - mx[b]); }
                    L[c][k][0] = mx[0] + __log2f(sm[0]);
                    L[c][k][1] = mx[1] + __log2f(sm[1]);
                    if (k == 0) {
                        const float hi = fmaxf(L[c][0][0], L[c][0][1]), lo = fminf(L[c][0][0], L[c][0][1]);
                        lse[c] = hi + __log2f(1.0f + __builtin_amdgcn_exp2f(lo - hi));
                    }
                } else {
                    float sm[2] = {0.f, 0.f};
#pragma unroll
                    for (int i = 0; i < NL; i++) sm[(info_gray(i) >> k) & 1] += v[c][i];
                    L[c][k][0] = info_log2(sm[0]);
                    L[c][k][1] = info_log2(sm[1]);
                }
            }
        // the two terms of every hypothesis are (axis c, level lv[j]) pairs
        const int lv[4] = {tI, S - tI, tQ, S - tQ};
        float A[2][4], G[2][4];
#pragma unroll
        for (int c = 0; c < 2; c++)
#pragma unroll
            for (int jj = 0; jj < 4; jj++) {
                const float pv = info_pick<NL>(v[c], lv[jj]);
                A[c][jj] = YMODE ? pv - lse[c] : info_log2(pv);
                const int g = info_gray(lv[jj]);
                float gs = 0.f;
#pragma unroll
                for (int k = 0; k < NB; k++) gs += ((g >> k) & 1) ? L[c][k][1] : L[c][k][0];
                G[c][jj] = YMODE ? gs - (float)NB * lse[c] : gs;
            }
        // decisions under rotation by 0, pi, pi/2, 3 pi/2 (SER_q, :97-123), and where the I' and the Q' term of each come from:
        // q'_I = q_I, rev q_I, rev q_Q, q_Q; q'_Q = q_Q, rev q_Q, q_I, rev q_I
        const int hI[4] = {d[0], S - d[0], S - d[1], d[1]}, hQ[4] = {d[1], S - d[1], d[0], S - d[0]};
        const int cI[4] = {0, 0, 1, 1}, jI[4] = {0, 1, 1, 0}, cQ[4] = {1, 1, 0, 0}, jQ[4] = {2, 3, 2, 3};
#pragma unroll
        for (int h = 0; h < 4; h++) {
            fs[2 * h + 0] += A[cI[h]][jI[h]] + A[cQ[h]][jQ[h]];
            fs[2 * h + 1] += G[cI[h]][jI[h]] + G[cQ[h]][jQ[h]];
            const int xI = info_gray(hI[h]) ^ info_gray(tI), xQ = info_gray(hQ[h]) ^ info_gray(tQ);
            se[h] += (xI | xQ) != 0;
            be[h] += __popc(xI) + __popc(xQ);
        }
    }

    const int lane = tid & 63, w = tid >> 6;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const float t = wave_sum_dpp(fs[i]);
        if (lane == 0) sh.f[w][i] = t;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int a = info_wave_sum(se[i]), b = info_wave_sum(be[i]);
        if (lane == 0) { sh.c[w][i] = a; sh.c[w][4 + i] = b; }
    }
    __syncthreads();
    if (tid == 0) {
        int tot[8];
        for (int i = 0; i < 8; i++) {
            tot[i] = 0;
            for (int k = 0; k < AINFO_WAVES; k++) tot[i] += sh.c[k][i];
        }
        int h = 0;
        for (int k = 1; k < 4; k++)
            if (tot[k] < tot[h]) h = k;                        // fewest symbol errors, ties to the smallest h
        float sa = 0.f, sg = 0.f;
        for (int k = 0; k < AINFO_WAVES; k++) { sa += sh.f[k][2 * h]; sg += sh.f[k][2 * h + 1]; }
        float H = 0.f;                                         // per-axis entropy of the run's pmf; a zero entry contributes 0
        for (int i = 0; i < NL; i++) {
            const float pi = Pg[run * NL + i];
            if (pi > 0.f) H -= pi * log2f(pi);
        }
        o[0] = 2.0f * H + sa / (float)len;
        o[1] = 2.0f * H + sg / (float)len;
        o[2] = (float)tot[4 + h] / ((float)(2 * NB) * (float)len);
        cn[0] = len; cn[1] = tot[h]; cn[2] = tot[4 + h]; cn[3] = h;
    }
}

}  // namespace vaeq

extern "C" int vaeq_awgn_info(int32_t R, int64_t N, int32_t n_lev, const float *q, const float *y, const void *data_f16, const float *amp,
                              const float *P, const float *amp_mean, const float *var, const int32_t *shift, float *info, int32_t *counts,
                              void *stream)
{
    if (R == 0) return VAEQ_OK;                                // an empty batch owns no memory: its pointers may be NULL
    if ((q != nullptr) == (y != nullptr)) return VAEQ_ERR_NULL;                                  // exactly one source of posteriors
    if (!data_f16 || !amp || !P || !shift || !info || !counts || (y && (!amp_mean || !var))) return VAEQ_ERR_NULL;
    if (R < 0 || N < 1 || N > 0x3fffffff) return VAEQ_ERR_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const __half *tx = reinterpret_cast<const __half *>(data_f16);
    return vaeq::dispatch_nlev(n_lev, [&](auto nl) {
        constexpr int NL = decltype(nl)::value;
        auto k = y ? vaeq::awgn_info_kernel<NL, true> : vaeq::awgn_info_kernel<NL, false>;
        return vaeq::launch(k, dim3(R), dim3(vaeq::AINFO_NT), 0, st, (int)N, q, y, tx, amp, P, amp_mean, var, shift, info, counts);
    });
}
