// vaeq_epilogue_info.hip -- information-rate figures of one DP frame on the device: achievable rate of symbol-wise mismatched decoding (AIR),
// generalised mutual information of the bit-wise decoder (GMI) and the pre-FEC bit error rate, per run and polarisation, over exactly the
// symbols the q-SER of vaeq_dp_epilogue keeps (same roll by shift_q, same polarisation exchange, same per-minibatch cut and frame-edge slice:
// vaeq_epilogue_keep.h).  The reference has no such metric; the definitions are closed-form (tests/_ref_info.py).
//
// One workgroup per (run, polarisation).  Every kept symbol's posteriors are read ONCE (q-mode: 2 n_lev floats from q; y-mode: the two
// equalised samples, demapped again in the log domain) and all eight hypotheses h = 4 flip + rot of SER_IQflip (shared_funcs.py:188-222) are
// accumulated in that pass; the winner -- fewest symbol errors of argmax(q), ties to the smallest h, so its count is the q-SER's -- is
// picked at the end.  What makes eight hypotheses cheap: a rotation only exchanges the axes and reverses the level order, and the
// binary-reflected Gray label of the reversed level differs from the level's in the top bit alone (g(n-1-i) = g(i) ^ n/2), so the bit-wise
// sums of a reversed posterior at level t are the unreversed ones at level n-1-t.  Per axis the 2 log2(n_lev) bit-wise sums are formed once;
// every hypothesis is then a selection among (axis, level in {t_I, n-1-t_I, t_Q, n-1-t_Q}).
// Integer counts are exact; float sums run per thread in symbol order, then over the wave's lanes (DPP, fixed order), then over the four waves
// in order: two calls give identical bits.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "vaeq.h"
#include "vaeq_common.h"
#include "vaeq_epilogue_keep.h"
#include "vaeq_info.h"
#include "vaeq_launch.h"
#include "vaeq_wave.h"

namespace vaeq {

constexpr int INFO_WAVES = EPI_NT / 64;

struct InfoShared {
    float f[INFO_WAVES][16];                  // [wave][2 h + (0: AIR terms, 1: GMI terms)]
    int c[INFO_WAVES][17];                    // [wave][h: symbol errors | 8 + h: bit errors | 16: kept]
};

template <int NL, bool YMODE>
__global__ __launch_bounds__(EPI_NT) void dp_epilogue_info_kernel(int N, int batch_len, const float *__restrict__ q, const float *__restrict__ y,
                                                                  const __half *__restrict__ txg, const float *__restrict__ amp_g,
                                                                  const float *__restrict__ Pg, const float *__restrict__ var,
                                                                  const float *__restrict__ nu_sc, const int32_t *__restrict__ shift,
                                                                  const int32_t *__restrict__ rflag, float *__restrict__ info,
                                                                  int32_t *__restrict__ counts)
{
    constexpr int S = NL - 1, NB = NL == 2 ? 1 : (NL == 4 ? 2 : 3);
    constexpr float LOG2E = 1.4426950408889634f;
    __shared__ InfoShared sh;
    const int run = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
    // the alignment the epilogue found; clamped to what it can find, so that a kept symbol's partner n + shift never leaves the row
    // (11 <= n, |shift| <= 10, and the window ends 11 + max|shift| before the row does)
    const int s0 = min(max(shift[run * 2 + 0], -HALF_SHIFT), HALF_SHIFT), s1 = min(max(shift[run * 2 + 1], -HALF_SHIFT), HALF_SHIFT);
    const int r = rflag[run] & 1, ms = max(abs(s0), abs(s1));
    const int sp = (p - r) & 1, sft = p ? s1 : s0;             // roll(r, 0): row p comes from row p - r; roll(-shift): out[n] = in[n + shift]
    const __half *txI = txg + ((size_t)run * 4 + p * 2) * N, *txQ = txI + N;
    const float *src = YMODE ? y + ((size_t)run * 4 + sp * 2) * N : q + ((size_t)run * 4 + sp * 2) * NL * N;
    const float scale = 0.5f * S;
    float amp[NL], pen[NL];
    float i2v = 0.f;
    if constexpr (YMODE) {
        const float nusc = nu_sc[run];
        i2v = 0.5f / var[run * 2 + sp];                        // the demapper of the RECEIVED polarisation made this row's q
#pragma unroll
        for (int i = 0; i < NL; i++) { amp[i] = amp_g[i]; pen[i] = nusc * (amp[i] * amp[i]); }
    }

    float fs[16];
    int se[8], be[8], kept = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) fs[i] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; i++) se[i] = be[i] = 0;

    KeepWalk kw(tid, N, batch_len, s0, ms);
    for (int n = tid; n < N; n += EPI_NT, kw.next()) {
        const int m = n + sft;
        if (!kw.keep(n) || m < 0 || m >= N) continue;
        kept++;
        const int tI = min(max((int)rintf(scale * __half2float(txI[n]) + scale), 0), S);         // shared_funcs.py:198
        const int tQ = min(max((int)rintf(scale * __half2float(txQ[n]) + scale), 0), S);
        // v[c][i]: q-mode the posterior q, y-mode its unnormalised log2 (soft_demap<NLEV>'s exponent, vaeq_common.h)
        float v[2][NL];
        int d[2];
#pragma unroll
        for (int c = 0; c < 2; c++) {
            if constexpr (YMODE) {
                const float yv = src[(size_t)c * N + m];
#pragma unroll
                for (int i = 0; i < NL; i++) {
                    const float dd = yv - amp[i];
                    v[c][i] = -(dd * dd * i2v + pen[i]) * LOG2E;
                }
            } else {
#pragma unroll
                for (int i = 0; i < NL; i++) v[c][i] = src[(size_t)(c * NL + i) * N + m];
            }
            float best = v[c][0];
            int bi = 0;
#pragma unroll
            for (int i = 1; i < NL; i++)
                if (v[c][i] > best) { best = v[c][i]; bi = i; }                                  // first maximum, as argmax (:201)
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
            for (int j = 0; j < 4; j++) {
                const float pv = info_pick<NL>(v[c], lv[j]);
                A[c][j] = YMODE ? pv - lse[c] : info_log2(pv);
                const int g = info_gray(lv[j]);
                float gs = 0.f;
#pragma unroll
                for (int k = 0; k < NB; k++) gs += ((g >> k) & 1) ? L[c][k][1] : L[c][k][0];
                G[c][j] = YMODE ? gs - (float)NB * lse[c] : gs;
            }
        // decisions under rotation by 0, pi, pi/2, 3 pi/2 (:201-217)
        const int hI[4] = {d[0], S - d[0], S - d[1], d[1]}, hQ[4] = {d[1], S - d[1], d[0], S - d[0]};
#pragma unroll
        for (int f = 0; f < 2; f++) {
            const int jq = f ? 3 : 2, jr = f ? 2 : 3;          // lv[jq] = TX Q level under the IQ flip f (:199), lv[jr] = its reverse
            // (axis, level) of the I' term and of the Q' term: q'_I = q_I, rev q_I, rev q_Q, q_Q; q'_Q = q_Q, rev q_Q, q_I, rev q_I
            const int cI[4] = {0, 0, 1, 1}, jI[4] = {0, 1, 1, 0}, cQ[4] = {1, 1, 0, 0}, jQ[4] = {jq, jr, jq, jr};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int h = 4 * f + k;
                fs[2 * h + 0] += A[cI[k]][jI[k]] + A[cQ[k]][jQ[k]];
                fs[2 * h + 1] += G[cI[k]][jI[k]] + G[cQ[k]][jQ[k]];
                const int xI = info_gray(hI[k]) ^ info_gray(tI), xQ = info_gray(hQ[k]) ^ info_gray(lv[jq]);
                se[h] += (xI | xQ) != 0;
                be[h] += __popc(xI) + __popc(xQ);
            }
        }
    }

    const int lane = tid & 63, w = tid >> 6;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const float t = wave_sum_dpp(fs[i]);
        if (lane == 0) sh.f[w][i] = t;
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int a = info_wave_sum(se[i]), b = info_wave_sum(be[i]);
        if (lane == 0) { sh.c[w][i] = a; sh.c[w][8 + i] = b; }
    }
    kept = info_wave_sum(kept);
    if (lane == 0) sh.c[w][16] = kept;
    __syncthreads();
    if (tid == 0) {
        int tot[17];
        for (int i = 0; i < 17; i++) {
            tot[i] = 0;
            for (int k = 0; k < INFO_WAVES; k++) tot[i] += sh.c[k][i];
        }
        int h = 0;
        for (int k = 1; k < 8; k++)
            if (tot[k] < tot[h]) h = k;                        // fewest symbol errors, ties to the smallest h
        float sa = 0.f, sg = 0.f;
        for (int k = 0; k < INFO_WAVES; k++) { sa += sh.f[k][2 * h]; sg += sh.f[k][2 * h + 1]; }
        float H = 0.f;                                         // per-axis entropy of the run's pmf; a zero entry contributes 0
        for (int i = 0; i < NL; i++) {
            const float pi = Pg[run * NL + i];
            if (pi > 0.f) H -= pi * log2f(pi);
        }
        float *o = info + ((size_t)run * 2 + p) * 3;
        int32_t *c = counts + ((size_t)run * 2 + p) * 4;
        const int K = tot[16];
        if (K == 0) {                                          // nothing kept is no measurement (the convention of the SER rows)
            o[0] = o[1] = o[2] = NAN;
            c[0] = c[1] = c[2] = c[3] = 0;
        } else {
            o[0] = 2.0f * H + sa / (float)K;
            o[1] = 2.0f * H + sg / (float)K;
            o[2] = (float)tot[8 + h] / ((float)(2 * NB) * (float)K);
            c[0] = K; c[1] = tot[h]; c[2] = tot[8 + h]; c[3] = h;
        }
    }
}

}  // namespace vaeq

extern "C" int vaeq_dp_epilogue_info(int32_t R, int64_t N, int32_t n_lev, int32_t batch_len, const float *q, const float *y, const void *tx_f16,
                                     const float *amp, const float *P, const float *var, const float *nu_sc, const int32_t *shift,
                                     const int32_t *rflag, float *info, int32_t *counts, void *stream)
{
    if (R == 0) return VAEQ_OK;                                // an empty batch owns no memory: its pointers may be NULL
    if ((q != nullptr) == (y != nullptr)) return VAEQ_ERR_NULL;                                  // exactly one source of posteriors
    if (!tx_f16 || !amp || !P || !shift || !rflag || !info || !counts || (y && (!var || !nu_sc))) return VAEQ_ERR_NULL;
    if (R < 0 || N < 2 * vaeq::EDGE + vaeq::N_SHIFT || N > 0x3fffffff || batch_len < 0 || (batch_len > 0 && N % batch_len)) return VAEQ_ERR_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const __half *tx = reinterpret_cast<const __half *>(tx_f16);
    return vaeq::dispatch_nlev(n_lev, [&](auto nl) {
        constexpr int NL = decltype(nl)::value;
        auto k = y ? vaeq::dp_epilogue_info_kernel<NL, true> : vaeq::dp_epilogue_info_kernel<NL, false>;
        return vaeq::launch(k, dim3(R, 2), dim3(vaeq::EPI_NT), 0, st, (int)N, batch_len, q, y, tx, amp, P, var, nu_sc, shift, rflag, info, counts);
    });
}
