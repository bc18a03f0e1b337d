// vaeq_info.h -- what the three information-rate kernels share (vaeq_epilogue_info.hip: a DP frame; vaeq_awgn_info.hip: an AWGN validation frame;
// vaeq_cma_info.hip: a frame of the constant-modulus DP baselines), which is the definition of their figures: the level of a TX sample and the
// clamp of a shift, the per-symbol body info_symbol (argmax, bit-wise sets, the terms of every hypothesis, their accumulation) and the tail
// info_finish (wave and workgroup sums, the winning hypothesis, the entropy, the K == 0 rule, the 3 + 4 outputs).  A kernel keeps its addressing,
// its pre-pass, its early-out and the one or two lines that form v, the posteriors (q-mode) or their unnormalised log2 (y-mode) of one symbol.
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "vaeq_epilogue_keep.h"
#include "vaeq_wave.h"

namespace vaeq {

__device__ __forceinline__ int info_gray(int i) { return i ^ (i >> 1); }
__device__ __forceinline__ float info_log2(float x) { return __log2f(fmaxf(x, FLT_MIN)); }       // l(x) of q-mode: an exact 0 costs 126 bit, not infinity
__device__ __forceinline__ int info_wave_sum(int v)
{
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
template <int NL>
__device__ __forceinline__ float info_pick(const float (&v)[NL], int l)     // v[l] without a register array indexed at run time
{
    float r = v[0];
#pragma unroll
    for (int i = 1; i < NL; i++) r = l == i ? v[i] : r;
    return r;
}
template <int NL>
__device__ __forceinline__ int info_tx_level(__half tx)                     // the level index of a TX sample (shared_funcs.py:198)
{
    constexpr float scale = 0.5f * (NL - 1);
    return min(max((int)rintf(scale * __half2float(tx) + scale), 0), NL - 1);
}
// an alignment clamped to what the epilogues can find, so that a kept symbol's partner n + shift never leaves the row
__device__ __forceinline__ int info_clamp_shift(int s) { return min(max(s, -HALF_SHIFT), HALF_SHIFT); }
// y-mode of the DP soft demapper: log2 of the unnormalised posterior of sample yv (soft_demap<NLEV>'s exponent, vaeq_common.h), pen[i] = nu_sc a_i^2,
// i2v = 1 / (2 var)
template <int NL>
__device__ __forceinline__ void info_demap_log2(float yv, const float (&amp)[NL], const float (&pen)[NL], float i2v, float (&v)[NL])
{
#pragma unroll
    for (int i = 0; i < NL; i++) {
        const float dd = yv - amp[i];
        v[i] = -(dd * dd * i2v + pen[i]) * 1.4426950408889634f;
    }
}

// One kept symbol, all NH hypotheses.  v[c][i]: axis c, level i -- q-mode the posterior q, y-mode its unnormalised log2; txI / txQ: the transmitted
// samples.  NH = 4: the rotations by 0, pi, pi/2, 3 pi/2 of SER_q (func_VAELE_MQAM_shaping.py:97-123); NH = 8: h = 4 flip + rot of SER_IQflip
// (shared_funcs.py:188-222), the flip reversing the TX Q level.  fs[2 h + (0: AIR terms, 1: GMI terms)], se[h] symbol errors, be[h] bit errors
// are added to.  (The samples are quantised here and not by the caller: the compiler simplifies this body before it inlines it, and handed the
// levels as plain integers it folds the level compares another way -- measured, that form cost the DP kernel's y-mode 1-2 %)
template <int NL, bool YMODE, int NH>
__device__ __forceinline__ void info_symbol(const float (&v)[2][NL], __half txI, __half txQ, float (&fs)[2 * NH], int (&se)[NH], int (&be)[NH])
{
    static_assert(NH == 4 || NH == 8, "four rotations, with or without the IQ flip");
    constexpr int S = NL - 1, NB = NL == 2 ? 1 : (NL == 4 ? 2 : 3);
    const int tI = info_tx_level<NL>(txI), tQ = info_tx_level<NL>(txQ);
    int d[2];
#pragma unroll
    for (int c = 0; c < 2; c++) {
        float best = v[c][0];
        int bi = 0;
#pragma unroll
        for (int i = 1; i < NL; i++)
            if (v[c][i] > best) { best = v[c][i]; bi = i; }    // first maximum, as argmax (:201)
        d[c] = bi;
    }
    // L[c][k][b]: log2 of the posterior mass of the levels whose label bit k is b; lse[c]: y-mode's log2 of the normaliser
    float L[2][NB][2], lse[2] = {0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
        for (int k = 0; k < NB; k++) {
            if constexpr (YMODE) {                             // log-sum-exp around each set's OWN maximum: no set underflows
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
    for (int f = 0; f < NH / 4; f++) {
        const int jq = f ? 3 : 2, jr = f ? 2 : 3;              // lv[jq] = TX Q level under the IQ flip f (:199), lv[jr] = its reverse
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

template <int NH, int WAVES>
struct InfoShared {
    float f[WAVES][2 * NH];                   // [wave][2 h + (0: AIR terms, 1: GMI terms)]
    int c[WAVES][2 * NH];                     // [wave][h: symbol errors | NH + h: bit errors]
    int kept[WAVES];                          // [wave] kept symbols, where info_finish counts them
};

// The tail of a workgroup of WAVES waves: the threads' sums over the wave's lanes (floats by DPP in a fixed order), over the waves in order; then
// thread 0 picks the hypothesis, forms the per-axis entropy of the pmf P[NL] and writes o[0..2] = AIR, GMI, BER and c[0..3] = kept, symbol errors,
// bit errors, hypothesis -- NaN and zeros when nothing is kept, which is no measurement (the convention of the SER rows).
// K: the symbols this thread kept, summed here (COUNT), or the symbols the workgroup kept, which every thread knows.
// The caller puts a __syncthreads() behind it before sh is used again.
template <int NL, int NH, int WAVES, bool COUNT>
__device__ __forceinline__ void info_finish(InfoShared<NH, WAVES> &sh, int tid, const float (&fs)[2 * NH], const int (&se)[NH], const int (&be)[NH],
                                            int K, const float *__restrict__ P, float *__restrict__ o, int32_t *__restrict__ c)
{
    constexpr int NB = NL == 2 ? 1 : (NL == 4 ? 2 : 3);
    const int lane = tid & 63, w = tid >> 6;
#pragma unroll
    for (int i = 0; i < 2 * NH; i++) {
        const float t = wave_sum_dpp(fs[i]);
        if (lane == 0) sh.f[w][i] = t;
    }
#pragma unroll
    for (int i = 0; i < NH; i++) {
        const int a = info_wave_sum(se[i]), b = info_wave_sum(be[i]);
        if (lane == 0) { sh.c[w][i] = a; sh.c[w][NH + i] = b; }
    }
    if constexpr (COUNT) {
        K = info_wave_sum(K);
        if (lane == 0) sh.kept[w] = K;
    }
    __syncthreads();
    if (tid == 0) {
        int tot[2 * NH];
        for (int i = 0; i < 2 * NH; i++) {
            tot[i] = 0;
            for (int k = 0; k < WAVES; k++) tot[i] += sh.c[k][i];
        }
        int h = 0;
        for (int k = 1; k < NH; k++)
            if (tot[k] < tot[h]) h = k;                        // fewest symbol errors, ties to the smallest h
        float sa = 0.f, sg = 0.f;
        for (int k = 0; k < WAVES; k++) { sa += sh.f[k][2 * h]; sg += sh.f[k][2 * h + 1]; }
        float H = 0.f;                                         // per-axis entropy of the run's pmf; a zero entry contributes 0
        for (int i = 0; i < NL; i++) {
            const float pi = P[i];
            if (pi > 0.f) H -= pi * log2f(pi);
        }
        if constexpr (COUNT) {
            K = 0;
            for (int k = 0; k < WAVES; k++) K += sh.kept[k];
        }
        if (K == 0) {
            o[0] = o[1] = o[2] = NAN;
            c[0] = c[1] = c[2] = c[3] = 0;
        } else {
            o[0] = 2.0f * H + sa / (float)K;
            o[1] = 2.0f * H + sg / (float)K;
            o[2] = (float)tot[NH + h] / ((float)(2 * NB) * (float)K);
            c[0] = K; c[1] = tot[h]; c[2] = tot[NH + h]; c[3] = h;
        }
    }
}

}  // namespace vaeq
