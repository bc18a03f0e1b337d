// vaeq_info.h -- the small helpers the information-rate kernels share (vaeq_epilogue_info.hip: a DP frame; vaeq_awgn_info.hip: an AWGN
// validation frame; vaeq_cma_info.hip: a frame of the constant-modulus DP baselines): the Gray label of a level, the floored log2 of a stored
// posterior, an integer wave sum, a register-array pick, and the y-mode body of one DP symbol.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>

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

// One kept symbol of a DP frame in y-mode, all eight hypotheses h = 4 flip + rot: the restatement of dp_epilogue_info_kernel<NL, true>'s loop body
// (vaeq_epilogue_info.hip, which keeps its own interleaved q- / y-mode text so that its instructions stay what they are) for kernels that
// address their samples differently (vaeq_cma_info.hip).  yv[c]: the sample of axis c, tI / tQ: the transmitted levels, pen[i] = nu_sc a_i^2,
// i2v = 1 / (2 var); fs[2 h + (0: AIR terms, 1: GMI terms)], se[h] symbol errors, be[h] bit errors are added to.
template <int NL>
__device__ __forceinline__ void info_symbol_y(const float (&yv)[2], int tI, int tQ, const float (&amp)[NL], const float (&pen)[NL], float i2v,
                                              float (&fs)[16], int (&se)[8], int (&be)[8])
{
    constexpr int S = NL - 1, NB = NL == 2 ? 1 : (NL == 4 ? 2 : 3);
    constexpr float LOG2E = 1.4426950408889634f;
    float v[2][NL];                                            // log2 of the unnormalised posterior (soft_demap<NLEV>'s exponent, vaeq_common.h)
    int d[2];
#pragma unroll
    for (int c = 0; c < 2; c++) {
#pragma unroll
        for (int i = 0; i < NL; i++) {
            const float dd = yv[c] - amp[i];
            v[c][i] = -(dd * dd * i2v + pen[i]) * LOG2E;
        }
        float best = v[c][0];
        int bi = 0;
#pragma unroll
        for (int i = 1; i < NL; i++)
            if (v[c][i] > best) { best = v[c][i]; bi = i; }    // first maximum, as argmax
        d[c] = bi;
    }
    // L[c][k][b]: log2 of the posterior mass of the levels whose label bit k is b, a log-sum-exp around each set's OWN maximum; lse[c]: the normaliser
    float L[2][NB][2], lse[2] = {0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
        for (int k = 0; k < NB; k++) {
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
        }
    const int lv[4] = {tI, S - tI, tQ, S - tQ};                // the two terms of every hypothesis are (axis c, level lv[j]) pairs
    float A[2][4], G[2][4];
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            A[c][j] = info_pick<NL>(v[c], lv[j]) - lse[c];
            const int g = info_gray(lv[j]);
            float gs = 0.f;
#pragma unroll
            for (int k = 0; k < NB; k++) gs += ((g >> k) & 1) ? L[c][k][1] : L[c][k][0];
            G[c][j] = gs - (float)NB * lse[c];
        }
    const int hI[4] = {d[0], S - d[0], S - d[1], d[1]}, hQ[4] = {d[1], S - d[1], d[0], S - d[0]};   // decisions under rotation by 0, pi, pi/2, 3 pi/2
#pragma unroll
    for (int f = 0; f < 2; f++) {
        const int jq = f ? 3 : 2, jr = f ? 2 : 3;              // lv[jq] = TX Q level under the IQ flip f, lv[jr] = its reverse
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

}  // namespace vaeq
