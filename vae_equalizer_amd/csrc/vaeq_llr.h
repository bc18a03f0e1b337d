// vaeq_llr.h -- the per-symbol body of the four LLR kernels (vaeq_epilogue_llr.hip: a DP frame; vaeq_awgn_llr.hip: an AWGN validation frame;
// vaeq_cma_llr.hip: a frame of the constant-modulus DP baselines; vaeq_awgn_track_llr.hip: a soft sequence of the AWGN baselines): the
// a-posteriori log-likelihood ratio of every label bit of one received symbol, and which of them is which transmitted bit under a hypothesis.
// What decides v -- window, alignment, pre-pass, load, demapper -- is vaeq_info.h's and vaeq_awgn_eval.h's, the text the information-rate
// siblings run.
//
// Level i of an axis carries the label g(i) = i ^ (i >> 1) (info_gray), b = log2 n_lev bits, bit b-1 the top one.  For a received axis c
//     lam[c][k] = ln 2 (L[c][k][0] - L[c][k][1])      nats, positive = bit 0, priors included
// with L[c][k][s] the log2 of the posterior mass of the levels whose label bit k is s -- vaeq_info.h's L of info_symbol.  These set sums are the
// one thing the pairs still state twice: with both bodies on one function every bit stayed, but the information-rate kernels' y-mode ran 0.4-3 %
// slower and one launch left the parent's range.  tests/test_llr_bits_gpu.py and tests/test_info_bits_gpu.py pin each copy's
// bits, and the LLR tests pin one to the other through the GMI, which is an exact function of the LLRs.
//   q-mode: info_log2 of the two set sums, added in ascending i; an exact 0 costs 126 bit, so every LLR is finite.
//   y-mode: v is the unnormalised log2 posterior; each set is a log-sum-exp around its own maximum, so no set underflows.
// Hypothesis h = 4 flip + rot (rot: 0, pi, pi/2, 3 pi/2, as in info_symbol) says where the transmitted axes are found:
//     rot     I' from              Q' from
//     0       axis 0               axis 1
//     pi      axis 0, reversed     axis 1, reversed
//     pi/2    axis 1, reversed     axis 0
//     3 pi/2  axis 1               axis 0, reversed
// and the flip reverses Q' once more.  Reversing the level order flips the top label bit only (g(n-1-i) = g(i) ^ n/2): "reversed" negates plane
// b-1 of that axis and nothing else.  h selects registers; no address depends on it.
#pragma once
#include <hip/hip_runtime.h>

#include "vaeq_info.h"

namespace vaeq {

constexpr int llr_bits(int n_lev) { return n_lev == 2 ? 1 : (n_lev == 4 ? 2 : 3); }

// lam[k] of one received axis
template <int NL, bool YMODE>
__device__ __forceinline__ void llr_axis(const float (&v)[NL], float (&lam)[llr_bits(NL)])
{
    constexpr float LN2 = 0.6931471805599453f;
#pragma unroll
    for (int k = 0; k < llr_bits(NL); k++) {
        float L0, L1;
        if constexpr (YMODE) {
            float mx[2] = {-INFINITY, -INFINITY}, sm[2] = {0.f, 0.f};
#pragma unroll
            for (int i = 0; i < NL; i++) { const int s = (info_gray(i) >> k) & 1; mx[s] = fmaxf(mx[s], v[i]); }
#pragma unroll
            for (int i = 0; i < NL; i++) { const int s = (info_gray(i) >> k) & 1; sm[s] += __builtin_amdgcn_exp2f(v[i] - mx[s]); }
            L0 = mx[0] + __log2f(sm[0]);
            L1 = mx[1] + __log2f(sm[1]);
        } else {
            float sm[2] = {0.f, 0.f};
#pragma unroll
            for (int i = 0; i < NL; i++) sm[(info_gray(i) >> k) & 1] += v[i];
            L0 = info_log2(sm[0]);
            L1 = info_log2(sm[1]);
        }
        lam[k] = LN2 * (L0 - L1);
    }
}

// One kept symbol: v[c][i] as info_symbol takes it (axis c, level i), h the hypothesis (the caller masks it to the ones it has) ->
// out[a * b + k] = the LLR of bit k of TX axis a (0 = I, 1 = Q)
template <int NL, bool YMODE>
__device__ __forceinline__ void llr_symbol(const float (&v)[2][NL], int h, float (&out)[2 * llr_bits(NL)])
{
    constexpr int NB = llr_bits(NL);
    float lam[2][NB];
    llr_axis<NL, YMODE>(v[0], lam[0]);
    llr_axis<NL, YMODE>(v[1], lam[1]);
    const int rot = h & 3;
    const bool swap = rot >= 2, revI = rot == 1 || rot == 2, revQ = (rot == 1 || rot == 3) != ((h & 4) != 0);
#pragma unroll
    for (int k = 0; k < NB; k++) {
        const float aI = swap ? lam[1][k] : lam[0][k], aQ = swap ? lam[0][k] : lam[1][k];
        out[k] = (k == NB - 1 && revI) ? -aI : aI;
        out[NB + k] = (k == NB - 1 && revQ) ? -aQ : aQ;
    }
}

}  // namespace vaeq
