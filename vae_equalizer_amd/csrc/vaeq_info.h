// vaeq_info.h -- what the information-rate kernels and their LLR siblings share (vaeq_epilogue_info / _llr.hip: a DP frame; vaeq_awgn_info /
// _llr.hip: an AWGN validation frame; vaeq_cma_info / _llr.hip: a frame of the constant-modulus DP baselines; vaeq_awgn_track_info / _llr.hip: a
// soft sequence of the AWGN baselines).  An LLR kernel reports the LLRs of the posteriors whose GMI its sibling reports only if both see the same
// symbols and the same floats, so everything that decides either is written once, here: the clamp of a shift, the DP alignment (InfoAlign), the
// CMA frame with its radius walk and two-stage addressing (CmaFrame, cma_radius_factor), the q-mode load and both demappers' exponents
// (info_load_q, info_demap_setup / info_demap_log2, info_awgn_log2); vaeq_awgn_eval.h holds the AWGN family's window and pre-passes.  The
// information-rate kernels' own definition follows: the level of a TX sample, the per-symbol body info_symbol (argmax, bit-wise sets, the terms
// of every hypothesis, their accumulation) and the tail info_finish (wave and workgroup sums, the winning hypothesis, the entropy, the K == 0
// rule, the 3 + 4 outputs); vaeq_llr.h holds the LLR body.
// A kernel keeps its launch shape, its early-out or plane stores and what is truly its own (KeepWalk, the tail calls, the split grid).
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
// the alignment a DP epilogue found for a run (11 <= n, |shift| <= 10, and the window ends 11 + max|shift| before the row does)
struct InfoAlign {
    int s0, s1, r, ms;
    template <class Run>                      // (an int in the one kernel, a size_t in the other: the index arithmetic stays the caller's)
    __device__ __forceinline__ InfoAlign(const int32_t *__restrict__ shift, const int32_t *__restrict__ rflag, Run run)
        : s0(info_clamp_shift(shift[run * 2 + 0])), s1(info_clamp_shift(shift[run * 2 + 1])), r(rflag[run] & 1), ms(max(abs(s0), abs(s1))) {}
    __device__ __forceinline__ int sp(int p) const { return (p - r) & 1; }   // roll(r, 0): row p comes from row p - r
    __device__ __forceinline__ int sft(int p) const { return p ? s1 : s0; }  // roll(-shift): out[n] = in[n + shift]
};

// q-mode: the stored posteriors of axis c of sample m, src = the 2 NL rows [axis][level][N] of the received polarisation
template <int NL>
__device__ __forceinline__ void info_load_q(const float *__restrict__ src, int N, int m, int c, float (&v)[NL])
{
#pragma unroll
    for (int i = 0; i < NL; i++) v[i] = src[(size_t)(c * NL + i) * N + m];
}
// y-mode of the DP soft demapper: the constants of run `run` whose posteriors polarisation `row` of var made -- amp[i], pen[i] = nu_sc a_i^2 and,
// returned, i2v = 1 / (2 var) ...  (dp_epilogue_info_kernel alone states these three lines itself: called from there, whatever the order of the
// loads and the type of run, the function moved that kernel's y-mode schedule and cost it 2.3 %)
template <int NL>
__device__ __forceinline__ float info_demap_setup(const float *__restrict__ amp_g, const float *__restrict__ nu_sc, const float *__restrict__ var,
                                                  size_t run, int row, float (&amp)[NL], float (&pen)[NL])
{
    const float nusc = nu_sc[run];
#pragma unroll
    for (int i = 0; i < NL; i++) { amp[i] = amp_g[i]; pen[i] = nusc * (amp[i] * amp[i]); }
    return 0.5f / var[run * 2 + row];
}
// ... and log2 of the unnormalised posterior of sample yv (soft_demap<NLEV>'s exponent, vaeq_common.h)
template <int NL>
__device__ __forceinline__ void info_demap_log2(float yv, const float (&amp)[NL], const float (&pen)[NL], float i2v, float (&v)[NL])
{
#pragma unroll
    for (int i = 0; i < NL; i++) {
        const float dd = yv - amp[i];
        v[i] = -(dd * dd * i2v + pen[i]) * 1.4426950408889634f;
    }
}
// y-mode of the AWGN reference's own demapper (func_VAELE_MQAM_shaping.py:229: -(y - a_i)^2 / var per axis, no 1/2, no prior term): log2 of the
// unnormalised posterior of the scaled sample yv, ivl = log2 e / var
constexpr float INFO_LOG2E = 1.4426950408889634f;
template <int NL>
__device__ __forceinline__ void info_awgn_log2(float yv, const float (&amp)[NL], float ivl, float (&v)[NL])
{
#pragma unroll
    for (int i = 0; i < NL; i++) {
        const float dd = yv - amp[i];
        v[i] = -(dd * dd) * ivl;
    }
}

// One frame of the constant-modulus DP baselines as vaeq_cma_epilogue aligned it, rebuilt from the raw y and the four alignment outputs:
//   stage c:  ya[p'][c][m] = y[(p' - r_c) & 1][c][(m + shift_c[p']) mod N],   W_c = [EDGE, endc)
//   stage q:  kept symbol n in [EDGE, endq) of output polarisation p reads ya[p' = (p - r_q) & 1][:, m = n + shift_q[p]]
// Both alignments are clamped to what the epilogue can find: with 11 <= n and a window that ends 11 + max|shift| before the row does, n + shift
// stays inside [1, N - 1) in either stage; only the stage-c roll of a sample outside W_c can wrap around the frame.
struct CmaFrame {
    int N, c0, c1, q0, q1, rc, rq, endc, endq;
    const float *yr;                          // y[run]: [2][2][N]
    const __half *txr;                        // tx[run]: [2][2][N]
    __device__ __forceinline__ CmaFrame(int run, int N_, const float *__restrict__ y, const __half *__restrict__ txg,
                                        const int32_t *__restrict__ shift_c, const int32_t *__restrict__ r_c,
                                        const int32_t *__restrict__ shift_q, const int32_t *__restrict__ r_q)
        : N(N_), c0(info_clamp_shift(shift_c[run * 2 + 0])), c1(info_clamp_shift(shift_c[run * 2 + 1])),
          q0(info_clamp_shift(shift_q[run * 2 + 0])), q1(info_clamp_shift(shift_q[run * 2 + 1])), rc(r_c[run] & 1), rq(r_q[run] & 1),
          endc(N_ - EDGE - max(abs(c0), abs(c1))), endq(N_ - EDGE - max(abs(q0), abs(q1))), yr(y + (size_t)run * 4 * N_),
          txr(txg + (size_t)run * 4 * N_) {}
    __device__ __forceinline__ bool kept(int n) const { return n >= EDGE && n < endq; }
    // the source of output polarisation p: pp, the stage-c aligned row it comes from (whose demapper made its posteriors), and that row's I row in y
    __device__ __forceinline__ int aligned_row(int p) const { return (p - rq) & 1; }
    __device__ __forceinline__ const float *y_row(int p) const { return yr + (size_t)(((aligned_row(p) - rc) & 1) * 2) * N; }
    // kept symbol n of output polarisation p -> its index ms in y_row(p), and g = fac exactly where its stage-c aligned index lies in W_c, else 1
    __device__ __forceinline__ int source(int p, int n, float fac, float &g) const
    {
        const int m = n + (p ? q1 : q0);                       // index in the stage-c aligned sequence, 1 <= m < N - 1
        int ms = m + (aligned_row(p) ? c1 : c0);               // index in y: -9 <= ms < N + 9, one wrap at most (N >= 43)
        if (ms >= N) ms -= N;
        if (ms < 0) ms += N;
        g = (m >= EDGE && m < endc) ? fac : 1.0f;
        return ms;
    }
};

// fac = sum_{p', m in W_c} |tx[p'][:, m]| / sum_{p', m in W_c} |ya[p'][:, m]|, the mean radius of TX over that of the stage-c aligned output, both
// polarisations (shared_funcs.py:242): per thread at stride EPI_NT, over the wave's lanes (DPP, fixed order), over the WAVES waves in order.  It
// multiplies every sample of W_c, so both kernels of the pair -- and on a split grid both workgroups of a run -- form it here, the same float.
// rad: [WAVES][2] floats of LDS.  Returns fac in every thread; degenerate: sum |ya| == 0, no radius, no normalisation -- the run keeps nothing.
template <int WAVES>
__device__ __forceinline__ float cma_radius_factor(const CmaFrame &f, float (*rad)[2], int tid, bool &degenerate)
{
    const int N = f.N;
    float st = 0.f, sy = 0.f;
    for (int n = tid; n < N; n += EPI_NT) {
        if (n < EDGE || n >= f.endc) continue;
#pragma unroll
        for (int pp = 0; pp < 2; pp++) {
            const int sp = (pp - f.rc) & 1, m = n + (pp ? f.c1 : f.c0);                          // 1 <= m < N - 1
            const float ti = __half2float(f.txr[(size_t)(pp * 2 + 0) * N + n]), tq = __half2float(f.txr[(size_t)(pp * 2 + 1) * N + n]);
            const float yi = f.yr[(size_t)(sp * 2 + 0) * N + m], yq = f.yr[(size_t)(sp * 2 + 1) * N + m];
            st += sqrtf(fmaf(ti, ti, tq * tq));
            sy += sqrtf(fmaf(yi, yi, yq * yq));
        }
    }
    st = wave_sum_dpp(st);
    sy = wave_sum_dpp(sy);
    if ((tid & 63) == 0) { rad[tid >> 6][0] = st; rad[tid >> 6][1] = sy; }
    __syncthreads();
    st = sy = 0.f;
    for (int k = 0; k < WAVES; k++) { st += rad[k][0]; sy += rad[k][1]; }
    degenerate = sy == 0.f;
    return st / sy;
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
