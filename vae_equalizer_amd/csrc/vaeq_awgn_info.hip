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
// This file holds the window, the pre-pass for the two means, the early-out and the VAE-LE demapper's exponent; the per-symbol body and the tail
// are vaeq_info.h's (info_symbol<NL, YMODE, 4>: no IQ flip; info_finish with K = len given, not counted), shared with the two DP kernels.
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

template <int NL, bool YMODE>
__global__ __launch_bounds__(AINFO_NT) void awgn_info_kernel(int N, const float *__restrict__ q, const float *__restrict__ y,
                                                             const __half *__restrict__ txg, const float *__restrict__ amp_g,
                                                             const float *__restrict__ Pg, const float *__restrict__ amp_mean,
                                                             const float *__restrict__ var, const int32_t *__restrict__ shift,
                                                             float *__restrict__ info, int32_t *__restrict__ counts)
{
    constexpr float LOG2E = 1.4426950408889634f;
    __shared__ float red[AINFO_WAVES];                         // eval_block_sum's scratch (y-mode: the two sums of |y_c|)
    __shared__ InfoShared<4, AINFO_WAVES> sh;
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
        sa0 = eval_block_sum<AINFO_NT>(sa0, red, tid);
        sa1 = eval_block_sum<AINFO_NT>(sa1, red, tid);
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
    float fs[8];
    int se[4], be[4];
#pragma unroll
    for (int i = 0; i < 8; i++) fs[i] = 0.f;
#pragma unroll
    for (int i = 0; i < 4; i++) se[i] = be[i] = 0;

    for (int j = tid; j < len; j += AINFO_NT) {
        const int m = AINFO_EDGE + sft + j, n = AINFO_EDGE + j;
        const __half txi = txI[n], txq = txQ[n];
        float v[2][NL];
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
        }
        info_symbol<NL, YMODE, 4>(v, txi, txq, fs, se, be);
    }
    info_finish<NL, 4, AINFO_WAVES, false>(sh, tid, fs, se, be, len, Pg + run * NL, o, cn);
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
