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
// This file holds the early-out and the accumulation.  The window, the pre-pass for the two means, the q-mode load and the VAE-LE demapper's
// exponent are the text awgn_llr_kernel runs as well (TrackWindow and awgn_row_scales of vaeq_awgn_eval.h, info_load_q and info_awgn_log2 of
// vaeq_info.h); the per-symbol body and the tail are vaeq_info.h's (info_symbol<NL, YMODE, 4>: no IQ flip; info_finish with K = len given, not
// counted), shared with the two DP kernels.
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

constexpr int AINFO_NT = 256, AINFO_WAVES = AINFO_NT / 64;

template <int NL, bool YMODE>
__global__ __launch_bounds__(AINFO_NT) void awgn_info_kernel(int N, const float *__restrict__ q, const float *__restrict__ y,
                                                             const __half *__restrict__ txg, const float *__restrict__ amp_g,
                                                             const float *__restrict__ Pg, const float *__restrict__ amp_mean,
                                                             const float *__restrict__ var, const int32_t *__restrict__ shift,
                                                             float *__restrict__ info, int32_t *__restrict__ counts)
{
    __shared__ float red[AINFO_WAVES];                         // eval_block_sum's scratch (y-mode: the two sums of |y_c|)
    __shared__ InfoShared<4, AINFO_WAVES> sh;
    const int run = blockIdx.x, tid = threadIdx.x;
    float *o = info + (size_t)run * 3;
    int32_t *cn = counts + (size_t)run * 4;
    // the window of validate_tail: kept symbol j < len pairs sample 11 + sft + j with TX symbol 11 + j; where it is not empty -10 <= sft <= N - 23,
    // so both stay inside [11, N - 11)
    const TrackWindow w(N, N, AWGN_EDGE, shift[run]);
    bool empty = w.empty;
    const int len = w.L;

    const float *src = YMODE ? y + (size_t)run * 2 * N : q + (size_t)run * 2 * NL * N;
    float amp[NL], sc[2] = {0.f, 0.f}, ivl = 0.f;
    if constexpr (YMODE) {
        if (!awgn_row_scales<AINFO_NT>(src, N, !empty, amp_mean[run], red, tid, sc)) empty = true;
        ivl = INFO_LOG2E / var[run];
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
        const int m = w.sample(j), n = AWGN_EDGE + j;
        const __half txi = txI[n], txq = txQ[n];
        float v[2][NL];
#pragma unroll
        for (int c = 0; c < 2; c++) {
            if constexpr (YMODE) info_awgn_log2<NL>(src[(size_t)c * N + m] * sc[c], amp, ivl, v[c]);
            else info_load_q<NL>(src, N, m, c, v[c]);
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
    if (!vaeq::awgn_frame_shape_ok(R, N)) return VAEQ_ERR_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const __half *tx = reinterpret_cast<const __half *>(data_f16);
    return vaeq::dispatch_nlev(n_lev, [&](auto nl) {
        constexpr int NL = decltype(nl)::value;
        auto k = y ? vaeq::awgn_info_kernel<NL, true> : vaeq::awgn_info_kernel<NL, false>;
        return vaeq::launch(k, dim3(R), dim3(vaeq::AINFO_NT), 0, st, (int)N, q, y, tx, amp, P, amp_mean, var, shift, info, counts);
    });
}
