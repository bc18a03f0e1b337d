// vaeq_cma_info.hip -- information-rate figures of one frame of the constant-modulus DP baselines on the device: AIR, GMI and pre-FEC BER per run
// and polarisation (the figures of vaeq_epilogue_info.hip), over exactly the symbols the soft-demapper SER of vaeq_cma_epilogue
// keeps.  The posteriors are the ones soft_dec (func_CMA_DP_MQAM_shaping.py:48) defines on the phase-corrected output after the constellation stage
// has aligned it and normalised its kept window in place (shared_funcs.py:242).  vaeq_cma_epilogue leaves neither that sequence nor q in memory, so
// this kernel redoes the two-stage addressing and the mean-radius factor from the raw y and the four alignment outputs of the epilogue:
//   stage c:  ya[p'][c][m] = y[(p' - r_c) & 1][c][(m + shift_c[p']) mod N],   W_c = [11, N - 11 - max|shift_c|)
//             fac = sum_{p', m in W_c} |tx[p'][:, m]| / sum_{p', m in W_c} |ya[p'][:, m]|,   yn = ya fac inside W_c, ya outside it
//   stage q:  kept symbol n in [11, N - 11 - max|shift_q|) of output polarisation p reads yn[p' = (p - r_q) & 1][:, m = n + shift_q[p]]
// and demaps it with var[p'] in the log domain.  What is this kernel's own is that addressing, the radius walk and the two calls of the tail; the
// per-symbol body, the tail and the demapper's exponent are vaeq_info.h's (info_symbol, info_finish, info_demap_log2), shared with the siblings.
//
// One workgroup per run, three walks: the first forms fac, the second and third the figures of output polarisation 0 and 1.
// y and tx are read, nothing but the 56 bytes of results per run is written.  Integer counts are exact; float sums run per thread in index order,
// then over the wave's lanes (DPP, fixed order), then over the four waves in order: two calls give identical bits, R runs in one call the bits of
// R single calls.
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

constexpr int CMA_INFO_WAVES = EPI_NT / 64;

template <int NL>
__global__ __launch_bounds__(EPI_NT) void cma_epilogue_info_kernel(int N, const float *__restrict__ y, const __half *__restrict__ txg,
                                                                   const float *__restrict__ amp_g, const float *__restrict__ Pg,
                                                                   const float *__restrict__ var, const float *__restrict__ nu_sc,
                                                                   const int32_t *__restrict__ shift_c, const int32_t *__restrict__ r_c,
                                                                   const int32_t *__restrict__ shift_q, const int32_t *__restrict__ r_q,
                                                                   float *__restrict__ info, int32_t *__restrict__ counts)
{
    __shared__ float rad[CMA_INFO_WAVES][2];                   // [wave][0: sum |tx|, 1: sum |ya|] over W_c
    __shared__ InfoShared<8, CMA_INFO_WAVES> sh;
    const int run = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    // both alignments clamped to what the epilogue can find: with 11 <= n and a window that ends 11 + max|shift| before the row does, n + shift
    // stays inside [1, N - 1) in either stage; only the stage-c roll of a sample outside W_c can wrap around the frame
    const int c0 = info_clamp_shift(shift_c[run * 2 + 0]), c1 = info_clamp_shift(shift_c[run * 2 + 1]);
    const int q0 = info_clamp_shift(shift_q[run * 2 + 0]), q1 = info_clamp_shift(shift_q[run * 2 + 1]);
    const int rc = r_c[run] & 1, rq = r_q[run] & 1;
    const int endc = N - EDGE - max(abs(c0), abs(c1)), endq = N - EDGE - max(abs(q0), abs(q1));   // W_c = [EDGE, endc), kept = [EDGE, endq)
    const float *yr = y + (size_t)run * 4 * N;
    const __half *txr = txg + (size_t)run * 4 * N;

    // ---- walk 1: mean radius of TX over mean radius of the stage-c aligned output, both polarisations, over W_c (shared_funcs.py:242)
    float st = 0.f, sy = 0.f;
    for (int n = tid; n < N; n += EPI_NT) {
        if (n < EDGE || n >= endc) continue;
#pragma unroll
        for (int pp = 0; pp < 2; pp++) {
            const int sp = (pp - rc) & 1, m = n + (pp ? c1 : c0);                                // 1 <= m < N - 1
            const float ti = __half2float(txr[(size_t)(pp * 2 + 0) * N + n]), tq = __half2float(txr[(size_t)(pp * 2 + 1) * N + n]);
            const float yi = yr[(size_t)(sp * 2 + 0) * N + m], yq = yr[(size_t)(sp * 2 + 1) * N + m];
            st += sqrtf(fmaf(ti, ti, tq * tq));
            sy += sqrtf(fmaf(yi, yi, yq * yq));
        }
    }
    st = wave_sum_dpp(st);
    sy = wave_sum_dpp(sy);
    if (lane == 0) { rad[w][0] = st; rad[w][1] = sy; }
    __syncthreads();
    st = sy = 0.f;
    for (int k = 0; k < CMA_INFO_WAVES; k++) { st += rad[k][0]; sy += rad[k][1]; }
    const bool degenerate = sy == 0.f;                         // no radius, no normalisation: the run reports the empty-window result
    const float fac = st / sy;

    // ---- walk 2, once per output polarisation p: its kept symbols
#pragma unroll 1
    for (int p = 0; p < 2; p++) {
        const int pp = (p - rq) & 1, sft = p ? q1 : q0;            // stage q: row p comes from aligned row p - r_q, out[n] = in[n + shift_q[p]]
        const int sp = (pp - rc) & 1, sfc = pp ? c1 : c0;          // stage c: aligned row p' comes from row p' - r_c of y, rolled by shift_c[p'] (wrapping)
        const float *yI = yr + (size_t)(sp * 2) * N, *yQ = yI + N;
        const __half *txI = txr + (size_t)(p * 2) * N, *txQ = txI + N;
        const float nusc = nu_sc[run];
        const float i2v = 0.5f / var[run * 2 + pp];                // the demapper of the stage-c aligned polarisation, as in the epilogue
        float amp[NL], pen[NL];
#pragma unroll
        for (int i = 0; i < NL; i++) { amp[i] = amp_g[i]; pen[i] = nusc * (amp[i] * amp[i]); }

        float fs[16];
        int se[8], be[8], kept = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) fs[i] = 0.f;
#pragma unroll
        for (int i = 0; i < 8; i++) se[i] = be[i] = 0;

        for (int n = tid; n < N && !degenerate; n += EPI_NT) {
            if (n < EDGE || n >= endq) continue;
            const int m = n + sft;                                 // index in the stage-c aligned sequence, 1 <= m < N - 1
            int ms = m + sfc;                                      // index in y: -9 <= ms < N + 9, one wrap at most (N >= 43)
            if (ms >= N) ms -= N;
            if (ms < 0) ms += N;
            const float g = (m >= EDGE && m < endc) ? fac : 1.0f;  // scaled exactly where the aligned index lies in W_c
            kept++;
            const __half txi = txI[n], txq = txQ[n];
            float v[2][NL];
            info_demap_log2<NL>(yI[ms] * g, amp, pen, i2v, v[0]);
            info_demap_log2<NL>(yQ[ms] * g, amp, pen, i2v, v[1]);
            info_symbol<NL, true, 8>(v, txi, txq, fs, se, be);
        }
        // (a degenerate run kept nothing: no normalisation is no measurement)
        info_finish<NL, 8, CMA_INFO_WAVES, true>(sh, tid, fs, se, be, kept, Pg + run * NL, info + ((size_t)run * 2 + p) * 3,
                                                 counts + ((size_t)run * 2 + p) * 4);
        __syncthreads();                                       // sh is reused by the next polarisation
    }
}

}  // namespace vaeq

extern "C" int vaeq_cma_epilogue_info(int32_t R, int64_t N, int32_t n_lev, const float *y, const void *tx_f16, const float *amp, const float *P,
                                      const float *var, const float *nu_sc, const int32_t *shift_c, const int32_t *r_c, const int32_t *shift_q,
                                      const int32_t *r_q, float *info, int32_t *counts, void *stream)
{
    if (R == 0) return VAEQ_OK;                                // an empty batch owns no memory: its pointers may be NULL
    if (!y || !tx_f16 || !amp || !P || !var || !nu_sc || !shift_c || !r_c || !shift_q || !r_q || !info || !counts) return VAEQ_ERR_NULL;
    if (R < 0 || N < 2 * vaeq::EDGE + vaeq::N_SHIFT || N > 0x3fffffff) return VAEQ_ERR_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const __half *tx = reinterpret_cast<const __half *>(tx_f16);
    return vaeq::dispatch_nlev(n_lev, [&](auto nl) {
        return vaeq::launch(vaeq::cma_epilogue_info_kernel<decltype(nl)::value>, dim3(R), dim3(vaeq::EPI_NT), 0, st, (int)N, y, tx, amp, P, var,
                            nu_sc, shift_c, r_c, shift_q, r_q, info, counts);
    });
}
