// vaeq_cma_llr.hip -- the per-bit a-posteriori LLRs of one frame of the constant-modulus DP baselines on the device: what a bit-wise (LDPC) decoder
// behind CMA / CMAbatch / CMAflex reads, and what the GMI of vaeq_cma_epilogue_info is the rate of.  The posteriors are that kernel's, term for
// term (vaeq_cma_info.hip has the derivation): both shifts clamped, the stage-c roll wrapping around the frame, the mean-radius factor
//     fac = sum_{p', m in W_c} |tx[p'][:, m]| / sum_{p', m in W_c} |ya[p'][:, m]|,   W_c = [11, N - 11 - max|shift_c|)
// applied exactly where a sample's stage-c index lies in W_c, and the demapper of the stage-c aligned row p' = (p - r_q) & 1.  Over the symbols it
// keeps, n in [11, N - 11 - max|shift_q|), and under the hypothesis it picked (hyp & 7), the LLRs land in TX order: plane a b + k of output
// polarisation p at TX index n is bit k of TX axis a; every other entry is an erasure, +0.0, and a run without a radius (sum |ya| == 0) is all zeros.
//
// 256 threads; grid (run, polarisation) for a batch that leaves the device idle otherwise, grid (run) -- one workgroup takes both polarisations
// in turn -- for a large one.  fac decides every LLR of the run, and the LLRs are those of the posteriors whose GMI is reported only if it is the
// same float: the radius walk is cma_epilogue_info_kernel's walk 1 restated (per thread at stride EPI_NT, wave_sum_dpp, the waves in order), and
// on the split grid each of the run's two workgroups redoes it identically.  After it the work is elementwise: thread t takes n = t, t + 256, ...,
// consecutive lanes on consecutive n, so every read and each of the 2 b plane stores is contiguous across the wave.  32 bytes of LDS (the cross-wave
// radius scratch), no atomics: two calls give identical bits, R runs in one call the bits of R single calls.
// This file holds the addressing and the radius walk; the per-symbol body is vaeq_llr.h's, the demapper's exponent vaeq_info.h's.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vaeq.h"
#include "vaeq_common.h"
#include "vaeq_epilogue_keep.h"
#include "vaeq_launch.h"
#include "vaeq_llr.h"
#include "vaeq_wave.h"

namespace vaeq {

constexpr int CMA_LLR_WAVES = EPI_NT / 64;
// Up to this many runs a run's two polarisations go to two workgroups (grid (R, 2)), beyond it to one (grid (R)): the two forms cross between 512
// and 1024 runs on the MI355X's 256 CUs (the bits are the same either way).
constexpr int CMA_LLR_SPLIT_MAX_R = 512;

template <int NL>
__global__ __launch_bounds__(EPI_NT) void cma_epilogue_llr_kernel(int N, const float *__restrict__ y, const __half *__restrict__ txg,
                                                                  const float *__restrict__ amp_g, const float *__restrict__ var,
                                                                  const float *__restrict__ nu_sc, const int32_t *__restrict__ shift_c,
                                                                  const int32_t *__restrict__ r_c, const int32_t *__restrict__ shift_q,
                                                                  const int32_t *__restrict__ r_q, const int32_t *__restrict__ hyp,
                                                                  float *__restrict__ llr)
{
    constexpr int NB = llr_bits(NL);
    __shared__ float rad[CMA_LLR_WAVES][2];                    // [wave][0: sum |tx|, 1: sum |ya|] over W_c
    const int run = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c0 = info_clamp_shift(shift_c[run * 2 + 0]), c1 = info_clamp_shift(shift_c[run * 2 + 1]);
    const int q0 = info_clamp_shift(shift_q[run * 2 + 0]), q1 = info_clamp_shift(shift_q[run * 2 + 1]);
    const int rc = r_c[run] & 1, rq = r_q[run] & 1;
    const int endc = N - EDGE - max(abs(c0), abs(c1)), endq = N - EDGE - max(abs(q0), abs(q1));   // W_c = [EDGE, endc), kept = [EDGE, endq)
    const float *yr = y + (size_t)run * 4 * N;
    const __half *txr = txg + (size_t)run * 4 * N;

    // ---- the radius walk: cma_epilogue_info_kernel's walk 1, expression for expression
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
    for (int k = 0; k < CMA_LLR_WAVES; k++) { st += rad[k][0]; sy += rad[k][1]; }
    const bool degenerate = sy == 0.f;                         // no radius, no normalisation: the run kept nothing
    const float fac = st / sy;

    // ---- the elementwise pass of output polarisation p (grid.y = 2: this workgroup's one; grid.y = 1: both in turn)
    for (int p = blockIdx.y; p < 2; p += gridDim.y) {
        const int pp = (p - rq) & 1, sft = p ? q1 : q0;            // stage q: row p comes from aligned row p - r_q, out[n] = in[n + shift_q[p]]
        const int sp = (pp - rc) & 1, sfc = pp ? c1 : c0;          // stage c: aligned row p' comes from row p' - r_c of y, rolled by shift_c[p'] (wrapping)
        const float *yI = yr + (size_t)(sp * 2) * N, *yQ = yI + N;
        const float nusc = nu_sc[run];
        const float i2v = 0.5f / var[run * 2 + pp];                // the demapper of the stage-c aligned polarisation, as in the epilogue
        float amp[NL], pen[NL];
#pragma unroll
        for (int i = 0; i < NL; i++) { amp[i] = amp_g[i]; pen[i] = nusc * (amp[i] * amp[i]); }
        const int h = hyp[run * 2 + p] & 7;
        float *dst = llr + ((size_t)run * 2 + p) * (2 * NB) * N;
        for (int n = tid; n < N; n += EPI_NT) {
            float out[2 * NB];
#pragma unroll
            for (int i = 0; i < 2 * NB; i++) out[i] = 0.f;         // an erasure
            if (!degenerate && n >= EDGE && n < endq) {
                const int m = n + sft;                             // index in the stage-c aligned sequence, 1 <= m < N - 1
                int ms = m + sfc;                                  // index in y: -9 <= ms < N + 9, one wrap at most (N >= 43)
                if (ms >= N) ms -= N;
                if (ms < 0) ms += N;
                const float g = (m >= EDGE && m < endc) ? fac : 1.0f;  // scaled exactly where the aligned index lies in W_c
                float v[2][NL];
                info_demap_log2<NL>(yI[ms] * g, amp, pen, i2v, v[0]);
                info_demap_log2<NL>(yQ[ms] * g, amp, pen, i2v, v[1]);
                llr_symbol<NL, true>(v, h, out);
            }
#pragma unroll
            for (int i = 0; i < 2 * NB; i++) dst[(size_t)i * N + n] = out[i];
        }
    }
}

}  // namespace vaeq

extern "C" int vaeq_cma_epilogue_llr(int32_t R, int64_t N, int32_t n_lev, const float *y, const void *tx_f16, const float *amp, const float *var,
                                     const float *nu_sc, const int32_t *shift_c, const int32_t *r_c, const int32_t *shift_q, const int32_t *r_q,
                                     const int32_t *hyp, float *llr, void *stream)
{
    if (R == 0) return VAEQ_OK;                                // an empty batch owns no memory: its pointers may be NULL
    if (!y || !tx_f16 || !amp || !var || !nu_sc || !shift_c || !r_c || !shift_q || !r_q || !hyp || !llr) return VAEQ_ERR_NULL;
    if (R < 0 || N < 2 * vaeq::EDGE + vaeq::N_SHIFT || N > 0x3fffffff) return VAEQ_ERR_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const __half *tx = reinterpret_cast<const __half *>(tx_f16);
    return vaeq::dispatch_nlev(n_lev, [&](auto nl) {
        return vaeq::launch(vaeq::cma_epilogue_llr_kernel<decltype(nl)::value>, dim3(R, R <= vaeq::CMA_LLR_SPLIT_MAX_R ? 2 : 1), dim3(vaeq::EPI_NT), 0, st, (int)N, y, tx, amp, var,
                            nu_sc, shift_c, r_c, shift_q, r_q, hyp, llr);
    });
}
