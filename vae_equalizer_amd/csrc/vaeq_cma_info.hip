// vaeq_cma_info.hip -- information-rate figures of one frame of the constant-modulus DP baselines on the device: AIR, GMI and pre-FEC BER per run
// and polarisation (the figures of vaeq_epilogue_info.hip), over exactly the symbols the soft-demapper SER of vaeq_cma_epilogue
// keeps.  The posteriors are the ones soft_dec (func_CMA_DP_MQAM_shaping.py:48) defines on the phase-corrected output after the constellation stage
// has aligned it and normalised its kept window in place (shared_funcs.py:242).  vaeq_cma_epilogue leaves neither that sequence nor q in memory, so
// this kernel redoes the two-stage addressing and the mean-radius factor from the raw y and the four alignment outputs of the epilogue:
//   stage c:  ya[p'][c][m] = y[(p' - r_c) & 1][c][(m + shift_c[p']) mod N],   W_c = [11, N - 11 - max|shift_c|)
//             fac = sum_{p', m in W_c} |tx[p'][:, m]| / sum_{p', m in W_c} |ya[p'][:, m]|,   yn = ya fac inside W_c, ya outside it
//   stage q:  kept symbol n in [11, N - 11 - max|shift_q|) of output polarisation p reads yn[p' = (p - r_q) & 1][:, m = n + shift_q[p]]
// and demaps it with var[p'] in the log domain.  That addressing, the radius walk and the demapper are vaeq_info.h's (CmaFrame, cma_radius_factor,
// info_demap_setup / info_demap_log2), the one text vaeq_cma_llr.hip runs as well; the per-symbol body and the tail are vaeq_info.h's too
// (info_symbol, info_finish).  What is this kernel's own is the accumulation over a polarisation's kept symbols and the two calls of the tail.
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
    __shared__ float rad[CMA_INFO_WAVES][2];                   // cma_radius_factor's scratch
    __shared__ InfoShared<8, CMA_INFO_WAVES> sh;
    const int run = blockIdx.x, tid = threadIdx.x;
    const CmaFrame f(run, N, y, txg, shift_c, r_c, shift_q, r_q);

    // ---- walk 1: the mean-radius factor; a degenerate run reports the empty-window result
    bool degenerate;
    const float fac = cma_radius_factor<CMA_INFO_WAVES>(f, rad, tid, degenerate);

    // ---- walk 2, once per output polarisation p: its kept symbols
#pragma unroll 1
    for (int p = 0; p < 2; p++) {
        const float *yI = f.y_row(p), *yQ = yI + N;
        const __half *txI = f.txr + (size_t)(p * 2) * N, *txQ = txI + N;
        float amp[NL], pen[NL];
        const float i2v = info_demap_setup<NL>(amp_g, nu_sc, var, run, f.aligned_row(p), amp, pen);   // the demapper of the stage-c aligned polarisation

        float fs[16];
        int se[8], be[8], kept = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) fs[i] = 0.f;
#pragma unroll
        for (int i = 0; i < 8; i++) se[i] = be[i] = 0;

        for (int n = tid; n < N && !degenerate; n += EPI_NT) {
            if (!f.kept(n)) continue;
            float g;
            const int ms = f.source(p, n, fac, g);
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
    if (!vaeq::epi_frame_shape_ok(R, N, 0)) return VAEQ_ERR_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const __half *tx = reinterpret_cast<const __half *>(tx_f16);
    return vaeq::dispatch_nlev(n_lev, [&](auto nl) {
        return vaeq::launch(vaeq::cma_epilogue_info_kernel<decltype(nl)::value>, dim3(R), dim3(vaeq::EPI_NT), 0, st, (int)N, y, tx, amp, P, var,
                            nu_sc, shift_c, r_c, shift_q, r_q, info, counts);
    });
}
