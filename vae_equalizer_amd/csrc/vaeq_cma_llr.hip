// vaeq_cma_llr.hip -- the per-bit a-posteriori LLRs of one frame of the constant-modulus DP baselines on the device: what a bit-wise (LDPC) decoder
// behind CMA / CMAbatch / CMAflex reads, and what the GMI of vaeq_cma_epilogue_info is the rate of.  The posteriors are that kernel's because the
// text that forms them is: CmaFrame, cma_radius_factor and the demapper of vaeq_info.h, which both kernels call (vaeq_cma_info.hip has the
// derivation) -- both shifts clamped, the stage-c roll wrapping around the frame, the mean-radius factor
//     fac = sum_{p', m in W_c} |tx[p'][:, m]| / sum_{p', m in W_c} |ya[p'][:, m]|,   W_c = [11, N - 11 - max|shift_c|)
// applied exactly where a sample's stage-c index lies in W_c, and the demapper of the stage-c aligned row p' = (p - r_q) & 1.  Over the symbols it
// keeps, n in [11, N - 11 - max|shift_q|), and under the hypothesis it picked (hyp & 7), the LLRs land in TX order: plane a b + k of output
// polarisation p at TX index n is bit k of TX axis a; every other entry is an erasure, +0.0, and a run without a radius (sum |ya| == 0) is all zeros.
//
// 256 threads; grid (run, polarisation) for a batch that leaves the device idle otherwise, grid (run) -- one workgroup takes both polarisations
// in turn -- for a large one.  fac decides every LLR of the run; on the split grid each of the run's two workgroups forms it identically.  After
// it the work is elementwise: thread t takes n = t, t + 256, ..., consecutive lanes on consecutive n, so every read and each of the 2 b plane
// stores is contiguous across the wave.  32 bytes of LDS (the cross-wave radius scratch), no atomics: two calls give identical bits, R runs in one
// call the bits of R single calls.
// This file holds the grid, the erasures and the plane stores; the per-symbol body is vaeq_llr.h's.
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
    __shared__ float rad[CMA_LLR_WAVES][2];                    // cma_radius_factor's scratch
    const int run = blockIdx.x, tid = threadIdx.x;
    const CmaFrame f(run, N, y, txg, shift_c, r_c, shift_q, r_q);
    bool degenerate;                                           // no radius, no normalisation: the run kept nothing
    const float fac = cma_radius_factor<CMA_LLR_WAVES>(f, rad, tid, degenerate);

    // ---- the elementwise pass of output polarisation p (grid.y = 2: this workgroup's one; grid.y = 1: both in turn)
    for (int p = blockIdx.y; p < 2; p += gridDim.y) {
        const float *yI = f.y_row(p), *yQ = yI + N;
        float amp[NL], pen[NL];
        const float i2v = info_demap_setup<NL>(amp_g, nu_sc, var, run, f.aligned_row(p), amp, pen);   // the demapper of the stage-c aligned polarisation
        const int h = hyp[run * 2 + p] & 7;
        float *dst = llr + ((size_t)run * 2 + p) * (2 * NB) * N;
        for (int n = tid; n < N; n += EPI_NT) {
            float out[2 * NB];
#pragma unroll
            for (int i = 0; i < 2 * NB; i++) out[i] = 0.f;         // an erasure
            if (!degenerate && f.kept(n)) {
                float g;
                const int ms = f.source(p, n, fac, g);
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
    if (!vaeq::epi_frame_shape_ok(R, N, 0)) return VAEQ_ERR_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const __half *tx = reinterpret_cast<const __half *>(tx_f16);
    return vaeq::dispatch_nlev(n_lev, [&](auto nl) {
        return vaeq::launch(vaeq::cma_epilogue_llr_kernel<decltype(nl)::value>, dim3(R, R <= vaeq::CMA_LLR_SPLIT_MAX_R ? 2 : 1), dim3(vaeq::EPI_NT), 0, st, (int)N, y, tx, amp, var,
                            nu_sc, shift_c, r_c, shift_q, r_q, hyp, llr);
    });
}
