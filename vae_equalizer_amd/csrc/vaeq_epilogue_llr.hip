// vaeq_epilogue_llr.hip -- the per-bit a-posteriori LLRs of one DP frame on the device: what a bit-wise (LDPC) decoder behind the equaliser reads,
// and what the GMI of vaeq_dp_epilogue_info is the rate of.  Over exactly the symbols that kernel keeps (same roll by shift_q, same polarisation
// exchange, same per-minibatch cut and frame-edge slice: vaeq_epilogue_keep.h) and under the hypothesis it picked, the LLRs land in TX order:
// plane a b + k of output polarisation p at TX index n is bit k of TX axis a of that symbol; a symbol outside the window is an erasure, +0.0.
//
// The work is elementwise, so it is spread as such: one thread per TX index n, consecutive lanes on consecutive n, a 256-symbol tile per
// workgroup, tiles on grid.x and (run, polarisation) on grid.y -- 15 runs of 10 000 symbols are 1200 workgroups, as 8192 runs are 655 360.
// A wave reads 64 consecutive floats of every row it needs (q-mode: 2 n_lev rows of q; y-mode: the two equalised samples, demapped again in
// the log domain) and writes 64 consecutive floats of each of the 2 b planes.  No LDS, no reduction, no atomics: two calls give identical bits.
// This file holds the tiling, the erasures and the plane stores; the alignment, the q-mode load and the demapper are the text
// dp_epilogue_info_kernel runs (vaeq_info.h: InfoAlign, info_load_q, info_demap_setup / info_demap_log2), the per-symbol body is vaeq_llr.h's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vaeq.h"
#include "vaeq_common.h"
#include "vaeq_epilogue_keep.h"
#include "vaeq_launch.h"
#include "vaeq_llr.h"

namespace vaeq {

constexpr int LLR_NT = 256, LLR_GRID_Y = 32768;

template <int NL, bool YMODE>
__global__ __launch_bounds__(LLR_NT) void dp_epilogue_llr_kernel(long long R2, int N, int batch_len, const float *__restrict__ q,
                                                                 const float *__restrict__ y, const float *__restrict__ amp_g,
                                                                 const float *__restrict__ var, const float *__restrict__ nu_sc,
                                                                 const int32_t *__restrict__ shift, const int32_t *__restrict__ rflag,
                                                                 const int32_t *__restrict__ hyp, float *__restrict__ llr)
{
    constexpr int NB = llr_bits(NL);
    const int n = blockIdx.x * LLR_NT + threadIdx.x;
    if (n >= N) return;
    for (long long rp = blockIdx.y; rp < R2; rp += gridDim.y) {      // (run, polarisation) pairs past the grid's y limit
        const size_t run = (size_t)(rp >> 1);
        const int p = (int)(rp & 1);
        const InfoAlign al(shift, rflag, run);
        const int sp = al.sp(p), m = n + al.sft(p);
        float out[2 * NB];
#pragma unroll
        for (int i = 0; i < 2 * NB; i++) out[i] = 0.f;         // an erasure
        if (epi_keep(n, N, batch_len, al.s0, al.ms) && m >= 0 && m < N) {
            float v[2][NL];
            if constexpr (YMODE) {
                const float *src = y + (run * 4 + sp * 2) * N;
                float amp[NL], pen[NL];
                const float i2v = info_demap_setup<NL>(amp_g, nu_sc, var, run, sp, amp, pen);   // the demapper of the RECEIVED polarisation made this row's q
#pragma unroll
                for (int c = 0; c < 2; c++) info_demap_log2<NL>(src[(size_t)c * N + m], amp, pen, i2v, v[c]);
            } else {
                const float *src = q + (run * 4 + sp * 2) * NL * N;
#pragma unroll
                for (int c = 0; c < 2; c++) info_load_q<NL>(src, N, m, c, v[c]);
            }
            llr_symbol<NL, YMODE>(v, hyp[rp] & 7, out);
        }
        float *dst = llr + (size_t)rp * (2 * NB) * N + n;
#pragma unroll
        for (int i = 0; i < 2 * NB; i++) dst[(size_t)i * N] = out[i];
    }
}

}  // namespace vaeq

extern "C" int vaeq_dp_epilogue_llr(int32_t R, int64_t N, int32_t n_lev, int32_t batch_len, const float *q, const float *y, const float *amp,
                                    const float *var, const float *nu_sc, const int32_t *shift, const int32_t *rflag, const int32_t *hyp,
                                    float *llr, void *stream)
{
    if (R == 0) return VAEQ_OK;                                // an empty batch owns no memory: its pointers may be NULL
    if ((q != nullptr) == (y != nullptr)) return VAEQ_ERR_NULL;                                  // exactly one source of posteriors
    if (!amp || !shift || !rflag || !hyp || !llr || (y && (!var || !nu_sc))) return VAEQ_ERR_NULL;
    if (!vaeq::epi_frame_shape_ok(R, N, batch_len)) return VAEQ_ERR_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t R2 = 2 * (int64_t)R;
    const dim3 grid((unsigned)((N + vaeq::LLR_NT - 1) / vaeq::LLR_NT), (unsigned)(R2 < vaeq::LLR_GRID_Y ? R2 : vaeq::LLR_GRID_Y));
    return vaeq::dispatch_nlev(n_lev, [&](auto nl) {
        constexpr int NL = decltype(nl)::value;
        auto k = y ? vaeq::dp_epilogue_llr_kernel<NL, true> : vaeq::dp_epilogue_llr_kernel<NL, false>;
        return vaeq::launch(k, grid, dim3(vaeq::LLR_NT), 0, st, (long long)R2, (int)N, batch_len, q, y, amp, var, nu_sc, shift, rflag, hyp, llr);
    });
}
