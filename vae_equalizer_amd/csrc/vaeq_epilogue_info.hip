// vaeq_epilogue_info.hip -- information-rate figures of one DP frame on the device: achievable rate of symbol-wise mismatched decoding (AIR),
// generalised mutual information of the bit-wise decoder (GMI) and the pre-FEC bit error rate, per run and polarisation, over exactly the
// symbols the q-SER of vaeq_dp_epilogue keeps (same roll by shift_q, same polarisation exchange, same per-minibatch cut and frame-edge slice:
// vaeq_epilogue_keep.h).  The reference has no such metric; the definitions are closed-form (tests/_ref_info.py).
//
// One workgroup per (run, polarisation).  Every kept symbol's posteriors are read ONCE (q-mode: 2 n_lev floats from q; y-mode: the two
// equalised samples, demapped again in the log domain) and all eight hypotheses h = 4 flip + rot of SER_IQflip (shared_funcs.py:188-222) are
// accumulated in that pass; the winner -- fewest symbol errors of argmax(q), ties to the smallest h, so its count is the q-SER's -- is
// picked at the end.  What makes eight hypotheses cheap: a rotation only exchanges the axes and reverses the level order, and the
// binary-reflected Gray label of the reversed level differs from the level's in the top bit alone (g(n-1-i) = g(i) ^ n/2), so the bit-wise
// sums of a reversed posterior at level t are the unreversed ones at level n-1-t.  Per axis the 2 log2(n_lev) bit-wise sums are formed once;
// every hypothesis is then a selection among (axis, level in {t_I, n-1-t_I, t_Q, n-1-t_Q}).
// Integer counts are exact; float sums run per thread in symbol order, then over the wave's lanes (DPP, fixed order), then over the four waves
// in order: two calls give identical bits.
// This file holds the walk over a thread's symbols (KeepWalk), the accumulation and the three lines of the demapper's constants; the alignment,
// the q-mode load and the demapper's exponent are vaeq_info.h's (InfoAlign, info_load_q, info_demap_log2), the text vaeq_epilogue_llr.hip runs,
// and so are the per-symbol body and the tail (info_symbol<NL, YMODE, 8>, info_finish), shared with vaeq_awgn_info.hip and vaeq_cma_info.hip.
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

constexpr int INFO_WAVES = EPI_NT / 64;

template <int NL, bool YMODE>
__global__ __launch_bounds__(EPI_NT) void dp_epilogue_info_kernel(int N, int batch_len, const float *__restrict__ q, const float *__restrict__ y,
                                                                  const __half *__restrict__ txg, const float *__restrict__ amp_g,
                                                                  const float *__restrict__ Pg, const float *__restrict__ var,
                                                                  const float *__restrict__ nu_sc, const int32_t *__restrict__ shift,
                                                                  const int32_t *__restrict__ rflag, float *__restrict__ info,
                                                                  int32_t *__restrict__ counts)
{
    __shared__ InfoShared<8, INFO_WAVES> sh;
    const int run = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
    const InfoAlign al(shift, rflag, run);
    const int sp = al.sp(p), sft = al.sft(p);
    const __half *txI = txg + ((size_t)run * 4 + p * 2) * N, *txQ = txI + N;
    const float *src = YMODE ? y + ((size_t)run * 4 + sp * 2) * N : q + ((size_t)run * 4 + sp * 2) * NL * N;
    float amp[NL], pen[NL];
    float i2v = 0.f;
    if constexpr (YMODE) {                                     // info_demap_setup's lines (vaeq_info.h says why they stand here)
        const float nusc = nu_sc[run];
        i2v = 0.5f / var[run * 2 + sp];                        // the demapper of the RECEIVED polarisation made this row's q
#pragma unroll
        for (int i = 0; i < NL; i++) { amp[i] = amp_g[i]; pen[i] = nusc * (amp[i] * amp[i]); }
    }

    float fs[16];
    int se[8], be[8], kept = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) fs[i] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; i++) se[i] = be[i] = 0;

    KeepWalk kw(tid, N, batch_len, al.s0, al.ms);
    for (int n = tid; n < N; n += EPI_NT, kw.next()) {
        const int m = n + sft;
        if (!kw.keep(n) || m < 0 || m >= N) continue;
        kept++;
        const __half txi = txI[n], txq = txQ[n];
        float v[2][NL];
#pragma unroll
        for (int c = 0; c < 2; c++) {
            if constexpr (YMODE) info_demap_log2<NL>(src[(size_t)c * N + m], amp, pen, i2v, v[c]);
            else info_load_q<NL>(src, N, m, c, v[c]);
        }
        info_symbol<NL, YMODE, 8>(v, txi, txq, fs, se, be);
    }
    info_finish<NL, 8, INFO_WAVES, true>(sh, tid, fs, se, be, kept, Pg + run * NL, info + ((size_t)run * 2 + p) * 3,
                                         counts + ((size_t)run * 2 + p) * 4);
}

}  // namespace vaeq

extern "C" int vaeq_dp_epilogue_info(int32_t R, int64_t N, int32_t n_lev, int32_t batch_len, const float *q, const float *y, const void *tx_f16,
                                     const float *amp, const float *P, const float *var, const float *nu_sc, const int32_t *shift,
                                     const int32_t *rflag, float *info, int32_t *counts, void *stream)
{
    if (R == 0) return VAEQ_OK;                                // an empty batch owns no memory: its pointers may be NULL
    if ((q != nullptr) == (y != nullptr)) return VAEQ_ERR_NULL;                                  // exactly one source of posteriors
    if (!tx_f16 || !amp || !P || !shift || !rflag || !info || !counts || (y && (!var || !nu_sc))) return VAEQ_ERR_NULL;
    if (!vaeq::epi_frame_shape_ok(R, N, batch_len)) return VAEQ_ERR_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const __half *tx = reinterpret_cast<const __half *>(tx_f16);
    return vaeq::dispatch_nlev(n_lev, [&](auto nl) {
        constexpr int NL = decltype(nl)::value;
        auto k = y ? vaeq::dp_epilogue_info_kernel<NL, true> : vaeq::dp_epilogue_info_kernel<NL, false>;
        return vaeq::launch(k, dim3(R, 2), dim3(vaeq::EPI_NT), 0, st, (int)N, batch_len, q, y, tx, amp, P, var, nu_sc, shift, rflag, info, counts);
    });
}
