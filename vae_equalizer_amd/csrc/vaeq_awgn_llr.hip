// vaeq_awgn_llr.hip -- the per-bit a-posteriori LLRs of one AWGN validation frame on the device: what a bit-wise (LDPC) decoder behind the
// equaliser reads, and what the GMI of vaeq_awgn_info is the rate of.  Over exactly the symbols that kernel keeps (TX index 11 + j, j < len =
// N - 22 - sh, reads sample 11 + sh + j) and under the rotation hypothesis it picked, the LLRs land in TX order: plane a b + k at TX index n is
// bit k of TX axis a of that symbol; a symbol outside the window is an erasure, +0.0.
//
// One 256-thread workgroup per run, as vaeq_awgn_info: y-mode normalises by m_c = sum_n |y_c[n]| / N over the WHOLE row, and the LLRs are those
// of the posteriors whose GMI is reported only if that sum is the same float -- so window, pre-pass, q-mode load and exponent are the text
// awgn_info_kernel runs (TrackWindow and awgn_row_scales of vaeq_awgn_eval.h, info_load_q and info_awgn_log2 of vaeq_info.h).  After the pre-pass
// the work is elementwise: thread t takes TX indices t, t + 256, ..., consecutive lanes on consecutive n, every read and every one of the 2 b
// plane stores contiguous across the wave.  An empty window, or m_c == 0, writes the whole row as zeros.  No atomics: two calls give identical bits.
// This file holds the erasures and the plane stores; the per-symbol body is vaeq_llr.h's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vaeq.h"
#include "vaeq_awgn_eval.h"
#include "vaeq_launch.h"
#include "vaeq_llr.h"
#include "vaeq_wave.h"

namespace vaeq {

constexpr int ALLR_NT = 256;

template <int NL, bool YMODE>
__global__ __launch_bounds__(ALLR_NT) void awgn_llr_kernel(int N, const float *__restrict__ q, const float *__restrict__ y,
                                                           const float *__restrict__ amp_g, const float *__restrict__ amp_mean,
                                                           const float *__restrict__ var, const int32_t *__restrict__ shift,
                                                           const int32_t *__restrict__ hyp, float *__restrict__ llr)
{
    constexpr int NB = llr_bits(NL);
    __shared__ float red[ALLR_NT / 64];                        // eval_block_sum's scratch (y-mode: the two sums of |y_c|)
    const int run = blockIdx.x, tid = threadIdx.x;
    const TrackWindow w(N, N, AWGN_EDGE, shift[run]);          // the window of awgn_info_kernel
    bool empty = w.empty;
    const int len = w.L;

    const float *src = YMODE ? y + (size_t)run * 2 * N : q + (size_t)run * 2 * NL * N;
    float amp[NL], sc[2] = {0.f, 0.f}, ivl = 0.f;
    if constexpr (YMODE) {
        if (!awgn_row_scales<ALLR_NT>(src, N, !empty, amp_mean[run], red, tid, sc)) empty = true;
        ivl = INFO_LOG2E / var[run];
#pragma unroll
        for (int i = 0; i < NL; i++) amp[i] = amp_g[i];
    }
    const int h = hyp[run] & 3;
    float *dst = llr + (size_t)run * (2 * NB) * N;
    for (int n = tid; n < N; n += ALLR_NT) {
        const int j = n - AWGN_EDGE;
        float out[2 * NB];
#pragma unroll
        for (int i = 0; i < 2 * NB; i++) out[i] = 0.f;         // an erasure
        if (!empty && j >= 0 && j < len) {
            const int m = w.sample(j);
            float v[2][NL];
#pragma unroll
            for (int c = 0; c < 2; c++) {
                if constexpr (YMODE) info_awgn_log2<NL>(src[(size_t)c * N + m] * sc[c], amp, ivl, v[c]);
                else info_load_q<NL>(src, N, m, c, v[c]);
            }
            llr_symbol<NL, YMODE>(v, h, out);
        }
#pragma unroll
        for (int i = 0; i < 2 * NB; i++) dst[(size_t)i * N + n] = out[i];
    }
}

}  // namespace vaeq

extern "C" int vaeq_awgn_llr(int32_t R, int64_t N, int32_t n_lev, const float *q, const float *y, const float *amp, const float *amp_mean,
                             const float *var, const int32_t *shift, const int32_t *hyp, float *llr, void *stream)
{
    if (R == 0) return VAEQ_OK;                                // an empty batch owns no memory: its pointers may be NULL
    if ((q != nullptr) == (y != nullptr)) return VAEQ_ERR_NULL;                                  // exactly one source of posteriors
    if (!amp || !shift || !hyp || !llr || (y && (!amp_mean || !var))) return VAEQ_ERR_NULL;
    if (!vaeq::awgn_frame_shape_ok(R, N)) return VAEQ_ERR_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return vaeq::dispatch_nlev(n_lev, [&](auto nl) {
        constexpr int NL = decltype(nl)::value;
        auto k = y ? vaeq::awgn_llr_kernel<NL, true> : vaeq::awgn_llr_kernel<NL, false>;
        return vaeq::launch(k, dim3(R), dim3(vaeq::ALLR_NT), 0, st, (int)N, q, y, amp, amp_mean, var, shift, hyp, llr);
    });
}
