// vaeq_awgn_llr.hip -- the per-bit a-posteriori LLRs of one AWGN validation frame on the device: what a bit-wise (LDPC) decoder behind the
// equaliser reads, and what the GMI of vaeq_awgn_info is the rate of.  Over exactly the symbols that kernel keeps (TX index 11 + j, j < len =
// N - 22 - sh, reads sample 11 + sh + j) and under the rotation hypothesis it picked, the LLRs land in TX order: plane a b + k at TX index n is
// bit k of TX axis a of that symbol; a symbol outside the window is an erasure, +0.0.
//
// One 256-thread workgroup per run, as vaeq_awgn_info: y-mode normalises by m_c = sum_n |y_c[n]| / N over the WHOLE row, and the LLRs are those
// of the posteriors whose GMI is reported only if that sum is the same float -- so the pre-pass is awgn_info_kernel's, term for term (per thread
// in index order, over the wave's lanes by DPP, over the four waves in order).  After it the work is elementwise: thread t takes TX indices
// t, t + 256, ..., consecutive lanes on consecutive n, every read and every one of the 2 b plane stores contiguous across the wave.
// An empty window, or m_c == 0, writes the whole row as zeros.  No atomics: two calls give identical bits.
// This file holds the window, the pre-pass and the VAE-LE demapper's exponent; the per-symbol body is vaeq_llr.h's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vaeq.h"
#include "vaeq_awgn_eval.h"
#include "vaeq_launch.h"
#include "vaeq_llr.h"
#include "vaeq_wave.h"

namespace vaeq {

constexpr int ALLR_NT = 256, ALLR_EDGE = 11;

template <int NL, bool YMODE>
__global__ __launch_bounds__(ALLR_NT) void awgn_llr_kernel(int N, const float *__restrict__ q, const float *__restrict__ y,
                                                           const float *__restrict__ amp_g, const float *__restrict__ amp_mean,
                                                           const float *__restrict__ var, const int32_t *__restrict__ shift,
                                                           const int32_t *__restrict__ hyp, float *__restrict__ llr)
{
    constexpr float LOG2E = 1.4426950408889634f;
    constexpr int NB = llr_bits(NL);
    __shared__ float red[ALLR_NT / 64];                        // eval_block_sum's scratch (y-mode: the two sums of |y_c|)
    const int run = blockIdx.x, tid = threadIdx.x;
    // the window of awgn_info_kernel (64-bit: N - 22 - sft leaves int32 for a shift nobody can find but anybody can pass); where it is not empty
    // -10 <= sft <= N - 23, so sample and TX index both stay inside [11, N - 11)
    const int sft = shift[run];
    const long long len64 = (long long)N - 2 * ALLR_EDGE - (long long)sft;
    bool empty = (long long)ALLR_EDGE + sft <= 0 || len64 <= 0;
    const int len = empty ? 0 : (int)len64;

    const float *src = YMODE ? y + (size_t)run * 2 * N : q + (size_t)run * 2 * NL * N;
    float amp[NL], sc[2] = {0.f, 0.f}, ivl = 0.f;
    if constexpr (YMODE) {
        float sa0 = 0.f, sa1 = 0.f;
        if (!empty) {                                          // (uniform: every thread of the workgroup takes the same side)
#pragma unroll 4
            for (int n = tid; n < N; n += ALLR_NT) { sa0 += fabsf(src[n]); sa1 += fabsf(src[(size_t)N + n]); }
        }
        sa0 = eval_block_sum<ALLR_NT>(sa0, red, tid);
        sa1 = eval_block_sum<ALLR_NT>(sa1, red, tid);
        const float m0 = sa0 / (float)N, m1 = sa1 / (float)N, A = amp_mean[run];
        if (m0 == 0.f || m1 == 0.f) empty = true;              // a component that is zero throughout has no normalisation: nothing to report
        sc[0] = A / m0; sc[1] = A / m1;
        ivl = LOG2E / var[run];
#pragma unroll
        for (int i = 0; i < NL; i++) amp[i] = amp_g[i];
    }
    const int h = hyp[run] & 3;
    float *dst = llr + (size_t)run * (2 * NB) * N;
    for (int n = tid; n < N; n += ALLR_NT) {
        const int j = n - ALLR_EDGE;
        float out[2 * NB];
#pragma unroll
        for (int i = 0; i < 2 * NB; i++) out[i] = 0.f;         // an erasure
        if (!empty && j >= 0 && j < len) {
            const int m = n + sft;                             // = 11 + sft + j
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
    if (R < 0 || N < 1 || N > 0x3fffffff) return VAEQ_ERR_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return vaeq::dispatch_nlev(n_lev, [&](auto nl) {
        constexpr int NL = decltype(nl)::value;
        auto k = y ? vaeq::awgn_llr_kernel<NL, true> : vaeq::awgn_llr_kernel<NL, false>;
        return vaeq::launch(k, dim3(R), dim3(vaeq::ALLR_NT), 0, st, (int)N, q, y, amp, amp_mean, var, shift, hyp, llr);
    });
}
