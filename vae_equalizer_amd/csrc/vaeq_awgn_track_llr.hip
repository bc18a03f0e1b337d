// vaeq_awgn_track_llr.hip -- the per-bit a-posteriori LLRs of the AWGN baselines on the device: what a bit-wise (LDPC) decoder behind the
// constant-modulus script's CPE output, the LMMSE output or the DFE's slicer input reads, and what the GMI of vaeq_awgn_track_info is the rate of.
// Window, both layouts, normalisation and demapper are that kernel's because the text is (TrackWindow, TrackRow, eval_radius_scale of
// vaeq_awgn_eval.h, info_awgn_log2 of vaeq_info.h, which both kernels call): kept symbol j < L = Nd - 2 edge - sh pairs sample edge + sh + j with
// TX symbol edge + j, scale = mean|tx| (L symbols) / mean|z| (ALL Lz = L + Nz - Nd samples of the slice), exponent -(zhat_c - a_i)^2 log2 e / var.
// Under the rotation that kernel picked (hyp & 3) the LLRs land in TX order: plane a b + k at TX index edge + j is bit k of TX axis a of that
// symbol; every other entry is an erasure, +0.0, and an empty window or a slice that is zero throughout is all zeros.
//
// One 256-thread workgroup per run.  scale multiplies every sample, and the LLRs are those of the posteriors whose GMI is reported only if it is
// the same float.  After the pre-pass the work is elementwise: thread t takes TX indices t, t + 256, ..., consecutive lanes on consecutive n,
// every read and each of the 2 b plane stores contiguous across the wave.  No atomics: two calls give identical bits.
// This file holds the erasures and the plane stores; the per-symbol body is vaeq_llr.h's.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vaeq.h"
#include "vaeq_awgn_eval.h"
#include "vaeq_launch.h"
#include "vaeq_llr.h"
#include "vaeq_wave.h"

namespace vaeq {

constexpr int TLLR_NT = 256;

template <int NL, bool INTERLEAVED>
__global__ __launch_bounds__(TLLR_NT) void awgn_track_llr_kernel(int Nz, int Nd, int edge, const float *__restrict__ zg,
                                                                 const __half *__restrict__ txg, const float *__restrict__ amp_g,
                                                                 const float *__restrict__ var, const int32_t *__restrict__ shift,
                                                                 const int32_t *__restrict__ hyp, float *__restrict__ llr)
{
    constexpr int NB = llr_bits(NL);
    __shared__ float red[TLLR_NT / 64];                        // eval_block_sum's scratch
    const int run = blockIdx.x, tid = threadIdx.x;
    const TrackWindow w(Nz, Nd, edge, shift[run]);             // an empty window walks nothing
    const int L = w.L, r0 = w.empty ? 0 : w.sample(0);
    const TrackRow<INTERLEAVED> track{zg + (size_t)run * 2 * Nz, Nz};
    const __half *txI = txg + (size_t)run * 2 * Nd + edge, *txQ = txI + Nd;
    float ar;
    const float scale = eval_radius_scale<TLLR_NT>(track, r0, w.Lz, txI, txQ, L, red, tid, ar);
    const bool empty = w.empty || ar == 0.f;                   // a slice that is zero throughout has no normalisation: nothing to report
    const float ivl = INFO_LOG2E / var[run];
    float amp[NL];
#pragma unroll
    for (int i = 0; i < NL; i++) amp[i] = amp_g[i];

    const int h = hyp[run] & 3;
    float *dst = llr + (size_t)run * (2 * NB) * Nd;
    for (int n = tid; n < Nd; n += TLLR_NT) {
        const int j = n - edge;
        float out[2 * NB];
#pragma unroll
        for (int i = 0; i < 2 * NB; i++) out[i] = 0.f;         // an erasure
        if (!empty && j >= 0 && j < L) {
            const float2 zs = track(r0 + j);
            float v[2][NL];
            info_awgn_log2<NL>(zs.x * scale, amp, ivl, v[0]);
            info_awgn_log2<NL>(zs.y * scale, amp, ivl, v[1]);
            llr_symbol<NL, true>(v, h, out);
        }
#pragma unroll
        for (int i = 0; i < 2 * NB; i++) dst[(size_t)i * Nd + n] = out[i];
    }
}

}  // namespace vaeq

extern "C" int vaeq_awgn_track_llr(int32_t R, int64_t Nz, int64_t Nd, int32_t n_lev, int32_t edge, int32_t interleaved, const float *z,
                                   const void *data_f16, const float *amp, const float *var, const int32_t *shift, const int32_t *hyp,
                                   float *llr, void *stream)
{
    if (R == 0) return VAEQ_OK;                                // an empty batch owns no memory: its pointers may be NULL
    if (!z || !data_f16 || !amp || !var || !shift || !hyp || !llr) return VAEQ_ERR_NULL;
    if (!vaeq::track_shape_ok(R, Nz, Nd, edge, interleaved)) return VAEQ_ERR_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const __half *tx = reinterpret_cast<const __half *>(data_f16);
    return vaeq::dispatch_nlev(n_lev, [&](auto nl) {
        constexpr int NL = decltype(nl)::value;
        auto k = interleaved ? vaeq::awgn_track_llr_kernel<NL, true> : vaeq::awgn_track_llr_kernel<NL, false>;
        return vaeq::launch(k, dim3(R), dim3(vaeq::TLLR_NT), 0, st, (int)Nz, (int)Nd, edge, z, tx, amp, var, shift, hyp, llr);
    });
}
