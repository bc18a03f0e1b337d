// vaeq_awgn_track_llr.hip -- the per-bit a-posteriori LLRs of the AWGN baselines on the device: what a bit-wise (LDPC) decoder behind the
// constant-modulus script's CPE output, the LMMSE output or the DFE's slicer input reads, and what the GMI of vaeq_awgn_track_info is the rate of.
// Window, both layouts, normalisation and demapper are that kernel's (vaeq_awgn_track_info.hip): kept symbol j < L = Nd - 2 edge - sh pairs
// sample edge + sh + j with TX symbol edge + j, scale = mean|tx| (L symbols) / mean|z| (ALL Lz = L + Nz - Nd samples of the slice), exponent
// -(zhat_c - a_i)^2 log2 e / var.  Under the rotation that kernel picked (hyp & 3) the LLRs land in TX order: plane a b + k at TX index edge + j is
// bit k of TX axis a of that symbol; every other entry is an erasure, +0.0, and an empty window or a slice that is zero throughout is all zeros.
//
// One 256-thread workgroup per run.  scale multiplies every sample, and the LLRs are those of the posteriors whose GMI is reported only if it is
// the same float -- so the pre-pass is awgn_track_info_kernel's restated, term for term (per thread strided in index order, the tail loop for the
// samples past the data, then eval_block_sum).  After it the work is elementwise: thread t takes TX indices t, t + 256, ..., consecutive lanes on
// consecutive n, every read and each of the 2 b plane stores contiguous across the wave.  No atomics: two calls give identical bits.
// This file holds the window, the pre-pass and the exponent; the per-symbol body is vaeq_llr.h's.
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
    constexpr float LOG2E = 1.4426950408889634f;
    constexpr int NB = llr_bits(NL);
    __shared__ float red[TLLR_NT / 64];                        // eval_block_sum's scratch
    const int run = blockIdx.x, tid = threadIdx.x;
    // the window of awgn_track_info_kernel (64-bit: the lengths leave int32 for a shift or an edge nobody can find but anybody can pass).  Where it
    // is not empty r0 >= 1, r0 + Lz = Nz - edge and edge + L = Nd - r0 < Nd: every index stays inside its row.
    const long long sft = shift[run], L64 = (long long)Nd - 2LL * edge - sft;
    bool empty = (long long)edge + sft <= 0 || L64 <= 0;       // (uniform: every thread of the workgroup takes the same side)
    const int L = empty ? 0 : (int)L64, Lz = empty ? 0 : L + (Nz - Nd), r0 = empty ? 0 : edge + (int)sft;
    const float *zr = zg + (size_t)run * 2 * Nz;
    auto track = [&](int m) {
        if constexpr (INTERLEAVED) return *reinterpret_cast<const float2 *>(zr + 2 * (size_t)m);
        else return make_float2(zr[m], zr[(size_t)Nz + m]);
    };

    // eval_ser's normalisation: scale = mean|tx| (L symbols) / mean|z| (all Lz samples of the slice); an empty window walks nothing
    float at = 0.f, ar = 0.f;
    if (!empty) {
        const __half *txI = txg + (size_t)run * 2 * Nd + edge, *txQ = txI + Nd;
        for (int m = tid; m < L; m += TLLR_NT) {
            const float t0 = __half2float(txI[m]), t1 = __half2float(txQ[m]);
            const float2 v = track(r0 + m);
            at += sqrtf(t0 * t0 + t1 * t1);
            ar += sqrtf(v.x * v.x + v.y * v.y);
        }
        for (int m = L + tid; m < Lz; m += TLLR_NT) {          // the samples past the data slice (LMMSE: one)
            const float2 v = track(r0 + m);
            ar += sqrtf(v.x * v.x + v.y * v.y);
        }
    }
    at = eval_block_sum<TLLR_NT>(at, red, tid);
    ar = eval_block_sum<TLLR_NT>(ar, red, tid);
    if (ar == 0.f) empty = true;                               // a slice that is zero throughout has no normalisation: nothing to report
    const float scale = (at / (float)L) / (ar / (float)Lz);
    const float ivl = LOG2E / var[run];
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
            const float zc[2] = {zs.x * scale, zs.y * scale};
            float v[2][NL];
#pragma unroll
            for (int c = 0; c < 2; c++)
#pragma unroll
                for (int i = 0; i < NL; i++) {
                    const float dd = zc[c] - amp[i];
                    v[c][i] = -(dd * dd) * ivl;
                }
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
    if (R < 0 || Nd < 1 || (Nz != Nd && Nz != Nd + 1) || Nz > 0x3fffffff || edge < 0 || (interleaved != 0 && interleaved != 1))
        return VAEQ_ERR_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const __half *tx = reinterpret_cast<const __half *>(data_f16);
    return vaeq::dispatch_nlev(n_lev, [&](auto nl) {
        constexpr int NL = decltype(nl)::value;
        auto k = interleaved ? vaeq::awgn_track_llr_kernel<NL, true> : vaeq::awgn_track_llr_kernel<NL, false>;
        return vaeq::launch(k, dim3(R), dim3(vaeq::TLLR_NT), 0, st, (int)Nz, (int)Nd, edge, z, tx, amp, var, shift, hyp, llr);
    });
}
