// vaeq_awgn_track_info.hip -- information-rate figures of the AWGN baselines on the device: achievable rate of symbol-wise mismatched decoding
// (AIR), generalised mutual information of the bit-wise decoder (GMI) and the pre-FEC bit error rate, per run, of a complex soft sequence z in
// memory -- the CPE output of the constant-modulus script, the LMMSE output, the DFE's slicer input -- over exactly the symbols the SER of its
// validator keeps (SER_CMA / SER_func on z[:, e+sh : -e] against data[:, e : -e-sh]; func_CMA_MQAM_shaping.py:231-232, DFE_MQAM_shaping.py:281,
// :293).  The reference has no such metric; the definitions are closed-form (include/vaeq.h, DESIGN.md section 5,
// tests/_ref_awgn_baseline_info.py).
//
// awgn_track_info_kernel: one 256-thread workgroup per run.  A pre-pass forms the validators' normalisation (eval_radius_scale, vaeq_awgn_eval.h,
// which eval_ser calls too: mean|tx| over the L kept symbols, mean|z| over ALL Lz samples of the slice, which for the LMMSE output is one more).
// Every kept symbol is then read ONCE, scaled, demapped by the AWGN reference's own demapper (info_awgn_log2, vaeq_info.h) in the log domain, and
// all four relabelings of eval_ser (e0..e3, in that order) accumulate in that pass; nothing else goes to memory.  Window, track, normalisation and
// exponent are the text awgn_track_llr_kernel runs as well; the per-symbol body and the tail are vaeq_info.h's (info_symbol<NL, true, 4>,
// info_finish with K = L given).  This file holds the early-outs and the accumulation.
// Integer counts are exact; float sums run in a fixed order without atomics: two calls give identical bits, R runs the bits of R single calls.
//
// dfe_soft_kernel: the soft sequence the reference's DFE never keeps -- the slicer input of dfe() (DFE_MQAM_shaping.py:215-221) rebuilt from the
// feed-forward output and the decisions vaeq_awgn_dfe returns, one thread per sample.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "vaeq.h"
#include "vaeq_awgn_eval.h"
#include "vaeq_info.h"
#include "vaeq_launch.h"
#include "vaeq_wave.h"

namespace vaeq {

constexpr int TINFO_NT = 256, TINFO_WAVES = TINFO_NT / 64;

template <int NL, bool INTERLEAVED>
__global__ __launch_bounds__(TINFO_NT) void awgn_track_info_kernel(int Nz, int Nd, int edge, const float *__restrict__ zg,
                                                                   const __half *__restrict__ txg, const float *__restrict__ amp_g,
                                                                   const float *__restrict__ Pg, const float *__restrict__ var,
                                                                   const int32_t *__restrict__ shift, float *__restrict__ info,
                                                                   int32_t *__restrict__ counts)
{
    __shared__ float red[TINFO_WAVES];                         // eval_block_sum's scratch
    __shared__ InfoShared<4, TINFO_WAVES> sh;
    const int run = blockIdx.x, tid = threadIdx.x;
    float *o = info + (size_t)run * 3;
    int32_t *cn = counts + (size_t)run * 4;
    auto nothing = [&]() {                                     // nothing kept is no measurement (the NaN of the validator's SER)
        if (tid == 0) {
            o[0] = o[1] = o[2] = NAN;
            cn[0] = cn[1] = cn[2] = cn[3] = 0;
        }
    };
    const TrackWindow w(Nz, Nd, edge, shift[run]);
    if (w.empty) {
        nothing();
        return;
    }
    const int L = w.L, r0 = w.sample(0);
    const TrackRow<INTERLEAVED> track{zg + (size_t)run * 2 * Nz, Nz};
    const __half *txI = txg + (size_t)run * 2 * Nd + edge, *txQ = txI + Nd;
    float ar;
    const float scale = eval_radius_scale<TINFO_NT>(track, r0, w.Lz, txI, txQ, L, red, tid, ar);
    if (ar == 0.f) {                                           // a slice that is zero throughout has no normalisation: no measurement
        nothing();
        return;
    }
    const float ivl = INFO_LOG2E / var[run];
    float amp[NL];
#pragma unroll
    for (int i = 0; i < NL; i++) amp[i] = amp_g[i];

    float fs[8];
    int se[4], be[4];
#pragma unroll
    for (int i = 0; i < 8; i++) fs[i] = 0.f;
#pragma unroll
    for (int i = 0; i < 4; i++) se[i] = be[i] = 0;
    for (int j = tid; j < L; j += TINFO_NT) {
        const float2 zs = track(r0 + j);
        float v[2][NL];
        info_awgn_log2<NL>(zs.x * scale, amp, ivl, v[0]);
        info_awgn_log2<NL>(zs.y * scale, amp, ivl, v[1]);
        info_symbol<NL, true, 4>(v, txI[j], txQ[j], fs, se, be);
    }
    info_finish<NL, 4, TINFO_WAVES, false>(sh, tid, fs, se, be, L, Pg + (size_t)run * NL, o, cn);
}

// z[p] = ff[p] + sum_{j < K2} fb[j] c(dec[p - 1 - j]) for p >= K2, c(i) = amp[i / n] + j amp[i % n]: plain complex products added to the
// feed-forward sample, j ascending (the order of :215-217); z[p] = c(dec[p]) for p < K2, where no slicer input exists.  Grid (ceil(N / 256), runs).
__global__ __launch_bounds__(256) void dfe_soft_kernel(int R, int N, int n_lev, int K2, const float2 *__restrict__ ff,
                                                       const float *__restrict__ fb, const int8_t *__restrict__ dec,
                                                       const float *__restrict__ amp, float2 *__restrict__ z)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= N) return;
    for (int run = blockIdx.y; run < R; run += gridDim.y) {
        const int8_t *dr = dec + (size_t)run * N;
        const float *fr = fb + (size_t)run * 2 * K2, *fi = fr + K2;
        auto point = [&](int q) {
            const int d = (uint8_t)dr[q];                      // < n_lev^2 (masked all the same: the lookups stay inside amp)
            return make_float2(amp[(d / n_lev) % n_lev], amp[d % n_lev]);
        };
        float2 out;
        if (p < K2) {
            out = point(p);
        } else {
            const float2 f = ff[(size_t)run * N + p];
            float sr = f.x, si = f.y;
            for (int j = 0; j < K2; j++) {
                const float2 c = point(p - 1 - j);
                sr = fmaf(fr[j], c.x, sr);
                sr = fmaf(-fi[j], c.y, sr);
                si = fmaf(fr[j], c.y, si);
                si = fmaf(fi[j], c.x, si);
            }
            out = make_float2(sr, si);
        }
        z[(size_t)run * N + p] = out;
    }
}

}  // namespace vaeq

extern "C" int vaeq_awgn_track_info(int32_t R, int64_t Nz, int64_t Nd, int32_t n_lev, int32_t edge, int32_t interleaved, const float *z,
                                    const void *data_f16, const float *amp, const float *P, const float *var, const int32_t *shift,
                                    float *info, int32_t *counts, void *stream)
{
    if (R == 0) return VAEQ_OK;                                // an empty batch owns no memory: its pointers may be NULL
    if (!z || !data_f16 || !amp || !P || !var || !shift || !info || !counts) return VAEQ_ERR_NULL;
    if (!vaeq::track_shape_ok(R, Nz, Nd, edge, interleaved)) return VAEQ_ERR_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const __half *tx = reinterpret_cast<const __half *>(data_f16);
    return vaeq::dispatch_nlev(n_lev, [&](auto nl) {
        constexpr int NL = decltype(nl)::value;
        auto k = interleaved ? vaeq::awgn_track_info_kernel<NL, true> : vaeq::awgn_track_info_kernel<NL, false>;
        return vaeq::launch(k, dim3(R), dim3(vaeq::TINFO_NT), 0, st, (int)Nz, (int)Nd, edge, z, tx, amp, P, var, shift, info, counts);
    });
}

extern "C" int vaeq_awgn_dfe_soft(int32_t R, int64_t N, int32_t n_lev, int32_t K2, const float *ff, const float *fb, const int8_t *dec,
                                  const float *amp, float *z, void *stream)
{
    if (R == 0) return VAEQ_OK;
    if (!ff || !fb || !dec || !amp || !z) return VAEQ_ERR_NULL;
    if (R < 0 || N < 1 || N > 0x3fffffff || !(n_lev == 2 || n_lev == 4 || n_lev == 8) || K2 < 1 || K2 > 10) return VAEQ_ERR_SHAPE;
    return vaeq::launch(vaeq::dfe_soft_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)(R < 65535 ? R : 65535)), dim3(256), 0,
                        reinterpret_cast<hipStream_t>(stream), R, (int)N, n_lev, K2, reinterpret_cast<const float2 *>(ff), fb, dec, amp,
                        reinterpret_cast<float2 *>(z));
}
