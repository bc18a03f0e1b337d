// vaeq_awgn_track_info.hip -- information-rate figures of the AWGN baselines on the device: achievable rate of symbol-wise mismatched decoding
// (AIR), generalised mutual information of the bit-wise decoder (GMI) and the pre-FEC bit error rate, per run, of a complex soft sequence z in
// memory -- the CPE output of the constant-modulus script, the LMMSE output, the DFE's slicer input -- over exactly the symbols the SER of its
// validator keeps (SER_CMA / SER_func on z[:, e+sh : -e] against data[:, e : -e-sh]; func_CMA_MQAM_shaping.py:231-232, DFE_MQAM_shaping.py:281,
// :293).  The reference has no such metric; the definitions are closed-form (include/vaeq.h, DESIGN.md section 5,
// tests/_ref_awgn_baseline_info.py).
//
// awgn_track_info_kernel: one 256-thread workgroup per run.  A pre-pass forms the two radius sums of the validators' normalisation (eval_ser,
// vaeq_awgn_eval.h: mean|tx| over the L kept symbols, mean|z| over ALL Lz samples of the slice, which for the LMMSE output is one more), in
// eval_ser's order: per thread strided in index order, then eval_block_sum.  Every kept symbol is then read ONCE, scaled, demapped by the AWGN
// reference's own demapper (func_VAELE_MQAM_shaping.py:229: -(zhat_c - a_i)^2 / var per axis, no 1/2, no prior term) in the log domain, and all
// four relabelings of eval_ser (e0..e3, in that order) accumulate in that pass; nothing else goes to memory.  The per-symbol body and the tail
// are vaeq_info.h's (info_symbol<NL, true, 4>, info_finish with K = L given): this file holds the window, the normalisation and the exponent.
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
    constexpr float LOG2E = 1.4426950408889634f;
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
    // the window: kept symbol j < L pairs sample r0 + j with TX symbol edge + j, and the slice of z holds Lz = L + (Nz - Nd) samples from r0 on.
    // Where it is not empty r0 >= 1, r0 + Lz = Nz - edge and edge + L = Nd - r0 < Nd: every index stays inside its row.  (64-bit: the lengths
    // leave int32 for a shift or an edge nobody can find but anybody can pass)
    const long long sft = shift[run], L64 = (long long)Nd - 2LL * edge - sft;
    if ((long long)edge + sft <= 0 || L64 <= 0) {              // (uniform: every thread of the workgroup takes the same side)
        nothing();
        return;
    }
    const int L = (int)L64, Lz = L + (Nz - Nd), r0 = edge + (int)sft;
    const float *zr = zg + (size_t)run * 2 * Nz;
    auto track = [&](int m) {
        if constexpr (INTERLEAVED) return *reinterpret_cast<const float2 *>(zr + 2 * (size_t)m);
        else return make_float2(zr[m], zr[(size_t)Nz + m]);
    };
    const __half *txI = txg + (size_t)run * 2 * Nd + edge, *txQ = txI + Nd;

    // eval_ser's normalisation: scale = mean|tx| (L symbols) / mean|z| (all Lz samples of the slice)
    float at = 0.f, ar = 0.f;
    for (int m = tid; m < L; m += TINFO_NT) {
        const float t0 = __half2float(txI[m]), t1 = __half2float(txQ[m]);
        const float2 v = track(r0 + m);
        at += sqrtf(t0 * t0 + t1 * t1);
        ar += sqrtf(v.x * v.x + v.y * v.y);
    }
    for (int m = L + tid; m < Lz; m += TINFO_NT) {             // the samples past the data slice (LMMSE: one)
        const float2 v = track(r0 + m);
        ar += sqrtf(v.x * v.x + v.y * v.y);
    }
    at = eval_block_sum<TINFO_NT>(at, red, tid);
    ar = eval_block_sum<TINFO_NT>(ar, red, tid);
    if (ar == 0.f) {                                           // a slice that is zero throughout has no normalisation: no measurement
        nothing();
        return;
    }
    const float scale = (at / (float)L) / (ar / (float)Lz);
    const float ivl = LOG2E / var[run];
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
        const float zc[2] = {zs.x * scale, zs.y * scale};
        float v[2][NL];
#pragma unroll
        for (int c = 0; c < 2; c++)
#pragma unroll
            for (int i = 0; i < NL; i++) {
                const float dd = zc[c] - amp[i];
                v[c][i] = -(dd * dd) * ivl;
            }
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
    if (R < 0 || Nd < 1 || (Nz != Nd && Nz != Nd + 1) || Nz > 0x3fffffff || edge < 0 || (interleaved != 0 && interleaved != 1))
        return VAEQ_ERR_SHAPE;
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
