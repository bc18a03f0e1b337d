// vaeq_awgn_eval.h -- the evaluation tail of the AWGN baselines on a track in memory, for one NT-thread workgroup per run:
//   find_shift_symb (func_CMA_MQAM_shaping.py:127-140 = DFE_MQAM_shaping.py:137-150) and SER_CMA / SER_func (:63-94 = DFE_MQAM_shaping.py:107-135).
// Shared by the CMA validation kernel (vaeq_awgn_cma.hip) and the LMMSE / DFE evaluation kernels (vaeq_awgn_dfe.hip).  A track is any
// callable m -> float2 (re, im) of the equaliser output; the TX reference is the fp16 data of the run.
// The window and the normalisation of that SER are also what the information-rate and LLR kernels of the AWGN family evaluate on
// (vaeq_awgn_track_info / _llr.hip on a track, vaeq_awgn_info / _llr.hip on a validation frame), so they are written once, here: TrackWindow,
// TrackRow, eval_radius_scale, awgn_row_scales.  A factor formed here multiplies every sample; two kernels that call the same function on the
// same run get the same float.
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "vaeq_wave.h"

namespace vaeq {

// Block sum of one float per thread in a fixed order (DPP wave sums, then the NT / 64 wave sums in wave order): deterministic and the same
// for every run of a batch.  red: NT / 64 floats.
template <int NT>
__device__ __forceinline__ float eval_block_sum(float v, float *red, int tid)
{
    v = wave_sum_dpp(v);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < NT / 64; w++) s += red[w];
    __syncthreads();
    return s;
}

// The window of a validator's SER, z[:, e+sh : -e] against data[:, e : -e-sh] (func_CMA_MQAM_shaping.py:231-232, DFE_MQAM_shaping.py:281, :293;
// with Nz = Nd = N and e = AWGN_EDGE the window of validate_tail, vaeq_validate.h): kept symbol j < L pairs sample r0 + j, r0 = edge + shift, with
// TX symbol edge + j, and the slice of z holds Lz = L + (Nz - Nd) samples from r0 on.  Where it is not empty r0 >= 1, r0 + Lz = Nz - edge and
// edge + L = Nd - r0 < Nd: every index stays inside its row.  (64-bit: the lengths leave int32 for a shift or an edge nobody can find but anybody
// can pass.)  An empty window has L = Lz = 0, so that it walks nothing.
constexpr int AWGN_EDGE = 11;
struct TrackWindow {
    bool empty;
    int L, Lz, edge, sft;
    __device__ __forceinline__ TrackWindow(int Nz, int Nd, int edge_, int shift) : edge(edge_), sft(shift)
    {
        const long long L64 = (long long)Nd - 2LL * edge - sft;
        empty = (long long)edge + sft <= 0 || L64 <= 0;        // (uniform: every thread of the workgroup takes the same side)
        L = empty ? 0 : (int)L64;
        Lz = empty ? 0 : L + (Nz - Nd);
    }
    __device__ __forceinline__ int sample(int j) const { return edge + sft + j; }   // of kept symbol j < L, or of slice sample j < Lz
};

// a track in memory: complex [Nz] (INTERLEAVED) or float [2][Nz] (planar)
template <bool INTERLEAVED>
struct TrackRow {
    const float *zr;
    int Nz;
    __device__ __forceinline__ float2 operator()(int m) const
    {
        if constexpr (INTERLEAVED) return *reinterpret_cast<const float2 *>(zr + 2 * (size_t)m);
        else return make_float2(zr[m], zr[(size_t)Nz + m]);
    }
};

// The radius normalisation of SER_CMA / SER_func on track[r0 : r0 + Lr] against the TX slice d0, d1 [L], Lr >= L:
// scale = mean|tx| (L symbols) / mean|track| (ALL Lr samples), per thread strided in index order, then eval_block_sum.  ar: sum |track|, whose
// zero means a slice without a normalisation.  red: NT / 64 floats.  Returns scale in every thread.
template <int NT, class Track>
__device__ __forceinline__ float eval_radius_scale(const Track &track, int r0, int Lr, const __half *d0, const __half *d1, int L, float *red,
                                                   int tid, float &ar)
{
    float at = 0.f;
    ar = 0.f;
    for (int m = tid; m < L; m += NT) {
        const float t0 = __half2float(d0[m]), t1 = __half2float(d1[m]);
        const float2 v = track(r0 + m);
        at += sqrtf(t0 * t0 + t1 * t1);
        ar += sqrtf(v.x * v.x + v.y * v.y);
    }
    for (int m = L + tid; m < Lr; m += NT) {                   // the track samples past the data slice (LMMSE: one)
        const float2 v = track(r0 + m);
        ar += sqrtf(v.x * v.x + v.y * v.y);
    }
    at = eval_block_sum<NT>(at, red, tid);
    ar = eval_block_sum<NT>(ar, red, tid);
    return (at / (float)L) / (ar / (float)Lr);
}

// The VAE-LE demapper's normalisation of a validation frame y[2][N] (func_VAELE_MQAM_shaping.py:228): sc[c] = A / m_c, m_c = sum_n |y_c[n]| / N
// over the WHOLE row, per thread in index order, then eval_block_sum; walk = false sums nothing (an empty window needs no factor).
// Returns false where a component is zero throughout: no normalisation, no measurement.
template <int NT>
__device__ __forceinline__ bool awgn_row_scales(const float *__restrict__ src, int N, bool walk, float A, float *red, int tid, float (&sc)[2])
{
    float sa0 = 0.f, sa1 = 0.f;
    if (walk) {                                                // (uniform: every thread of the workgroup takes the same side)
#pragma unroll 4
        for (int n = tid; n < N; n += NT) { sa0 += fabsf(src[n]); sa1 += fabsf(src[(size_t)N + n]); }
    }
    sa0 = eval_block_sum<NT>(sa0, red, tid);
    sa1 = eval_block_sum<NT>(sa1, red, tid);
    const float m0 = sa0 / (float)N, m1 = sa1 / (float)N;
    sc[0] = A / m0; sc[1] = A / m1;
    return m0 != 0.f && m1 != 0.f;
}

// find_shift_symb(track, tx, n_shift) (n_shift <= 64): corr[rail][i] = sum_m tx[rail][hs + m] * track(i + m).x, m < 1000 - hs, one wave per
// dot product; the I-rail peak wins when it reaches 0.02 * len (len = the track's length, rx.shape[-1]), else the larger of both peaks.
// corr: [2][64] floats in LDS.  Returns the shift in every thread.
template <int NT, class Track>
__device__ __forceinline__ int eval_find_shift(const Track &track, const __half *tx0, const __half *tx1, int n_shift, int len,
                                               float (*corr)[64], int *sh_shift, int tid)
{
    const int lane = tid & 63, wv = tid >> 6;
    const int hsh = n_shift / 2, nm = 1000 - hsh;
    for (int q = wv; q < 2 * n_shift; q += NT / 64) {
        const int rail = q / n_shift, i = q - rail * n_shift;
        const __half *t = rail ? tx1 : tx0;
        float acc = 0.f;
        for (int m = lane; m < nm; m += 64) acc = fmaf(__half2float(t[hsh + m]), track(i + m).x, acc);
        acc = wave_sum_dpp(acc);
        if (lane == 0) corr[rail][i] = acc;
    }
    __syncthreads();
    if (tid == 0) {
        float mI = -1.f, mQ = -1.f;
        int aI = 0, aQ = 0;
        for (int i = 0; i < n_shift; i++) {                    // argmax: the first index on ties, as torch.argmax
            const float vI = fabsf(corr[0][i]), vQ = fabsf(corr[1][i]);
            if (vI > mI) { mI = vI; aI = i; }
            if (vQ > mQ) { mQ = vQ; aQ = i; }
        }
        const float thr = (float)(0.02 * (double)len);         // 0.02 * rx.shape[-1] compared in float32
        *sh_shift = (mI >= thr ? aI : (mQ >= mI ? aQ : aI)) - hsh;
    }
    __syncthreads();
    return *sh_shift;
}

// SER(track[r0 : r0 + Lr], tx[:, d : d + L]) with Lr >= L: rescale by mean|tx| (L symbols) / mean|track| (all Lr samples), per-axis
// nearest-level decisions on the first L samples, minimum error rate over the 0 / pi / pi/4 / 3pi/4 relabelings.  Lr = L + 1 is the LMMSE
// evaluation of DFE_MQAM_shaping.py:282 (its output slice is one sample longer than the data slice).  lev: n_lev levels (LDS or registers).
// The result is valid in thread 0.
template <int NT, class Track>
__device__ __forceinline__ float eval_ser(const Track &track, int r0, int Lr, const __half *d0, const __half *d1, int L, const float *lev,
                                          int n_lev, float *red, int tid)
{
    float ar;
    const float scale = eval_radius_scale<NT>(track, r0, Lr, d0, d1, L, red, tid, ar);
    const float sl = 0.5f * (float)(n_lev - 1);
    const int top = n_lev - 1;                                 // 2 * scale: the level index mirror
    int e0 = 0, e1 = 0, e2 = 0, e3 = 0;
    for (int m = tid; m < L; m += NT) {
        const float2 v = track(r0 + m);
        // the distance to level 0 is one fused multiply-add, the others a rounded product minus the level (the contraction the CMA
        // validation kernel compiled to before this code was shared: written out so that it cannot change with the caller)
        const float sI = __fmul_rn(v.x, scale), sQ = __fmul_rn(v.y, scale);
        int cI = 0, cQ = 0;
        float bI = fabsf(fmaf(v.x, scale, -lev[0])), bQ = fabsf(fmaf(v.y, scale, -lev[0]));
        for (int l = 1; l < n_lev; l++) {                      // argmin: the first index on ties
            const float dI = fabsf(__fsub_rn(sI, lev[l])), dQ = fabsf(__fsub_rn(sQ, lev[l]));
            if (dI < bI) { bI = dI; cI = l; }
            if (dQ < bQ) { bQ = dQ; cQ = l; }
        }
        const int tI = (int)rintf(__fadd_rn(__fmul_rn(sl, __half2float(d0[m])), sl));
        const int tQ = (int)rintf(__fadd_rn(__fmul_rn(sl, __half2float(d1[m])), sl));
        e0 += (tI != cI) | (tQ != cQ);
        e1 += (tI != top - cI) | (tQ != top - cQ);
        e2 += (tI != top - cQ) | (tQ != cI);
        e3 += (tI != cQ) | (tQ != top - cI);
    }
    const float f0 = eval_block_sum<NT>((float)e0, red, tid), f1 = eval_block_sum<NT>((float)e1, red, tid);   // counts < 2^24: exact in float
    const float f2 = eval_block_sum<NT>((float)e2, red, tid), f3 = eval_block_sum<NT>((float)e3, red, tid);
    const float fL = (float)L;
    return fminf(fminf(f0 / fL, f1 / fL), fminf(f2 / fL, f3 / fL));
}

}  // namespace vaeq
