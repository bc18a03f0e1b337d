// vaeq_awgn_cma.hip -- the constant-modulus baseline of the AWGN scripts (AWGN_channel/func_CMA_MQAM_shaping.py, driven by
// Eval_run_shaping_cma.py).  NOT the DP CMA of vaeq_cma.hip with one polarisation removed:
//
//   CMA (:142-168): ONE complex FIR h[2][M] (re, im) on the UNSCALED frame (no division by the mean power), out0 = y0 h0 - y1 h1,
//   out1 = y0 h1 + y1 h0, e = R - out0^2 - out1^2, h0 += 2 lr e (out0 y0 + out1 y1), h1 += 2 lr e (out1 y0 - out0 y1) after every symbol
//   (eval = True).  Symbol j reads the zero-padded samples [sps j, sps j + 2 mh] and lands at k = j - (mh - mh / sps): the first symbols wrap
//   to the END of out / e -- kept, because in validation they shape the CPE's moving average over the frame's last ~250 symbols.
//   CPE (:170-198): 4th power, 501-tap zero-padded moving average, atan2(ma_im, -ma_re) / 4, de-rotation -- WITHOUT the pi/2 unwrapping of the
//   DP CPE (vaeq_cpe).
//   find_shift_symb (:127-140): correlation of tx[0, 10:1000] with the I rail of the CPE output at 21 lags (Q rail of tx as the fallback).
//   SER_CMA (:63-94): rescale by mean|tx| / mean|rx| (tx = the fp16 TX symbols), per-axis nearest-level decisions, minimum over the 0 / pi /
//   pi/4 / 3pi/4 relabelings.
//
// awgn_cma_kernel: the training pass (and CMA(..., eval=False) with update = 0); sequential in the symbol index, one 64-lane wave per run,
// lanes over taps.  awgn_cma_validate_kernel: one evaluated epoch (:225-232) -- FIR with the fixed taps, CPE, find_shift_symb and SER_CMA --
// in one launch, one 1024-thread workgroup per run, parallel over symbols.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vaeq.h"
#include "vaeq_awgn_eval.h"
#include "vaeq_common.h"
#include "vaeq_launch.h"
#include "vaeq_wave.h"

#ifndef AWGN_CMA_AHEAD
#define AWGN_CMA_AHEAD 8                                       // symbols whose windows are in flight ahead of the one being computed
#endif

namespace vaeq {

// HALF (M <= 31): lanes 0..31 form the partial products of out0, lanes 32..63 those of out1 (both halves hold tap lane & 31): a symbol costs
// one half-wave row sum (4 DPP adds, 4 readlanes) instead of two full wave sums.  !HALF: lane = tap, two wave sums (M <= 63).
template <bool HALF>
__global__ __launch_bounds__(64) void awgn_cma_kernel(int N, int sps, int M, int update, const float *__restrict__ rx, float Rc,
                                                      float *__restrict__ h, const float *__restrict__ lr, float *__restrict__ loss,
                                                      float *__restrict__ out, float *__restrict__ eout)
{
    constexpr int D = AWGN_CMA_AHEAD;
    const int run = blockIdx.x, lane = threadIdx.x;
    const int tl = HALF ? (lane & 31) : lane;
    const bool upper = HALF && lane >= 32;
    const int mh = M / 2, K = N / sps, joff = mh - mh / sps;  // kraw = j - joff (:160)
    const float *x0 = rx + (size_t)run * 2 * N, *x1 = x0 + N;
    const bool tap = tl < M;
    float *hrun = h + (size_t)run * 2 * M;
    float h0 = tap ? hrun[tl] : 0.f, h1 = tap ? hrun[M + tl] : 0.f;
    const float two_lr = 2.0f * lr[run];
    float *o0 = out ? out + (size_t)run * 2 * K : nullptr, *erun = eout ? eout + (size_t)run * K : nullptr;
    // window sample of tap tl for symbol j: padded position sps j + tl = sample sps j + tl - mh, zero outside the frame.  The load (from a
    // clamped index: no divergent branch on the chain) and the zero mask are apart: the mask is applied when the symbol is computed, so the
    // select does not wait for the load D symbols early.  Positions past the end -- the look-ahead of the last symbols -- are masked too.
    auto inside = [&](int j) {
        const int sx = sps * j + tl - mh;
        return tap && sx >= 0 && sx < N;
    };
    auto fetch = [&](int j, float &a, float &b) {
        const int sc = inside(j) ? sps * j + tl - mh : 0;
        a = x0[sc];
        b = x1[sc];
    };
    // The per-symbol chain is: two sums, one error, one rank-1 update.  What must not sit on it is memory latency: the windows of the next D
    // symbols are in flight (a register ring, static slots through the unrolled inner loop), and outputs are parked one symbol per lane and
    // leave 64 symbols at a time as coalesced rows (a per-symbol store would make every next window wait for it: gfx9 counts stores in vmcnt).
    float q0[D], q1[D];
#pragma unroll
    for (int d = 0; d < D; d++) fetch(d, q0[d], q1[d]);
    float keep0 = 0.f, keep1 = 0.f, keep2 = 0.f, esum = 0.f;
    for (int j0 = 0; j0 < K; j0 += D) {
#pragma unroll
        for (int d = 0; d < D; d++) {
            const int j = j0 + d;
            if (j >= K) break;                                 // uniform
            const bool ok = inside(j);
            const float y0 = ok ? q0[d] : 0.f, y1 = ok ? q1[d] : 0.f;
            fetch(j + D, q0[d], q1[d]);
            float s0, s1;
            if constexpr (HALF) {
                float p = upper ? fmaf(y0, h1, y1 * h0) : fmaf(y0, h0, -(y1 * h1));
                p += dpp_f<0xB1>(p);                           // sums inside each 16-lane row ...
                p += dpp_f<0x4E>(p);
                p += dpp_f<0x141>(p);
                p += dpp_f<0x140>(p);
                const int b = __builtin_bit_cast(int, p);
                auto rl = [](int v, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(v, l)); };
                s0 = rl(b, 0) + rl(b, 16);                     // ... rows 0 + 1 = out0, rows 2 + 3 = out1
                s1 = rl(b, 32) + rl(b, 48);
            } else {
                s0 = wave_sum_dpp(fmaf(y0, h0, -(y1 * h1)));
                s1 = wave_sum_dpp(fmaf(y0, h1, y1 * h0));
            }
            const float e = Rc - s0 * s0 - s1 * s1;
            esum += fabsf(e);
            if (lane == (j & 63)) { keep0 = s0; keep1 = s1; keep2 = e; }
            if ((j & 63) == 63 || j == K - 1) {                // uniform: flush the parked symbols (j & ~63) .. j
                const int jl = (j & ~63) + lane;
                if (jl <= j) {
                    const int kr = jl - joff, kl = kr < 0 ? kr + K : kr;
                    if (o0) { o0[kl] = keep0; o0[K + kl] = keep1; }
                    if (erun) erun[kl] = keep2;
                }
            }
            if (update) {                                      // :164-166
                const float ge = two_lr * e;
                h0 += ge * (s0 * y0 + s1 * y1);
                h1 += ge * (s1 * y0 - s0 * y1);
            }
        }
    }
    if (lane == 0) loss[run] = esum / (float)K;                // torch.mean(torch.abs(e)) (:222), symbol order
    if (update && tap && !upper) {
        hrun[tl] = h0;
        hrun[M + tl] = h1;
    }
}

constexpr int AV_NT = 1024;                                    // threads of the validation workgroup
constexpr int AV_CH = 17;                                      // LDS form: symbols per thread (odd: the chunks start on different banks)
constexpr int AV_LDS_K = AV_NT * AV_CH;                        // longest frame (symbols) whose track lives in LDS: 8 * 17408 B = 136 KiB
constexpr int AV_MA = 501;                                     // CPE moving-average length (:172)

__device__ __forceinline__ void pow4(float2 v, float &r, float &i)   // (a + jb)^4 = a^4 - 6 a^2 b^2 + b^4 + j 4 (a^3 b - a b^3)  (:178-181)
{
    const float a2 = v.x * v.x, b2 = v.y * v.y;
    r = a2 * a2 - 6.0f * a2 * b2 + b2 * b2;
    i = 4.0f * (a2 * v.x * v.y - v.x * b2 * v.y);
}

// LDS: the equalised track [K] float2 lives in LDS and is phase-corrected in place (K <= AV_LDS_K).  !LDS: raw and corrected tracks in the
// global workspace ws[R][2][K] float2 (any K; N_valid = 50 000 in the script's alternative setting).
template <bool LDS>
__global__ __launch_bounds__(AV_NT) void awgn_cma_validate_kernel(int N, int sps, int M, int n_lev, int n_shift, const float *__restrict__ rx,
                                                                  const float *__restrict__ h, const float *__restrict__ amp,
                                                                  const __half *__restrict__ data, float2 *__restrict__ ws,
                                                                  float *__restrict__ ser, int32_t *__restrict__ shift_out,
                                                                  float *__restrict__ cpe_out)
{
    extern __shared__ float2 av_track[];
    __shared__ float csr[AV_NT], csi[AV_NT];                   // chunk sums of the 4th power
    __shared__ float red[AV_NT / 64];
    __shared__ float corr[2][64];
    __shared__ float hs[2][64];
    __shared__ float lev[8];
    __shared__ int sh_shift;
    const int run = blockIdx.x, tid = threadIdx.x;
    const int K = N / sps, mh = M / 2, joff = mh - mh / sps;
    const float *x0 = rx + (size_t)run * 2 * N, *x1 = x0 + N;
    float2 *tr = LDS ? av_track : ws + (size_t)run * 2 * K;    // equalised track (k order)
    float2 *yc = LDS ? av_track : tr + K;                      // phase-corrected track
    if (tid < M) {
        hs[0][tid] = h[(size_t)run * 2 * M + tid];
        hs[1][tid] = h[(size_t)run * 2 * M + M + tid];
    }
    if (tid < n_lev) lev[tid] = amp[tid];
    __syncthreads();
    // 1. CMA(..., eval=False) (:154-162): the two dot products of each output as in the reference, symbol j -> k = j - joff (wrapped)
    for (int j = tid; j < K; j += AV_NT) {
        float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;          // y0.h0, y1.h1, y0.h1, y1.h0
        const int s0 = sps * j - mh;
        for (int t = 0; t < M; t++) {
            const int s = s0 + t;
            if (s >= 0 && s < N) {                             // (divergent only in the zero padding at the frame's ends)
                const float v0 = x0[s], v1 = x1[s];
                a0 = fmaf(v0, hs[0][t], a0);
                a1 = fmaf(v1, hs[1][t], a1);
                b0 = fmaf(v0, hs[1][t], b0);
                b1 = fmaf(v1, hs[0][t], b1);
            }
        }
        const int kr = j - joff;
        tr[kr < 0 ? kr + K : kr] = make_float2(a0 - a1, b0 + b1);
    }
    __syncthreads();
    // 2. CPE (:170-198).  A thread owns one chunk of consecutive symbols; the 4th power is recomputed from the track where it is read.
    const int chunk = ((K + AV_NT - 1) / AV_NT) | 1, n0 = min(K, tid * chunk), n1 = min(K, n0 + chunk), half = AV_MA / 2;
    {
        float cr = 0.f, ci = 0.f;
        for (int n = n0; n < n1; n++) {
            float r, i;
            pow4(tr[n], r, i);
            cr += r;
            ci += i;
        }
        csr[tid] = cr;
        csi[tid] = ci;
    }
    __syncthreads();
    float sr = 0.f, si = 0.f;                                  // window sum over [n - half, n + half] (zero outside), first by chunks
    if (n0 < n1) {
        const int lo0 = max(0, n0 - half), hi0 = min(K - 1, n0 + half);
        const int c0 = (lo0 + chunk - 1) / chunk, c1 = (hi0 + 1) / chunk;
        float r, i;
        if (c0 < c1) {
            for (int m = lo0; m < c0 * chunk; m++) { pow4(tr[m], r, i); sr += r; si += i; }
            for (int c = c0; c < c1; c++) { sr += csr[c]; si += csi[c]; }
            for (int m = c1 * chunk; m <= hi0; m++) { pow4(tr[m], r, i); sr += r; si += i; }
        } else {
            for (int m = lo0; m <= hi0; m++) { pow4(tr[m], r, i); sr += r; si += i; }
        }
    }
    auto phase_step = [&](int n) {                             // phase of symbol n (no unwrapping), then slide the window to n + 1
        const float ph = atan2f(si / (float)AV_MA, -sr / (float)AV_MA) * 0.25f;
        const int lo = n - half, hi_ = n + half + 1;
        float r, i;
        if (hi_ < K) { pow4(tr[hi_], r, i); sr += r; si += i; }
        if (lo >= 0) { pow4(tr[lo], r, i); sr -= r; si -= i; }
        return ph;
    };
    auto derotate = [](float2 v, float ph) {
        float sn, cs;
        sincosf(ph, &sn, &cs);
        return make_float2(v.x * cs - v.y * sn, v.y * cs + v.x * sn);
    };
    if constexpr (LDS) {                                       // in place: every window read ends before the first corrected write
        float ph[AV_CH];
#pragma unroll
        for (int c = 0; c < AV_CH; c++)
            if (n0 + c < n1) ph[c] = phase_step(n0 + c);
        __syncthreads();
#pragma unroll
        for (int c = 0; c < AV_CH; c++)
            if (n0 + c < n1) yc[n0 + c] = derotate(tr[n0 + c], ph[c]);
    } else {
        for (int n = n0; n < n1; n++) yc[n] = derotate(tr[n], phase_step(n));
    }
    __syncthreads();
    if (cpe_out) {
        float *c0 = cpe_out + (size_t)run * 2 * K;
        for (int n = tid; n < K; n += AV_NT) {
            const float2 v = yc[n];
            c0[n] = v.x;
            c0[K + n] = v.y;
        }
    }
    // 3. find_shift_symb (:127-140) and 4. SER_CMA(out_cpe[:, 11+shift:-11], data[:, 11:-11-shift]) (:63-94, :231): vaeq_awgn_eval.h
    const __half *tx0 = data + (size_t)run * 2 * K, *tx1 = tx0 + K;
    auto track = [&](int m) { return yc[m]; };
    const int shift = eval_find_shift<AV_NT>(track, tx0, tx1, n_shift, K, corr, &sh_shift, tid);
    const int L = K - 22 - shift;
    const float s = eval_ser<AV_NT>(track, 11 + shift, L, tx0 + 11, tx1 + 11, L, lev, n_lev, red, tid);
    if (tid == 0) {
        ser[run] = s;
        if (shift_out) shift_out[run] = shift;
    }
}

}  // namespace vaeq

extern "C" int vaeq_awgn_cma(int32_t R, int64_t N, int32_t sps, int32_t M, int32_t update, const float *rx, float R_mod, float *h,
                             const float *lr, float *loss, float *out, float *e, void *stream)
{
    if (R < 0 || N <= 0 || N > 0x3fffffff || sps < 1 || sps > 8 || N % sps != 0 || !vaeq::fir_shape_ok(sps, M) || N / sps < M)
        return VAEQ_ERR_SHAPE;
    if (R == 0) return VAEQ_OK;                                // an empty batch owns no memory: its pointers may be NULL
    if (!rx || !h || !lr || !loss) return VAEQ_ERR_NULL;
    auto k = M <= 31 ? vaeq::awgn_cma_kernel<true> : vaeq::awgn_cma_kernel<false>;
    vaeq::note_kernel("vaeq::awgn_cma_kernel<%s>", M <= 31 ? "true" : "false");
    return vaeq::launch(k, dim3(R), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), (int)N, sps, M, update ? 1 : 0, rx, R_mod, h, lr, loss, out, e);
}

static bool awgn_cma_validate_shape(int32_t R, int64_t N, int32_t sps, int32_t M, int32_t n_lev, int32_t n_shift)
{
    return R >= 0 && N > 0 && N <= 0x3fffffff && sps >= 1 && sps <= 8 && N % sps == 0 && vaeq::fir_shape_ok(sps, M) &&
           (n_lev == 2 || n_lev == 4 || n_lev == 8) && n_shift >= 1 && (n_shift & 1) == 1 && n_shift <= 23 && N / sps >= 1000 + n_shift;
}

extern "C" int64_t vaeq_awgn_cma_validate_ws_bytes(int32_t R, int64_t N, int32_t sps)
{
    if (R < 0 || N <= 0 || sps < 1 || N % sps != 0) return VAEQ_ERR_SHAPE;
    const int64_t K = N / sps;
    return K <= vaeq::AV_LDS_K ? 0 : (int64_t)R * 2 * K * (int64_t)sizeof(float2);
}

extern "C" int vaeq_awgn_cma_validate(int32_t R, int64_t N, int32_t sps, int32_t M, int32_t n_lev, int32_t n_shift, const float *rx,
                                      const float *h, const float *amp, const void *data_f16, float *ws, float *ser, int32_t *shift,
                                      float *cpe_out, void *stream)
{
    if (!awgn_cma_validate_shape(R, N, sps, M, n_lev, n_shift)) return VAEQ_ERR_SHAPE;
    if (R == 0) return VAEQ_OK;
    const int64_t K = N / sps;
    const bool lds = K <= vaeq::AV_LDS_K;
    if (!rx || !h || !amp || !data_f16 || !ser || (!lds && !ws)) return VAEQ_ERR_NULL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const __half *d = reinterpret_cast<const __half *>(data_f16);
    float2 *w = reinterpret_cast<float2 *>(ws);
    vaeq::note_kernel("vaeq::awgn_cma_validate_kernel<%s>", lds ? "true" : "false");
    if (lds)
        return vaeq::launch(vaeq::awgn_cma_validate_kernel<true>, dim3(R), dim3(vaeq::AV_NT), (size_t)K * sizeof(float2), st, (int)N, sps, M, n_lev, n_shift,
                            rx, h, amp, d, w, ser, shift, cpe_out);
    return vaeq::launch(vaeq::awgn_cma_validate_kernel<false>, dim3(R), dim3(vaeq::AV_NT), 0, st, (int)N, sps, M, n_lev, n_shift, rx, h, amp, d, w, ser, shift,
                        cpe_out);
}
