// vaeq_ops.hip -- the stand-alone (differentiable) operators of the drop-in surface, one workgroup per run unless noted:
//   DP    soft_demap, dp_forward (inference-mode butterfly FIR), dp_loss, dp_loss_bwd, dp_forward_bwd, and the input gradients dp_loss_bwd_x, dp_forward_bwd_x
//   AWGN  awgn_forward, awgn_loss, awgn_loss_bwd, awgn_forward_bwd, and the input gradients awgn_loss_bwd_x, awgn_forward_bwd_x
// so that a reference-style loop
//     q, out = net(x, ...); loss, _ = loss_function_shaping(q, x, h_est, ...); loss.backward(); optimizer.step()
// runs on HIP kernels through the torch.autograd.Function wrappers (vae_equalizer_amd/autograd_ops.py).  None of this is the training
// hot path (the fused vaeq_dp_train / vaeq_awgn_train).  A loss kernel and its backward share their first four phases -- moments of q,
// residual e = x - h (*) mu, the variance window sums VS, and C -- and the two AWGN forward kernels share the FIR: each phase is written
// once below.  The DP and AWGN families stay apart: their LDS layouts (dynamic vs. static taps), ceilings and transcendentals differ.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vaeq.h"
#include "vaeq_common.h"
#include "vaeq_launch.h"

namespace vaeq {

// soft_dec (shared_funcs.py:529-542): one thread per (run, pol, I/Q, symbol); q rows written coalesced along N.
template <int NLEV>
__global__ __launch_bounds__(256) void soft_demap_kernel(int64_t N, const float *__restrict__ y, const float *__restrict__ amp_g,
                                                         const float *__restrict__ var, const float *__restrict__ nu_sc,
                                                         float *__restrict__ q)
{
    const int run = blockIdx.z, oc = blockIdx.y, o = oc >> 1, c = oc & 1;
    float amp[NLEV], amp2[NLEV];
#pragma unroll
    for (int i = 0; i < NLEV; i++) { amp[i] = amp_g[i]; amp2[i] = amp[i] * amp[i]; }
    const float i2v = 0.5f / var[run * 2 + o], nusc = nu_sc[run];
    const float *yr = y + ((size_t)run * 4 + oc) * N;
    float *qr = q + ((size_t)run * 4 * NLEV + (size_t)o * 2 * NLEV + c * NLEV) * N;
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += (int64_t)gridDim.x * blockDim.x) {
        float qq[NLEV];
        soft_demap<NLEV>(yr[n], amp, amp2, i2v, nusc, qq);
#pragma unroll
        for (int i = 0; i < NLEV; i++) qr[(size_t)i * N + n] = qq[i];
    }
}

// twoXtwoFIR.forward without training (shared_funcs.py:500-527): one thread per (run, o, symbol).
// Taps of the run in LDS; samples straight from global (L1/L2 absorb the 2*M-fold reuse).
template <int NLEV>
__global__ __launch_bounds__(256) void dp_forward_kernel(int64_t N, int sps, int M, const float *__restrict__ x, const float *__restrict__ W,
                                                         const float *__restrict__ amp_g, const float *__restrict__ var,
                                                         const float *__restrict__ nu_sc, float *__restrict__ q, float *__restrict__ yout)
{
    __shared__ float Ws[8 * 64];
    const int run = blockIdx.z, o = blockIdx.y;
    for (int i = threadIdx.x; i < 8 * M; i += blockDim.x) Ws[i] = W[(size_t)run * 8 * M + i];
    __syncthreads();
    float amp[NLEV], amp2[NLEV];
#pragma unroll
    for (int i = 0; i < NLEV; i++) { amp[i] = amp_g[i]; amp2[i] = amp[i] * amp[i]; }
    const float i2v = 0.5f / var[run * 2 + o], nusc = nu_sc[run];
    const int64_t L = N * sps;
    const int mh = M / 2;
    const float *xb = x + (size_t)run * 4 * L;
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += (int64_t)gridDim.x * blockDim.x) {
        float yI = 0.f, yQ = 0.f;
        for (int p = 0; p < 2; p++) {
            const float *xr = xb + (size_t)(p * 2 + 0) * L, *xi = xb + (size_t)(p * 2 + 1) * L;
            const float *wr = Ws + (o * 4 + p) * M, *wi = Ws + (o * 4 + 2 + p) * M;
            for (int k = 0; k < M; k++) {
                const int64_t s = n * sps + k - mh;
                if (s < 0 || s >= L) continue;
                const float a_ = xr[s], b_ = xi[s];
                yI = fmaf(wr[k], a_, yI);
                yI = fmaf(-wi[k], b_, yI);
                yQ = fmaf(wr[k], b_, yQ);
                yQ = fmaf(wi[k], a_, yQ);
            }
        }
        yout[((size_t)run * 4 + o * 2 + 0) * N + n] = yI;
        yout[((size_t)run * 4 + o * 2 + 1) * N + n] = yQ;
        if (q) {
#pragma unroll
            for (int c = 0; c < 2; c++) {
                float qq[NLEV];
                soft_demap<NLEV>(c ? yQ : yI, amp, amp2, i2v, nusc, qq);
#pragma unroll
                for (int i = 0; i < NLEV; i++) q[((size_t)run * 4 * NLEV + (size_t)o * 2 * NLEV + c * NLEV + i) * N + n] = qq[i];
            }
        }
    }
}

// ---- phases shared by dp_loss_kernel and dp_loss_bwd_kernel (loss_function_shaping, shared_funcs.py:92-137)

// moments of q (:107-113): mu[4][B], vr[4][B]; KL: returns this thread's share of sum q log(q / P + 1e-12) over the inner symbols (:131-132)
template <int NLEV, bool KL>
__device__ __forceinline__ float dp_moments(int B, int mh, const float *__restrict__ qr, const float (&amp)[NLEV], const float (&invP)[NLEV],
                                            float *mu, float *vr)
{
    float kl = 0.f;
    for (int it = threadIdx.x; it < 4 * B; it += 256) {
        const int vc = it / B, n = it - vc * B;
        float qq[NLEV], m1 = 0.f;
#pragma unroll
        for (int i = 0; i < NLEV; i++) { qq[i] = qr[((size_t)vc * NLEV + i) * B + n]; m1 = fmaf(amp[i], qq[i], m1); }
        float m2 = 0.f;
        const bool inr = n >= mh && n < B - mh;
#pragma unroll
        for (int i = 0; i < NLEV; i++) {
            const float d = amp[i] - m1;
            m2 = fmaf(qq[i] * d, d, m2);
            if (KL && inr) kl = fmaf(qq[i], __logf(qq[i] * invP[i] + 1e-12f), kl);
        }
        mu[it] = m1;
        vr[it] = m2;
    }
    return kl;
}

// e = x - D (:123-127) and this thread's share of sum |e|^2 per polarisation; STORE: e is kept in es[2][2][nm]
template <bool STORE>
__device__ __forceinline__ void dp_residual(int B, int sps, int M, const float *__restrict__ xr, const float *hs, const float *mu, float *es,
                                            float &se0, float &se1)
{
    const int L = B * sps, mh = M / 2, Mh = 2 * mh, nm = L - Mh;
    for (int it = threadIdx.x; it < 2 * nm; it += 256) {
        const int chi = it / nm, t = it - chi * nm;
        float dr = 0.f, di = 0.f;
        for (int v = 0; v < 2; v++) {
            const float *hr = hs + ((chi * 2 + v) * 2 + 0) * M, *hi = hr + M;
            for (int j = (t + Mh) % sps; j <= Mh; j += sps) {
                const int np = (t + Mh - j) / sps;
                const float a_ = mu[(v * 2 + 0) * B + np], b_ = mu[(v * 2 + 1) * B + np];
                dr = fmaf(hr[j], a_, dr); dr = fmaf(-hi[j], b_, dr);
                di = fmaf(hi[j], a_, di); di = fmaf(hr[j], b_, di);
            }
        }
        const float er = xr[(size_t)(chi * 2 + 0) * L + mh + t] - dr, ei = xr[(size_t)(chi * 2 + 1) * L + mh + t] - di;
        if (STORE) {
            es[(chi * 2 + 0) * nm + t] = er;
            es[(chi * 2 + 1) * nm + t] = ei;
        }
        if (chi) se1 += er * er + ei * ei; else se0 += er * er + ei * ei;
    }
}

// VS[v][j] (:128): the variances of the symbols that tap j of polarisation v touches
__device__ __forceinline__ void dp_var_sums(int B, int sps, int M, const float *vr, float *VS)
{
    const int Mh = 2 * (M / 2), nm = B * sps - Mh;
    for (int it = threadIdx.x; it < 2 * M; it += 256) {
        const int v = it / M, j = it - v * M;
        const int lo = (Mh - j + sps - 1) / sps, hi_ = (nm - 1 + Mh - j) / sps;
        float acc = 0.f;
        for (int np = lo; np <= hi_; np++) acc += vr[(v * 2 + 0) * B + np] + vr[(v * 2 + 1) * B + np];
        VS[it] = acc;
    }
}

// C_chi = sum |e_chi|^2 + sum_j |h_j|^2 VS[j], from the reduced sums C0 = red[0], C1 = red[1]
__device__ __forceinline__ void dp_C(int M, const float *hs, const float *VS, float &C0, float &C1)
{
    for (int i = 0; i < 2 * M; i++) {
        const int v = i / M, j = i - v * M;
        const float a0 = hs[((0 * 2 + v) * 2 + 0) * M + j], b0 = hs[((0 * 2 + v) * 2 + 1) * M + j];
        const float a1 = hs[((1 * 2 + v) * 2 + 0) * M + j], b1 = hs[((1 * 2 + v) * 2 + 1) * M + j];
        C0 = fmaf(a0 * a0 + b0 * b0, VS[i], C0);
        C1 = fmaf(a1 * a1 + b1 * b1, VS[i], C1);
    }
}

// loss_function_shaping alone (shared_funcs.py:92-137): moments of q in LDS, values only.
template <int NLEV>
__global__ __launch_bounds__(256) void dp_loss_kernel(int B, int sps, int M, const float *__restrict__ q, const float *__restrict__ x,
                                                      const float *__restrict__ h, const float *__restrict__ amp_g,
                                                      const float *__restrict__ P, float *__restrict__ loss, float *__restrict__ var_est)
{
    extern __shared__ float4 smem4[];
    float *sm = reinterpret_cast<float *>(smem4);
    const int run = blockIdx.x, tid = threadIdx.x;
    const int L = B * sps, mh = M / 2, nm = L - 2 * mh;
    float *mu = sm, *vr = sm + 4 * B, *hs = vr + 4 * B, *VS = hs + 8 * M, *red = VS + 2 * M;
    float amp[NLEV], invP[NLEV];
#pragma unroll
    for (int i = 0; i < NLEV; i++) { amp[i] = amp_g[i]; invP[i] = 1.0f / P[(size_t)run * NLEV + i]; }
    const float *qr = q + (size_t)run * 4 * NLEV * B, *xr = x + (size_t)run * 4 * L;
    for (int i = tid; i < 8 * M; i += 256) hs[i] = h[(size_t)run * 8 * M + i];
    const float kl = dp_moments<NLEV, true>(B, mh, qr, amp, invP, mu, vr);
    __syncthreads();
    float se0 = 0.f, se1 = 0.f;
    dp_residual<false>(B, sps, M, xr, hs, mu, nullptr, se0, se1);
    dp_var_sums(B, sps, M, vr, VS);
    block_reduce3<256>(se0, se1, kl, red);
    if (tid == 0) {
        float C0 = red[0], C1 = red[1];
        dp_C(M, hs, VS, C0, C1);
        loss[run] = (float)nm * (logf(C0) + logf(C1)) + red[2];
        var_est[run * 2 + 0] = C0 / (float)nm;
        var_est[run * 2 + 1] = C1 / (float)nm;
    }
}

// d loss / d q and d loss / d h_est of loss_function_shaping (shared_funcs.py:92-137), times the upstream gradient g_up[run].
template <int NLEV>
__global__ __launch_bounds__(256) void dp_loss_bwd_kernel(int B, int sps, int M, const float *__restrict__ q, const float *__restrict__ x,
                                                          const float *__restrict__ h, const float *__restrict__ amp_g,
                                                          const float *__restrict__ P, const float *__restrict__ g_up,
                                                          float *__restrict__ gq, float *__restrict__ gh)
{
    extern __shared__ float4 smem4[];
    float *sm = reinterpret_cast<float *>(smem4);
    const int run = blockIdx.x, tid = threadIdx.x;
    const int L = B * sps, mh = M / 2, Mh = 2 * mh, nm = L - Mh;
    float *mu = sm, *vr = mu + 4 * B, *es = vr + 4 * B, *hs = es + 4 * nm, *VS = hs + 8 * M, *red = VS + 2 * M;
    float amp[NLEV], invP[NLEV];
#pragma unroll
    for (int i = 0; i < NLEV; i++) { amp[i] = amp_g[i]; invP[i] = 1.0f / P[(size_t)run * NLEV + i]; }
    const float *qr = q + (size_t)run * 4 * NLEV * B, *xr = x + (size_t)run * 4 * L;
    float *gqr = gq + (size_t)run * 4 * NLEV * B;
    const float up = g_up[run];
    for (int i = tid; i < 8 * M; i += 256) hs[i] = h[(size_t)run * 8 * M + i];
    dp_moments<NLEV, false>(B, mh, qr, amp, invP, mu, vr);
    __syncthreads();
    float se0 = 0.f, se1 = 0.f;
    dp_residual<true>(B, sps, M, xr, hs, mu, es, se0, se1);
    dp_var_sums(B, sps, M, vr, VS);
    block_reduce3<256>(se0, se1, 0.f, red);
    float C0 = red[0], C1 = red[1];
    dp_C(M, hs, VS, C0, C1);
    const float gC0 = up * (float)nm / C0, gC1 = up * (float)nm / C1;
    for (int it = tid; it < 4 * M; it += 256) {                 // d/dh
        const int cv = it / M, j = it - cv * M, chi = cv >> 1, v = cv & 1;
        const int lo = (Mh - j + sps - 1) / sps, hi_ = (nm - 1 + Mh - j) / sps;
        const float *er = es + (chi * 2 + 0) * nm, *ei = er + nm;
        float ar = 0.f, ai = 0.f;
        for (int np = lo; np <= hi_; np++) {
            const int t = np * sps - Mh + j;
            const float c_ = mu[(v * 2 + 0) * B + np], d_ = mu[(v * 2 + 1) * B + np];
            ar = fmaf(er[t], c_, ar); ar = fmaf(ei[t], d_, ar);
            ai = fmaf(ei[t], c_, ai); ai = fmaf(-er[t], d_, ai);
        }
        const float gC = chi ? gC1 : gC0, vs = VS[v * M + j];
        const int ir = (cv * 2 + 0) * M + j, ii = ir + M;
        gh[(size_t)run * 8 * M + ir] = gC * (-2.0f * ar + 2.0f * hs[ir] * vs);
        gh[(size_t)run * 8 * M + ii] = gC * (-2.0f * ai + 2.0f * hs[ii] * vs);
    }
    for (int it = tid; it < 2 * B; it += 256) {                 // d/dq through mu, rho and the KL term
        const int v = it / B, n = it - v * B, sx = n * sps;
        const int jlo = max(0, Mh - sx), jhi = min(Mh, nm - 1 + Mh - sx);
        float ur = 0.f, ui = 0.f, gv = 0.f;
        for (int chi = 0; chi < 2; chi++) {
            const float *er = es + (chi * 2 + 0) * nm + (sx - Mh), *ei = er + nm;
            const float *hr = hs + ((chi * 2 + v) * 2 + 0) * M, *hi = hr + M;
            float pr = 0.f, pi = 0.f, ph = 0.f;
            for (int j = jlo; j <= jhi; j++) {
                pr = fmaf(er[j], hr[j], pr); pr = fmaf(ei[j], hi[j], pr);
                pi = fmaf(ei[j], hr[j], pi); pi = fmaf(-er[j], hi[j], pi);
                ph = fmaf(hr[j], hr[j], ph); ph = fmaf(hi[j], hi[j], ph);
            }
            const float gC = chi ? gC1 : gC0;
            ur = fmaf(-2.0f * gC, pr, ur);
            ui = fmaf(-2.0f * gC, pi, ui);
            gv = fmaf(gC, ph, gv);
        }
        const bool inr = n >= mh && n < B - mh;
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const int ix = (v * 2 + c) * B + n;
            const float A = (c ? ui : ur) - 2.0f * mu[ix] * gv;  // dL/dmu (Var = rho - mu^2, :113)
#pragma unroll
            for (int i = 0; i < NLEV; i++) {
                const size_t qi = ((size_t)(v * 2 + c) * NLEV + i) * B + n;
                float g = amp[i] * A + amp[i] * amp[i] * gv;
                if (inr) {
                    const float r = qr[qi] * invP[i], re = r + 1e-12f;
                    g += up * (logf(re) + r / re);               // d/dq [q log(q/P + eps)]  (:131-132)
                }
                gqr[qi] = g;
            }
        }
    }
}

// d loss / d x of loss_function_shaping (shared_funcs.py:92-137), times the upstream gradient g_up[run]: e = x - D enters C_chi as |e|^2, so
// gx[chi][c][mh + t] = g_up (nm / C_chi) 2 e[chi][c][t] on the nm inner samples and exactly 0 on the mh samples at either end.
template <int NLEV>
__global__ __launch_bounds__(256) void dp_loss_bwd_x_kernel(int B, int sps, int M, const float *__restrict__ q, const float *__restrict__ x,
                                                            const float *__restrict__ h, const float *__restrict__ amp_g,
                                                            const float *__restrict__ g_up, float *__restrict__ gx)
{
    extern __shared__ float4 smem4[];
    float *sm = reinterpret_cast<float *>(smem4);
    const int run = blockIdx.x, tid = threadIdx.x;
    const int L = B * sps, mh = M / 2, Mh = 2 * mh, nm = L - Mh;
    float *mu = sm, *vr = mu + 4 * B, *es = vr + 4 * B, *hs = es + 4 * nm, *VS = hs + 8 * M, *red = VS + 2 * M;
    float amp[NLEV], invP[NLEV];
#pragma unroll
    for (int i = 0; i < NLEV; i++) { amp[i] = amp_g[i]; invP[i] = 1.0f; }       // (the KL term does not depend on x)
    const float *qr = q + (size_t)run * 4 * NLEV * B, *xr = x + (size_t)run * 4 * L;
    for (int i = tid; i < 8 * M; i += 256) hs[i] = h[(size_t)run * 8 * M + i];
    dp_moments<NLEV, false>(B, mh, qr, amp, invP, mu, vr);
    __syncthreads();
    float se0 = 0.f, se1 = 0.f;
    dp_residual<true>(B, sps, M, xr, hs, mu, es, se0, se1);
    dp_var_sums(B, sps, M, vr, VS);
    block_reduce3<256>(se0, se1, 0.f, red);
    float C0 = red[0], C1 = red[1];
    dp_C(M, hs, VS, C0, C1);
    const float up = g_up[run], gC0 = up * (float)nm / C0, gC1 = up * (float)nm / C1;
    float *gxr = gx + (size_t)run * 4 * L;
    for (int it = tid; it < 4 * L; it += 256) {
        const int xc = it / L, s = it - xc * L, t = s - mh;
        gxr[it] = (t >= 0 && t < nm) ? (xc >> 1 ? gC1 : gC0) * (2.0f * es[xc * nm + t]) : 0.f;
    }
}

// d loss / d W of twoXtwoFIR.forward (shared_funcs.py:500-527) given d loss / d q and (optionally) d loss / d out.
template <int NLEV>
__global__ __launch_bounds__(256) void dp_forward_bwd_kernel(int N, int sps, int M, const float *__restrict__ x, const float *__restrict__ q,
                                                             const float *__restrict__ y, const float *__restrict__ gq, const float *__restrict__ gy_in,
                                                             const float *__restrict__ amp_g, const float *__restrict__ var,
                                                             float *__restrict__ gW)
{
    extern __shared__ float4 smem4[];
    float *gy = reinterpret_cast<float *>(smem4);               // [2][2][N]
    const int run = blockIdx.x, tid = threadIdx.x, L = N * sps, mh = M / 2;
    float amp[NLEV];
#pragma unroll
    for (int i = 0; i < NLEV; i++) amp[i] = amp_g[i];
    const float *qr = q + (size_t)run * 4 * NLEV * N, *gqr = gq + (size_t)run * 4 * NLEV * N, *yr = y + (size_t)run * 4 * N;
    const float *xr = x + (size_t)run * 4 * L;
    for (int it = tid; it < 4 * N; it += 256) {                 // softmin backward (:521-523): dz_i = q_i (gq_i - sum q gq), dz_i/dy = -(y-a_i)/var
        const int oc = it / N, n = it - oc * N, o = oc >> 1;
        float qq[NLEV], dot = 0.f;
#pragma unroll
        for (int i = 0; i < NLEV; i++) { qq[i] = qr[((size_t)oc * NLEV + i) * N + n]; dot = fmaf(qq[i], gqr[((size_t)oc * NLEV + i) * N + n], dot); }
        const float yy = yr[(size_t)oc * N + n], iv = 1.0f / var[run * 2 + o];
        float g = gy_in ? gy_in[((size_t)run * 4 + oc) * N + n] : 0.f;
#pragma unroll
        for (int i = 0; i < NLEV; i++) g = fmaf(qq[i] * (gqr[((size_t)oc * NLEV + i) * N + n] - dot), -(yy - amp[i]) * iv, g);
        gy[it] = g;
    }
    __syncthreads();
    for (int it = tid; it < 4 * M; it += 256) {                 // conv weight gradient through the channel packing (:505,507)
        const int op = it / M, k = it - op * M, o = op >> 1, p = op & 1;
        float ar = 0.f, ai = 0.f;
        for (int n = 0; n < N; n++) {
            const int s = n * sps + k - mh;
            if (s < 0 || s >= L) continue;
            const float a_ = gy[(o * 2 + 0) * N + n], b_ = gy[(o * 2 + 1) * N + n], c_ = xr[(size_t)(p * 2 + 0) * L + s], d_ = xr[(size_t)(p * 2 + 1) * L + s];
            ar = fmaf(a_, c_, ar); ar = fmaf(b_, d_, ar);
            ai = fmaf(b_, c_, ai); ai = fmaf(-a_, d_, ai);
        }
        gW[(size_t)run * 8 * M + (o * 4 + p) * M + k] = ar;
        gW[(size_t)run * 8 * M + (o * 4 + 2 + p) * M + k] = ai;
    }
}

// dL/dout of twoXtwoFIR.forward into gy[2][2][N] (LDS): softmin backward (:521-523) plus the upstream gradient on `out` (gy_in, nullable) -- the
// first phase of dp_forward_bwd_kernel above, statement for statement (that kernel keeps it inline: moving it here changes its register
// allocation, and its instruction stream is held fixed)
template <int NLEV>
__device__ __forceinline__ void dp_dy(int run, int N, const float *qr, const float *gqr, const float *yr,
                                      const float *gy_in, const float (&amp)[NLEV], const float *var, float *gy)
{
    for (int it = threadIdx.x; it < 4 * N; it += 256) {
        const int oc = it / N, n = it - oc * N, o = oc >> 1;
        float qq[NLEV], dot = 0.f;
#pragma unroll
        for (int i = 0; i < NLEV; i++) { qq[i] = qr[((size_t)oc * NLEV + i) * N + n]; dot = fmaf(qq[i], gqr[((size_t)oc * NLEV + i) * N + n], dot); }
        const float yy = yr[(size_t)oc * N + n], iv = 1.0f / var[run * 2 + o];
        float g = gy_in ? gy_in[((size_t)run * 4 + oc) * N + n] : 0.f;
#pragma unroll
        for (int i = 0; i < NLEV; i++) g = fmaf(qq[i] * (gqr[((size_t)oc * NLEV + i) * N + n] - dot), -(yy - amp[i]) * iv, g);
        gy[it] = g;
    }
}

// d loss / d x of twoXtwoFIR.forward (shared_funcs.py:500-516), the transposed strided correlation in gather form:
//   gx[p][s] = sum_o sum_{k : (s + mh - k) % sps == 0, n = (s + mh - k) / sps in [0, N)} conj(w[o][p][k]) dy[o][n]
// one thread per (polarisation, sample); o ascending, then k ascending: a fixed order, no atomics.  gy[2][2][N] and the taps in LDS.
template <int NLEV>
__global__ __launch_bounds__(256) void dp_forward_bwd_x_kernel(int N, int sps, int M, const float *__restrict__ W, const float *__restrict__ q,
                                                               const float *__restrict__ y, const float *__restrict__ gq, const float *__restrict__ gy_in,
                                                               const float *__restrict__ amp_g, const float *__restrict__ var,
                                                               float *__restrict__ gx)
{
    extern __shared__ float4 smem4[];
    float *gy = reinterpret_cast<float *>(smem4), *Ws = gy + 4 * N;     // [2][2][N] | [2][4][M]
    const int run = blockIdx.x, tid = threadIdx.x, L = N * sps, mh = M / 2;
    float amp[NLEV];
#pragma unroll
    for (int i = 0; i < NLEV; i++) amp[i] = amp_g[i];
    const float *qr = q + (size_t)run * 4 * NLEV * N, *gqr = gq + (size_t)run * 4 * NLEV * N, *yr = y + (size_t)run * 4 * N;
    for (int i = tid; i < 8 * M; i += 256) Ws[i] = W[(size_t)run * 8 * M + i];
    dp_dy<NLEV>(run, N, qr, gqr, yr, gy_in, amp, var, gy);
    __syncthreads();
    float *gxr = gx + (size_t)run * 4 * L;
    for (int it = tid; it < 2 * L; it += 256) {
        const int p = it / L, s = it - p * L, c = s + mh;
        // the taps that reach a symbol: k = c (mod sps), c - (N - 1) sps <= k <= c (both bounds are congruent to c already)
        const int klo = max(c % sps, c - (N - 1) * sps), khi = min(M - 1, c);
        float ar = 0.f, ai = 0.f;
        for (int o = 0; o < 2; o++) {
            const float *wr = Ws + (o * 4 + p) * M, *wi = Ws + (o * 4 + 2 + p) * M;
            const float *gI = gy + (o * 2 + 0) * N, *gQ = gI + N;
            for (int k = klo, n = (c - klo) / sps; k <= khi; k += sps, n--) {
                const float a_ = gI[n], b_ = gQ[n], c_ = wr[k], d_ = wi[k];
                ar = fmaf(c_, a_, ar); ar = fmaf(d_, b_, ar);
                ai = fmaf(c_, b_, ai); ai = fmaf(-d_, a_, ai);
            }
        }
        gxr[(size_t)(p * 2 + 0) * L + s] = ar;
        gxr[(size_t)(p * 2 + 1) * L + s] = ai;
    }
}

// ---- phases shared by the AWGN kernels.  Taps, VS and the reduction scratch are static __shared__ here; mu / vr / e are the dynamic block.

// y = (W0 - j W1) * x with zero padding (twoFIR.forward, func_VAELE_MQAM_shaping.py:214-227) into y0 / y1 (global or LDS), and this
// thread's share of sum |y| per axis.  I: the index type of the caller (the forward takes 64-bit lengths, its backward keeps y in LDS).
template <class I>
__device__ __forceinline__ void awgn_fir_abs(I N, int sps, int M, const float *__restrict__ x0, const float *__restrict__ x1, const float *Ws,
                                             float *y0, float *y1, float &sa0, float &sa1)
{
    const I L = N * sps;
    const int pad = (M - 1) / 2;
    for (I n = (int)threadIdx.x; n < N; n += 256) {
        float yI = 0.f, yQ = 0.f;
        for (int k = 0; k < M; k++) {
            const I s = n * sps + k - pad;
            if (s < 0 || s >= L) continue;
            const float a_ = x0[s], b_ = x1[s];
            yI = fmaf(Ws[k], a_, yI); yI = fmaf(Ws[M + k], b_, yI);
            yQ = fmaf(Ws[k], b_, yQ); yQ = fmaf(-Ws[M + k], a_, yQ);
        }
        y0[n] = yI; y1[n] = yQ;
        sa0 += fabsf(yI); sa1 += fabsf(yQ);
    }
}

// moments of q: mu[2][B], vr[2][B]; KL: returns this thread's share of sum q log(q invP + 1e-12) over the inner symbols
template <int NLEV, bool KL>
__device__ __forceinline__ float awgn_moments(int B, int mh, const float *__restrict__ qr, const float (&amp)[NLEV], const float (&invP)[NLEV],
                                              float *mu, float *vr)
{
    float klsum = 0.f;
    for (int it = threadIdx.x; it < 2 * B; it += 256) {
        const int c = it / B, n = it - c * B;
        const bool inr = (n >= mh) && (n < B - mh);
        float qq[NLEV], e1 = 0.f, e2 = 0.f;
#pragma unroll
        for (int i = 0; i < NLEV; i++) { qq[i] = qr[(size_t)(c * NLEV + i) * B + n]; e1 = fmaf(amp[i], qq[i], e1); }
#pragma unroll
        for (int i = 0; i < NLEV; i++) {
            const float d = amp[i] - e1;
            e2 = fmaf(qq[i] * d, d, e2);
            if (KL && inr) klsum = fmaf(qq[i], __logf(qq[i] * invP[i] + 1e-12f), klsum);
        }
        mu[it] = e1; vr[it] = e2;
    }
    return klsum;
}

// e = x - D and this thread's share of sum |e|^2; STORE: e is kept in es[2][nm]
template <bool STORE>
__device__ __forceinline__ float awgn_residual(int B, int sps, int M, const float *__restrict__ x0, const float *__restrict__ x1, const float *hs,
                                               const float *mu, float *es)
{
    const int mh = M / 2, Mh = 2 * mh, nm = B * sps - Mh;
    float se = 0.f;
    for (int t = threadIdx.x; t < nm; t += 256) {
        float dr = 0.f, di = 0.f;
        for (int j = (t + Mh) % sps; j <= Mh; j += sps) {
            const int np = (t + Mh - j) / sps;
            const float a_ = mu[np], b_ = mu[B + np], c_ = hs[j], d_ = hs[M + j];
            dr = fmaf(c_, a_, dr); dr = fmaf(-d_, b_, dr);
            di = fmaf(c_, b_, di); di = fmaf(d_, a_, di);
        }
        const float er = x0[mh + t] - dr, ei = x1[mh + t] - di;
        if (STORE) { es[t] = er; es[nm + t] = ei; }
        se += er * er + ei * ei;
    }
    return se;
}

__device__ __forceinline__ void awgn_var_sums(int B, int sps, int M, const float *vr, float *VS)
{
    const int Mh = 2 * (M / 2), nm = B * sps - Mh;
    for (int j = threadIdx.x; j < M; j += 256) {
        const int lo = (Mh - j + sps - 1) / sps, hi_ = (nm - 1 + Mh - j) / sps;
        float acc = 0.f;
        for (int np = lo; np <= hi_; np++) acc += vr[np] + vr[B + np];
        VS[j] = acc;
    }
}

// C = sum |e|^2 + sum_j |h_j|^2 VS[j], from the reduced sum C = red[0]
__device__ __forceinline__ float awgn_C(int M, const float *hs, const float *VS, float C)
{
    for (int j = 0; j < M; j++) C = fmaf(hs[j] * hs[j] + hs[M + j] * hs[M + j], VS[j], C);
    return C;
}

// twoFIR.forward in eval mode on N symbols (validation, :311-313): two passes over y.
template <int NLEV>
__global__ __launch_bounds__(256) void awgn_forward_kernel(int64_t N, int sps, int M, const float *__restrict__ x, const float *__restrict__ W,
                                                           const float *__restrict__ amp_g, const float *__restrict__ amp_mean,
                                                           const float *__restrict__ var, float *__restrict__ q, float *__restrict__ yout)
{
    __shared__ float Ws[2 * 64];
    __shared__ float red[64];
    const int run = blockIdx.x, tid = threadIdx.x;
    for (int i = tid; i < 2 * M; i += 256) Ws[i] = W[(size_t)run * 2 * M + i];
    __syncthreads();
    const int64_t L = N * sps;
    const float *x0 = x + (size_t)run * 2 * L, *x1 = x0 + L;
    float *y0 = yout + (size_t)run * 2 * N, *y1 = y0 + N;
    float sa0 = 0.f, sa1 = 0.f;
    awgn_fir_abs<int64_t>(N, sps, M, x0, x1, Ws, y0, y1, sa0, sa1);
    block_reduce3<256>(sa0, sa1, 0.f, red);
    if (!q) return;
    float amp[NLEV], amp2[NLEV];
#pragma unroll
    for (int i = 0; i < NLEV; i++) { amp[i] = amp_g[i]; amp2[i] = 0.f; }
    const float A = amp_mean[run], ivar = 1.0f / var[run];
    const float s0 = A / (red[0] / (float)N), s1 = A / (red[1] / (float)N);
    for (int64_t it = tid; it < 2 * N; it += 256) {      // any thread's y: the barriers of block_reduce3 ordered the writes above before these reads
        const int c = it >= N;
        const int64_t n = it - (c ? N : 0);
        float qq[NLEV];
        // soft_demap computes -(d^2 * i2v + nusc*a^2): i2v = 1/var, nusc = 0 gives (yhat-a)^2/var (:229)
        soft_demap<NLEV>((c ? y1[n] : y0[n]) * (c ? s1 : s0), amp, amp2, ivar, 0.f, qq);
#pragma unroll
        for (int i = 0; i < NLEV; i++) q[((size_t)run * 2 * NLEV + c * NLEV + i) * N + n] = qq[i];
    }
}

// Stand-alone ELBO of the single-polarisation variants for a given q (values only):
//   func_VAELE_MQAM_shaping.loss_function (:63-95):  nm log C + sum q log(q / P + 1e-12)      (P != nullptr)
//   func_VAENN_MQAM.loss_function (:63-95):          nm log C + sum q log(q + 1e-12)          (P == nullptr)
// q[R][2n][B], x[R][2][B*sps], h[R][2][M] -> loss[R].
template <int NLEV>
__global__ __launch_bounds__(256) void awgn_loss_kernel(int B, int sps, int M, const float *__restrict__ q, const float *__restrict__ x,
                                                        const float *__restrict__ h, const float *__restrict__ amp_g, const float *__restrict__ P,
                                                        float *__restrict__ loss)
{
    extern __shared__ float4 smem4[];
    float *sm = reinterpret_cast<float *>(smem4);
    __shared__ float red[64];
    __shared__ float hs[2 * 64], VS[64];
    const int run = blockIdx.x, tid = threadIdx.x;
    const int L = B * sps, mh = M / 2, nm = L - 2 * mh;
    float *mu = sm, *vr = sm + 2 * B;
    float amp[NLEV], invP[NLEV];
#pragma unroll
    for (int i = 0; i < NLEV; i++) { amp[i] = amp_g[i]; invP[i] = P ? 1.0f / P[(size_t)run * NLEV + i] : 1.0f; }
    for (int i = tid; i < 2 * M; i += 256) hs[i] = h[(size_t)run * 2 * M + i];
    const float *qr = q + (size_t)run * 2 * NLEV * B, *x0 = x + (size_t)run * 2 * L, *x1 = x0 + L;
    const float klsum = awgn_moments<NLEV, true>(B, mh, qr, amp, invP, mu, vr);
    __syncthreads();
    const float se = awgn_residual<false>(B, sps, M, x0, x1, hs, mu, nullptr);
    awgn_var_sums(B, sps, M, vr, VS);
    block_reduce3<256>(se, klsum, 0.f, red);
    if (tid == 0) loss[run] = (float)nm * logf(awgn_C(M, hs, VS, red[0])) + red[1];
}

// Backward of the stand-alone AWGN ELBO (for the autograd wrappers; the fused training kernels do not use it):
// g_up[R] = upstream d/dloss -> gq[R][2n][B] = dL/dq, gh[R][2][M] = dL/dh.  P == nullptr: the VAE-NN form (entropy).
template <int NLEV>
__global__ __launch_bounds__(256) void awgn_loss_bwd_kernel(int B, int sps, int M, const float *__restrict__ q, const float *__restrict__ x,
                                                            const float *__restrict__ h, const float *__restrict__ amp_g,
                                                            const float *__restrict__ P, const float *__restrict__ g_up, float *__restrict__ gq,
                                                            float *__restrict__ gh)
{
    extern __shared__ float4 smem4[];
    float *sm = reinterpret_cast<float *>(smem4);
    __shared__ float red[64];
    __shared__ float hs[2 * 64], VS[64];
    const int run = blockIdx.x, tid = threadIdx.x;
    const int L = B * sps, mh = M / 2, Mh = 2 * mh, nm = L - Mh;
    float *mu = sm, *vr = sm + 2 * B, *es = sm + 4 * B;       // es[2][nm]
    float amp[NLEV], invP[NLEV];
#pragma unroll
    for (int i = 0; i < NLEV; i++) { amp[i] = amp_g[i]; invP[i] = P ? 1.0f / P[(size_t)run * NLEV + i] : 1.0f; }
    for (int i = tid; i < 2 * M; i += 256) hs[i] = h[(size_t)run * 2 * M + i];
    const float *qr = q + (size_t)run * 2 * NLEV * B, *x0 = x + (size_t)run * 2 * L, *x1 = x0 + L;
    awgn_moments<NLEV, false>(B, mh, qr, amp, invP, mu, vr);
    __syncthreads();
    const float se = awgn_residual<true>(B, sps, M, x0, x1, hs, mu, es);
    awgn_var_sums(B, sps, M, vr, VS);
    block_reduce3<256>(se, 0.f, 0.f, red);
    const float C = awgn_C(M, hs, VS, red[0]);
    const float up = g_up[run], gC = up * (float)nm / C;
    for (int j = tid; j < M; j += 256) {
        const int lo = (Mh - j + sps - 1) / sps, hi_ = (nm - 1 + Mh - j) / sps;
        float ar = 0.f, ai = 0.f;
        for (int np = lo; np <= hi_; np++) {
            const int t = np * sps - Mh + j;
            const float a_ = es[t], b_ = es[nm + t], c_ = mu[np], d_ = mu[B + np];
            ar = fmaf(a_, c_, ar); ar = fmaf(b_, d_, ar);
            ai = fmaf(b_, c_, ai); ai = fmaf(-a_, d_, ai);
        }
        gh[(size_t)run * 2 * M + j] = gC * (-2.0f * ar + 2.0f * hs[j] * VS[j]);
        gh[(size_t)run * 2 * M + M + j] = gC * (-2.0f * ai + 2.0f * hs[M + j] * VS[j]);
    }
    float *gqr = gq + (size_t)run * 2 * NLEV * B;
    for (int n = tid; n < B; n += 256) {
        const int sx = n * sps;
        const int jlo = max(0, Mh - sx), jhi = min(Mh, nm - 1 + Mh - sx);
        const float *er = es + (sx - Mh), *ei = er + nm;
        float pr = 0.f, pi = 0.f, ph = 0.f;
        for (int j = jlo; j <= jhi; j++) {
            const float a_ = er[j], b_ = ei[j], c_ = hs[j], d_ = hs[M + j];
            pr = fmaf(a_, c_, pr); pr = fmaf(b_, d_, pr);
            pi = fmaf(b_, c_, pi); pi = fmaf(-a_, d_, pi);
            ph = fmaf(c_, c_, ph); ph = fmaf(d_, d_, ph);
        }
        const float gv = gC * ph;
        const bool inr = (n >= mh) && (n < B - mh);
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const float gmu = -2.0f * gC * (c ? pi : pr) - 2.0f * mu[c * B + n] * gv;
#pragma unroll
            for (int i = 0; i < NLEV; i++) {
                const float qq = qr[(size_t)(c * NLEV + i) * B + n];
                float g = amp[i] * gmu + amp[i] * amp[i] * gv;
                if (inr) { const float r = qq * invP[i], re = r + 1e-12f; g += up * (__logf(re) + r / re); }
                gqr[(size_t)(c * NLEV + i) * B + n] = g;
            }
        }
    }
}

// d loss / d x of the stand-alone AWGN ELBO: gx[c][mh + t] = g_up (nm / C) 2 e[c][t] on the nm inner samples, exactly 0 on the mh samples
// at either end (the KL / entropy term does not depend on x, so P plays no part).
template <int NLEV>
__global__ __launch_bounds__(256) void awgn_loss_bwd_x_kernel(int B, int sps, int M, const float *__restrict__ q, const float *__restrict__ x,
                                                              const float *__restrict__ h, const float *__restrict__ amp_g,
                                                              const float *__restrict__ g_up, float *__restrict__ gx)
{
    extern __shared__ float4 smem4[];
    float *sm = reinterpret_cast<float *>(smem4);
    __shared__ float red[64];
    __shared__ float hs[2 * 64], VS[64];
    const int run = blockIdx.x, tid = threadIdx.x;
    const int L = B * sps, mh = M / 2, Mh = 2 * mh, nm = L - Mh;
    float *mu = sm, *vr = sm + 2 * B, *es = sm + 4 * B;       // es[2][nm]
    float amp[NLEV], invP[NLEV];
#pragma unroll
    for (int i = 0; i < NLEV; i++) { amp[i] = amp_g[i]; invP[i] = 1.0f; }
    for (int i = tid; i < 2 * M; i += 256) hs[i] = h[(size_t)run * 2 * M + i];
    const float *qr = q + (size_t)run * 2 * NLEV * B, *x0 = x + (size_t)run * 2 * L, *x1 = x0 + L;
    awgn_moments<NLEV, false>(B, mh, qr, amp, invP, mu, vr);
    __syncthreads();
    const float se = awgn_residual<true>(B, sps, M, x0, x1, hs, mu, es);
    awgn_var_sums(B, sps, M, vr, VS);
    block_reduce3<256>(se, 0.f, 0.f, red);
    const float C = awgn_C(M, hs, VS, red[0]);
    const float gC = g_up[run] * (float)nm / C;
    float *gxr = gx + (size_t)run * 2 * L;
    for (int it = tid; it < 2 * L; it += 256) {
        const int c = it / L, s = it - c * L, t = s - mh;
        gxr[it] = (t >= 0 && t < nm) ? gC * (2.0f * es[c * nm + t]) : 0.f;
    }
}

// Backward of twoFIR.forward (func_VAELE_MQAM_shaping.py:214-231): upstream gq[R][2n][N] (and optionally gy on the un-normalised
// output) -> gW[R][2][M].  Recomputes the forward (y, mean |y|, yhat, q), then softmax backward with dz_i/dyhat = -2 (yhat - a_i) / var,
// the normalisation's Jacobian and the tap correlation.  One workgroup per run, y and dL/dy in LDS.
template <int NLEV>
__global__ __launch_bounds__(256) void awgn_forward_bwd_kernel(int N, int sps, int M, const float *__restrict__ x, const float *__restrict__ W,
                                                               const float *__restrict__ amp_g, const float *__restrict__ amp_mean,
                                                               const float *__restrict__ var, const float *__restrict__ gq,
                                                               const float *__restrict__ gy_up, float *__restrict__ gW)
{
    extern __shared__ float4 smem4[];
    float *ys = reinterpret_cast<float *>(smem4), *gys = ys + 2 * N;
    __shared__ float Ws[2 * 64];
    __shared__ float red[64];
    const int run = blockIdx.x, tid = threadIdx.x;
    for (int i = tid; i < 2 * M; i += 256) Ws[i] = W[(size_t)run * 2 * M + i];
    __syncthreads();
    const int L = N * sps, pad = (M - 1) / 2;
    const float *x0 = x + (size_t)run * 2 * L, *x1 = x0 + L;
    float sa0 = 0.f, sa1 = 0.f;
    awgn_fir_abs<int>(N, sps, M, x0, x1, Ws, ys, ys + N, sa0, sa1);
    block_reduce3<256>(sa0, sa1, 0.f, red);
    float amp[NLEV];
#pragma unroll
    for (int i = 0; i < NLEV; i++) amp[i] = amp_g[i];
    const float A = amp_mean[run], ivar = 1.0f / var[run];
    const float m0 = red[0] / (float)N, m1 = red[1] / (float)N;
    __syncthreads();
    const float *gqr = gq + (size_t)run * 2 * NLEV * N;
    float dt0 = 0.f, dt1 = 0.f;
    for (int it = tid; it < 2 * N; it += 256) {
        const int c = it / N, n = it - c * N;
        const float yh = ys[it] / (c ? m1 : m0) * A;
        float z[NLEV], zmax = -3.0e38f, ssum = 0.f, dot = 0.f, g = 0.f;
#pragma unroll
        for (int i = 0; i < NLEV; i++) { const float d = yh - amp[i]; z[i] = -(d * d * ivar); zmax = fmaxf(zmax, z[i]); }
#pragma unroll
        for (int i = 0; i < NLEV; i++) { z[i] = __expf(z[i] - zmax); ssum += z[i]; }
#pragma unroll
        for (int i = 0; i < NLEV; i++) { z[i] /= ssum; dot = fmaf(z[i], gqr[(size_t)(c * NLEV + i) * N + n], dot); }
#pragma unroll
        for (int i = 0; i < NLEV; i++) g = fmaf(z[i] * (gqr[(size_t)(c * NLEV + i) * N + n] - dot), -2.0f * (yh - amp[i]) * ivar, g);
        gys[it] = g;                                           // dL/dyhat
        if (c) dt1 = fmaf(g, ys[it], dt1); else dt0 = fmaf(g, ys[it], dt0);
    }
    block_reduce3<256>(dt0, dt1, 0.f, red);
    {
        const float s0_ = A / m0, s1_ = A / m1, k0_ = red[0] * A / (m0 * m0) / (float)N, k1_ = red[1] * A / (m1 * m1) / (float)N;
        __syncthreads();
        for (int n = tid; n < N; n += 256) {                   // normalisation backward (:228) + the upstream gradient on `out`
            const float yI = ys[n], yQ = ys[N + n];
            const float sgI = (float)(yI > 0.f) - (float)(yI < 0.f), sgQ = (float)(yQ > 0.f) - (float)(yQ < 0.f);
            gys[n] = gys[n] * s0_ - k0_ * sgI + (gy_up ? gy_up[(size_t)run * 2 * N + n] : 0.f);
            gys[N + n] = gys[N + n] * s1_ - k1_ * sgQ + (gy_up ? gy_up[(size_t)run * 2 * N + N + n] : 0.f);
        }
    }
    __syncthreads();
    for (int k = tid; k < M; k += 256) {                       // dL/dW0[k] = sum gI x0 + gQ x1, dL/dW1[k] = sum gI x1 - gQ x0
        float g0 = 0.f, g1 = 0.f;
        for (int n = 0; n < N; n++) {
            const int sx = n * sps + k - pad;
            if (sx < 0 || sx >= L) continue;
            const float a_ = gys[n], b_ = gys[N + n], c_ = x0[sx], d_ = x1[sx];
            g0 = fmaf(a_, c_, g0); g0 = fmaf(b_, d_, g0);
            g1 = fmaf(a_, d_, g1); g1 = fmaf(-b_, c_, g1);
        }
        gW[(size_t)run * 2 * M + k] = g0;
        gW[(size_t)run * 2 * M + M + k] = g1;
    }
}

// dL/dy of twoFIR.forward (func_VAELE_MQAM_shaping.py:214-231) -- everything awgn_forward_bwd_kernel above does before its tap correlation, statement
// for statement (that kernel keeps it inline: its instruction stream is held fixed) -- into gys[2][N], with the forward's un-normalised y recomputed into ys[2][N] (both LDS): y, mean |y|, yhat, q again, then softmax backward
// with dz_i/dyhat = -2 (yhat - a_i) / var, the normalisation's Jacobian (:228) and the upstream gradient gy_up (nullable) on `out`.
// The caller puts a barrier between this and its reads of gys.
template <int NLEV>
__device__ __forceinline__ void awgn_dy(int run, int N, int sps, int M, const float *x0, const float *x1, const float *Ws,
                                        float *red, const float *amp_g, const float *amp_mean,
                                        const float *var, const float *gq, const float *gy_up, float *ys,
                                        float *gys)
{
    const int tid = threadIdx.x;
    float sa0 = 0.f, sa1 = 0.f;
    awgn_fir_abs<int>(N, sps, M, x0, x1, Ws, ys, ys + N, sa0, sa1);
    block_reduce3<256>(sa0, sa1, 0.f, red);
    float amp[NLEV];
#pragma unroll
    for (int i = 0; i < NLEV; i++) amp[i] = amp_g[i];
    const float A = amp_mean[run], ivar = 1.0f / var[run];
    const float m0 = red[0] / (float)N, m1 = red[1] / (float)N;
    __syncthreads();
    const float *gqr = gq + (size_t)run * 2 * NLEV * N;
    float dt0 = 0.f, dt1 = 0.f;
    for (int it = tid; it < 2 * N; it += 256) {
        const int c = it / N, n = it - c * N;
        const float yh = ys[it] / (c ? m1 : m0) * A;
        float z[NLEV], zmax = -3.0e38f, ssum = 0.f, dot = 0.f, g = 0.f;
#pragma unroll
        for (int i = 0; i < NLEV; i++) { const float d = yh - amp[i]; z[i] = -(d * d * ivar); zmax = fmaxf(zmax, z[i]); }
#pragma unroll
        for (int i = 0; i < NLEV; i++) { z[i] = __expf(z[i] - zmax); ssum += z[i]; }
#pragma unroll
        for (int i = 0; i < NLEV; i++) { z[i] /= ssum; dot = fmaf(z[i], gqr[(size_t)(c * NLEV + i) * N + n], dot); }
#pragma unroll
        for (int i = 0; i < NLEV; i++) g = fmaf(z[i] * (gqr[(size_t)(c * NLEV + i) * N + n] - dot), -2.0f * (yh - amp[i]) * ivar, g);
        gys[it] = g;                                           // dL/dyhat
        if (c) dt1 = fmaf(g, ys[it], dt1); else dt0 = fmaf(g, ys[it], dt0);
    }
    block_reduce3<256>(dt0, dt1, 0.f, red);
    {
        const float s0_ = A / m0, s1_ = A / m1, k0_ = red[0] * A / (m0 * m0) / (float)N, k1_ = red[1] * A / (m1 * m1) / (float)N;
        __syncthreads();
        for (int n = tid; n < N; n += 256) {                   // normalisation backward (:228) + the upstream gradient on `out`
            const float yI = ys[n], yQ = ys[N + n];
            const float sgI = (float)(yI > 0.f) - (float)(yI < 0.f), sgQ = (float)(yQ > 0.f) - (float)(yQ < 0.f);
            gys[n] = gys[n] * s0_ - k0_ * sgI + (gy_up ? gy_up[(size_t)run * 2 * N + n] : 0.f);
            gys[N + n] = gys[N + n] * s1_ - k1_ * sgQ + (gy_up ? gy_up[(size_t)run * 2 * N + N + n] : 0.f);
        }
    }
}

// d loss / d x of twoFIR.forward: dL/dy (awgn_dy, normalisation Jacobian and gy_up included), then the transposed strided correlation in
// gather form with w = W0 - j W1:  gx[s] = sum_{k : (s + pad - k) % sps == 0, n = (s + pad - k) / sps in [0, N)} conj(w[k]) dy[n],
// one thread per sample, k ascending.
template <int NLEV>
__global__ __launch_bounds__(256) void awgn_forward_bwd_x_kernel(int N, int sps, int M, const float *__restrict__ x, const float *__restrict__ W,
                                                                 const float *__restrict__ amp_g, const float *__restrict__ amp_mean,
                                                                 const float *__restrict__ var, const float *__restrict__ gq,
                                                                 const float *__restrict__ gy_up, float *__restrict__ gx)
{
    extern __shared__ float4 smem4[];
    float *ys = reinterpret_cast<float *>(smem4), *gys = ys + 2 * N;
    __shared__ float Ws[2 * 64];
    __shared__ float red[64];
    const int run = blockIdx.x, tid = threadIdx.x;
    for (int i = tid; i < 2 * M; i += 256) Ws[i] = W[(size_t)run * 2 * M + i];
    __syncthreads();
    const int L = N * sps, pad = (M - 1) / 2;
    const float *x0 = x + (size_t)run * 2 * L, *x1 = x0 + L;
    awgn_dy<NLEV>(run, N, sps, M, x0, x1, Ws, red, amp_g, amp_mean, var, gq, gy_up, ys, gys);
    __syncthreads();
    float *gx0 = gx + (size_t)run * 2 * L, *gx1 = gx0 + L;
    for (int s = tid; s < L; s += 256) {
        const int c = s + pad, klo = max(c % sps, c - (N - 1) * sps), khi = min(M - 1, c);
        float g0 = 0.f, g1 = 0.f;
        for (int k = klo, n = (c - klo) / sps; k <= khi; k += sps, n--) {
            const float a_ = gys[n], b_ = gys[N + n], c_ = Ws[k], d_ = Ws[M + k];
            g0 = fmaf(c_, a_, g0); g0 = fmaf(-d_, b_, g0);     // yI = W0 x0 + W1 x1, yQ = W0 x1 - W1 x0
            g1 = fmaf(d_, a_, g1); g1 = fmaf(c_, b_, g1);
        }
        gx0[s] = g0;
        gx1[s] = g1;
    }
}

// one thread per symbol, at most 4096 workgroups along x
static unsigned symbol_blocks(int64_t N) { return (unsigned)((N + 255) / 256 > 4096 ? 4096 : (N + 255) / 256); }

}  // namespace vaeq

using vaeq::dispatch_nlev;
using vaeq::launch;

// In every wrapper: an empty batch owns no memory (its pointers may be NULL), then NULL before SHAPE before LDS before n_lev.

extern "C" int vaeq_soft_demap(int32_t R, int64_t N, int32_t n_lev, const float *y, const float *amp, const float *var,
                               const float *nu_sc, float *q, void *stream)
{
    if (R == 0 || N == 0) return VAEQ_OK;
    if (!y || !amp || !var || !nu_sc || !q) return VAEQ_ERR_NULL;
    if (R < 0 || N < 0) return VAEQ_ERR_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return dispatch_nlev(n_lev, [&](auto nl) {
        return launch(vaeq::soft_demap_kernel<decltype(nl)::value>, dim3(vaeq::symbol_blocks(N), 4, R), dim3(256), 0, st, N, y, amp, var, nu_sc, q);
    });
}

extern "C" int vaeq_dp_forward(int32_t R, int64_t N, int32_t sps, int32_t M, int32_t n_lev, const float *x, const float *W,
                               const float *amp, const float *var, const float *nu_sc, float *q, float *y, void *stream)
{
    if (R == 0 || N == 0) return VAEQ_OK;
    if (!x || !W || !amp || !var || !nu_sc || !y) return VAEQ_ERR_NULL;
    if (R < 0 || N < 0 || !vaeq::fir_shape_ok(sps, M)) return VAEQ_ERR_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return dispatch_nlev(n_lev, [&](auto nl) {
        return launch(vaeq::dp_forward_kernel<decltype(nl)::value>, dim3(vaeq::symbol_blocks(N), 2, R), dim3(256), 0, st, N, sps, M, x, W, amp, var,
                      nu_sc, q, y);
    });
}

extern "C" int vaeq_dp_loss(int32_t R, int32_t B, int32_t sps, int32_t M, int32_t n_lev, const float *q, const float *x,
                            const float *h, const float *amp, const float *P, float *loss, float *var_est, void *stream)
{
    if (R == 0) return VAEQ_OK;
    if (!q || !x || !h || !amp || !P || !loss || !var_est) return VAEQ_ERR_NULL;
    if (R < 0 || !vaeq::loss_shape_ok(B, sps, M)) return VAEQ_ERR_SHAPE;
    const size_t lds = sizeof(float) * (size_t)(8 * B + 8 * M + 2 * M + 64);
    if (lds > vaeq::LDS_MAX) return VAEQ_ERR_LDS;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return dispatch_nlev(n_lev, [&](auto nl) {
        return launch(vaeq::dp_loss_kernel<decltype(nl)::value>, dim3(R), dim3(256), lds, st, B, sps, M, q, x, h, amp, P, loss, var_est);
    });
}

extern "C" int vaeq_dp_loss_bwd(int32_t R, int32_t B, int32_t sps, int32_t M, int32_t n_lev, const float *q, const float *x, const float *h,
                                const float *amp, const float *P, const float *g_up, float *gq, float *gh, void *stream)
{
    if (R == 0) return VAEQ_OK;
    if (!q || !x || !h || !amp || !P || !g_up || !gq || !gh) return VAEQ_ERR_NULL;
    if (R < 0 || !vaeq::loss_shape_ok(B, sps, M)) return VAEQ_ERR_SHAPE;
    const size_t lds = sizeof(float) * (size_t)(8 * B + 4 * (B * sps - 2 * (M / 2)) + 10 * M + 64);
    if (lds > vaeq::LDS_MAX) return VAEQ_ERR_LDS;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return dispatch_nlev(n_lev, [&](auto nl) {
        return launch(vaeq::dp_loss_bwd_kernel<decltype(nl)::value>, dim3(R), dim3(256), lds, st, B, sps, M, q, x, h, amp, P, g_up, gq, gh);
    });
}

extern "C" int vaeq_dp_forward_bwd(int32_t R, int32_t N, int32_t sps, int32_t M, int32_t n_lev, const float *x, const float *q, const float *y,
                                   const float *gq, const float *gy, const float *amp, const float *var, float *gW, void *stream)
{
    if (R == 0) return VAEQ_OK;
    if (!x || !q || !y || !gq || !amp || !var || !gW) return VAEQ_ERR_NULL;
    if (R < 0 || N <= 0 || !vaeq::fir_shape_ok(sps, M)) return VAEQ_ERR_SHAPE;
    const size_t lds = sizeof(float) * (size_t)4 * N;
    if (lds > vaeq::LDS_MAX) return VAEQ_ERR_LDS;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return dispatch_nlev(n_lev, [&](auto nl) {
        return launch(vaeq::dp_forward_bwd_kernel<decltype(nl)::value>, dim3(R), dim3(256), lds, st, N, sps, M, x, q, y, gq, gy, amp, var, gW);
    });
}

extern "C" int vaeq_awgn_forward(int32_t R, int64_t N, int32_t sps, int32_t M, int32_t n_lev, const float *x, const float *W,
                                 const float *amp, const float *amp_mean, const float *var, float *q, float *y, void *stream)
{
    if (R == 0 || N == 0) return VAEQ_OK;
    if (!x || !W || !amp || !amp_mean || !var || !y) return VAEQ_ERR_NULL;
    if (R < 0 || N < 0 || !vaeq::fir_shape_ok(sps, M)) return VAEQ_ERR_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return dispatch_nlev(n_lev, [&](auto nl) {
        return launch(vaeq::awgn_forward_kernel<decltype(nl)::value>, dim3(R), dim3(256), 0, st, N, sps, M, x, W, amp, amp_mean, var, q, y);
    });
}

extern "C" int vaeq_awgn_loss(int32_t R, int32_t B, int32_t sps, int32_t M, int32_t n_lev, const float *q, const float *x, const float *h,
                              const float *amp, const float *P, float *loss, void *stream)
{
    if (R == 0) return VAEQ_OK;
    if (!q || !x || !h || !amp || !loss) return VAEQ_ERR_NULL;
    if (R < 0 || !vaeq::loss_shape_ok(B, sps, M)) return VAEQ_ERR_SHAPE;
    const size_t lds = (size_t)4 * B * sizeof(float);
    if (lds > vaeq::LDS_MAX_BESIDE_STATIC) return VAEQ_ERR_LDS;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return dispatch_nlev(n_lev, [&](auto nl) {
        return launch(vaeq::awgn_loss_kernel<decltype(nl)::value>, dim3(R), dim3(256), lds, st, B, sps, M, q, x, h, amp, P, loss);
    });
}

extern "C" int vaeq_awgn_loss_bwd(int32_t R, int32_t B, int32_t sps, int32_t M, int32_t n_lev, const float *q, const float *x, const float *h,
                                  const float *amp, const float *P, const float *g_up, float *gq, float *gh, void *stream)
{
    if (R == 0) return VAEQ_OK;
    if (!q || !x || !h || !amp || !g_up || !gq || !gh) return VAEQ_ERR_NULL;
    if (R < 0 || !vaeq::loss_shape_ok(B, sps, M)) return VAEQ_ERR_SHAPE;
    const size_t lds = ((size_t)4 * B + 2 * ((size_t)B * sps - 2 * (M / 2))) * sizeof(float);
    if (lds > vaeq::LDS_MAX_BESIDE_STATIC) return VAEQ_ERR_LDS;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return dispatch_nlev(n_lev, [&](auto nl) {
        return launch(vaeq::awgn_loss_bwd_kernel<decltype(nl)::value>, dim3(R), dim3(256), lds, st, B, sps, M, q, x, h, amp, P, g_up, gq, gh);
    });
}

extern "C" int vaeq_awgn_forward_bwd(int32_t R, int32_t N, int32_t sps, int32_t M, int32_t n_lev, const float *x, const float *W, const float *amp,
                                     const float *amp_mean, const float *var, const float *gq, const float *gy, float *gW, void *stream)
{
    if (R == 0) return VAEQ_OK;
    if (!x || !W || !amp || !amp_mean || !var || !gq || !gW) return VAEQ_ERR_NULL;
    if (R < 0 || N <= 0 || !vaeq::fir_shape_ok(sps, M)) return VAEQ_ERR_SHAPE;
    const size_t lds = (size_t)4 * N * sizeof(float);
    if (lds > vaeq::LDS_MAX_BESIDE_STATIC) return VAEQ_ERR_LDS;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return dispatch_nlev(n_lev, [&](auto nl) {
        return launch(vaeq::awgn_forward_bwd_kernel<decltype(nl)::value>, dim3(R), dim3(256), lds, st, N, sps, M, x, W, amp, amp_mean, var, gq, gy, gW);
    });
}

// ---- input gradients (d/dx): the same checks as the sibling that yields the parameter gradients, and the instantiation reported to vaeq_last_kernel

extern "C" int vaeq_dp_forward_bwd_x(int32_t R, int32_t N, int32_t sps, int32_t M, int32_t n_lev, const float *W, const float *q, const float *y,
                                     const float *gq, const float *gy, const float *amp, const float *var, float *gx, void *stream)
{
    if (R == 0) return VAEQ_OK;
    if (!W || !q || !y || !gq || !amp || !var || !gx) return VAEQ_ERR_NULL;
    if (R < 0 || N <= 0 || !vaeq::fir_shape_ok(sps, M)) return VAEQ_ERR_SHAPE;
    const size_t lds = sizeof(float) * ((size_t)4 * N + 8 * M);
    if (lds > vaeq::LDS_MAX) return VAEQ_ERR_LDS;
    if ((int64_t)N * sps > 0x1fffffff) return VAEQ_ERR_SHAPE;           // (4 N sps gradient samples are indexed in 32 bits)
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return dispatch_nlev(n_lev, [&](auto nl) {
        vaeq::note_kernel("vaeq::dp_forward_bwd_x_kernel<%d>", (int)decltype(nl)::value);
        return launch(vaeq::dp_forward_bwd_x_kernel<decltype(nl)::value>, dim3(R), dim3(256), lds, st, N, sps, M, W, q, y, gq, gy, amp, var, gx);
    });
}

extern "C" int vaeq_dp_loss_bwd_x(int32_t R, int32_t B, int32_t sps, int32_t M, int32_t n_lev, const float *q, const float *x, const float *h,
                                  const float *amp, const float *g_up, float *gx, void *stream)
{
    if (R == 0) return VAEQ_OK;
    if (!q || !x || !h || !amp || !g_up || !gx) return VAEQ_ERR_NULL;
    if (R < 0 || !vaeq::loss_shape_ok(B, sps, M)) return VAEQ_ERR_SHAPE;
    const size_t lds = sizeof(float) * (size_t)(8 * B + 4 * (B * sps - 2 * (M / 2)) + 10 * M + 64);
    if (lds > vaeq::LDS_MAX) return VAEQ_ERR_LDS;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return dispatch_nlev(n_lev, [&](auto nl) {
        vaeq::note_kernel("vaeq::dp_loss_bwd_x_kernel<%d>", (int)decltype(nl)::value);
        return launch(vaeq::dp_loss_bwd_x_kernel<decltype(nl)::value>, dim3(R), dim3(256), lds, st, B, sps, M, q, x, h, amp, g_up, gx);
    });
}

extern "C" int vaeq_awgn_forward_bwd_x(int32_t R, int32_t N, int32_t sps, int32_t M, int32_t n_lev, const float *x, const float *W,
                                       const float *amp, const float *amp_mean, const float *var, const float *gq, const float *gy, float *gx,
                                       void *stream)
{
    if (R == 0) return VAEQ_OK;
    if (!x || !W || !amp || !amp_mean || !var || !gq || !gx) return VAEQ_ERR_NULL;
    if (R < 0 || N <= 0 || !vaeq::fir_shape_ok(sps, M)) return VAEQ_ERR_SHAPE;
    const size_t lds = (size_t)4 * N * sizeof(float);
    if (lds > vaeq::LDS_MAX_BESIDE_STATIC) return VAEQ_ERR_LDS;
    if ((int64_t)N * sps > 0x3fffffff) return VAEQ_ERR_SHAPE;           // (2 N sps gradient samples are indexed in 32 bits)
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return dispatch_nlev(n_lev, [&](auto nl) {
        vaeq::note_kernel("vaeq::awgn_forward_bwd_x_kernel<%d>", (int)decltype(nl)::value);
        return launch(vaeq::awgn_forward_bwd_x_kernel<decltype(nl)::value>, dim3(R), dim3(256), lds, st, N, sps, M, x, W, amp, amp_mean, var, gq, gy,
                      gx);
    });
}

extern "C" int vaeq_awgn_loss_bwd_x(int32_t R, int32_t B, int32_t sps, int32_t M, int32_t n_lev, const float *q, const float *x, const float *h,
                                    const float *amp, const float *g_up, float *gx, void *stream)
{
    if (R == 0) return VAEQ_OK;
    if (!q || !x || !h || !amp || !g_up || !gx) return VAEQ_ERR_NULL;
    if (R < 0 || !vaeq::loss_shape_ok(B, sps, M)) return VAEQ_ERR_SHAPE;
    const size_t lds = ((size_t)4 * B + 2 * ((size_t)B * sps - 2 * (M / 2))) * sizeof(float);
    if (lds > vaeq::LDS_MAX_BESIDE_STATIC) return VAEQ_ERR_LDS;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return dispatch_nlev(n_lev, [&](auto nl) {
        vaeq::note_kernel("vaeq::awgn_loss_bwd_x_kernel<%d>", (int)decltype(nl)::value);
        return launch(vaeq::awgn_loss_bwd_x_kernel<decltype(nl)::value>, dim3(R), dim3(256), lds, st, B, sps, M, q, x, h, amp, g_up, gx);
    });
}
