// vaeq_nn_ops.hip -- the VAE-NN encoder as a stand-alone differentiable operator (AWGN_channel/func_VAENN_MQAM.py: Net :170-188, Net_BN :190-211):
// forward with a mode flag and backward for an ARBITRARY upstream gradient dL/dq, on the network's own parameters
//   theta_net = [fc1.weight C*2*k1 | fc1.bias C | fc2.weight C*C*k2 | fc2.bias C ( | batch1.weight C | batch1.bias C )],  C = 2 n_lev
// (h_est belongs to the loss, not to these calls).  They back func_VAENN_MQAM.Net / Net_BN through autograd_ops.nn_encode; the product's training
// loop stays the fused nn_train_kernel of vaeq_nn.hip, whose device helpers (vaeq_nn_dev.h) do the convolutions and their gradients here too --
// 64-QAM and 16-QAM on v_mfma_f32_16x16x4_f32, 4-QAM on the vector ALU.
//
//   nn_enc_forward_kernel      eval-mode forward (Net in either mode, Net_BN after net.eval()): the tiled forward of vaeq_nn_forward, any length
//   nn_enc_bn_forward_kernel   Net_BN in training mode: batch statistics over the L samples (biased variance), saved (mean, 1 / std) for the
//                              backward pass, running statistics moved by momentum 0.1 with the unbiased variance (as nn_train_kernel does in a step)
//   nn_enc_backward_x_kernel   the same pass plus the input gradient dL/dx (the transpose of fc1 applied to dL/d(fc1 output), on the vector ALU)
//   nn_enc_backward_kernel     softmax backward per axis -> fc2 weight / bias gradients -> transposed strided convolution -> BatchNorm backward
//                              (MODE 1: batch statistics, with the mean and variance terms; MODE 2: running statistics, a per-channel scale) -> ELU'
//                              -> fc1 weight / bias gradients.  ELU(fc1(x)) is RECOMPUTED from x: the state saved by the forward is q plus 2 C numbers.
// One workgroup per run with the whole input resident in LDS (the training-mode forward and the backward pass are bounded by the 160 KiB of a CU:
// vaeq_nn_enc_lds_bytes); every sum runs in a fixed order inside that workgroup -- no atomics, results bit-reproducible and independent of R.
// The reference's residual x_res (:183-185) is the same number for every logit of an axis and cancels in the softmax: it is left out, as everywhere.
#include "vaeq_nn_dev.h"

namespace vaeq {

// LDS layout of the two resident kernels; bwd adds what the gradient GEMMs need (rows of ones, zero guard columns around dL/dlogits, the [k][c][cc]
// copy of fc2.weight, the gradient vector, scratch for split weight-gradient sums) -- the conventions of nn_layout, without the loss and Adam arrays.
__host__ __device__ inline NNLayout nn_enc_layout(int L, int sps, int n, int k1, int k2, bool bn, bool bwd)
{
    NNLayout l = {};
    const int N = (L + sps - 1) / sps;
    l.C = 2 * n; l.L = L; l.p1 = k1 / 2; l.p2 = k2 / 2;
    l.Lx = pad4(L + 2 * l.p1 + 8);
    l.Lz = pad4(L + 2 * l.p2 + 4);
    const bool mf = nn_mf(n);
    const int CP = nn_cp(n);
    if (mf)
        while ((l.Lz & 7) != 4) l.Lz += 4;
    l.nm = L;
    l.NW1 = l.C * 2 * k1;
    l.oW1 = 0; l.oB1 = l.NW1; l.oW2 = l.oB1 + l.C; l.oB2 = l.oW2 + l.C * l.C * k2;
    l.oG = l.oB2 + l.C; l.oBt = l.oG + l.C;
    l.oH = l.NP = bn ? l.oBt + l.C : l.oG;
    int o = 0;
    auto take = [&](int cnt) { int r = o; o += pad4(cnt); return r; };
    const int one = (mf && bwd) ? 1 : 0;
    l.xs = take((2 + one) * l.Lx);
    l.z1 = take((CP + (bn ? 0 : one)) * l.Lz);
    l.zb = bn ? take((CP + one) * l.Lz) : l.z1;
    l.bnst = take(bn ? 2 * l.C : 0);                    // mean, 1 / std
    l.A0 = one ? 4 : 0;
    l.AS = N;
    if (one) {
        l.AS = 16 * ((N + 15) / 16) + 2 * l.A0;
        while ((l.AS & 7) != 4) l.AS += 4;
    }
    l.a2 = take(CP * l.AS + 2 * l.A0);
    l.mu = take(bwd ? 4 * N : 0);                       // scratch of mfma_wgrad16
    l.vr = l.es = l.VS = l.PH = l.mu;
    l.th = take(l.NP);
    l.gr = take(bwd ? l.NP : 0);
    l.am = l.av = l.ax = l.gr;
    l.w1t = take(mf ? 64 * ((((k1 + 1) / 2) + 1) & ~1) : l.NW1 + 7 * l.C);
    l.w2t = take(mf ? 256 * k2 : l.C * l.C * k2 + 7 * l.C);
    l.w2u = take(bwd ? CP * CP * k2 : 0);
    l.red = take(64);
    l.total = o;
    return l;
}

// BatchNorm1d in training mode on the LDS-resident ELU output (the pass of nn_train_kernel): z1 <- zhat, zb <- gamma zhat + beta; one wave per channel.
// STATS: compute the batch statistics (and hand them to `done(c, mean, rstd, var)`); otherwise normalise with bnst = (mean, 1 / std) as given.
template <int NT, int NLEV, bool STATS, typename DoneF>
__device__ __forceinline__ void nn_enc_batchnorm(const NNLayout &l, const float *th, float *z1, float *zb, float *bnst, DoneF done)
{
    constexpr int C = 2 * NLEV, NWV = NT / 64, NVM = 10;
    const int L = l.L, Lz = l.Lz, p2 = l.p2, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const bool inreg = L <= 64 * NVM;                          // a lane's share of a channel row stays in registers (same summation order either way)
    for (int c = wv; c < C; c += NWV) {
        float *zr = z1 + c * Lz + p2;
        float zv[NVM];
        float mean, rstd;
        if (inreg) {
#pragma unroll
            for (int u = 0; u < NVM; u++) { const int sx = lane + 64 * u; zv[u] = ldsv(zr + (sx < L ? sx : L - 1)); }
        }
        if constexpr (STATS) {
            float sm_ = 0.f, sv = 0.f;
            if (inreg) {
#pragma unroll
                for (int u = 0; u < NVM; u++) sm_ += lane + 64 * u < L ? zv[u] : 0.f;
            } else
                for (int sx = lane; sx < L; sx += 64) sm_ += zr[sx];
            mean = wave_sum_fast(sm_) / (float)L;
            if (inreg) {
#pragma unroll
                for (int u = 0; u < NVM; u++) { const float d = zv[u] - mean; sv = lane + 64 * u < L ? fmaf(d, d, sv) : sv; }
            } else
                for (int sx = lane; sx < L; sx += 64) { const float d = zr[sx] - mean; sv = fmaf(d, d, sv); }
            const float var = wave_sum_fast(sv) / (float)L;
            rstd = 1.0f / sqrtf(var + 1e-5f);
            if (lane == 0) done(c, mean, rstd, var);
        } else {
            mean = bnst[c]; rstd = bnst[C + c];
        }
        const float ga = th[l.oG + c], be = th[l.oBt + c];
        if (inreg) {
#pragma unroll
            for (int u = 0; u < NVM; u++) {
                const int sx = lane + 64 * u;
                const float zh = (zv[u] - mean) * rstd;
                if (sx < L) { zr[sx] = zh; zb[c * Lz + p2 + sx] = fmaf(ga, zh, be); }
            }
        } else
            for (int sx = lane; sx < L; sx += 64) {
                const float zh = (zr[sx] - mean) * rstd;
                zr[sx] = zh;
                zb[c * Lz + p2 + sx] = fmaf(ga, zh, be);
            }
    }
}

// ---- eval-mode forward, tiled over any length: x[R][2][L], theta_net[R][NP] -> q[R][C][N], N = ceil(L / sps)
// (tile = symbols per pass: NN_TILE, or fewer where 16 channel rows of NN_TILE sps samples do not fit the LDS -- 64-QAM at sps >= 7)
template <int NT, int NLEV>
__global__ __launch_bounds__(NT) void nn_enc_forward_kernel(int L, int sps, int k1, int k2, int tile, const float *__restrict__ x,
                                                            const float *__restrict__ theta, const float *__restrict__ bn_running,
                                                            float *__restrict__ q)
{
    extern __shared__ float4 smem4[];
    float *sm = reinterpret_cast<float *>(smem4);
    constexpr int C = 2 * NLEV;
    const int tid = threadIdx.x, run = blockIdx.x;
    const bool bn = bn_running != nullptr;
    const NNLayout l = nn_layout(tile, sps, 1, NLEV, k1, k2, bn, true);
    const int NP = l.oH, N = (L + sps - 1) / sps;              // the network's part of nn_layout's vector
    float *xs = sm + l.xs, *z1 = sm + l.z1, *a2 = sm + l.a2, *th = sm + l.th, *w1t = sm + l.w1t, *w2t = sm + l.w2t;
    float *aff = bn ? sm + l.bnst + 4 * C : nullptr;
    for (int i = tid; i < NP; i += NT) th[i] = theta[(size_t)run * NP + i];
    __syncthreads();
    if (bn && tid < C) {                                       // running statistics folded into one affine map per channel
        const float sc = th[l.oG + tid] / sqrtf(bn_running[(size_t)run * 2 * C + C + tid] + 1e-5f);
        aff[tid] = sc;
        aff[C + tid] = th[l.oBt + tid] - bn_running[(size_t)run * 2 * C + tid] * sc;
    }
    nn_transpose_weights<NT, NLEV>(l, k1, k2, th, w1t, w2t);
    __syncthreads();
    const float *x0 = x + (size_t)run * 2 * (size_t)L, *x1 = x0 + L;
    for (int n0 = 0; n0 < N; n0 += tile) {
        const int Bt = min(tile, N - n0);
        if (tile == NN_TILE)
            nn_forward_tile<NT, NLEV>(l, sps, k1, k2, (int64_t)L, x0, x1, n0, Bt, xs, z1, a2, th, w1t, w2t, aff);
        else {                                                 // the same three phases with the logits' row stride = tile
            const int p1 = l.p1, p2 = l.p2, zlo = n0 * sps - p2, Lz_need = (Bt - 1) * sps + k2, xlo = zlo - p1, Lx_need = Lz_need + 2 * p1;
            for (int i = tid; i < 2 * (Lx_need + 4); i += NT) {
                const int row = i / (Lx_need + 4), c = i - row * (Lx_need + 4), sx = xlo + c;
                xs[row * l.Lx + c] = (c < Lx_need && sx >= 0 && sx < L) ? (row ? x1[sx] : x0[sx]) : 0.f;
            }
            __syncthreads();
            nn_fc1_elu<NT, NLEV>(l, k1, xs, th, w1t, z1 - p2, Lz_need, zlo, L, aff);
            __syncthreads();
            nn_fc2<NT, NLEV>(l, sps, k2, Bt, tile, z1, th, w2t, a2);
            __syncthreads();
        }
        for (int it = tid; it < 2 * Bt; it += NT) {
            const int axq = it / Bt, n = it - axq * Bt;
            float z[NLEV], zmax = -3.0e38f, ssum = 0.f;
#pragma unroll
            for (int i = 0; i < NLEV; i++) { z[i] = a2[(axq * NLEV + i) * tile + n]; zmax = fmaxf(zmax, z[i]); }
#pragma unroll
            for (int i = 0; i < NLEV; i++) { z[i] = __expf(z[i] - zmax); ssum += z[i]; }
#pragma unroll
            for (int i = 0; i < NLEV; i++) q[((size_t)run * C + axq * NLEV + i) * N + n0 + n] = z[i] / ssum;
        }
        __syncthreads();
    }
}

// ---- Net_BN.forward in training mode: the whole input resident, batch statistics over its L samples
template <int NT, int NLEV>
__global__ __launch_bounds__(NT) void nn_enc_bn_forward_kernel(int L, int sps, int k1, int k2, const float *__restrict__ x,
                                                               const float *__restrict__ theta, float *__restrict__ bn_running,
                                                               float *__restrict__ bn_saved, float *__restrict__ q)
{
    extern __shared__ float4 smem4[];
    float *sm = reinterpret_cast<float *>(smem4);
    constexpr int C = 2 * NLEV;
    const int tid = threadIdx.x, run = blockIdx.x;
    const NNLayout l = nn_enc_layout(L, sps, NLEV, k1, k2, true, false);
    const int N = (L + sps - 1) / sps, NP = l.NP, AS = l.AS;
    float *xs = sm + l.xs, *z1 = sm + l.z1, *zb = sm + l.zb, *bnst = sm + l.bnst, *a2 = sm + l.a2, *th = sm + l.th, *w1t = sm + l.w1t, *w2t = sm + l.w2t;
    for (int i = tid; i < l.total; i += NT) sm[i] = 0.f;       // halos, padding rows and every cell a tile may read past its columns: zero
    __syncthreads();
    for (int i = tid; i < NP; i += NT) th[i] = theta[(size_t)run * NP + i];
    const float *xr = x + (size_t)run * 2 * (size_t)L;
    for (int i = tid; i < 2 * L; i += NT) {
        const int row = i / L, c = i - row * L;
        xs[row * l.Lx + l.p1 + c] = xr[i];
    }
    __syncthreads();
    nn_transpose_weights<NT, NLEV>(l, k1, k2, th, w1t, w2t);
    __syncthreads();
    nn_fc1_elu<NT, NLEV>(l, k1, xs, th, w1t, z1, L, 0, L);
    __syncthreads();
    float *rs = bn_running ? bn_running + (size_t)run * 2 * C : nullptr, *sv = bn_saved ? bn_saved + (size_t)run * 2 * C : nullptr;
    nn_enc_batchnorm<NT, NLEV, true>(l, th, z1, zb, bnst, [&](int c, float mean, float rstd, float var) {
        if (sv) { sv[c] = mean; sv[C + c] = rstd; }
        if (rs) {                                              // running statistics: momentum 0.1, unbiased variance
            rs[c] = 0.9f * rs[c] + 0.1f * mean;
            rs[C + c] = 0.9f * rs[C + c] + 0.1f * (var * (float)L / (float)(L - 1));
        }
    });
    __syncthreads();
    nn_fc2<NT, NLEV>(l, sps, k2, N, AS, zb, th, w2t, a2);
    __syncthreads();
    for (int it = tid; it < 2 * N; it += NT) {
        const int axq = it / N, n = it - axq * N;
        float z[NLEV], zmax = -3.0e38f, ssum = 0.f;
#pragma unroll
        for (int i = 0; i < NLEV; i++) { z[i] = a2[(axq * NLEV + i) * AS + n]; zmax = fmaxf(zmax, z[i]); }
#pragma unroll
        for (int i = 0; i < NLEV; i++) { z[i] = __expf(z[i] - zmax); ssum += z[i]; }
#pragma unroll
        for (int i = 0; i < NLEV; i++) q[((size_t)run * C + axq * NLEV + i) * N + n] = z[i] / ssum;
    }
}

// ---- backward: (x, theta_net, q, dL/dq, BatchNorm statistics) -> dL/dtheta_net.  MODE 0: Net; 1: Net_BN, training (stats = saved mean | 1 / std);
// 2: Net_BN, eval (stats = running_mean | running_var: the normalisation is a fixed affine map, no mean / variance terms)
template <int NT, int NLEV, int MODE>
__global__ __launch_bounds__(NT) void nn_enc_backward_kernel(int L, int sps, int k1, int k2, const float *__restrict__ x,
                                                             const float *__restrict__ theta, const float *__restrict__ q,
                                                             const float *__restrict__ gq, const float *__restrict__ stats,
                                                             float *__restrict__ g_out)
{
    constexpr bool GX = false;
    float *const gx = nullptr;
#include "vaeq_nn_enc_backward_body.h"
}

// ---- backward with the input gradient: the same pass (the same dL/dtheta_net, bit for bit) plus gx[R][2][L]
template <int NT, int NLEV, int MODE>
__global__ __launch_bounds__(NT) void nn_enc_backward_x_kernel(int L, int sps, int k1, int k2, const float *__restrict__ x,
                                                               const float *__restrict__ theta, const float *__restrict__ q,
                                                               const float *__restrict__ gq, const float *__restrict__ stats,
                                                               float *__restrict__ g_out, float *__restrict__ gx)
{
    constexpr bool GX = true;
#include "vaeq_nn_enc_backward_body.h"
}

static bool nn_enc_shape_ok(int sps, int n_lev, int k1, int k2)
{
    if (sps <= 0 || sps > 8 || !(n_lev == 2 || n_lev == 4 || n_lev == 8)) return false;
    return k1 > 0 && (k1 & 1) && k1 <= 63 && k2 > 0 && (k2 & 1) && k2 <= 9;
}

constexpr int64_t NN_ENC_LMAX = 1 << 20;                   // far past the LDS ceiling: keeps the layout arithmetic inside 32 bits

template <int NLEV>
static int launch_nn_enc_forward(int R, int L, int sps, int k1, int k2, bool bn, bool training, const float *x, const float *theta,
                                 float *bn_running, float *bn_saved, float *q, hipStream_t st)
{
    if (bn && training) {
        const size_t lds = (size_t)nn_enc_layout(L, sps, NLEV, k1, k2, true, true).total * 4;      // the ceiling of the backward pass, so that what
        if (lds > LDS_MAX) return VAEQ_ERR_LDS;                                                   // this call accepts can be differentiated
        auto k = nn_enc_bn_forward_kernel<512, NLEV>;
        const size_t ldf = (size_t)nn_enc_layout(L, sps, NLEV, k1, k2, true, false).total * 4;
        note_kernel("vaeq::nn_enc_bn_forward_kernel<512, %d>", NLEV);
        return launch(k, dim3(R), dim3(512), ldf, st, L, sps, k1, k2, x, theta, bn_running, bn_saved, q);
    }
    int tile = NN_TILE;
    size_t lds = (size_t)nn_layout(tile, sps, 1, NLEV, k1, k2, bn, true).total * 4;
    while (lds > LDS_MAX && tile > 15) {
        tile = tile / 2;                                       // 127, 63, 31, 15
        lds = (size_t)nn_layout(tile, sps, 1, NLEV, k1, k2, bn, true).total * 4;
    }
    if (lds > LDS_MAX) return VAEQ_ERR_LDS;
    note_kernel("vaeq::nn_enc_forward_kernel<1024, %d>", NLEV);
    return launch(nn_enc_forward_kernel<1024, NLEV>, dim3(R), dim3(1024), lds, st, L, sps, k1, k2, tile, x, theta, bn ? bn_running : nullptr, q);
}

template <int NLEV>
static int launch_nn_enc_backward(int R, int L, int sps, int k1, int k2, int mode, const float *x, const float *theta, const float *q,
                                  const float *gq, const float *stats, float *g, hipStream_t st)
{
    const size_t lds = (size_t)nn_enc_layout(L, sps, NLEV, k1, k2, mode != 0, true).total * 4;
    if (lds > LDS_MAX) return VAEQ_ERR_LDS;
    auto k = mode == 0 ? nn_enc_backward_kernel<512, NLEV, 0> : mode == 1 ? nn_enc_backward_kernel<512, NLEV, 1> : nn_enc_backward_kernel<512, NLEV, 2>;
    note_kernel("vaeq::nn_enc_backward_kernel<512, %d, %d>", NLEV, mode);
    return launch(k, dim3(R), dim3(512), lds, st, L, sps, k1, k2, x, theta, q, gq, stats, g);
}

template <int NLEV>
static int launch_nn_enc_backward_x(int R, int L, int sps, int k1, int k2, int mode, const float *x, const float *theta, const float *q,
                                    const float *gq, const float *stats, float *g, float *gx, hipStream_t st)
{
    const size_t lds = (size_t)nn_enc_layout(L, sps, NLEV, k1, k2, mode != 0, true).total * 4;     // the input gradient needs no LDS of its own
    if (lds > LDS_MAX) return VAEQ_ERR_LDS;
    auto k = mode == 0 ? nn_enc_backward_x_kernel<512, NLEV, 0> : mode == 1 ? nn_enc_backward_x_kernel<512, NLEV, 1> : nn_enc_backward_x_kernel<512, NLEV, 2>;
    note_kernel("vaeq::nn_enc_backward_x_kernel<512, %d, %d>", NLEV, mode);
    return launch(k, dim3(R), dim3(512), lds, st, L, sps, k1, k2, x, theta, q, gq, stats, g, gx);
}

}  // namespace vaeq

extern "C" int64_t vaeq_nn_enc_param_count(int32_t n_lev, int32_t k1, int32_t k2, int32_t batch_norm)
{
    if (!vaeq::nn_enc_shape_ok(1, n_lev, k1, k2)) return VAEQ_ERR_SHAPE;
    return vaeq::nn_enc_layout(64, 1, n_lev, k1, k2, batch_norm != 0, false).NP;
}

extern "C" int64_t vaeq_nn_enc_lds_bytes(int64_t L, int32_t sps, int32_t n_lev, int32_t k1, int32_t k2, int32_t batch_norm)
{
    if (!vaeq::nn_enc_shape_ok(sps, n_lev, k1, k2) || L <= 0 || L > vaeq::NN_ENC_LMAX) return VAEQ_ERR_SHAPE;
    return (int64_t)vaeq::nn_enc_layout((int)L, sps, n_lev, k1, k2, batch_norm != 0, true).total * 4;
}

extern "C" int vaeq_nn_enc_forward(int32_t R, int64_t L, int32_t sps, int32_t n_lev, int32_t k1, int32_t k2, int32_t batch_norm, int32_t training,
                                   const float *x, const float *theta_net, float *bn_running, float *bn_saved, float *q, void *stream)
{
    if (R == 0 || L == 0) return VAEQ_OK;
    if (!x || !theta_net || !q) return VAEQ_ERR_NULL;
    const bool bn = batch_norm != 0, tr = training != 0;
    if (bn && !tr && !bn_running) return VAEQ_ERR_NULL;        // (training mode: bn_running NULL = no running statistics kept; bn_saved NULL = not saved)
    if (R < 0 || L < 0 || L > 0x3fffffff || !vaeq::nn_enc_shape_ok(sps, n_lev, k1, k2)) return VAEQ_ERR_SHAPE;
    if (bn && tr) {
        if (L < 2) return VAEQ_ERR_SHAPE;                      // the unbiased variance of one sample (PyTorch refuses it too)
        if (L > vaeq::NN_ENC_LMAX) return VAEQ_ERR_LDS;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return vaeq::dispatch_nlev(n_lev, [&](auto nl) {
        return vaeq::launch_nn_enc_forward<decltype(nl)::value>(R, (int)L, sps, k1, k2, bn, tr, x, theta_net, bn_running, bn_saved, q, st);
    });
}

extern "C" int vaeq_nn_enc_backward(int32_t R, int64_t L, int32_t sps, int32_t n_lev, int32_t k1, int32_t k2, int32_t batch_norm, int32_t training,
                                    const float *x, const float *theta_net, const float *q, const float *gq, const float *bn_stats,
                                    float *g_theta_net, void *stream)
{
    if (R == 0) return VAEQ_OK;
    if (!x || !theta_net || !q || !gq || !g_theta_net || (batch_norm && !bn_stats)) return VAEQ_ERR_NULL;
    if (R < 0 || L <= 0 || !vaeq::nn_enc_shape_ok(sps, n_lev, k1, k2)) return VAEQ_ERR_SHAPE;
    if (L > vaeq::NN_ENC_LMAX) return VAEQ_ERR_LDS;
    const int mode = batch_norm ? (training ? 1 : 2) : 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return vaeq::dispatch_nlev(n_lev, [&](auto nl) {
        return vaeq::launch_nn_enc_backward<decltype(nl)::value>(R, (int)L, sps, k1, k2, mode, x, theta_net, q, gq, bn_stats, g_theta_net, st);
    });
}

extern "C" int vaeq_nn_enc_backward_x(int32_t R, int64_t L, int32_t sps, int32_t n_lev, int32_t k1, int32_t k2, int32_t batch_norm, int32_t training,
                                      const float *x, const float *theta_net, const float *q, const float *gq, const float *bn_stats,
                                      float *g_theta_net, float *gx, void *stream)
{
    if (R == 0) return VAEQ_OK;
    if (!x || !theta_net || !q || !gq || !g_theta_net || !gx || (batch_norm && !bn_stats)) return VAEQ_ERR_NULL;
    if (R < 0 || L <= 0 || !vaeq::nn_enc_shape_ok(sps, n_lev, k1, k2)) return VAEQ_ERR_SHAPE;
    if (L > vaeq::NN_ENC_LMAX) return VAEQ_ERR_LDS;
    const int mode = batch_norm ? (training ? 1 : 2) : 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return vaeq::dispatch_nlev(n_lev, [&](auto nl) {
        return vaeq::launch_nn_enc_backward_x<decltype(nl)::value>(R, (int)L, sps, k1, k2, mode, x, theta_net, q, gq, bn_stats, g_theta_net, gx, st);
    });
}
