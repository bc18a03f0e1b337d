// vaeq_nn_dev.h -- device helpers of the VAE-NN kernels, shared by vaeq_nn.hip (fused training loop, validation) and vaeq_nn_ops.hip
// (the stand-alone encoder forward / backward behind func_VAENN_MQAM.Net / Net_BN): the LDS layout, the wave reductions, the MFMA
// convolutions and their gradients, fc1 + ELU, fc2 and the tiled eval-mode forward.
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vaeq.h"
#include "vaeq_common.h"
#include "vaeq_launch.h"
#include "vaeq_validate.h"
#include "vaeq_wave.h"

#ifndef VAEQ_NN_MFMA8
#define VAEQ_NN_MFMA8 1                                // 16-QAM (8 channels) on the 16-row MFMA path of 64-QAM, rows 8..15 zero (0: the vector-ALU path)
#endif

namespace vaeq {

// which alphabets run the convolutions on v_mfma_f32_16x16x4_f32, and the channel rows their LDS buffers carry (MFMA rows: 16)
__host__ __device__ constexpr bool nn_mf(int n) { return n == 8 || (n == 4 && VAEQ_NN_MFMA8); }
__host__ __device__ constexpr int nn_cp(int n) { return nn_mf(n) ? 16 : 2 * n; }

struct NNLayout {
    int C, L, p1, p2, Lx, Lz, mh, Mh, nm, NP, NW1, oW1, oB1, oW2, oB2, oG, oBt, oH;
    int AS, A0;                                        // row stride / first column of a2 (training, C = 16: zero guard columns around the B logits of a row)
    int ES, PH;                                        // row stride of the zero-guarded residual rows; offset of the |h|^2 prefix sums
    int xs, z1, zb, bnst, a2, mu, vr, es, VS, th, gr, am, av, ax, w1t, w2t, w2u, red, total;
};

__host__ __device__ inline NNLayout nn_layout(int B, int sps, int M, int n, int k1, int k2, bool bn = false, bool eval = false)
{
    NNLayout l;
    l.C = 2 * n; l.L = B * sps; l.p1 = k1 / 2; l.p2 = k2 / 2;
    l.Lx = pad4(l.L + 2 * l.p1 + 8);                   // zero halo + room for the 4-wide windows of the last quad
    l.Lz = pad4(l.L + 2 * l.p2 + 4);
    const bool mf = nn_mf(n);
    const int CP = nn_cp(n);                           // channel rows in LDS (MFMA path: 16, the rows past C stay zero)
    if (mf)                                            // MFMA path: row stride an odd multiple of 4 dwords, so that 16 channels x 4
        while ((l.Lz & 7) != 4) l.Lz += 4;             // consecutive samples (an MFMA operand / result) fall into 64 different banks
    l.mh = M / 2; l.Mh = 2 * l.mh; l.nm = l.L - l.Mh;
    l.NW1 = l.C * 2 * k1;
    l.oW1 = 0; l.oB1 = l.NW1; l.oW2 = l.oB1 + l.C; l.oB2 = l.oW2 + l.C * l.C * k2;
    l.oG = l.oB2 + l.C; l.oBt = l.oG + l.C;            // BatchNorm weight / bias (Net_BN only)
    l.oH = bn ? l.oBt + l.C : l.oG; l.NP = l.oH + 2 * M;
    int o = 0;
    auto take = [&](int cnt) { int r = o; o += pad4(cnt); return r; };
    const int one = (mf && !eval) ? 1 : 0;         // training on the MFMA path: a row of ones behind the input rows and behind the channel rows (the
                                                       // bias columns of the weight-gradient GEMMs read it like any other operand row: mfma_wgrad16, ROW1)
    l.xs = take((2 + one) * l.Lx);
    l.z1 = take((CP + (bn ? 0 : one)) * l.Lz);         // (Net_BN: fc2's input, and with it the row of ones, is zb)
    l.zb = bn && !eval ? take((CP + one) * l.Lz) : l.z1;      // Net_BN: BatchNorm output (fc2's input); z1 then holds the normalised zhat
                                                       // (eval mode folds the running statistics into fc1's epilogue: no second buffer)
    l.bnst = take(bn ? 6 * l.C : 0);                   // mean, rstd (batch) | running_mean, running_var | eval scale, shift
    // training on the MFMA path: the backward pass through fc2 reads dL/dlogits at n + shift, shift in [-4, 4], for whole 16-column tiles -- with
    // A0 zero columns in front, the row padded to whole tiles + A0 behind and a stride = 4 (mod 8) (conflict-free MFMA operand reads) no read needs a
    // clamp or a condition (a conditional LDS read costs a branch and an exposed round trip each: mfma_convT16)
    l.A0 = (mf && !eval) ? 4 : 0;
    l.AS = B;
    if (mf && !eval) {
        l.AS = 16 * ((B + 15) / 16) + 2 * l.A0;
        while ((l.AS & 7) != 4) l.AS += 4;
    }
    l.a2 = take(CP * l.AS + 2 * l.A0);
    l.mu = take(2 * B); l.vr = take(2 * B);
    l.ES = pad4(l.nm + 2 * l.Mh + 4);                  // Mh zeros | nm residual samples | Mh + 4 zeros (nn_train_kernel)
    l.es = take(2 * l.ES);
    l.VS = take(M);
    l.PH = take(M + 1);
    l.th = take(l.NP);
    const int NPt = eval ? 0 : l.NP;                   // gradient and AMSGrad state: training only
    l.gr = take(NPt); l.am = take(NPt); l.av = take(NPt); l.ax = take(NPt);
    // transposed weight copies: MFMA path = the walk order of mfma_conv16 (16 channel columns, 64 floats per k-step), else [i][k][c] / [cc][k][c]
    l.w1t = take(mf ? 64 * ((((k1 + 1) / 2) + 1) & ~1) : l.NW1 + 7 * l.C);
    l.w2t = take(mf ? 256 * k2 : l.C * l.C * k2 + 7 * l.C);
    l.w2u = take(eval ? 0 : CP * CP * k2);             // fc2.weight as [k][c][cc] (backward through fc2)
    l.red = take(64);
    l.total = o;
    return l;
}

// Sum C per-lane partials over the 64 lanes of a wave, all C at once: log2(C) halving rounds (a lane hands over half of its values
// and keeps the other half) followed by plain butterflies -- C-1 + (6 - log2 C) cross-lane moves instead of 6 C.  Afterwards every
// lane holds the total of channel wave_reduce_channel<C>(lane).  Fixed order: bitwise reproducible.
template <int C>
__device__ __forceinline__ int wave_reduce_channel(int lane)
{
    int c = 0;
#pragma unroll
    for (int m = 32, bit = C >> 1; bit >= 1; m >>= 1, bit >>= 1) c |= (lane & m) ? bit : 0;
    return c;
}

template <int C, int HALF, int MASK>
struct WaveHalve {                                             // compile-time recursion: every register index below is static
    static __device__ __forceinline__ void run(float (&acc)[C], int lane)
    {
        const bool up = (lane & MASK) != 0;                    // upper lanes keep the upper half of the channel range
#pragma unroll
        for (int i = 0; i < HALF; i++) {
            const float send = up ? acc[i] : acc[i + HALF], keep = up ? acc[i + HALF] : acc[i];
            acc[i] = keep + __shfl_xor(send, MASK, 64);
        }
        if constexpr (HALF > 1) WaveHalve<C, HALF / 2, MASK / 2>::run(acc, lane);
    }
};

template <int C>
__device__ __forceinline__ float wave_reduce_scatter(float (&acc)[C], int lane)
{
    WaveHalve<C, C / 2, 32>::run(acc, lane);
    float v = acc[0];
#pragma unroll
    for (int m = 32 / C; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// Weight gradient of one group of 4 adjacent taps for all C output channels: lanes stride over the rows (samples / symbols), a row's
// 4 input values and C upstream gradients give 4 C MACs (2 C v_pk_fma_f32) per 4 + C LDS reads; then four reduce-scatters.
// out(t, c, sum) is called by one lane per (tap t, channel c).
template <int C, typename OutF>
__device__ __forceinline__ void nn_tapgroup_grad(int n_rows, const float *in, int in_step, const float *g, int g_cstride, bool ones, int lane,
                                                 OutF out)
{
    typedef float v2f __attribute__((ext_vector_type(2)));
    v2f acc[C][2];
#pragma unroll
    for (int c = 0; c < C; c++) acc[c][0] = acc[c][1] = v2f{0.f, 0.f};
    for (int r = lane; r < n_rows; r += 64) {
        const float *ip = in + r * in_step;
        const v2f xA = ones ? v2f{1.f, 0.f} : v2f{ip[0], ip[1]}, xB = ones ? v2f{0.f, 0.f} : v2f{ip[2], ip[3]};
#pragma unroll
        for (int c = 0; c < C; c++) {
            const float gv = g[c * g_cstride + r];
            acc[c][0] += gv * xA;
            acc[c][1] += gv * xB;
        }
    }
    constexpr int WR = 64 / C;
    const int cme = wave_reduce_channel<C>(lane);
#pragma unroll
    for (int t = 0; t < 4; t++) {
        float tmp[C];
#pragma unroll
        for (int c = 0; c < C; c++) tmp[c] = (t & 1) ? acc[c][t >> 1].y : acc[c][t >> 1].x;
        const float sum = wave_reduce_scatter<C>(tmp, lane);
        if ((lane & (WR - 1)) == 0) out(t, cme, sum);
    }
}

// the lane-group walks of the two convolutions (mfma_conv16 below; shared by nn_transpose_weights and the callers)
__host__ __device__ inline int conv16_fc1_steps(int k1) { return (((k1 + 1) / 2) + 1) & ~1; }      // taps of a half, rounded up to whole trips
__host__ __device__ inline int conv16_fc2_steps(int k2) { return 4 * k2; }

// ---- transposed weight copies (after every parameter update): w1t[(i k1 + k) C + c], w2t[(cc k2 + k) C + c]
template <int NT, int NLEV>
__device__ __forceinline__ void nn_transpose_weights(const NNLayout &l, int k1, int k2, const float *th, float *w1t, float *w2t,
                                                     float *w2u = nullptr)
{
    constexpr int C = 2 * NLEV;
    if constexpr (nn_mf(NLEV)) {
        // the walk order of mfma_conv16: w1t[(4 t + lg) 16 + c] = fc1.weight[c][lg >> 1][(lg & 1) Th + t] (0 past the half / past k1),
        //                                w2t[(4 t + lg) 16 + c] = fc2.weight[c][4 lg + t / k2][t % k2];  channels / input channels >= C (16-QAM: 8..15): 0
        const int T1 = conv16_fc1_steps(k1), Th = (k1 + 1) / 2;
        for (int j = threadIdx.x; j < 64 * T1; j += NT) {
            const int c = j & 15, lg = (j >> 4) & 3, t = j >> 6, i = lg >> 1, k = (lg & 1) * Th + t;
            w1t[j] = (t < Th && k < k1 && c < C) ? th[l.oW1 + (c * 2 + i) * k1 + k] : 0.f;
        }
        for (int j = threadIdx.x; j < 64 * 4 * k2; j += NT) {
            const int c = j & 15, lg = (j >> 4) & 3, t = j >> 6, cc = 4 * lg + t / k2, k = t % k2;
            w2t[j] = (c < C && cc < C) ? th[l.oW2 + (c * C + cc) * k2 + k] : 0.f;
        }
        if (w2u)
            for (int j = threadIdx.x; j < 256 * k2; j += NT) {
                const int cc = j & 15, c = (j >> 4) & 15, k = j >> 8;
                w2u[j] = (c < C && cc < C) ? th[l.oW2 + (c * C + cc) * k2 + k] : 0.f;
            }
        return;
    } else {
    for (int j = threadIdx.x; j < l.NW1; j += NT) {
        const int c = j % C, ik = j / C, i = ik / k1, k = ik - i * k1;
        w1t[j] = th[l.oW1 + (c * 2 + i) * k1 + k];
    }
    for (int j = threadIdx.x; j < C * C * k2; j += NT) {
        const int c = j % C, r = j / C, cc = r / k2, k = r - cc * k2;
        w2t[j] = th[l.oW2 + (c * C + cc) * k2 + k];
    }
    for (int j = threadIdx.x; j < 7 * C; j += NT) w1t[l.NW1 + j] = w2t[C * C * k2 + j] = 0.f;
    }
    if (w2u)
        for (int j = threadIdx.x; j < C * C * k2; j += NT) {
            const int cc = j % C, r = j / C, c = r % C, k = r / C;
            w2u[j] = th[l.oW2 + (c * C + cc) * k2 + k];
        }
}

// ---- C = 16 (64-QAM): the three convolutions and their weight gradients as GEMMs on v_mfma_f32_16x16x4_f32 -- f32 in, f32 accumulate,
// every output one exact fmaf chain.  Operand maps (cdna_hip_programming.md): A[m = lane & 15][k = lane >> 4], B[k = lane >> 4][n = lane & 15],
// D[m = 4 (lane >> 4) + reg][n = lane & 15].  M is always the 16 channels.
typedef float f32x4 __attribute__((ext_vector_type(4)));

// Sum over the 64 lanes on the vector ALU (DPP row operations + four v_readlane; the row sums as in vaeq_wave.h's wave_sum_dpp): vaeq_common.h's wave_sum is
// a butterfly of six ds_bpermute, i.e. six DEPENDENT LDS round trips -- the BatchNorm statistics take four such sums per channel.  Fixed order.
// (not folded into wave_sum_dpp: that one ends on two DPP broadcasts + one v_readlane, other instructions than these)
__device__ __forceinline__ float wave_sum_fast(float v)
{
    v += dpp_f<0xB1>(v);                                       // quad_perm:[1,0,3,2]
    v += dpp_f<0x4E>(v);                                       // quad_perm:[2,3,0,1]
    v += dpp_f<0x141>(v);                                      // row_half_mirror
    v += dpp_f<0x140>(v);                                      // row_mirror: every lane of a 16-lane row holds the row's sum
    const int b = __builtin_bit_cast(int, v);
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0)), r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32)), r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
    return (r0 + r1) + (r2 + r3);
}
// block_reduce3 (vaeq_common.h) with the wave sums above: results in red[0..2] for every thread; red needs 3 (NT / 64) + 4 floats; ends with a barrier
template <int NT>
__device__ __forceinline__ void nn_block_reduce3(float a, float b, float c, float *red)
{
    constexpr int NW = NT / 64;
    a = wave_sum_fast(a);
    b = wave_sum_fast(b);
    c = wave_sum_fast(c);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[4 + w * 3 + 0] = a; red[4 + w * 3 + 1] = b; red[4 + w * 3 + 2] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
        for (int i = 0; i < NW; i++) { s0 += red[4 + i * 3]; s1 += red[4 + i * 3 + 1]; s2 += red[4 + i * 3 + 2]; }
        red[0] = s0; red[1] = s1; red[2] = s2;
    }
    __syncthreads();
}

// ldsv: a 4-byte LDS read the compiler must leave where the source puts it (vaeq_wave.h, beside lds2).  Used wherever a
// read from a CLAMPED (always valid) address feeds a select: an ordinary load is sunk into a branch of its own behind its own s_waitcnt lgkmcnt(0)
// (the backend will not speculate it), i.e. one exposed LDS round trip per operand -- the pattern round 3 found in the epilogue kernel and, with the ISA
// in hand, here: 35 such branches per tile group of the transposed convolution.
// lds1: the operand reads of the MFMA loops below, an ORDINARY load -- the backend places each read in front of the v_mfma it feeds, and with two waves
// per SIMD that order beats reads pinned ahead of the matrix instructions.  It stays a function: the same loads written in place
// compile to other instruction streams in 34 kernels (tools/compare_isa.py).
__device__ __forceinline__ float lds1(const float *p) { return *p; }

// Conv1d with 16 output channels:  D[c][col] = bias[c] + sum over the (input row, tap) pairs of  w * in[row rstride + tap + col cstep].
// The 4 k-rows of a v_mfma_f32_16x16x4_f32 (lane group lg = lane >> 4) do NOT take four consecutive (row, tap) pairs: each group WALKS ITS OWN
// sequence -- fc1 (2 input rows): group lg owns row lg >> 1 and the taps of half lg & 1; fc2 (16 rows): group lg owns rows 4 lg .. 4 lg + 3, tap by tap
// -- so that the sample offset of k-step t is  lbase(lane) + off(t)  with off(t) THE SAME for all lanes: a scalar (an instruction immediate once the
// shape is baked) instead of per-lane index arithmetic for every operand read.  On gfx950 the f32 MFMA runs on the vector FMA pipe: a vector
// instruction inside the loop does not hide behind the matrix passes, it adds to them (round 2's loop: 22 vector instructions per 10 MFMAs).
//   off(t) walks:  k = t, t + 1, ... ; at k == kdw: k = 0 and the base advances by rstride   (fc1: kdw = INT_MAX: off(t) = t)
//   wt[(4 t + lg) 16 + c] = weight of channel c for the pair group lg reaches at step t (0 where it has none): nn_transpose_weights
// T k-steps (even: a trip = two k-steps; the operands of the next trip are fetched while the current 2 TB MFMAs run).  Columns past ncols (the last
// tile, and tiles past the last one) are READ -- from padded or neighbouring, always finite LDS cells -- and dropped: no clamps.
// out(c0, col, acc): the lane's channels c0 .. c0 + 3 of column col.  LEAN: the k-step loop stays a loop (the half-minibatch kernel of vaeq_nn.hip).
template <int NT, int TB, bool LEAN = false, typename OutF>
__device__ __forceinline__ void mfma_conv16(const float *wt, int T, int lbase, int kdw, int rstride, const float *in, int cstep, int ncols,
                                            const float *bias, OutF out, int creal = 16)
{
    constexpr int NWV = NT / 64;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lc = lane & 15, lg = lane >> 4;
    const int ntile = (ncols + 15) >> 4, K8 = T >> 1;
    // (creal < 16: the channels past it have zero weights and get a zero bias: their outputs are exact zeros)
    const f32x4 b4 = 4 * lg < creal ? *reinterpret_cast<const f32x4 *>(bias + 4 * lg) : f32x4{0.f, 0.f, 0.f, 0.f};
    for (int tg = wv * TB; tg < ntile; tg += NWV * TB) {
        f32x4 acc[TB];
#pragma unroll
        for (int u = 0; u < TB; u++) acc[u] = b4;
        const float *bp = in + lbase + (tg * 16 + lc) * cstep;          // tile u: + 16 u cstep
        int ob = 0, ok = 0;                                             // off(t) = ob + ok (uniform)
        auto ld = [&](int t, float &a, float (&b)[TB]) {
            a = lds1(wt + 64 * t + lane);
#pragma unroll
            for (int u = 0; u < TB; u++) b[u] = lds1(bp + ob + ok + 16 * u * cstep);
            ok++;
            if (ok == kdw) { ok = 0; ob += rstride; }
        };
        float a0, a1, b0[TB], b1[TB];
        ld(0, a0, b0);
        ld(1, a1, b1);
        auto trip = [&](int t2) {
            const float x0 = a0, x1 = a1;
            float y0[TB], y1[TB];
#pragma unroll
            for (int u = 0; u < TB; u++) { y0[u] = b0[u]; y1[u] = b1[u]; }
            const int tn = 2 * t2 + 2;                                  // past the end: the walk simply continues (finite cells), and the 128 floats
                                                                        // behind wt (another LDS array) are fetched; neither is used
            ld(tn, a0, b0);
            ld(tn + 1, a1, b1);
#pragma unroll
            for (int u = 0; u < TB; u++) acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(x0, y0[u], acc[u], 0, 0, 0);
#pragma unroll
            for (int u = 0; u < TB; u++) acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(x1, y1[u], acc[u], 0, 0, 0);
        };
        if constexpr (LEAN) {
#pragma unroll 1
            for (int t2 = 0; t2 < K8; t2++) trip(t2);
        } else {
            for (int t2 = 0; t2 < K8; t2++) trip(t2);
        }
#pragma unroll
        for (int u = 0; u < TB; u++) {
            const int col = (tg + u) * 16 + lc;
            if (col < ncols) out(4 * lg, col, acc[u]);
        }
    }
}
// Weight gradient of such a convolution:  G[c][j] = sum_{r < nrows} g[c gstride + r] * in[(j / kd) rstride + j % kd + r rstep]  for j < J,
// and the bias gradient G[c][J] = sum_r g[c gstride + r] as one more column.  Waves = (column tile, part of the row range); parts are
// combined through `scratch` (cap floats; every thread of the block must make this call: it may hold a barrier).  Four k-steps of
// operands are fetched per trip, four accumulators take them in turn.
// out(c0, j, acc): the lane's channels c0 .. c0 + 3 of column j <= J.
// ROW1: `in` carries a row of ones as row J / kd (J a multiple of kd) and every operand array may be read up to 16 rows past its end: the bias column is
// then a column like any other, the pointers advance unconditionally and the trip count is a scalar -- per four matrix instructions two vector
// instructions instead of twelve (four selects, a guarded pointer advance, an exec-mask loop).  That matters more than it looks: on gfx950 the f32 MFMA
// runs on the vector FMA pipe, so every vector instruction inside an MFMA loop ADDS to the loop's time instead of hiding behind the matrix passes.
template <int NT, bool ROW1 = false, typename OutF>
__device__ __forceinline__ void mfma_wgrad16(const float *g, int gstride, int nrows, const float *in, int rstep, int J, int kd, int rstride,
                                             float *scratch, int cap, OutF out, int zpad = 0, int onesrow = -1)
{
    constexpr int NWV = NT / 64;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lc = lane & 15, lg = lane >> 4;
    const int ntile = (J + 1 + 15) >> 4, ntw = ntile < NWV ? ntile : NWV;
    int nsplit = NWV / ntw;
    if ((nsplit - 1) * ntw * 256 > cap) nsplit = 1 + cap / (ntw * 256);
    const int tile0 = wv % ntw, part = wv / ntw;
    // ROW1: g is ZERO in the zpad rows behind nrows (zero halo / guard cells of its array): when that covers it, the row range is rounded up to whole trips
    // of four k-steps and no part has a ragged last trip (the clamped path below: ~100 instructions and eight serial reads for two or three k-steps)
    if constexpr (ROW1) {
        const int up = (nrows + 15) & ~15;
        if (up - nrows <= zpad) nrows = up;
    }
    const int steps = (nrows + 3) >> 2, sp = (((steps + nsplit - 1) / nsplit) + 3) & ~3;     // k-steps per part, a multiple of 4
    for (int tile = tile0; tile < ntile; tile += ntw) {            // more than one trip only when ntile > NWV (then nsplit == 1)
        f32x4 acc[4];
#pragma unroll
        for (int q = 0; q < 4; q++) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (part < nsplit) {
            const int j = tile * 16 + lc;
            // (ROW1: the bias column J -- and the padding columns behind it, whose results are dropped -- read the row of ones, row `onesrow` of `in`)
            const int jq = j / kd, ji = ROW1 ? (j < J ? jq : (onesrow >= 0 ? onesrow : J / kd)) : (j < J ? jq : 0);
            const int joff = ROW1 ? ji * rstride + (j < J ? j - jq * kd : j - J) : (j < J ? ji * rstride + (j - ji * kd) : 0);
            const bool ones = !ROW1 && j == J;
            const float *gp = g + lc * gstride;
            const int t1 = min(steps, (part + 1) * sp);
            // main trips: four k-steps whose rows all exist -- plain pointer walks, the next trip's operands are fetched while the
            // current four MFMAs run; the (at most one) ragged trip at the end of the row range takes the clamped path below
            const int t0 = part * sp, tfull = nrows >> 2;
            int nmain = max(0, (min(t1, tfull) - t0) >> 2);
            if constexpr (ROW1) nmain = __builtin_amdgcn_readfirstlane(nmain);     // (uniform over the wave: part and tile are)
            const float *pa = gp + 4 * t0 + lg, *pb = in + joff + (4 * t0 + lg) * rstep;
            const int sa = 4, sb = 4 * rstep;
            float an[4], bn[4];
#pragma unroll
            for (int q = 0; q < 4; q++) { an[q] = lds1(pa + q * sa); bn[q] = lds1(pb + q * sb); }       // (in range even when nmain == 0: rows < 4 t0 + 16 <= padded arrays)
            if constexpr (ROW1) {
                // two operand sets alternate (no register copies): trip m + 1 is fetched before trip m's matrix instructions, trip m + 2 before those of m + 1
                float a1[4], b1[4];
                auto mma = [&](const float (&x)[4], const float (&y)[4]) {
#pragma unroll
                    for (int q = 0; q < 4; q++) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[q], y[q], acc[q], 0, 0, 0);
                };
                int m = 0;
                for (; m + 2 <= nmain; m += 2) {
                    pa += 4 * sa; pb += 4 * sb;
#pragma unroll
                    for (int q = 0; q < 4; q++) { a1[q] = lds1(pa + q * sa); b1[q] = lds1(pb + q * sb); }
                    mma(an, bn);
                    pa += 4 * sa; pb += 4 * sb;
#pragma unroll
                    for (int q = 0; q < 4; q++) { an[q] = lds1(pa + q * sa); bn[q] = lds1(pb + q * sb); }   // (past the last trip: read, never used)
                    mma(a1, b1);
                }
                if (m < nmain) mma(an, bn);
            } else
            for (int m = 0; m < nmain; m++) {
                float av[4], bv[4];
#pragma unroll
                for (int q = 0; q < 4; q++) { av[q] = an[q]; bv[q] = ones ? 1.0f : bn[q]; }
                if (m + 1 < nmain) { pa += 4 * sa; pb += 4 * sb; }
#pragma unroll
                for (int q = 0; q < 4; q++) { an[q] = lds1(pa + q * sa); bn[q] = lds1(pb + q * sb); }
#pragma unroll
                for (int q = 0; q < 4; q++) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q], bv[q], acc[q], 0, 0, 0);
            }
            for (int t = t0 + 4 * nmain; t < t1; t += 4) {
                float av[4], bv[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {                      // rows past the end (of the array or of this part): clamped reads, zero gradient
                    const int r = 4 * (t + q) + lg, rb = r < nrows ? r : nrows - 1;
                    const float a_ = ldsv(gp + rb), b_ = ldsv(in + joff + rb * rstep);
                    av[q] = (r < nrows && t + q < t1) ? a_ : 0.f;
                    bv[q] = ones ? 1.0f : b_;
                }
#pragma unroll
                for (int q = 0; q < 4; q++) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q], bv[q], acc[q], 0, 0, 0);
            }
            acc[0] += acc[1]; acc[2] += acc[3]; acc[0] += acc[2];
            if (part > 0) {
                float *sp_ = scratch + ((part - 1) * ntw + tile0) * 256 + lane;
                sp_[0] = acc[0].x; sp_[64] = acc[0].y; sp_[128] = acc[0].z; sp_[192] = acc[0].w;
            }
        }
        if (nsplit > 1) __syncthreads();
        if (part == 0) {
            for (int q = 1; q < nsplit; q++) {
                const float *sp_ = scratch + ((q - 1) * ntw + tile0) * 256 + lane;
                acc[0].x += sp_[0]; acc[0].y += sp_[64]; acc[0].z += sp_[128]; acc[0].w += sp_[192];
            }
            const int j = tile * 16 + lc;
            if (j <= J) out(4 * lg, j, acc[0]);
        }
    }
}

// Backward through the strided Conv1d fc2 (16 -> 16 channels):  gz[cc][s] = sum_{c, k : (s + p2 - k) % sps == 0} w2u[(k 16 + c) 16 + cc] * g2[c GS + (s + p2 - k) / sps],
// one polyphase component of s at a time (for each only every sps-th tap contributes).  g2 = dL/dlogits in the ZERO-GUARDED layout of nn_layout (row
// stride GS, columns -A0 .. 16 ceil(B / 16) + A0 - 1 readable, zeros outside [0, B)): every operand read is unconditional, the operands of
// the next tap are in flight while the current tap's 4 TB matrix instructions run, and the epilogue reads what it needs of the old buffer (pre) for
// all its outputs before it writes any (post) -- round 2's form had each of these reads in a branch of its own behind its own s_waitcnt lgkmcnt(0)
// (35 exposed LDS round trips per tile group: 4.1 us for 0.8 us of matrix passes).
template <int NT, int TB, typename PreF, typename PostF>
__device__ __forceinline__ void mfma_convT16(const float *w2u, int k2, int p2, int sps, const float *g2, int GS, int L, PreF pre, PostF post)
{
    constexpr int NWV = NT / 64;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lc = lane & 15, lg = lane >> 4;
    for (int ph = 0; ph < sps; ph++) {
        const int kf = (ph + p2) % sps, nk = kf < k2 ? (k2 - kf + sps - 1) / sps : 0;
        const int ncols = (L - ph + sps - 1) / sps, ntile = (ncols + 15) >> 4;      // columns m: s = sps m + ph
        for (int tg = wv * TB; tg < ntile; tg += NWV * TB) {
            f32x4 acc[TB];
#pragma unroll
            for (int u = 0; u < TB; u++) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            const float *gb = g2 + lg * GS + tg * 16 + lc;                          // + 4 cb GS + 16 u + nsh
            const float *wb = w2u + lg * 16 + lc;                                   // + (k 16 + 4 cb) 16
            float av[2][4], bv[2][4][TB];
            auto ld = [&](int kj, float (&a_)[4], float (&b_)[4][TB]) {
                const int k = kf + kj * sps, nsh = (ph + p2 - k) / sps;             // exact division (may be negative)
#pragma unroll
                for (int cb = 0; cb < 4; cb++) {
                    a_[cb] = lds1(wb + (k * 16 + 4 * cb) * 16);
#pragma unroll
                    for (int u = 0; u < TB; u++) b_[cb][u] = lds1(gb + 4 * cb * GS + 16 * u + nsh);
                }
            };
            auto mm = [&](const float (&a_)[4], const float (&b_)[4][TB]) {
#pragma unroll
                for (int cb = 0; cb < 4; cb++)
#pragma unroll
                    for (int u = 0; u < TB; u++) acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_[cb], b_[cb][u], acc[u], 0, 0, 0);
            };
            if (nk > 0) ld(0, av[0], bv[0]);
            for (int kj = 0; kj < nk; kj += 2) {                                     // two register sets alternate (no copies)
                if (kj + 1 < nk) ld(kj + 1, av[1], bv[1]);
                mm(av[0], bv[0]);
                if (kj + 1 < nk) {
                    if (kj + 2 < nk) ld(kj + 2, av[0], bv[0]);
                    mm(av[1], bv[1]);
                }
            }
            float old[TB][4];
#pragma unroll
            for (int u = 0; u < TB; u++) {
                const int m = (tg + u) * 16 + lc, mc = m < ncols ? m : ncols - 1;
#pragma unroll
                for (int t = 0; t < 4; t++) old[u][t] = pre(4 * lg + t, sps * mc + ph);
            }
#pragma unroll
            for (int u = 0; u < TB; u++) {
                const int m = (tg + u) * 16 + lc;
                const float gg[4] = {acc[u].x, acc[u].y, acc[u].z, acc[u].w};
                if (m < ncols) {
#pragma unroll
                    for (int t = 0; t < 4; t++) post(4 * lg + t, sps * m + ph, gg[t], old[u][t]);
                }
            }
        }
    }
}

// The same for the samples s in [s_lo, s_lo + s_cnt) only (s_lo a multiple of sps): the half-minibatch kernel below.  out(cc0, s, acc) with the absolute s.
template <int NT, int TB, typename OutF>
__device__ __forceinline__ void mfma_convT16_range(const float *w2u, int k2, int p2, int sps, const float *g2, int B, int s_lo, int s_cnt, OutF out)
{
    constexpr int NWV = NT / 64;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lc = lane & 15, lg = lane >> 4;
    const int m_lo = s_lo / sps;
    for (int ph = 0; ph < sps; ph++) {
        const int kf = (ph + p2) % sps, nk = kf < k2 ? (k2 - kf + sps - 1) / sps : 0;
        const int ncols = (s_cnt - ph + sps - 1) / sps, ntile = (ncols + 15) >> 4;
        for (int tg = wv * TB; tg < ntile; tg += NWV * TB) {
            f32x4 acc[TB];
#pragma unroll
            for (int u = 0; u < TB; u++) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int kj = 0; kj < nk; kj++) {
                const int k = kf + kj * sps, nsh = (ph + p2 - k) / sps;             // exact division (may be negative)
                float av[4], bv[4][TB];
#pragma unroll
                for (int cb = 0; cb < 4; cb++) {
                    const int c = 4 * cb + lg;
                    av[cb] = w2u[(k * 16 + c) * 16 + lc];
#pragma unroll
                    for (int u = 0; u < TB; u++) {
                        const int n = m_lo + (tg + u) * 16 + lc + nsh, nc = n < 0 ? 0 : (n < B ? n : B - 1);
                        const float b_ = g2[c * B + nc];
                        bv[cb][u] = (n >= 0 && n < B) ? b_ : 0.f;
                    }
                }
#pragma unroll
                for (int cb = 0; cb < 4; cb++)
#pragma unroll
                    for (int u = 0; u < TB; u++) acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[cb], bv[cb][u], acc[u], 0, 0, 0);
            }
#pragma unroll
            for (int u = 0; u < TB; u++) {
                const int m = (tg + u) * 16 + lc;
                if (m < ncols) out(4 * lg, sps * (m_lo + m) + ph, acc[u]);
            }
        }
    }
}

// ---- forward on one LDS-resident window: xs (zero-haloed input) -> z1 (ELU output, zero-haloed) -> a2 (logits).
// item = (channel quad, sample): consecutive lanes take consecutive samples (conflict-free x reads and z1 writes), the four
// channels' weights of a tap come from one 16-byte broadcast read.
template <int NT, int NLEV, bool LEAN = false>
__device__ __forceinline__ void nn_fc1_elu(const NNLayout &l, int k1, const float *xs, const float *th, const float *w1t, float *z1, int Lvalid,
                                           int zlo, int zhi, const float *aff = nullptr)
{
    // z1p[c][p2 + s] for s in [0, Lvalid); entries whose absolute position (zlo + s) lies outside [0, zhi) are fc2's zero padding
    constexpr int C = 2 * NLEV, CQ = C / 4;
    if constexpr (nn_mf(NLEV)) {
        const int lg = (threadIdx.x & 63) >> 4;
        mfma_conv16<NT, (NT >= 1024 ? 2 : 5), LEAN>(w1t, conv16_fc1_steps(k1), (lg >> 1) * l.Lx + (lg & 1) * ((k1 + 1) / 2), 0x7fffffff, 0, xs, 1, Lvalid, th + l.oB1, [&](int c0, int sy, f32x4 acc) {
            const int pos = zlo + sy;
            const bool in = pos >= 0 && pos < zhi;
            const float av[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
            for (int t = 0; t < 4; t++) {
                float z = av[t] > 0.f ? av[t] : __expf(av[t]) - 1.0f;                     // F.elu, alpha = 1 (:177)
                if (aff && c0 + t < C) z = fmaf(aff[c0 + t], z, aff[C + c0 + t]);         // eval-mode BatchNorm: running statistics folded
                z1[(c0 + t) * l.Lz + l.p2 + sy] = in ? z : 0.f;                           // (rows past C: ELU(0) = 0)
            }
        }, C);
        return;
    }
    typedef float v2f __attribute__((ext_vector_type(2)));     // channel pairs: every MAC below is a v_pk_fma_f32
    const int H = (Lvalid + 1) / 2;                            // a thread takes samples sx and sx + H: one weight read feeds 8 MACs
    for (int it = threadIdx.x; it < CQ * H; it += NT) {
        const int cq = it / H, sx = it - cq * H;
        const float4 b = *reinterpret_cast<const float4 *>(th + l.oB1 + 4 * cq);
        v2f a01 = {b.x, b.y}, a23 = {b.z, b.w}, c01 = a01, c23 = a23;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const float *xp = xs + i * l.Lx + sx;              // out[s] = sum_k w[k] x[s + k - p1]: the haloed index of x[s + k - p1] is s + k
            const float4 *w = reinterpret_cast<const float4 *>(w1t + (i * k1) * C + 4 * cq);
            for (int k = 0; k < k1; k++) {
                const float xv = xp[k], xw = xp[H + k];
                const float4 w4 = w[k * CQ];
                const v2f w01 = {w4.x, w4.y}, w23 = {w4.z, w4.w};
                a01 += w01 * xv; a23 += w23 * xv;
                c01 += w01 * xw; c23 += w23 * xw;
            }
        }
        const float av[2][4] = {{a01.x, a01.y, a23.x, a23.y}, {c01.x, c01.y, c23.x, c23.y}};
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int sy = sx + u * H;
            if (sy >= Lvalid) continue;
            const int pos = zlo + sy;
            const bool in = pos >= 0 && pos < zhi;
#pragma unroll
            for (int t = 0; t < 4; t++) {
                float z = av[u][t] > 0.f ? av[u][t] : __expf(av[u][t]) - 1.0f;           // F.elu, alpha = 1 (:177)
                if (aff) z = fmaf(aff[4 * cq + t], z, aff[C + 4 * cq + t]);              // eval-mode BatchNorm: running statistics folded
                z1[(4 * cq + t) * l.Lz + l.p2 + sy] = in ? z : 0.f;
            }
        }
    }
}

template <int NT, int NLEV, bool LEAN = false>
__device__ __forceinline__ void nn_fc2(const NNLayout &l, int sps, int k2, int Bt, int astride, const float *z1, const float *th, const float *w2t,
                                       float *a2)
{
    constexpr int C = 2 * NLEV, CQ = C / 4;
    if constexpr (nn_mf(NLEV)) {
        const int lg = (threadIdx.x & 63) >> 4;
        mfma_conv16<NT, (NT >= 1024 ? 1 : 3), LEAN>(w2t, conv16_fc2_steps(k2), 4 * lg * l.Lz, k2, l.Lz, z1, sps, Bt, th + l.oB2, [&](int c0, int n, f32x4 acc) {
            a2[(c0 + 0) * astride + n] = acc.x; a2[(c0 + 1) * astride + n] = acc.y;
            a2[(c0 + 2) * astride + n] = acc.z; a2[(c0 + 3) * astride + n] = acc.w;
        }, C);
        return;
    }
    typedef float v2f __attribute__((ext_vector_type(2)));
    const int H = (Bt + 1) / 2;
    for (int it = threadIdx.x; it < CQ * H; it += NT) {
        const int cq = it / H, n = it - cq * H;
        const float4 b = *reinterpret_cast<const float4 *>(th + l.oB2 + 4 * cq);
        v2f a01 = {b.x, b.y}, a23 = {b.z, b.w}, c01 = a01, c23 = a23;
        const float4 *w = reinterpret_cast<const float4 *>(w2t + 4 * cq);
        for (int cc = 0; cc < C; cc++) {
            const float *zp = z1 + cc * l.Lz + n * sps;        // z1[n sps + k - p2] -> haloed index n sps + k
            for (int k = 0; k < k2; k++) {
                const float zv = zp[k], zw = zp[H * sps + k];
                const float4 w4 = w[(cc * k2 + k) * CQ];
                const v2f w01 = {w4.x, w4.y}, w23 = {w4.z, w4.w};
                a01 += w01 * zv; a23 += w23 * zv;
                c01 += w01 * zw; c23 += w23 * zw;
            }
        }
        a2[(4 * cq + 0) * astride + n] = a01.x; a2[(4 * cq + 1) * astride + n] = a01.y;
        a2[(4 * cq + 2) * astride + n] = a23.x; a2[(4 * cq + 3) * astride + n] = a23.y;
        if (n + H < Bt) {
            a2[(4 * cq + 0) * astride + n + H] = c01.x; a2[(4 * cq + 1) * astride + n + H] = c01.y;
            a2[(4 * cq + 2) * astride + n + H] = c23.x; a2[(4 * cq + 3) * astride + n + H] = c23.y;
        }
    }
}

// ---- eval-mode forward over N symbols in tiles (validation, :293-301): q[R][C][N]
constexpr int NN_TILE = 255;                           // symbols per tile: (255 - 1) sps + k2 = 511 z1 samples at sps = 2, k2 = 3 -> 32 MFMA column tiles = 2 per wave of 1024 threads

template <int NT, int NLEV>
__device__ __forceinline__ void nn_forward_tile(const NNLayout &l, int sps, int k1, int k2, int64_t Ltot, const float *x0, const float *x1,
                                                int n0, int Bt, float *xs, float *z1, float *a2, const float *th, const float *w1t, const float *w2t,
                                                const float *aff = nullptr)
{
    // tile symbols n0 .. n0+Bt-1: z1 needed at absolute positions [n0 sps - p2, (n0+Bt-1) sps + k2 - p2), x p1 beyond that on both sides
    const int tid = threadIdx.x, p1 = l.p1, p2 = l.p2;
    const int zlo = n0 * sps - p2, Lz_need = (Bt - 1) * sps + k2, xlo = zlo - p1, Lx_need = Lz_need + 2 * p1;
    for (int i = tid; i < 2 * (Lx_need + 4); i += NT) {
        const int row = i / (Lx_need + 4), c = i - row * (Lx_need + 4);
        const int64_t sx = (int64_t)xlo + c;
        xs[row * l.Lx + c] = (c < Lx_need && sx >= 0 && sx < Ltot) ? (row ? x1[sx] : x0[sx]) : 0.f;
    }
    __syncthreads();
    // fc1 writes z1p[c][p2 + s] for s in [0, Lz_need) with absolute position zlo + s: shift the base so that p2 + s -> s
    nn_fc1_elu<NT, NLEV>(l, k1, xs, th, w1t, z1 - p2, Lz_need, zlo, (int)Ltot, aff);
    __syncthreads();
    nn_fc2<NT, NLEV>(l, sps, k2, Bt, NN_TILE, z1, th, w2t, a2);   // haloed index of z1[n sps + k - p2] relative to zlo is n sps + k
    __syncthreads();
}

}  // namespace vaeq
