// vaeq_awgn_wave.hip -- wave-per-run fast path of the single-polarisation (AWGN / ISI channel) VAE-LE training loop (gfx950).
//
// Same math as vaeq_awgn.hip (AWGN_channel/func_VAELE_MQAM_shaping.py: twoFIR.forward :214-231, loss_function :63-95,
// Adam(amsgrad=True) :283) and the same mapping ideas as vaeq_dp_wave.hip, with two differences:
//   * minibatches are longer (350 symbols in the reference's sweep), so a lane owns one symbol PAIR PER ROUND, NR = ceil(B/128)
//     rounds; the convolution-shaped phases walk the taps once and feed all rounds from each tap read;
//   * the equaliser output is normalised to the constellation's mean amplitude before the demapper (:228), which adds a
//     wave-wide sum of |y| on the way forward and its Jacobian (one more dot product) on the way back.
// The tap gradients dL/dw[k], dL/dh[j] are summed by threads = (group of 4 taps, part of the sum range) (TapBlocks below); lane (k, half 0) of
// wave 0 owns w[k], lane (j, half 1) owns h[j]: parameter, Adam first/second moment and AMSGrad maximum all live in that lane's registers.
//
// Supported here: sps == 2, B even, 2*(M/2)+2 <= B <= 1024, M in {9, 17, 25}; everything else takes the generic kernel.
// B <= 384: one wavefront per run (NR <= 3 rounds; more rounds spill); 384 < B <= 1024: two to four wavefronts x two rounds.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "vaeq.h"
#include "vaeq_common.h"
#include "vaeq_launch.h"
#include "vaeq_wave.h"

#ifndef VAEQ_AWGN_BAKED_FULL
#define VAEQ_AWGN_BAKED_FULL 1
#endif

namespace vaeq {

struct AwgnWaveLayout {
    int Lph, Uph;
    int X, E, U, PSv, W, H, PSh, VS, XP, RED, total;   // byte offsets (the dL/dy buffer aliases U)
};

__host__ __device__ inline AwgnWaveLayout awgn_wave_layout(int B, int M, int NW = 1)
{
    AwgnWaveLayout l;
    l.Lph = wave_lph(2 * B + M - 1);
    l.Uph = B / 2 + 1;
    int o = 0;
    auto take = [&](int bytes) { int r = o; o += (bytes + 15) & ~15; return r; };
    l.X = take(4 * l.Lph * 8);
    l.E = take(4 * l.Lph * 8);
    const int ubytes = 2 * l.Uph * 8, gbytes = B * 8;
    l.U = take(ubytes > gbytes ? ubytes : gbytes);
    l.PSv = take((B + 1) * 4);
    l.W = take(M * 8);
    l.H = take((M + 1) * 8);                           // one zero pad tap: j = M
    l.PSh = take((M + 1) * 4);
    l.VS = take(M * 4);
    l.XP = take(256 * NW * 8);                         // partial tap-gradient sums [group][tap in group][part] (complex): 4 per thread
    l.RED = take(NW > 1 ? 64 * 4 : 0);                 // NW > 1: cross-wave sums and scan offsets
    l.total = o;
    return l;
}

// acc[r][sym] = sum_k taps[k] (x) x_r[2*sym + k] for the symbol pair of every round; xp[r] = the lane's phase-0 pointer in round r.
// With up to two rounds per lane: the first tap group starts the accumulators and the 8-byte LDS reads stay ds_read_b64 (lds2): +4 % at B = 512.  With
// three rounds the kernel is register-starved and that form costs more in spills than it saves (43 spilled dwords, -8 % at B = 350): round 1's form there.
template <int M, int NR, bool LEAN = (NR >= 3)>
__device__ __forceinline__ void wave_fir(cacc (&acc)[NR][2], const float2 *(&xp)[NR], int Lph, const float2 *taps)
{
    if constexpr (LEAN) {                           // register-starved (three rounds per lane): zeroed accumulators, ordinary loads
#pragma unroll
        for (int r = 0; r < NR; r++) acc[r][0] = acc[r][1] = cacc0();
        constexpr int G = M / 4;
    #pragma unroll 1
        for (int g = 0; g < G; g++) {                      // taps 4g..4g+3, samples c' = 4g..4g+5
            const float2 t0 = taps[4 * g], t1 = taps[4 * g + 1], t2 = taps[4 * g + 2], t3 = taps[4 * g + 3];
    #pragma unroll
            for (int r = 0; r < NR; r++) {
                const float2 *xg = xp[r] + g;
                const float2 x0 = xg[0], x1 = xg[Lph], x2 = xg[2 * Lph], x3 = xg[3 * Lph], x4 = xg[1], x5 = xg[Lph + 1];
                cmac(acc[r][0], t0.x, t0.y, x0); cmac(acc[r][1], t0.x, t0.y, x2);
                cmac(acc[r][0], t1.x, t1.y, x1); cmac(acc[r][1], t1.x, t1.y, x3);
                cmac(acc[r][0], t2.x, t2.y, x2); cmac(acc[r][1], t2.x, t2.y, x4);
                cmac(acc[r][0], t3.x, t3.y, x3); cmac(acc[r][1], t3.x, t3.y, x5);
            }
        }
    #pragma unroll
        for (int k = 4 * G; k < M; k++) {                  // remaining 1 or 3 taps
            const float2 t = taps[k];
    #pragma unroll
            for (int r = 0; r < NR; r++) {
                cmac(acc[r][0], t.x, t.y, xp[r][(k & 3) * Lph + (k >> 2)]);
                cmac(acc[r][1], t.x, t.y, xp[r][((k + 2) & 3) * Lph + ((k + 2) >> 2)]);
            }
        }
    } else {
        constexpr int G = M / 4;
        auto group = [&](int g, auto first) {              // taps 4g..4g+3, samples c' = 4g..4g+5
            constexpr bool F = decltype(first)::value;
            const v2f t0 = lds2(taps + 4 * g), t1 = lds2(taps + 4 * g + 1), t2 = lds2(taps + 4 * g + 2), t3 = lds2(taps + 4 * g + 3);
    #pragma unroll
            for (int r = 0; r < NR; r++) {
                const float2 *xg = xp[r] + g;
                const v2f x0 = lds2(xg), x1 = lds2(xg + Lph), x2 = lds2(xg + 2 * Lph), x3 = lds2(xg + 3 * Lph), x4 = lds2(xg + 1), x5 = lds2(xg + Lph + 1);
                cmacf<F>(acc[r][0], t0, x0); cmacf<F>(acc[r][1], t0, x2);
                cmac(acc[r][0], t1, x1); cmac(acc[r][1], t1, x3);
                cmac(acc[r][0], t2, x2); cmac(acc[r][1], t2, x4);
                cmac(acc[r][0], t3, x3); cmac(acc[r][1], t3, x5);
            }
        };
        group(0, std::true_type{});
    #pragma unroll 1
        for (int g = 1; g < G; g++) group(g, std::false_type{});
    #pragma unroll
        for (int k = 4 * G; k < M; k++) {                  // remaining 1 or 3 taps
            const v2f t = lds2(taps + k);
    #pragma unroll
            for (int r = 0; r < NR; r++) {
                cmac(acc[r][0], t, lds2(xp[r] + (k & 3) * Lph + (k >> 2)));
                cmac(acc[r][1], t, lds2(xp[r] + ((k + 2) & 3) * Lph + ((k + 2) >> 2)));
            }
        }
    }
}

// Blocked tap-gradient sums.  A thread = (group of 4 taps, part of the sum range): per pair of terms it
// reads 7 (dL/dh) / 8 (dL/dw) operands for 8 complex MACs -- the (tap, half) mapping of the DP kernel feeds ONE MAC per operand pair here
// (one polarisation), i.e. one LDS read per packed FMA and 4 x the loop trips.  NG groups x PARTS parts <= 64 NW threads; trip counts are uniform
// (a scalar loop), terms past the end of a part's range are masked.  The partial sums go through LDS (XP); the tap's owner lane adds its
// PARTS partials in a fixed order: bitwise reproducible.
//
// Bank conflicts (tools/lds_bank_model.py restates the loops' addresses): a part starts `trips` symbol pairs after the previous one, and with
// lane = group * parts + part both 32-lane halves of a wave hold parts whose operand windows alias the same banks -- at M = 25, B = 350
// (7 groups x 9 parts x 19 / 20 trips) the 7 + 8 operand reads of a trip take 26 + 36 half-wave passes instead of 14 + 16: that is the kernel's
// 33 % LDS conflict rate.  CF ("conflict-free", -DVAEQ_AWGN_CF=1; B = 350 baked only): 8 parts, parts 0..3 in the first half-wave and 4..7 in the
// second, 23 (dL/dh) / 24 (dL/dw) trips per part -- strides of 46 / 48 dwords put the four 14-dword windows of a half-wave on disjoint banks --
// and dL/dy stored planar (even / odd symbols): every read one pass per half-wave, 42 % fewer LDS passes, 21 % more trips.  MEASURED SLOWER
// (2.78 vs 2.66 ms per 8192 runs x 30 steps, three alternations on one box, profiles/r03/awgn_conflict_free_blocks_ab.txt): the two phases are
// bound by their packed FMAs, not by LDS -- the conflicts hide behind the arithmetic, the extra trips do not.  Off.
#ifndef VAEQ_AWGN_CF
#define VAEQ_AWGN_CF 0
#endif
template <int M, int NW, int BL = 0> struct TapBlocks {
    static constexpr int mh = M / 2;
    static constexpr bool CF = VAEQ_AWGN_CF && M == 25 && NW == 1 && BL == 350;
    static constexpr int NG0 = (mh + 1 + 3) / 4, NG1 = (mh + 3) / 4;     // dL/dh: groups of even taps (a = 0..mh) / odd taps (a = 0..mh-1)
    static constexpr int NGH = NG0 + NG1, PH = CF ? 8 : 64 * NW / NGH;   // parts per group (all NW waves of the run take part)
    static constexpr int NGW = (M + 3) / 4, PW = CF ? 8 : 64 * NW / NGW; // dL/dw: groups of 4 consecutive taps
    static constexpr int NITH = 23, NITW = 24;                           // CF: trips per part
    // thread -> (group, part); lanes without a block shadow a working lane of their own half-wave (same address: a broadcast, no extra pass)
    static __device__ __forceinline__ void map(int gl, int NG, int P, int &grp, int &prt, bool &gv)
    {
        if constexpr (CF) {
            const int hw = gl >> 5, li = gl & 31, pp = li / NG;
            gv = pp < 4;
            grp = gv ? li - pp * NG : 0;
            prt = 4 * hw + (gv ? pp : 0);
        } else {
            grp = gl / P; prt = gl - grp * P;
            gv = grp < NG;
            if (!gv) grp = 0;
        }
    }
};

// NW = wavefronts per run (1: no barriers; 2..4 for B > 384, see vaeq_dp_wave_kernel.h): wave wv owns the pairs 64 NR wv + 64 r + lane.
// BL > 0: the minibatch length baked into the kernel (LDS offsets immediate, trip counts constant)
template <int M, int NLEV, int NR, int NW = 1, int BL = 0>
__global__ __launch_bounds__(64 * NW, 2) void awgn_wave_kernel(const vaeq_awgn_args a)
{
    constexpr int mh = M / 2, Mh = 2 * mh;
    constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;
    extern __shared__ float4 smem4[];
    char *sm = reinterpret_cast<char *>(smem4);
    const int gl = threadIdx.x, lane = NW > 1 ? (gl & 63) : gl, wv = NW > 1 ? (gl >> 6) : 0, run = blockIdx.x;
    const int l0 = lane + 64 * NR * wv;                       // first pair of this lane
    constexpr int NT = 64 * NW;
    constexpr bool LEAN = NR >= 3 && !(BL && VAEQ_AWGN_BAKED_FULL);   // three rounds per lane are register-starved unless the shape is baked
    const int B = BL ? BL : a.B, L = 2 * B, nm = L - Mh, P2 = B / 2, nq = (nm + 3) / 4;
    const float rB = 1.0f / (float)B;
    const AwgnWaveLayout lay = awgn_wave_layout(B, M, NW);
    const int Lph = lay.Lph, Uph = lay.Uph;
    float2 *Xs = reinterpret_cast<float2 *>(sm + lay.X), *Es = reinterpret_cast<float2 *>(sm + lay.E);
    float2 *Us = reinterpret_cast<float2 *>(sm + lay.U), *GY = Us;
    float2 *Wt = reinterpret_cast<float2 *>(sm + lay.W);       // [k] = (W0[k], -W1[k]): y = sum_k Wt[k] * x   (w = W0 - j W1)
    float2 *Ht = reinterpret_cast<float2 *>(sm + lay.H);       // [j] = (re, im), j = 0..M (j = M: zero pad)
    float *PSv = reinterpret_cast<float *>(sm + lay.PSv);      // [B+1] exclusive prefix sums of v_I + v_Q
    float *PSh = reinterpret_cast<float *>(sm + lay.PSh);      // [M+1] exclusive prefix sums of gC |h_j|^2
    float *VS = reinterpret_cast<float *>(sm + lay.VS);        // [M]
    float *RED = reinterpret_cast<float *>(sm + lay.RED);      // NW > 1 only

    float amp[NLEV], nlogP[NLEV];
#pragma unroll
    for (int i = 0; i < NLEV; i++) {
        amp[i] = a.amp[i];
        nlogP[i] = -logf(a.P[(size_t)run * NLEV + i]);
    }
    const float A = a.amp_mean[run], var = a.var[run];
    const float c2 = LOG2E / var, ivar2 = 2.0f / var;          // z_i = -(yhat - a_i)^2 / var: no 1/2, no PCS term (:229)
    const float lr = a.lr[run];

    // All of it, the padding between the arrays and XP included: the blocked tap-gradient loops below run uniform trip counts and read their U / x
    // operands past a part's range (up to PH / PW pairs beyond U, which at B < 128 is past PSv, into the pads of W, PSh, VS and into XP); the
    // terms are masked by a zero e / gy factor, and 0 * (NaN left in LDS by an earlier kernel) is NaN.
    for (int i = gl; i < lay.total / 8; i += NT) Xs[i] = make_float2(0.f, 0.f);           // X, E, U, PSv, W, H (incl. the pad tap), PSh, VS, XP, RED
    __syncthreads();
    const int tk = lane & 31, half = lane >> 5;
    const bool worker = tk < M, owner = worker && wv == 0, wown = owner && half == 0, hown = owner && half == 1;
    const size_t g0 = (size_t)run * 2 * M + tk, g1 = g0 + M;
    float p0 = 0.f, p1 = 0.f, am0 = 0.f, am1 = 0.f, av0 = 0.f, av1 = 0.f, ax0 = 0.f, ax1 = 0.f;   // parameter pair + Adam state
    {
        float *pp = half ? a.h : a.W, *pm = half ? a.adam_mh : a.adam_mW, *pv = half ? a.adam_vh : a.adam_vW,
              *px = half ? a.adam_xh : a.adam_xW;
        if (owner) {
            p0 = pp[g0]; p1 = pp[g1];
            am0 = pm[g0]; am1 = pm[g1];
            av0 = pv[g0]; av1 = pv[g1];
            ax0 = px[g0]; ax1 = px[g1];
            if (half) Ht[tk] = make_float2(p0, p1); else Wt[tk] = make_float2(p0, -p1);
        }
    }
    int step = a.step[run];
    double b1t = pow(0.9, (double)step), b2t = pow(0.999, (double)step);
    __syncthreads();

    const size_t No = (size_t)a.steps * B;
    float *qf = a.q_out ? a.q_out + (size_t)run * 2 * NLEV * No : nullptr;
    float *yf = a.y_out ? a.y_out + (size_t)run * 2 * No : nullptr;
    bool act[NR], qa[NR];
    const float2 *xp[NR], *ep[NR], *up[NR], *xq[NR];
#pragma unroll
    for (int r = 0; r < NR; r++) {
        const int pr = l0 + 64 * r;
        act[r] = pr < P2;                                      // lane owns symbols 2 pr, 2 pr + 1 in round r
        qa[r] = pr < nq;                                       // ... and the residual quad t = 4 pr .. 4 pr + 3
        xp[r] = Xs + (act[r] ? pr : 0);                        // idle lanes shadow lane 0 (reads stay inside the arrays)
        ep[r] = Es + (act[r] ? pr : 0);
        up[r] = Us + (qa[r] ? pr : 0);
        xq[r] = Xs + (qa[r] ? pr : 0);
    }

    // the window of the NEXT step is fetched into registers while the current step computes
    // (buffer loads: a lane without a symbol pair passes an out-of-range offset and reads zeros.  As `act ? *p : 0` every one of the 2 NR loads sat in an
    //  exec-masked branch of its own with an s_waitcnt vmcnt(0) directly behind it -- the "prefetch" was 2 NR serial HBM round trips in the middle of the step)
    float4 pf[NR][2];
    const __amdgpu_buffer_rsrc_t xr = make_rsrc(a.rx + (size_t)run * 2 * (size_t)a.S, (uint32_t)(2 * a.S) * 4u);
    auto fetch = [&](int s) {
        const uint32_t vo = ((uint32_t)s * (uint32_t)L + 4u * (uint32_t)l0) * 4u;
#pragma unroll
        for (int r = 0; r < NR; r++)
#pragma unroll
            for (int row = 0; row < 2; row++)
                pf[r][row] = bld128(xr, act[r] ? vo + 1024u * (uint32_t)r : OOB, (uint32_t)row * (uint32_t)a.S * 4u);
    };
    fetch(0);
#pragma unroll 1
    for (int s = 0; s < a.steps; s++) {
        // ============ P0: prefetched window -> LDS (polyphase scatter; halo stays zero)
#pragma unroll
        for (int r = 0; r < NR; r++) {
            if (act[r]) {
                const float4 I4 = pf[r][0], Q4 = pf[r][1];
                const float xi[4] = {I4.x, I4.y, I4.z, I4.w}, xq_[4] = {Q4.x, Q4.y, Q4.z, Q4.w};
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int c = mh + i;                      // + 4*pr: phase (c & 3) is lane independent
                    Xs[(c & 3) * Lph + l0 + 64 * r + (c >> 2)] = make_float2(xi[i], xq_[i]);
                }
            }
        }
        sync_lds<NW>();

        // ============ P1: FIR for the lane's symbol pairs; mean |y| per axis (:228)
        float2 y[NR][2];
        {
            cacc ya[NR][2];
            wave_fir<M, NR, LEAN>(ya, xp, Lph, Wt);
#pragma unroll
            for (int r = 0; r < NR; r++)
#pragma unroll
                for (int sy = 0; sy < 2; sy++) {
                    const float2 v = cfin(ya[r][sy]);
                    y[r][sy] = act[r] ? v : make_float2(0.f, 0.f);
                }
        }
        float sa0 = 0.f, sa1 = 0.f;
#pragma unroll
        for (int r = 0; r < NR; r++) {
            asm volatile("" : "+v"(y[r][0].x), "+v"(y[r][0].y), "+v"(y[r][1].x), "+v"(y[r][1].y));   // pin (see vaeq_dp_wave.hip)
            sa0 += fabsf(y[r][0].x) + fabsf(y[r][1].x);
            sa1 += fabsf(y[r][0].y) + fabsf(y[r][1].y);
            if (yf && act[r]) {                                // un-normalised output (:227,231)
                float *rI = yf + (size_t)s * B + 2 * (l0 + 64 * r);
                *reinterpret_cast<float2 *>(rI) = make_float2(y[r][0].x, y[r][1].x);
                *reinterpret_cast<float2 *>(rI + No) = make_float2(y[r][0].y, y[r][1].y);
            }
        }
        float sav[2] = {wave_sum_dpp(sa0), wave_sum_dpp(sa1)};     // DPP sums / scans: no LDS round trips (see vaeq_wave.h)
        waves_sum<NW, 2>(sav, RED, lane, wv);
        // uniform scalars: hardware reciprocals (1 ulp) instead of IEEE division sequences executed by every lane
        const float m0 = sav[0] * rB, m1 = sav[1] * rB;
        const float sc0 = A * __builtin_amdgcn_rcpf(m0), sc1 = A * __builtin_amdgcn_rcpf(m1);

        // ============ P2: soft demap + moments (registers), mu -> LDS, prefix sums of the variances
        float mv[NR][2][2], mt3[NR][2][2], mkc[NR][2][2];      // [round][sym][c]
        float klsum = 0.f, vv[NR][2];
#pragma unroll
        for (int r = 0; r < NR; r++) {
            const int n0 = 2 * (l0 + 64 * r);
            const bool inr0 = (n0 >= mh) && (n0 < B - mh) && act[r];                  // KL slice (:91)
            const bool inr1 = (n0 + 1 >= mh) && (n0 + 1 < B - mh) && act[r];
            float2 muv[2];
#pragma unroll
            for (int c = 0; c < 2; c++) {
                const v2f yy = (c ? v2f{y[r][0].y, y[r][1].y} : v2f{y[r][0].x, y[r][1].x}) * (c ? sc1 : sc0);
                v2f z[NLEV], q[NLEV];
                float zm0 = -3.0e38f, zm1 = -3.0e38f;
#pragma unroll
                for (int i = 0; i < NLEV; i++) {
                    const v2f d = yy - amp[i];
                    z[i] = -(d * d * c2);
                    zm0 = fmaxf(zm0, z[i].x);
                    zm1 = fmaxf(zm1, z[i].y);
                }
                const v2f zmax = {zm0, zm1};
                v2f ssum = {0.f, 0.f};
#pragma unroll
                for (int i = 0; i < NLEV; i++) {
                    z[i] -= zmax;
                    q[i] = v2f{__builtin_amdgcn_exp2f(z[i].x), __builtin_amdgcn_exp2f(z[i].y)};
                    ssum += q[i];
                }
                const v2f rs = {__builtin_amdgcn_rcpf(ssum.x), __builtin_amdgcn_rcpf(ssum.y)};
                v2f e1 = {0.f, 0.f};
#pragma unroll
                for (int i = 0; i < NLEV; i++) {
                    q[i] *= rs;
                    e1 += q[i] * amp[i];
                }
                // log(q_i/P_i) from the softmax's own logits (see vaeq_dp_wave.hip / DESIGN.md)
                v2f e2 = {0.f, 0.f}, e3 = {0.f, 0.f}, kk = {0.f, 0.f}, kl = {0.f, 0.f};
#pragma unroll
                for (int i = 0; i < NLEV; i++) {
                    const v2f d = amp[i] - e1, qd = q[i] * d, g = z[i] * LN2 + nlogP[i];
                    e2 += qd * d;
                    e3 += qd * d * d;
                    kk += qd * g;
                    kl += q[i] * g;
                }
                if (inr0) klsum += kl.x - __builtin_amdgcn_logf(ssum.x) * LN2;
                if (inr1) klsum += kl.y - __builtin_amdgcn_logf(ssum.y) * LN2;
                asm volatile("" : "+v"(e2), "+v"(e3), "+v"(kk), "+v"(klsum));           // pin
                mv[r][0][c] = e2.x; mv[r][1][c] = e2.y;
                mt3[r][0][c] = e3.x; mt3[r][1][c] = e3.y;
                mkc[r][0][c] = inr0 ? kk.x : 0.f;
                mkc[r][1][c] = inr1 ? kk.y : 0.f;
                if (c) { muv[0].y = e1.x; muv[1].y = e1.y; } else { muv[0].x = e1.x; muv[1].x = e1.y; }
                if (qf && act[r]) {
#pragma unroll
                    for (int i = 0; i < NLEV; i++)
                        *reinterpret_cast<v2f *>(qf + (size_t)(c * NLEV + i) * No + (size_t)s * B + n0) = q[i];
                }
            }
            vv[r][0] = act[r] ? mv[r][0][0] + mv[r][0][1] : 0.f;
            vv[r][1] = act[r] ? mv[r][1][0] + mv[r][1][1] : 0.f;
            if (act[r]) {                                      // U[n]: even symbols in phase 0, odd in phase 1
                Us[l0 + 64 * r] = muv[0];
                Us[Uph + l0 + 64 * r] = muv[1];
            }
        }
        {
            float carry = 0.f, inc[NR];
#pragma unroll
            for (int r = 0; r < NR; r++) {
                inc[r] = wave_incl_scan_dpp(vv[r][0] + vv[r][1]) + carry;
                carry = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, inc[r]), 63));
            }
            float base = 0.f;
            if constexpr (NW > 1) {                            // totals of the waves below (fixed order)
                if (lane == 0) RED[8 + wv] = carry;
                sync_lds<NW>();
#pragma unroll
                for (int w = 0; w < NW - 1; w++)
                    if (w < wv) base += RED[8 + w];
            }
#pragma unroll
            for (int r = 0; r < NR; r++) {
                const int n0 = 2 * (l0 + 64 * r);
                if (act[r]) {
                    PSv[n0 + 1] = inc[r] + base - vv[r][1];
                    PSv[n0 + 2] = inc[r] + base;
                }
            }
            if (gl == 0) PSv[0] = 0.f;
        }
        sync_lds<NW>();
        if (wown) {
            const int lo = (Mh - tk + 1) >> 1, hi_ = (nm - 1 + Mh - tk) >> 1;
            VS[tk] = PSv[hi_ + 1] - PSv[lo];
        }
        sync_lds<NW>();

        // ============ P3: residual e = x - D for the quads t = 4 pr .. 4 pr + 3
        //   D[2 tau + par] = sum_a h[2a + par] U[tau + mh - a],   tau in {2 pr, 2 pr + 1}, a = 0..mh
        float se = 0.f;
        {
            cacc D[NR][4];
            if constexpr (LEAN) {                              // (see wave_fir)
    #pragma unroll
                for (int r = 0; r < NR; r++)
    #pragma unroll
                    for (int i = 0; i < 4; i++) D[r][i] = cacc0();
                auto step_a = [&](int r, float2 he, float2 ho, float2 ulo, float2 uhi) {
                    cmac(D[r][0], he.x, he.y, ulo); cmac(D[r][1], ho.x, ho.y, ulo);
                    cmac(D[r][2], he.x, he.y, uhi); cmac(D[r][3], ho.x, ho.y, uhi);
                };
                constexpr int NA = mh + 1, NB = NA / 2;
    #pragma unroll 1
                for (int b = 0; b < NB; b++) {                     // a = 2b, 2b+1;  d = mh - 2b: samples d+1, d, d-1
                    const float2 he0 = Ht[4 * b], ho0 = Ht[4 * b + 1], he1 = Ht[4 * b + 2], ho1 = Ht[4 * b + 3];
                    constexpr int ph = mh & 1;
                    const int sl = (mh >> 1) - b;
    #pragma unroll
                    for (int r = 0; r < NR; r++) {
                        const float2 ud = up[r][ph * Uph + sl];
                        const float2 udp = up[r][(ph ^ 1) * Uph + sl + ph];
                        const float2 udm = up[r][(ph ^ 1) * Uph + sl + ph - 1];
                        step_a(r, he0, ho0, ud, udp);
                        step_a(r, he1, ho1, udm, ud);
                    }
                }
                if (NA & 1) {                                      // a = mh: d = 0
                    const float2 he = Ht[2 * mh], ho = Ht[2 * mh + 1];
    #pragma unroll
                    for (int r = 0; r < NR; r++) step_a(r, he, ho, up[r][0], up[r][Uph]);
                }
            } else {
                auto step_a = [&](int r, v2f he, v2f ho, v2f ulo, v2f uhi, auto first) {
                    constexpr bool F = decltype(first)::value;
                    cmacf<F>(D[r][0], he, ulo); cmacf<F>(D[r][1], ho, ulo);
                    cmacf<F>(D[r][2], he, uhi); cmacf<F>(D[r][3], ho, uhi);
                };
                constexpr int NA = mh + 1, NB = NA / 2;
                if (NA & 1) {                                      // a = mh: d = 0 (first: it starts the accumulators)
                    const v2f he = lds2(Ht + 2 * mh), ho = lds2(Ht + 2 * mh + 1);
    #pragma unroll
                    for (int r = 0; r < NR; r++) step_a(r, he, ho, lds2(up[r]), lds2(up[r] + Uph), std::true_type{});
                } else {
    #pragma unroll
                    for (int r = 0; r < NR; r++)
    #pragma unroll
                        for (int i = 0; i < 4; i++) D[r][i] = cacc0();
                }
    #pragma unroll 1
                for (int b = 0; b < NB; b++) {                     // a = 2b, 2b+1;  d = mh - 2b: samples d+1, d, d-1
                    const v2f he0 = lds2(Ht + 4 * b), ho0 = lds2(Ht + 4 * b + 1), he1 = lds2(Ht + 4 * b + 2), ho1 = lds2(Ht + 4 * b + 3);
                    constexpr int ph = mh & 1;
                    const int sl = (mh >> 1) - b;
    #pragma unroll
                    for (int r = 0; r < NR; r++) {
                        const v2f ud = lds2(up[r] + ph * Uph + sl);
                        const v2f udp = lds2(up[r] + (ph ^ 1) * Uph + sl + ph);
                        const v2f udm = lds2(up[r] + (ph ^ 1) * Uph + sl + ph - 1);
                        step_a(r, he0, ho0, ud, udp, std::false_type{});
                        step_a(r, he1, ho1, udm, ud, std::false_type{});
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < NR; r++)
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int ce = Mh + i;
                    const float2 x = xq[r][(ce & 3) * Lph + (ce >> 2)];
                    const float2 Dv = cfin(D[r][i]);
                    float2 e = make_float2(x.x - Dv.x, x.y - Dv.y);
                    if (!qa[r] || 4 * (l0 + 64 * r) + i >= nm) e = make_float2(0.f, 0.f);
                    if (qa[r]) Es[(ce & 3) * Lph + l0 + 64 * r + (ce >> 2)] = e;
                    se += e.x * e.x + e.y * e.y;
                }
        }
        {
            float sk[2] = {wave_sum_dpp(se), wave_sum_dpp(klsum)};
            waves_sum<NW, 2>(sk, RED + 16, lane, wv);
            se = sk[0]; klsum = sk[1];
        }
        float hq = 0.f;
        if (worker) {
            const float2 hc = Ht[tk];
            hq = hc.x * hc.x + hc.y * hc.y;
        }
        const float vsl = worker ? VS[tk] : 0.f;
        const float C = se + wave_sum_dpp(half ? 0.f : hq * vsl);
        const float gC = (float)nm * __builtin_amdgcn_rcpf(C);
        if (gl == 0 && a.loss) a.loss[(size_t)run * a.steps + s] = (float)nm * LN2 * __builtin_amdgcn_logf(C) + klsum;
        {
            const float inc = half_incl_scan_dpp(gC * hq);     // inclusive scan within each 32-lane half
            if (wown) PSh[tk + 1] = inc;
            if (gl == 0) PSh[0] = 0.f;
        }
        sync_lds<NW>();

        // ============ P4a: dL/dh, lane = (j = tk, half of the tau range)
        step += 1;
        b1t *= 0.9;
        b2t *= 0.999;
        const float ss = lr * __builtin_amdgcn_rcpf((float)(1.0 - b1t));
        const float rbc2s = __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf((float)(1.0 - b2t)));
        float gh0 = 0.f, gh1 = 0.f;
        {
            float2 acc;
            {
                using TB = TapBlocks<M, NW, BL>;
                int g, prt;
                bool gv;                                                   // lanes without a block idle (they shadow group 0)
                TB::map(gl, TB::NGH, TB::PH, g, prt, gv);
                const int par = g >= TB::NG0 ? 1 : 0, a0 = 4 * (par ? g - TB::NG0 : g);
                const int T = nm >> 1, Tm = (T + 1) >> 1, nit = TB::CF ? TB::NITH : (Tm + TB::PH - 1) / TB::PH;   // terms per tap (nm is even: both parities alike), tau pairs, pairs per part
                const int m0 = prt * nit;
                const int ceA = par + Mh, ceB = par + Mh + 2, n0 = mh - a0 - 3;                            // U window of the 4 taps: n0 + 2m + (0..4)
                const float2 *eA = Es + (ceA & 3) * Lph + (ceA >> 2) + m0, *eB = Es + (ceB & 3) * Lph + (ceB >> 2) + m0;
                const int d = n0 & 1;
                const float2 *uE = Us + d * Uph + (n0 >> 1) + m0, *uO = Us + (d ^ 1) * Uph + (n0 >> 1) + d + m0;   // k = 0, 2, 4 / k = 1, 3
                cacc c4[4];
#pragma unroll
                for (int i = 0; i < 4; i++) c4[i] = cacc0();
#pragma unroll 1
                for (int m = 0; m < nit; m++) {                // uniform trip count: a scalar loop
                    const bool in = m0 + m < Tm;
                    v2f e0 = lds2(eA + m), f0 = lds2(eB + m);
                    const v2f w0 = lds2(uE + m), w1 = lds2(uO + m), w2 = lds2(uE + m + 1), w3 = lds2(uO + m + 1), w4 = lds2(uE + m + 2);
                    if (!in) { e0 = v2f{0.f, 0.f}; f0 = v2f{0.f, 0.f}; }
                    if (2 * (m0 + m) + 1 >= T) f0 = v2f{0.f, 0.f};         // odd T: the last pair has one term
                    cmac(c4[0], w3, e0); cmac(c4[1], w2, e0); cmac(c4[2], w1, e0); cmac(c4[3], w0, e0);   // tau = 2m  : tap a0 + i <- U[n0 + 2m + 3 - i]
                    cmac(c4[0], w4, f0); cmac(c4[1], w3, f0); cmac(c4[2], w2, f0); cmac(c4[3], w1, f0);   // tau = 2m+1: U[n0 + 2m + 4 - i]
                }
                float2 *XP = reinterpret_cast<float2 *>(sm + lay.XP);
                if (gv) {
#pragma unroll
                    for (int i = 0; i < 4; i++) XP[(g * 4 + i) * TB::PH + prt] = cfinc(c4[i]);            // e * conj(U), this part
                }
                sync_lds<NW>();
                acc = make_float2(0.f, 0.f);
                if (hown) {                                                // owner of h[j = tk]: add the parts in a fixed order
                    const int par_ = tk & 1, aa = tk >> 1, go = (par_ ? TB::NG0 : 0) + (aa >> 2);
                    const float2 *xp_ = XP + (go * 4 + (aa & 3)) * TB::PH;
#pragma unroll
                    for (int q = 0; q < TB::PH; q++) { const float2 v = xp_[q]; acc.x += v.x; acc.y += v.y; }
                }
            }
            if (hown) {
                gh0 = gC * (-2.0f * acc.x + 2.0f * p0 * vsl);
                gh1 = gC * (-2.0f * acc.y + 2.0f * p1 * vsl);
                if (!a.no_update) {
                    adam_update_amsgrad_fast(p0, am0, av0, ax0, gh0, ss, rbc2s);
                    adam_update_amsgrad_fast(p1, am1, av1, ax1, gh1, ss, rbc2s);
                }
            }
        }
        asm volatile("" : "+v"(p0), "+v"(p1), "+v"(gh0), "+v"(gh1));
        if (s + 1 < a.steps) fetch(s + 1);

        // ============ P4b: dL/dU (the FIR shape on e with conj(h)), dL/dyhat, normalisation backward
        float2 gy[NR][2];
        {
            float dt0 = 0.f, dt1 = 0.f;
            {
                cacc cu[NR][2];
                wave_fir<M, NR, LEAN>(cu, ep, Lph, Ht);
#pragma unroll
                for (int r = 0; r < NR; r++)
#pragma unroll
                    for (int sy = 0; sy < 2; sy++) {
                        const float2 au = cfinc(cu[r][sy]);    // e * conj(h)
                        const int sx = 2 * (2 * (l0 + 64 * r) + sy);
                        const int jlo = max(0, Mh - sx), jhi = max(jlo - 1, min(Mh, nm - 1 + Mh - sx));
                        const float gv = PSh[jhi + 1] - PSh[jlo];
                        const float ur = -2.0f * gC * au.x, ui = -2.0f * gC * au.y;
                        float gI = ivar2 * (ur * mv[r][sy][0] + gv * mt3[r][sy][0] + mkc[r][sy][0]);
                        float gQ = ivar2 * (ui * mv[r][sy][1] + gv * mt3[r][sy][1] + mkc[r][sy][1]);
                        if (!act[r]) gI = gQ = 0.f;
                        gy[r][sy] = make_float2(gI, gQ);
                        dt0 = fmaf(gI, y[r][sy].x, dt0);
                        dt1 = fmaf(gQ, y[r][sy].y, dt1);
                    }
            }
            {
                float dv[2] = {wave_sum_dpp(dt0), wave_sum_dpp(dt1)};
                waves_sum<NW, 2>(dv, RED + 24, lane, wv);
                dt0 = dv[0]; dt1 = dv[1];
            }
            const float k0_ = dt0 * A * __builtin_amdgcn_rcpf(m0 * m0) * rB, k1_ = dt1 * A * __builtin_amdgcn_rcpf(m1 * m1) * rB;
#pragma unroll
            for (int r = 0; r < NR; r++)
#pragma unroll
                for (int sy = 0; sy < 2; sy++) {
                    const float yI = y[r][sy].x, yQ = y[r][sy].y;
                    const float sgI = (float)(yI > 0.f) - (float)(yI < 0.f), sgQ = (float)(yQ > 0.f) - (float)(yQ < 0.f);
                    gy[r][sy].x = gy[r][sy].x * sc0 - k0_ * sgI;
                    gy[r][sy].y = gy[r][sy].y * sc1 - k1_ * sgQ;
                }
        }
        sync_lds<NW>();                                       // every read of U / old h is done (GY aliases U)
#pragma unroll
        for (int r = 0; r < NR; r++)
            if (act[r]) {
                if constexpr (TapBlocks<M, NW, BL>::CF) {             // planar: even symbols | odd symbols (Uph >= B / 2 apart)
                    GY[l0 + 64 * r] = gy[r][0];
                    GY[Uph + l0 + 64 * r] = gy[r][1];
                } else {
                    GY[2 * (l0 + 64 * r)] = gy[r][0];
                    GY[2 * (l0 + 64 * r) + 1] = gy[r][1];
                }
            }
        if (hown && !a.no_update) Ht[tk] = make_float2(p0, p1);
        sync_lds<NW>();

        // ============ P5: dL/dw, lane = (k = tk, half of the symbol range)
        float gw0 = 0.f, gw1 = 0.f;
        {
            float2 acc;
            {
                using TB = TapBlocks<M, NW, BL>;
                int grp, prt;
                bool gv;
                TB::map(gl, TB::NGW, TB::PW, grp, prt, gv);
                const int k0 = 4 * grp;                                    // taps k0 .. k0 + 3: x[4m + k0 + (0..5)] for the symbol pair (2m, 2m+1)
                const int Bp = B >> 1, nit = TB::CF ? TB::NITW : (Bp + TB::PW - 1) / TB::PW, m0 = prt * nit;
                const float2 *gya = TB::CF ? GY + m0 : GY + 2 * m0, *gyb = TB::CF ? GY + Uph + m0 : GY + 2 * m0 + 1;
                constexpr int gst = TB::CF ? 1 : 2;
                const float2 *xw = Xs + (k0 >> 2) + m0;                    // sample c = 4m + k0 + j sits at [(j & 3) Lph + m + (k0 >> 2) + (j >> 2)]
                cacc c4[4];
#pragma unroll
                for (int i = 0; i < 4; i++) c4[i] = cacc0();
#pragma unroll 1
                for (int m = 0; m < nit; m++) {                // uniform trip count: a scalar loop
                    v2f g0_ = lds2(gya + gst * m), g1_ = lds2(gyb + gst * m);                              // gy[2m], gy[2m+1]
                    const v2f x0 = lds2(xw + m), x1 = lds2(xw + Lph + m), x2 = lds2(xw + 2 * Lph + m), x3 = lds2(xw + 3 * Lph + m);
                    const v2f x4 = lds2(xw + m + 1), x5 = lds2(xw + Lph + m + 1);
                    if (m0 + m >= Bp) { g0_ = v2f{0.f, 0.f}; g1_ = v2f{0.f, 0.f}; }
                    cmac(c4[0], x0, g0_); cmac(c4[1], x1, g0_); cmac(c4[2], x2, g0_); cmac(c4[3], x3, g0_);   // n = 2m  : x[2n + k0 + i]
                    cmac(c4[0], x2, g1_); cmac(c4[1], x3, g1_); cmac(c4[2], x4, g1_); cmac(c4[3], x5, g1_);   // n = 2m+1: two samples on
                }
                float2 *XP = reinterpret_cast<float2 *>(sm + lay.XP);
                if (gv) {
#pragma unroll
                    for (int i = 0; i < 4; i++) XP[(grp * 4 + i) * TB::PW + prt] = cfinc(c4[i]);          // gy * conj(x), this part
                }
                sync_lds<NW>();
                acc = make_float2(0.f, 0.f);
                if (wown) {
                    const float2 *xp_ = XP + ((tk >> 2) * 4 + (tk & 3)) * TB::PW;
#pragma unroll
                    for (int q = 0; q < TB::PW; q++) { const float2 v = xp_[q]; acc.x += v.x; acc.y += v.y; }
                }
            }
            if (wown) {
                gw0 = acc.x;
                gw1 = -acc.y;
                if (!a.no_update) {
                    adam_update_amsgrad_fast(p0, am0, av0, ax0, gw0, ss, rbc2s);
                    adam_update_amsgrad_fast(p1, am1, av1, ax1, gw1, ss, rbc2s);
                    Wt[tk] = make_float2(p0, -p1);
                }
            }
        }
        if (s == a.steps - 1 && owner) {
            if (a.dbg_gW && !half) { a.dbg_gW[g0] = gw0; a.dbg_gW[g1] = gw1; }
            if (a.dbg_gh && half) { a.dbg_gh[g0] = gh0; a.dbg_gh[g1] = gh1; }
        }
        sync_lds<NW>();
    }

    if (owner && !a.no_update) {
        float *pp = half ? a.h : a.W, *pm = half ? a.adam_mh : a.adam_mW, *pv = half ? a.adam_vh : a.adam_vW,
              *px = half ? a.adam_xh : a.adam_xW;
        pp[g0] = p0; pp[g1] = p1;
        pm[g0] = am0; pm[g1] = am1;
        pv[g0] = av0; pv[g1] = av1;
        px[g0] = ax0; px[g1] = ax1;
    }
    if (gl == 0 && !a.no_update) a.step[run] = step;
}

template <int M, int NLEV, int NR, int NW = 1, int BL = 0>
static int launch_awgn_wave_k(const vaeq_awgn_args &a, hipStream_t st)
{
    const size_t lds = (size_t)awgn_wave_layout(a.B, M, NW).total;
    auto k = awgn_wave_kernel<M, NLEV, NR, NW, BL>;
    note_kernel("vaeq::awgn_wave_kernel<%d, %d, %d, %d, %d>", M, NLEV, NR, NW, BL);   // every template argument, as rocprofv3 prints the name
    return launch(k, dim3(a.R), dim3(64 * NW), lds, st, a);
}

template <int M, int NLEV>
static int launch_awgn_wave_r(const vaeq_awgn_args &a, hipStream_t st)
{
    if (M == 25 && a.B == 350) return launch_awgn_wave_k<M, NLEV, 3, 1, M == 25 ? 350 : 0>(a, st);   // the reference's minibatch (Eval_run_shaping_vaele.py:26), baked
    switch ((a.B / 2 + 63) / 64) {
    case 1: return launch_awgn_wave_k<M, NLEV, 1>(a, st);
    case 2: return launch_awgn_wave_k<M, NLEV, 2>(a, st);
    case 3: return launch_awgn_wave_k<M, NLEV, 3>(a, st);       // (three waves x one round would need <= 128 VGPRs to keep the runs per CU: 79 spilled dwords)
    case 4: return launch_awgn_wave_k<M, NLEV, 2, 2>(a, st);   // B <= 512: two wavefronts x two rounds
    case 5:
    case 6: return launch_awgn_wave_k<M, NLEV, 2, 3>(a, st);   // B <= 768
    case 7:
    case 8: return launch_awgn_wave_k<M, NLEV, 2, 4>(a, st);   // B <= 1024
    }
    return VAEQ_ERR_SHAPE;
}

template <int M>
static int launch_awgn_wave_lev(const vaeq_awgn_args &a, hipStream_t st)
{
    return dispatch_nlev(a.n_lev, [&](auto nl) { return launch_awgn_wave_r<M, decltype(nl)::value>(a, st); });
}

// Whether the wave-per-run kernel covers this call (else the generic kernel runs).
bool awgn_wave_supported(const vaeq_awgn_args &a)
{
    if (a.sps != 2 || (a.B & 1) || a.B > 1024 || a.B < 2 * (a.M / 2) + 2) return false;
    if (!(a.M == 25 || a.M == 17 || a.M == 9)) return false;
    if ((a.S & 3) || (reinterpret_cast<uintptr_t>(a.rx) & 15)) return false;              // 16-byte window loads
    if (a.q_out && (reinterpret_cast<uintptr_t>(a.q_out) & 7)) return false;
    if (a.y_out && (reinterpret_cast<uintptr_t>(a.y_out) & 7)) return false;
    return true;
}

int launch_awgn_wave(const vaeq_awgn_args &a, hipStream_t st)
{
    switch (a.M) {
    case 25: return launch_awgn_wave_lev<25>(a, st);
    case 17: return launch_awgn_wave_lev<17>(a, st);
    case 9: return launch_awgn_wave_lev<9>(a, st);
    }
    return VAEQ_ERR_SHAPE;
}

int64_t awgn_wave_lds(int B, int M) { return (int64_t)awgn_wave_layout(B, M, B <= 384 ? 1 : (B / 2 + 127) / 128).total; }

}  // namespace vaeq
