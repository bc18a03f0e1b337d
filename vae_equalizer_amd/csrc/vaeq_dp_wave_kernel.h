// vaeq_dp_wave_kernel.h -- wave-per-run fast path of the DP VAE-LE / VAEflex training loop (gfx950).
//
// One 64-lane wavefront = one run (B <= 128); no workgroup barriers, everything between HBM and the taps lives in LDS/VGPRs.
// Same math as vaeq_dp.hip (see the derivation there and in DESIGN.md); what changes is the mapping:
//
//   * lane l owns the symbol pair (2l, 2l+1) of the minibatch (B <= 128): FIR, soft demap, the per-symbol moments
//     (kept in registers until the backward pass) and dL/dy are all done by the owning lane; q and y leave as one
//     8-byte store per lane and row (400 contiguous bytes per row and step at B = 100).
//   * every convolution-shaped phase is register-blocked over that pair and over both outputs: the taps of a group of four are read once
//     (LDS broadcasts) and feed 32 packed FMAs
//     (FIR:  y[n]      = sum_k w[k] x[2n+k],
//      dL/dU[n]        = sum_j e[2n+j] conj(h[j])    -- the same shape on the residual e, both chi in one loop,
//      D[t], t=4l..4l+3: the zero-stuffed convolution, written as two polyphase symbol-rate FIRs on mu).
//   * sample-rate arrays (x, e) are stored 4-way polyphase in LDS (index c -> [c & 3][c >> 2]) and the symbol-rate mu
//     2-way, so that the stride-4 / stride-2 accesses of consecutive lanes hit consecutive 8-byte LDS words.
//   * the two correlation-shaped gradients (dL/dh: 100 outputs x 88 terms, dL/dw: 100 x 100) are laid out as
//     lane = (tap, half of the sum range); halves are combined with one cross-half shuffle; the lane that ends up
//     with a gradient also owns that parameter's Adam moments (LDS rows of their own) and writes the updated tap to LDS.
//   * every 8-byte LDS read is pinned to one ds_read_b64 (lds2), the tap loops are two-deep software pipelines (pipe2) whose first
//     term starts the accumulators (at the baked B = 100 their stages also hand the cells they share to one another in registers, pipe2_carry);
//     streamed rows go through buffer descriptors (scalar row offsets, out-of-range offsets as masks).
//   * wave sums and prefix scans run on DPP in a fixed order: bitwise reproducible, no LDS round trips.
//   (DESIGN.md section 5 has the measurements behind each of these.)
//
// Supported here: sps == 2, B even, 2*(M/2)+2 <= B <= 1024, M in {9, 13, 17, 21, 25, 31}; everything else takes the
// generic kernel of vaeq_dp.hip.  BT > 0 bakes the minibatch length into the kernel (all LDS offsets immediate).
// B <= 128 runs as ONE wavefront per run (NW = 1, described above); 128 < B <= 256 as two, B <= 512 as four and B <= 1024 as
// eight wavefronts per run (NW = 2, 4, 8: same code, thread 64 wv + lane owns the pair, see dp_wave_kernel).  Instantiated in
// vaeq_dp_wave.hip (NW = 1), vaeq_dp_wave_mw.hip (NW = 2, 4) and vaeq_dp_wave_mw8.hip (NW = 8).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "vaeq.h"
#include "vaeq_common.h"
#include "vaeq_launch.h"
#include "vaeq_wave.h"

// -DVAEQ_PHASE_STAMPS: shader-clock stamps around the phases of the LAST step of one wave under full load, written over loss[0..] of the launch
// (tools/probe_dp_phases.py reads them; the build is for that probe only: tools/build_phase_probe.sh dp_wave).
#ifdef VAEQ_PHASE_STAMPS
#define VAEQ_STAMP(i) do { if (s == a.steps - 1) tst[i] = __builtin_readcyclecounter(); } while (0)
#define VAEQ_XSTAMP(i) do { if (s == a.steps - 1) tsx[i] = __builtin_readcyclecounter(); } while (0)   // inside the two tap-gradient phases
#else
#define VAEQ_STAMP(i) do { } while (0)
#define VAEQ_XSTAMP(i) do { } while (0)
#endif
#define VAEQ_NSTAMP 12
// Experiment knob of tools/snap_variant.sh builds (the default is what ships): software pipelining of the tap loops
#ifndef VAEQ_PIPE
#define VAEQ_PIPE 1
#endif
#define VAEQ_BT_FRAMES 16                              // frames per launch whose Adam bias corrections restart exactly like a launch's (vaeq_dp_train)
#ifndef VAEQ_WPS
#define VAEQ_WPS 2                                     // workgroups per SIMD the register budget is sized for (3 would need <= 168 VGPRs: it spills)
#endif

namespace vaeq {

// Sum of a complex tap gradient over the two 32-lane halves, for the half that keeps it, as the 8-byte pair (re, im) the Adam update goes on with: a0
// belongs to the taps the lower half owns, a1 to the upper half's; returns a0[lane] + a0[lane ^ 32] in the lower and a1[lane] + a1[lane ^ 32] in the upper
// half (the lane's own part is one addend and its partner's the other in either half: IEEE addition commutes, the sums are bitwise the same).  Per
// component, v_permlane32_swap exchanges a0's upper half with a1's lower half: the lower lanes then hold (a0 own, a0 partner), the upper lanes
// (a1 partner, a1 own).  The two swaps leave the addends in two aligned register pairs, so the sum is ONE v_pk_add_f32 and nothing is moved (left to
// itself the optimiser pairs the four reals of a lane by what the update does with them first, and re-pairs them with v_mov before and after)
__device__ __forceinline__ v2f half_sum2(v2f a0, v2f a1)
{
    const float a0x = a0.x, a0y = a0.y, a1x = a1.x, a1y = a1.y;   // (scalars first: __builtin_bit_cast of a vector element reads the vector's first bytes)
    const auto rx = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, a0x), __builtin_bit_cast(unsigned, a1x), false, false);
    const auto ry = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, a0y), __builtin_bit_cast(unsigned, a1y), false, false);
    v2f r0 = {__builtin_bit_cast(float, (unsigned)rx[0]), __builtin_bit_cast(float, (unsigned)ry[0])};
    v2f r1 = {__builtin_bit_cast(float, (unsigned)rx[1]), __builtin_bit_cast(float, (unsigned)ry[1])};
    asm volatile("" : "+v"(r0), "+v"(r1));                 // pin: the addends stay 8-byte registers
    return r0 + r1;
}

// adam_update_fast (vaeq_common.h) on the real and the imaginary part of a tap at once: the same operations with the same roundings, element by element
// (what the scalar form contracts is spelled out), on pairs that are born aligned -- gradient, moments and tap each arrive as (re, im).  The optimiser
// packs the scalar form too, but by operation: (g, v) x (0.001, 0.999), (g_re, g_im) - (m_re, m_im), ... -- two or three v_mov per packed instruction.
__device__ __forceinline__ void adam_update_fast2(v2f &p, v2f &m, v2f &v, v2f g, float step_size, float rbc2s)
{
    m = __builtin_elementwise_fma(g - m, v2f{0.1f, 0.1f}, m);
    v = v * 0.999f;
    v = __builtin_elementwise_fma(0.001f * g, g, v);
    // (the denominators as two scalar fmas, between the transcendentals that are scalar anyway: packed, the uniform rbc2s would be kept as a (rbc2s, rbc2s)
    //  register pair from the first update of a step to the last, through the kernel's register peak)
    const float d0 = fmaf(__builtin_amdgcn_sqrtf(v.x), rbc2s, 1e-8f), d1 = fmaf(__builtin_amdgcn_sqrtf(v.y), rbc2s, 1e-8f);
    const v2f rd = {__builtin_amdgcn_rcpf(d0), __builtin_amdgcn_rcpf(d1)};
    p = __builtin_elementwise_fma(-step_size * m, rd, p);
}

struct WaveLayout {
    int Lph, Uph;                                      // float2 per polyphase component of x/e and of mu
    int X, E, U, PSv, W, H, PSh, VS, MOM, RED, XG, total;   // byte offsets (the dL/dy buffer aliases U)
};

__host__ __device__ inline WaveLayout wave_layout(int B, int M, int NW = 1)
{
    WaveLayout l;
    const int len = 2 * B + M - 1;                     // L + 2*mh samples incl. zero halo
    const int lph = wave_lph(len);
    l.Lph = lph;
    l.Uph = B / 2 + 1;
    int o = 0;
    auto take = [&](int bytes) { int r = o; o += (bytes + 15) & ~15; return r; };
    l.X = take(2 * 4 * lph * 8);
    l.E = take(2 * 4 * lph * 8);
    const int ubytes = 2 * 2 * l.Uph * 8, gbytes = 2 * B * 8;
    l.U = take(ubytes > gbytes ? ubytes : gbytes);
    l.PSv = take(2 * (B + 1) * 4);
    l.W = take(2 * M * 16);
    l.H = take(2 * 2 * (M + 1) * 8);                   // one zero pad tap per (chi, nu): j = M
    l.PSh = take(2 * (M + 1) * 4);
    l.VS = take(2 * M * 4);
    l.MOM = take(16 * 64 * 4);                         // Adam moments of the taps a lane owns: [16][64 lanes] (registers are the scarcer resource)
    l.RED = take(NW > 1 ? 64 * 4 : 0);                 // NW > 1: cross-wave scan offsets and sums
    l.XG = take((NW - 1) * 4 * 64 * 4);                // ... and the tap-gradient partial sums of waves 1..NW-1
    l.total = o;
    return l;
}

// Cells that consecutive stages of the convolution-shaped tap loops share (the baked B = 100, M = 25 kernel carries them in registers instead of
// reading them again, pipe2_carry).  All indices are relative to the lane's base cell.
//   FIR, dL/dU: stage g reads the sample cells 4g + j, j = 0..5, at xg[0], xg[Lph], xg[2 Lph], xg[3 Lph], xg[1], xg[Lph + 1] (xg = xp + g, 4-way
//               polyphase): j = 4, 5 of stage g are j = 0, 1 of stage g + 1, and cell 4G of the tap left over after G stages is j = 4 of stage G - 1.
//   D (D3Map):  stage b reads the mu cells mh - 2b + d, d = -1..2, at uo[sl - 1], ue[sl], uo[sl], ue[sl + 1] (sl = mh / 2 - b, 2-way polyphase,
//               mh even): d = -1, 0 of stage b are d = 1, 2 of stage b + 1.
// (The cells U[3 m + 0..2] of the a = mh term, read ahead of the D loops, are d = -1, 0 of the LAST stage and one cell below; they are consumed first:
//  keeping two of them to the end of both loops would take registers through the whole phase and a peeled last trip, for 4 of 827 reads.  Left alone.)
struct CellCarry {
    static constexpr int fir_off(int g, int j, int Lph) { return g + (j < 4 ? j * Lph : (j - 4) * Lph + 1); }   // what the code adds to xp
    static constexpr int poly4(int c, int Lph) { return (c & 3) * Lph + (c >> 2); }
    static constexpr int d3_off(int b, int d, int mh, int Uph) { return (d & 1 ? Uph : 0) + (mh >> 1) - b + (d == -1 ? -1 : d == 2 ? 1 : 0); }   // added to ue
    static constexpr int poly2(int c, int Uph) { return (c & 1) * Uph + (c >> 1); }
    // the carried cell is the one the next stage would have read, every offset is the polyphase place of its cell, and no read leaves its array
    static constexpr bool fir_exact(int B, int M)
    {
        const int G = M / 4, len = 2 * B + M - 1, Lph = wave_lph(len);
        if (M % 4 != 1 || G < 2 || G % 2) return false;                          // one tap left over; pipe2_carry: an even number of stages
        for (int g = 0; g < G; g++)
            for (int j = 0; j < 6; j++) {
                if (fir_off(g, j, Lph) != poly4(4 * g + j, Lph)) return false;
                if (4 * (B / 2 - 1) + 4 * g + j >= len) return false;               // the last lane with a symbol pair
                if (g + 1 < G && j >= 4 && fir_off(g, j, Lph) != fir_off(g + 1, j - 4, Lph)) return false;
            }
        return poly4(4 * G, Lph) == fir_off(G - 1, 4, Lph) && 4 * (B / 2 - 1) + 4 * G + 2 < len;   // the left-over tap's two cells: 4G (carried), 4G + 2
    }
    static constexpr bool d3_exact(int B, int M)
    {
        const int mh = M / 2, NB = (mh + 1) / 2, Uph = B / 2 + 1, T = B - mh;
        if ((mh & 1) || NB < 2 || NB % 2) return false;
        for (int b = 0; b < NB; b++)
            for (int d = -1; d <= 2; d++) {
                // even lane base (3 m even): ue is the even phase; odd base: ue = phase 1, uo = phase 0 one slot up -- the same offsets on swapped rows
                if (d3_off(b, d, mh, Uph) != poly2(mh - 2 * b + d, Uph)) return false;
                if (mh - 2 * b + d < 0 || 3 * (D3Map_nm_lanes(T) - 1) + mh - 2 * b + d >= 2 * Uph) return false;
                if (b + 1 < NB && d <= 0 && d3_off(b, d, mh, Uph) != d3_off(b + 1, d + 2, mh, Uph)) return false;
            }
        return true;
    }
    static constexpr int D3Map_nm_lanes(int T) { return (T + 2) / 3; }           // D3Map::nm_lanes (defined below; asserted equal there)
};
static_assert(CellCarry::fir_exact(100, 25), "B = 100: the FIR / dL/dU stages must carry exactly the cells the next stage would have read, inside x / e");
static_assert(CellCarry::d3_exact(100, 25), "B = 100: the D stages must carry exactly the mu cells the next stage would have read, inside U");

// The taps of the FIR and dL/dU loops arrive as 16-byte reads (lds4), two neighbouring taps each: the FIR's tap k is the float4 Wt[p][k]; a dL/dU stage g
// reads the pairs (4g, 4g + 1), (4g + 2, 4g + 3) of four Ht rows.  (The D loop keeps its 8-byte tap reads: measured, 16-byte reads there add nothing to
// the other two)
// Aligned by construction: wave_layout rounds every array up to 16 bytes, so lay.W and lay.H are multiples of 16 for every shape, and a pair starts at
// the even tap 4g (+ 2).  What can fail is held here: every Ht row starts 16-byte aligned only if its MP = M + 1 taps of 8 bytes are an even number, and
// no pair may leave its row (the last one ends at tap 4 (G - 1) + 3 <= M - 1; the left-over tap stays an 8-byte read).
struct Tap16 {
    static constexpr bool exact(int M) { return (M + 1) % 2 == 0 && 4 * (M / 4 - 1) + 3 <= M - 1; }
};
static_assert(Tap16::exact(25), "M = 25: every Ht row must start 16-byte aligned and every 16-byte tap read must end inside its row");

// MACs whose tap is one half of a 16-byte read (lds4).  The low pair is left to the compiler; the high pair takes the explicit form (cmac16), or the backend
// copies its second dword before the broadcast.  (All MACs of a loop as asm statements is no alternative: the hazard recognizer cannot look into a statement
// and puts an s_nop 0 between two of them wherever it cannot rule out a forwarding hazard -- two per trip in the dL/dU loop.)
template <bool FIRST, bool HI>
__device__ __forceinline__ void cmacf_half(cacc &c, v2f t, v2f v)
{
    if constexpr (HI) cmacf16<FIRST>(c, t, v);
    else cmacf<FIRST>(c, t, v);
}
// the two taps a, b of one 16-byte read (its low and its high pair) on one sample.  BOTH: the low pair's MAC in the explicit form too -- the FIR loop needs
// it (left to the compiler, the low pairs that live across the loop's back edge are split into dwords and copied: four v_mov_b32 at the end of every trip)
template <bool FIRST, bool BOTH = false>
__device__ __forceinline__ void mac2(cacc (&c)[2], v2f a, v2f b, v2f x)
{
    cmacf_half<FIRST, BOTH>(c[0], a, x);
    cmacf_half<FIRST, true>(c[1], b, x);
}
template <int N> using tapc = std::integral_constant<int, N>;

// pair_fir (below) for the baked B = 100 kernel: the same stages, but stage g >= 1 takes its first two sample cells from the registers of stage g - 1
// (12 reads per 32 packed FMAs instead of 14) and the left-over tap its first cell from the last stage's.  Every output keeps its terms, their order and
// its even / odd sub-chains; stage 0 is pair_fir's, statement for statement (it decides which first product is rounded on its own).
template <int M, bool INIT>
__device__ __forceinline__ void pair_fir_carry(cacc (&acc)[2][2], cacc (&acc2)[2][2], const float2 *xp, int Lph, const float4 *wq)
{
    constexpr int G = M / 4;
    // tap k = the float4 (wr[o0], wi[o0], wr[o1], wi[o1]): one 16-byte read, its halves (o = 0, o = 1) feeding the MACs in place (mac2)
    auto tap = [&](int k, v2f &a, v2f &b) { const v4f q = lds4(wq + k); a = lo2(q); b = hi2(q); };
    auto taps = [&](int g, v2f (&r)[14]) {
#pragma unroll
        for (int t = 0; t < 4; t++) tap(4 * g + t, r[6 + 2 * t], r[7 + 2 * t]);
    };
    auto loadF = [&](v2f (&r)[14]) {
        r[0] = lds2(xp); r[1] = lds2(xp + Lph); r[2] = lds2(xp + 2 * Lph); r[3] = lds2(xp + 3 * Lph); r[4] = lds2(xp + 1); r[5] = lds2(xp + Lph + 1);
        taps(0, r);
    };
    auto loadM = [&](int g, v2f (&r)[14]) { r[2] = lds2(xp + g + 2 * Lph); r[3] = lds2(xp + g + 3 * Lph); taps(g, r); };
    auto loadL = [&](int g, v2f (&r)[14]) { r[4] = lds2(xp + g + 1); r[5] = lds2(xp + g + Lph + 1); };
    auto fma0 = [&](const v2f (&r)[14]) {
        // INIT: a chain starts as the sum of two products, taps 0 and 2 (acc2: 1 and 3).  The backend contracts that sum as fma(first, round(second)): the SECOND
        // product is the one rounded alone (pinned bits), so the explicit form multiplies it first and adds the first term to it
        if constexpr (INIT) {
            mac2<true, true>(acc[0], r[10], r[11], r[2]); mac2<true, true>(acc[1], r[10], r[11], r[4]);
            mac2<true, true>(acc2[0], r[12], r[13], r[3]); mac2<true, true>(acc2[1], r[12], r[13], r[5]);
        }
        mac2<false, true>(acc[0], r[6], r[7], r[0]); mac2<false, true>(acc[1], r[6], r[7], r[2]);
        mac2<false, true>(acc2[0], r[8], r[9], r[1]); mac2<false, true>(acc2[1], r[8], r[9], r[3]);
        if constexpr (!INIT) {
            mac2<false, true>(acc[0], r[10], r[11], r[2]); mac2<false, true>(acc[1], r[10], r[11], r[4]);
            mac2<false, true>(acc2[0], r[12], r[13], r[3]); mac2<false, true>(acc2[1], r[12], r[13], r[5]);
        }
    };
    auto stage = [&](const v2f (&r)[14], const v2f (&p)[14], auto mid) {          // p[4], p[5]: this stage's cells j = 0, 1
        mac2<false, true>(acc[0], r[6], r[7], p[4]); mac2<false, true>(acc2[0], r[8], r[9], p[5]);
        // (volatile: stays in front of the loads into p[4], p[5])
        asm volatile("" : "+v"(acc[0][0].a), "+v"(acc[0][0].b), "+v"(acc[0][1].a), "+v"(acc[0][1].b), "+v"(acc2[0][0].a), "+v"(acc2[0][0].b),
                     "+v"(acc2[0][1].a), "+v"(acc2[0][1].b));
        mid();
        mac2<false, true>(acc[1], r[6], r[7], r[2]); mac2<false, true>(acc2[1], r[8], r[9], r[3]);
        mac2<false, true>(acc[0], r[10], r[11], r[2]); mac2<false, true>(acc[1], r[10], r[11], r[4]);
        mac2<false, true>(acc2[0], r[12], r[13], r[3]); mac2<false, true>(acc2[1], r[12], r[13], r[5]);
    };
    constexpr int k = 4 * G;                                                       // the left-over tap (even: into acc)
    v2f ta, tb, xb;
    auto pre = [&]() { tap(k, ta, tb); xb = lds2(xp + ((k + 2) & 3) * Lph + ((k + 2) >> 2)); };
    auto post = [&](const v2f (&r)[14]) { mac2<false, true>(acc[0], ta, tb, r[4]); mac2<false, true>(acc[1], ta, tb, xb); };
    pipe2_carry<14>(G, loadF, loadM, loadL, fma0, stage, pre, post);
}

// y[sym] += sum_k taps[k] * x[4l + 2*sym + k] for the lane's symbol pair, one input polarisation (FIR): T = float4 tap quads
// (o0.re, o0.im, o1.re, o1.im), acc[sym][o] += w * x.  xp = phase-0 pointer of the lane (slot = lane).
// A dependent v_pk_fma_f32 can issue only every ~12 cycles (measured: one wave with 8 accumulator chains reaches 64 % of the packed-FMA rate,
// tools/ubench/coissue.hip), and with 2 waves per SIMD a wave is often alone in its FMA burst -- so every convolution-shaped phase keeps 16
// independent chains: here the even taps accumulate into acc, the odd taps into acc2 (the caller adds them once at the end).
// INIT: the first taps start the accumulators (no zeroing); else they are added to.
// SPLIT = false (shapes not baked into the kernel, where run-time strides already cost registers): all taps into acc, acc2 untouched.
// CARRY (the baked B = 100 kernel): the sample cells a stage shares with the one before stay in registers, see CellCarry and pair_fir_carry.
template <int M, bool INIT, bool PIPE = true, bool SPLIT = true, bool CARRY = false>
__device__ __forceinline__ void pair_fir(cacc (&acc)[2][2], cacc (&accx)[2][2], const float2 *xp, int Lph, const float4 *wq)
{
    if constexpr (CARRY) {
        static_assert(PIPE && SPLIT, "the carried form is the pipelined, split one");
        pair_fir_carry<M, INIT>(acc, accx, xp, Lph, wq);
        return;
    }
    cacc (&acc2)[2][2] = SPLIT ? accx : acc;
    auto tapA = [&](int k) -> v2f { return lds2(reinterpret_cast<const float2 *>(wq + k)); };       // (re, im) of o = 0
    auto tapB = [&](int k) -> v2f { return lds2(reinterpret_cast<const float2 *>(wq + k) + 1); };   // (re, im) of o = 1
    constexpr int G = M / 4;
    // stage g: taps 4g..4g+3, samples c' = 4g..4g+5 -- 14 independent 8-byte LDS reads feeding 32 packed FMAs
    auto load = [&](int g, v2f (&r)[14]) {
        const float2 *xg = xp + g;
        r[0] = lds2(xg); r[1] = lds2(xg + Lph); r[2] = lds2(xg + 2 * Lph); r[3] = lds2(xg + 3 * Lph); r[4] = lds2(xg + 1); r[5] = lds2(xg + Lph + 1);
#pragma unroll
        for (int t = 0; t < 4; t++) { r[6 + 2 * t] = tapA(4 * g + t); r[7 + 2 * t] = tapB(4 * g + t); }
    };
    auto fma = [&](int, const v2f (&r)[14], auto first) {
        constexpr bool F = decltype(first)::value;     // the very first taps start the accumulators (cmul): nothing to zero
        cmacf<F>(acc[0][0], r[6], r[0]); cmacf<F>(acc[0][1], r[7], r[0]); cmacf<F>(acc[1][0], r[6], r[2]); cmacf<F>(acc[1][1], r[7], r[2]);
        cmacf<F && SPLIT>(acc2[0][0], r[8], r[1]); cmacf<F && SPLIT>(acc2[0][1], r[9], r[1]);
        cmacf<F && SPLIT>(acc2[1][0], r[8], r[3]); cmacf<F && SPLIT>(acc2[1][1], r[9], r[3]);
        cmac(acc[0][0], r[10], r[2]); cmac(acc[0][1], r[11], r[2]); cmac(acc[1][0], r[10], r[4]); cmac(acc[1][1], r[11], r[4]);
        cmac(acc2[0][0], r[12], r[3]); cmac(acc2[0][1], r[13], r[3]); cmac(acc2[1][0], r[12], r[5]); cmac(acc2[1][1], r[13], r[5]);
    };
    pipe2<14, INIT, PIPE>(G, load, fma);
#pragma unroll
    for (int k = 4 * G; k < M; k++) {                  // remaining 1 or 3 taps
        const v2f a = tapA(k), b = tapB(k);
        const v2f xa = lds2(xp + (k & 3) * Lph + (k >> 2)), xb = lds2(xp + ((k + 2) & 3) * Lph + ((k + 2) >> 2));
        if (k & 1) { cmac(acc2[0][0], a, xa); cmac(acc2[0][1], b, xa); cmac(acc2[1][0], a, xb); cmac(acc2[1][1], b, xb); }
        else { cmac(acc[0][0], a, xa); cmac(acc[0][1], b, xa); cmac(acc[1][0], a, xb); cmac(acc[1][1], b, xb); }
    }
}

// dL/dU for the lane's symbol pair: the FIR's shape on the residual e with conjugated channel taps, acc[chi][sym][nu] += e[chi] * conj(h[chi][nu]),
// BOTH chi in one loop (16 independent accumulator chains, see pair_fir).  ep = phase-0 pointer of the lane into e[chi = 0] (chi = 1: + 4 Lph);
// ht[chi * 2 + nu] = the tap rows (float2, MP apart).  Runs at the kernel's register peak (the demapper's moments are live): one operand set.
template <int M, bool MERGE = true, bool CARRY = false>
__device__ __forceinline__ void pair_du(cacc (&acc)[2][2][2], const float2 *ep, int Lph, const float2 *ht, int MP)
{
    constexpr int G = M / 4;
    // operands of one chi for taps 4g..4g+3: 6 samples c' = 4g..4g+5 and the 4 taps of the rows nu = 0, 1 -- 14 independent LDS reads, 32 packed FMAs
    auto cells = [&](int chi, int g, v2f *x) {
        const float2 *xg = ep + chi * 4 * Lph + g;
        x[0] = lds2(xg); x[1] = lds2(xg + Lph); x[2] = lds2(xg + 2 * Lph); x[3] = lds2(xg + 3 * Lph); x[4] = lds2(xg + 1); x[5] = lds2(xg + Lph + 1);
    };
    auto load1 = [&](int chi, int g, v2f *x) {
        cells(chi, g, x);
#pragma unroll
        for (int t = 0; t < 4; t++) { x[6 + 2 * t] = lds2(ht + (chi * 2 + 0) * MP + 4 * g + t); x[7 + 2 * t] = lds2(ht + (chi * 2 + 1) * MP + 4 * g + t); }
    };
    auto fma1 = [&](int chi, const v2f *x, int t, auto first) {                // tap 4g + t of both rows on both symbols
        constexpr bool F = decltype(first)::value;
        cmacf<F>(acc[chi][0][0], x[6 + 2 * t], x[t]); cmacf<F>(acc[chi][0][1], x[7 + 2 * t], x[t]);
        cmacf<F>(acc[chi][1][0], x[6 + 2 * t], x[t + 2]); cmacf<F>(acc[chi][1][1], x[7 + 2 * t], x[t + 2]);
    };
    if constexpr (CARRY) {
        // the merged form for the baked B = 100 kernel: stage g >= 1 takes the sample cells j = 0, 1 of both chi from the registers of stage g - 1 (CellCarry:
        // 24 reads per 64 packed FMAs instead of 28), the left-over tap its first cell from the last stage's.  Every chain keeps its terms and their order
        // (tap 4g .. 4g + 3); stage 0 is the plain one, statement for statement.  Per chi -- the carry restarts where the array changes
        static_assert(MERGE && M % 4 == 1, "the carried form is the merged one, with one tap left over");
        // The taps 4g .. 4g + 3 of a row are two 16-byte aligned pairs (Tap16): two 16-byte reads per row, their halves feeding the MACs in place
        auto taps = [&](int chi, int g, v2f *x) {
#pragma unroll
            for (int nu = 0; nu < 2; nu++)
#pragma unroll
                for (int t = 0; t < 4; t += 2) {
                    const v4f q = lds4(ht + (chi * 2 + nu) * MP + 4 * g + t);
                    x[6 + nu + 2 * t] = lo2(q); x[8 + nu + 2 * t] = hi2(q);
                }
        };
        // tap 4g + t of both rows on both symbols (s0, s1: their cells); the odd taps are the high pairs of their reads
        auto fmat = [&](int chi, const v2f *x, auto tc, auto first, v2f s0, v2f s1) {
            constexpr int t = decltype(tc)::value;
            constexpr bool F = decltype(first)::value, HI = t & 1;
            cmacf_half<F, HI>(acc[chi][0][0], x[6 + 2 * t], s0); cmacf_half<F, HI>(acc[chi][0][1], x[7 + 2 * t], s0);
            cmacf_half<F, HI>(acc[chi][1][0], x[6 + 2 * t], s1); cmacf_half<F, HI>(acc[chi][1][1], x[7 + 2 * t], s1);
        };
        auto fmao = [&](int chi, const v2f *x, auto tc, auto first) { fmat(chi, x, tc, first, x[decltype(tc)::value], x[decltype(tc)::value + 2]); };   // its own cells
        auto loadF = [&](v2f (&r)[28]) {
#pragma unroll
            for (int chi = 0; chi < 2; chi++) { cells(chi, 0, r + 14 * chi); taps(chi, 0, r + 14 * chi); }
        };
        auto loadM = [&](int g, v2f (&r)[28]) {
#pragma unroll
            for (int chi = 0; chi < 2; chi++) {
                const float2 *xg = ep + chi * 4 * Lph + g;
                v2f *x = r + 14 * chi;
                x[2] = lds2(xg + 2 * Lph); x[3] = lds2(xg + 3 * Lph);
                taps(chi, g, x);
            }
        };
        auto loadL = [&](int g, v2f (&r)[28]) {
#pragma unroll
            for (int chi = 0; chi < 2; chi++) { r[14 * chi + 4] = lds2(ep + chi * 4 * Lph + g + 1); r[14 * chi + 5] = lds2(ep + chi * 4 * Lph + g + Lph + 1); }
        };
        auto fma0 = [&](const v2f (&r)[28]) {
            // a chain starts as the sum of the products of taps 0 and 1, which the backend contracts as fma(tap 0, round(tap 1)): the product of tap 1 (the high
            // pair, explicit form) is the one rounded alone (pinned bits), so it comes first and tap 0's term is added to it
            fmao(0, r, tapc<1>{}, std::true_type{}); fmao(1, r + 14, tapc<1>{}, std::true_type{});
            fmao(0, r, tapc<0>{}, std::false_type{}); fmao(1, r + 14, tapc<0>{}, std::false_type{});
            fmao(0, r, tapc<2>{}, std::false_type{}); fmao(1, r + 14, tapc<2>{}, std::false_type{});
            fmao(0, r, tapc<3>{}, std::false_type{}); fmao(1, r + 14, tapc<3>{}, std::false_type{});
        };
        auto stage = [&](const v2f (&r)[28], const v2f (&p)[28], auto) {           // p[14 chi + 4], p[14 chi + 5]: this stage's cells j = 0, 1
            fmat(0, r, tapc<0>{}, std::false_type{}, p[4], r[2]); fmat(1, r + 14, tapc<0>{}, std::false_type{}, p[14 + 4], r[14 + 2]);
            fmat(0, r, tapc<1>{}, std::false_type{}, p[5], r[3]); fmat(1, r + 14, tapc<1>{}, std::false_type{}, p[14 + 5], r[14 + 3]);
            fmao(0, r, tapc<2>{}, std::false_type{}); fmao(1, r + 14, tapc<2>{}, std::false_type{});
            fmao(0, r, tapc<3>{}, std::false_type{}); fmao(1, r + 14, tapc<3>{}, std::false_type{});
        };
        constexpr int k = 4 * G;                                                   // the left-over tap
        v2f ta[2], tb[2], xb[2];
        auto pre = [&]() {
#pragma unroll
            for (int chi = 0; chi < 2; chi++) {
                ta[chi] = lds2(ht + (chi * 2 + 0) * MP + k); tb[chi] = lds2(ht + (chi * 2 + 1) * MP + k);
                xb[chi] = lds2(ep + chi * 4 * Lph + ((k + 2) & 3) * Lph + ((k + 2) >> 2));
            }
        };
        auto post = [&](const v2f (&r)[28]) {
#pragma unroll
            for (int chi = 0; chi < 2; chi++) {
                cmac(acc[chi][0][0], ta[chi], r[14 * chi + 4]); cmac(acc[chi][0][1], tb[chi], r[14 * chi + 4]);
                cmac(acc[chi][1][0], ta[chi], xb[chi]); cmac(acc[chi][1][1], tb[chi], xb[chi]);
            }
        };
        pipe2_carry<28, false>(G, loadF, loadM, loadL, fma0, stage, pre, post);
        return;
    } else if constexpr (MERGE) {                      // both chi per stage: 28 reads feeding 64 FMAs on 16 chains
        auto load = [&](int g, v2f (&r)[28]) { load1(0, g, r); load1(1, g, r + 14); };
        auto fma = [&](int, const v2f (&r)[28], auto first) {
            fma1(0, r, 0, first); fma1(1, r + 14, 0, first);
#pragma unroll
            for (int t = 1; t < 4; t++) { fma1(0, r, t, std::false_type{}); fma1(1, r + 14, t, std::false_type{}); }
        };
        pipe2<28, true, false>(G, load, fma);
    } else {                                           // one chi after the other (half the operand registers)
#pragma unroll
        for (int chi = 0; chi < 2; chi++) {
            auto load = [&](int g, v2f (&r)[14]) { load1(chi, g, r); };
            auto fma = [&](int, const v2f (&r)[14], auto first) {
                fma1(chi, r, 0, first);
#pragma unroll
                for (int t = 1; t < 4; t++) fma1(chi, r, t, std::false_type{});
            };
            pipe2<14, true, false>(G, load, fma);
        }
    }
#pragma unroll
    for (int k = 4 * G; k < M; k++)                    // remaining 1 or 3 taps
#pragma unroll
        for (int chi = 0; chi < 2; chi++) {
            const float2 *xp = ep + chi * 4 * Lph;
            const v2f a = lds2(ht + (chi * 2 + 0) * MP + k), b = lds2(ht + (chi * 2 + 1) * MP + k);
            const v2f xa = lds2(xp + (k & 3) * Lph + (k >> 2)), xb = lds2(xp + ((k + 2) & 3) * Lph + ((k + 2) >> 2));
            cmac(acc[chi][0][0], a, xa); cmac(acc[chi][0][1], b, xa); cmac(acc[chi][1][0], a, xb); cmac(acc[chi][1][1], b, xb);
        }
}

// Whether the dL/dh (T = B - mh terms per parity) and dL/dw (B / 2 pairs) sums split into NP parts of equal, non-zero length.
constexpr bool uniform_parts(int B, int M, int NP)
{
    const int mh = M / 2, nm = 2 * B - 2 * mh;
    for (int par = 0; par < 2; par++) {
        const int T = (nm - par + 1) >> 1, Th = ((T + 2 * NP - 1) / (2 * NP)) << 1;
        int n0 = -1;
        for (int part = 0; part < NP; part++) {
            const int ma = (part * Th) >> 1, e = part * Th + Th, mb = ((T < e ? T : e) + 1) >> 1;
            if (mb - ma <= 0 || (n0 >= 0 && mb - ma != n0)) return false;
            n0 = mb - ma;
        }
    }
    const int Bq = ((B + 2 * NP - 1) / (2 * NP)) << 1;
    int n0 = -1;
    for (int part = 0; part < NP; part++) {
        const int ma = (part * Bq) >> 1, e = part * Bq + Bq, mb = (B < e ? B : e) >> 1;
        if (mb - ma <= 0 || (n0 >= 0 && mb - ma != n0)) return false;
        n0 = mb - ma;
    }
    return true;
}

// D phase (P3) of the baked B = 100, M = 25 kernel on one wave: the 2 chi x T (T = B - mh = 88) outputs pairs D[chi, 2 tau], D[chi, 2 tau + 1] are
// independent of each other, and 2 T = 176 <= 64 x 3: lane L takes chi = L >> 5 and the TPL = 3 consecutive tau = 3 m + i of m = L & 31; the NM = 30
// lanes m < NM of each half cover tau = 0..T-1, the two lanes beyond shadow m = 0 (no divergence, nothing stored).  Only m = NM - 1 has units past T
// (tau = 88, 89): computed from cells inside the arrays, never stored.  208 complex MACs per lane become 150.
// (No other phase splits like this: FIR, dL/dU and the demapper have 200 independent units > 192, the two tap gradients are sums with pinned parts.)
struct D3Map {
    static constexpr int TPL = 3;                                              // tau per lane
    static constexpr int nm_lanes(int T) { return (T + TPL - 1) / TPL; }       // working lanes per chi
    static constexpr int chi(int lane) { return lane >> 5; }
    static constexpr bool works(int lane, int T) { return (lane & 31) < nm_lanes(T); }
    static constexpr int m(int lane, int T) { return works(lane, T) ? (lane & 31) : 0; }
    static constexpr bool stores(int lane, int i, int T) { return works(lane, T) && TPL * m(lane, T) + i < T; }
    // every (chi, tau < T) is stored by exactly one (lane, i), nothing else is, and no mu cell beyond U[0 .. 2 Uph - 1] is read (a = 0: tau + mh)
    static constexpr bool exact(int B, int M)
    {
        const int mh = M / 2, T = B - mh, Uph = B / 2 + 1;
        if (nm_lanes(T) > 32 || T > 128) return false;
        for (int c = 0; c < 2; c++) {
            int cnt[128] = {};
            for (int lane = 0; lane < 64; lane++)
                for (int i = 0; i < TPL; i++) {
                    const int tau = TPL * m(lane, T) + i;
                    if (tau + mh >= 2 * Uph) return false;
                    if (chi(lane) != c || !stores(lane, i, T)) continue;
                    if (tau >= T) return false;
                    cnt[tau]++;
                }
            for (int tau = 0; tau < 128; tau++)
                if (cnt[tau] != (tau < T ? 1 : 0)) return false;
        }
        return true;
    }
};
static_assert(D3Map::exact(100, 25), "B = 100: three tau per lane must cover tau = 0..87 of both chi exactly once");

// Tap-gradient phases (P4a dL/dh, P5 dL/dw) of the baked B = 100, M = 25 kernel on one wave.  In both sums a lane's two operand streams advance
// together, so two neighbouring taps of one parity share their per-lane operands:
//   dL/dh[chi, nu, j = 2a + par] = sum_tau e[chi, 2 tau + par] conj(U[nu, tau + mh - a]):  tap a + 1 reads at tau + 1 the U cell tap a read at tau,
//   dL/dw[o, p, k = 2a + par]    = sum_n   gy[o, n] conj(x[p, 2n + k]):                    tap a reads at n + 1 the x cell tap a + 1 read at n.
// A lane is (c, half, par, slot): c = chi resp. o, half = which half of the sum range, slot = the tap pair (a, a + 1) = (2 slot, 2 slot + 1) of parity
// par -- the 13 even taps make 7 slots (the last one holds a = 12 alone), the 12 odd taps 6: 13 slots x 2 c = 26 lanes in each 32-lane half, the
// lanes beyond shadow lane 0.  The lane keeps the accumulators [tap of the pair][nu resp. p]; per term it reads ONE cell of its own c (e resp. gy),
// the two cells (nu resp. p = 0, 1) of the pair's READ tap (dL/dh: a, dL/dw: a + 1), and has the other tap's two cells in registers: the read tap's
// cells of the term before (tap_pair_sum).  12 per-lane LDS reads per 32 packed FMAs instead of 16; every output's chain keeps its terms and their order.
// The two halves meet on v_permlane32_swap over the pair: the lower half keeps tap a = 2 slot, the upper half a + 1, both nu resp. p -- that lane owns
// those four reals, their Adam moments and the tap's write to LDS (one map for h and W: lane -> (c, j)).
struct TapPairMap {
    static constexpr int se(int M) { return ((M + 1) / 2 + 1) / 2; }          // slots of the even taps (a = 0 .. (M - 1) / 2)
    static constexpr int ns(int M) { return se(M) + (M / 2 + 1) / 2; }        // ... plus those of the odd taps (a = 0 .. M / 2 - 1)
    static constexpr bool works(int lane, int M) { return (lane & 31) < 2 * ns(M); }
    static constexpr int idx(int lane, int M) { return works(lane, M) ? (lane & 31) : 0; }
    static constexpr int c(int lane, int M) { return idx(lane, M) >= ns(M) ? 1 : 0; }
    static constexpr int s(int lane, int M) { return idx(lane, M) - c(lane, M) * ns(M); }
    static constexpr int par(int lane, int M) { return s(lane, M) >= se(M) ? 1 : 0; }
    static constexpr int alo(int lane, int M) { return 2 * (s(lane, M) - par(lane, M) * se(M)); }      // the pair's lower tap
    static constexpr int tap(int lane, int M, int x) { return 2 * (alo(lane, M) + x) + par(lane, M); }  // j resp. k of the pair's tap x = 0, 1
    static constexpr int kept(int lane, int M) { return tap(lane, M, lane >> 5); }                       // the tap whose sum the lane ends up with
    static constexpr bool owns(int lane, int M) { return works(lane, M) && kept(lane, M) < M; }
    // which half of the sum range the lane takes.  dL/dh: chi = 1 takes them the other way round (a sum's two halves still sit 32 lanes apart and
    // their addition commutes) -- the e rows of the two chi are a multiple of 64 banks apart, and with equal offsets the two chi of a half-wave
    // would collide on every e read (tools/lds_bank_model.py dp_tappair: 2 passes, 1 this way); gy, x and U have no such collision
    static constexpr int part_h(int lane, int M) { return (lane >> 5) ^ c(lane, M); }
    static constexpr int part_w(int lane) { return lane >> 5; }
    static constexpr int dh_pairs(int B, int M) { return (B - M / 2) / 4; }    // (tau, tau + 1) pairs per half of dL/dh; (n, n + 1) pairs per half of dL/dw:
    static constexpr int dw_pairs(int B) { return B / 4; }                     // what uniform_parts() finds for two parts
    // every (c, j < M, half) is summed by exactly one lane and every (c, j < M) kept by exactly one; no consumed read leaves its array: U[nu][0 .. 2 Uph - 1],
    // e and x cells below 2 B + M - 1 (a tap past M - 1, the upper tap of the slot that holds a = 12 alone: inside the phase rows), gy[o][0 .. B - 1]
    static constexpr bool exact(int B, int M)
    {
        const int mh = M / 2, Mh = 2 * mh, nm = 2 * B - Mh, T = nm / 2, Uph = B / 2 + 1, len = 2 * B + M - 1, Lph = wave_lph(len);
        if (M > 31 || (mh & 1) || (nm & 1) || (T & 3) || (B & 3) || 2 * ns(M) > 32 || !uniform_parts(B, M, 2)) return false;
        int sumh[2][32][2] = {}, sumw[2][32][2] = {}, own[2][32] = {};
        for (int lane = 0; lane < 64; lane++) {
            const int p = par(lane, M), a = alo(lane, M);
            if (works(lane, M))
                for (int x = 0; x < 2; x++)
                    if (tap(lane, M, x) < M) {
                        sumh[c(lane, M)][tap(lane, M, x)][part_h(lane, M)]++;
                        sumw[c(lane, M)][tap(lane, M, x)][part_w(lane)]++;
                    }
            if (c(lane, M) != c(lane ^ 32, M) || tap(lane, M, 0) != tap(lane ^ 32, M, 0)) return false;   // the two halves of a sum: 32 lanes apart
            if (owns(lane, M)) own[c(lane, M)][kept(lane, M)]++;
            // dL/dh: read tap a, pairs m = ma .. ma + n - 1: e cells Mh + par + 4 m (+ 2), U cells 2 m + mh - a (+ 1); the term before the first: one cell lower
            const int nh = dh_pairs(B, M), mah = part_h(lane, M) * nh;
            const bool up = tap(lane, M, 1) < M;                                // the pair's upper tap exists (else its first operand is read from the read tap's cell)
            if (2 * mah + mh - a - (up ? 1 : 0) < 0 || 2 * (mah + nh - 1) + mh - a + 1 >= 2 * Uph) return false;
            if (Mh + p + 4 * (mah + nh - 1) + 2 >= len) return false;
            // dL/dw: read tap k = tap(., 1), pairs m: x cells k + 4 m (+ 2), gy cells 2 m, 2 m + 1; the term before the first: x cell k + 4 ma - 2
            const int nw = dw_pairs(B), maw = part_w(lane) * nw, k = tap(lane, M, 1);
            if (2 * (maw + nw - 1) + 1 >= B) return false;
            if (k + 4 * (maw + nw - 1) + 2 >= (up ? len : 4 * Lph)) return false;
        }
        for (int cc = 0; cc < 2; cc++)
            for (int j = 0; j < 32; j++) {
                if (own[cc][j] != (j < M ? 1 : 0)) return false;
                for (int hf = 0; hf < 2; hf++)
                    if (sumh[cc][j][hf] != (j < M ? 1 : 0) || sumw[cc][j][hf] != (j < M ? 1 : 0)) return false;
            }
        return true;
    }
};
static_assert(TapPairMap::exact(100, 25), "B = 100: the tap pairs must sum every (c, tap, half) once, own every (c, tap) once and read inside their arrays");

// One half of the tap-gradient sums of a TapPairMap lane over the N pairs m = 0 .. N - 1 of its range: for y = 0, 1 (nu resp. p)
//   acc[0][y] = sum_m  tA_y(m) (x) sA(m)       + tB_y(m) (x) sB(m)        -- the pair's read tap,
//   acc[1][y] = sum_m  tB_y(m - 1) (x) sA(m)   + tA_y(m) (x) sB(m)        -- its other tap, whose operands are the read tap's one term earlier,
// with sA(m) = sA[SS m], sB(m) = sB[SS m], tA_y(m) = tA[y TN + m], tB_y(m) = tB[y TN + m] and tB_y(-1) = tC[y TN].  Every sum keeps the two
// sub-chains of the plain loops (the first addend of each m into one, the second into the other, the first term starting the chain, the two added
// once at the end).  A stage is two pairs: 12 LDS reads feeding 32 packed FMAs, two-deep like pipe2 (loads run one stage past the end, never consumed,
// inside the LDS allocation).  The last two reads of a stage (tB of its second pair) are what the next stage's first FMAs (head) take from registers:
// the stage after that loads them behind its predecessor's head, into the registers just freed -- no copies on the back edge.
template <int N, int SS>
__device__ __forceinline__ void tap_pair_sum(cacc (&ca)[2][2], const float2 *sA, const float2 *sB, const float2 *tA, const float2 *tB, int TN,
                                             const float2 *tC)
{
    constexpr int NST = N / 2;
    static_assert(NST >= 2, "at least two stages");
    cacc cb[2][2];
    auto loadM = [&](int i, v2f (&r)[12]) {
        const int m = 2 * i;
        r[0] = lds2(sA + SS * m); r[1] = lds2(sB + SS * m); r[2] = lds2(tA + m); r[3] = lds2(tA + TN + m); r[4] = lds2(tB + m); r[5] = lds2(tB + TN + m);
        r[6] = lds2(sA + SS * (m + 1)); r[7] = lds2(sB + SS * (m + 1)); r[8] = lds2(tA + m + 1); r[9] = lds2(tA + TN + m + 1);
    };
    auto loadL = [&](int i, v2f (&r)[12]) { r[10] = lds2(tB + 2 * i + 1); r[11] = lds2(tB + TN + 2 * i + 1); };
    auto head = [&](const v2f (&r)[12], const v2f (&p)[12], auto first) {      // p: the stage before
        constexpr bool F = decltype(first)::value;
        // pin: the cells used as taps stay 8-byte registers up to their use (the optimiser otherwise splits the sets that live across the loop's back edge
        // into halves at their loads: copies behind s_waitcnt lgkmcnt(9..0) at the end of every trip, see D3Map's loop)
        v2f q0 = p[10], q1 = p[11];
        asm volatile("" : "+v"(q0), "+v"(q1));
        cmacf<F>(ca[1][0], q0, r[0]); cmacf<F>(ca[1][1], q1, r[0]);
        asm volatile("" : "+v"(ca[1][0].a), "+v"(ca[1][0].b), "+v"(ca[1][1].a), "+v"(ca[1][1].b));   // (volatile: stays in front of the loads into p[10], p[11])
    };
    auto rest = [&](const v2f (&r)[12]) {
        v2f a0 = r[2], a1 = r[3], b0 = r[4], b1 = r[5];
        asm volatile("" : "+v"(a0), "+v"(a1), "+v"(b0), "+v"(b1));            // (pin: see head)
        cmac(ca[0][0], a0, r[0]); cmac(ca[0][1], a1, r[0]); cmac(cb[0][0], b0, r[1]); cmac(cb[0][1], b1, r[1]);
        cmac(cb[1][0], a0, r[1]); cmac(cb[1][1], a1, r[1]);
        v2f c0 = r[8], c1 = r[9];
        asm volatile("" : "+v"(c0), "+v"(c1) : "v"(r[10]), "v"(r[11]));        // (r[10], r[11] live on into the next stage's head: inputs only, or they are copied)
        cmac(ca[0][0], c0, r[6]); cmac(ca[0][1], c1, r[6]); cmac(cb[0][0], r[10], r[7]); cmac(cb[0][1], r[11], r[7]);
        cmac(ca[1][0], b0, r[6]); cmac(ca[1][1], b1, r[6]); cmac(cb[1][0], c0, r[7]); cmac(cb[1][1], c1, r[7]);
    };
    // the first stage starts the chains.  Which of a chain's first two products is rounded on its own is part of the pinned bits: in the plain loops the
    // backend contracts  t0 v0 + t1 v1  of the first sub-chain as fma(t1, v1, t0 v0) and of the second as fma(t0, v0, t1 v1).  Spelled out and pinned here
    auto rest0 = [&](const v2f (&r)[12]) {
        cmul(ca[0][0], r[2], r[0]); cmul(ca[0][1], r[3], r[0]);
        cmul(cb[0][0], r[10], r[7]); cmul(cb[0][1], r[11], r[7]); cmul(cb[1][0], r[8], r[7]); cmul(cb[1][1], r[9], r[7]);
        asm volatile("" : "+v"(ca[0][0].a), "+v"(ca[0][0].b), "+v"(ca[0][1].a), "+v"(ca[0][1].b));
        asm volatile("" : "+v"(cb[0][0].a), "+v"(cb[0][0].b), "+v"(cb[0][1].a), "+v"(cb[0][1].b));
        asm volatile("" : "+v"(cb[1][0].a), "+v"(cb[1][0].b), "+v"(cb[1][1].a), "+v"(cb[1][1].b));
        cmac(cb[0][0], r[4], r[1]); cmac(cb[0][1], r[5], r[1]); cmac(cb[1][0], r[2], r[1]); cmac(cb[1][1], r[3], r[1]);
        cmac(ca[0][0], r[8], r[6]); cmac(ca[0][1], r[9], r[6]); cmac(ca[1][0], r[4], r[6]); cmac(ca[1][1], r[5], r[6]);
    };
    v2f A[12], B[12];
    B[10] = lds2(tC); B[11] = lds2(tC + TN);
    loadM(0, A); loadL(0, A); loadM(1, B);
    head(A, B, std::true_type{}); loadL(1, B); rest0(A);
    int i = 1;
#pragma unroll 1
    for (; i + 1 < NST; i += 2) {                          // B holds stage i, A[10], A[11] what is left of stage i - 1
        loadM(i + 1, A); head(B, A, std::false_type{}); loadL(i + 1, A); rest(B);
        loadM(i + 2, B); head(A, B, std::false_type{}); loadL(i + 2, B); rest(A);
    }
    constexpr bool LB = NST % 2 == 0;                      // the last stage is in B (and still to do), else in A (done)
    v2f t[6];
    if constexpr (N & 1) {                                 // an odd last pair: its reads go out before the last stage's FMAs
        constexpr int m = N - 1;
        t[0] = lds2(sA + SS * m); t[1] = lds2(sB + SS * m); t[2] = lds2(tA + m); t[3] = lds2(tA + TN + m); t[4] = lds2(tB + m); t[5] = lds2(tB + TN + m);
    }
    if constexpr (LB) { head(B, A, std::false_type{}); rest(B); }
    if constexpr (N & 1) {
        const v2f (&p)[12] = LB ? B : A;
        cmac(ca[1][0], p[10], t[0]); cmac(ca[1][1], p[11], t[0]); cmac(ca[0][0], t[2], t[0]); cmac(ca[0][1], t[3], t[0]);
        cmac(cb[0][0], t[4], t[1]); cmac(cb[0][1], t[5], t[1]); cmac(cb[1][0], t[2], t[1]); cmac(cb[1][1], t[3], t[1]);
    }
#pragma unroll
    for (int x = 0; x < 2; x++)
#pragma unroll
        for (int y = 0; y < 2; y++) { ca[x][y].a += cb[x][y].a; ca[x][y].b += cb[x][y].b; }
}

// OUT: 0 = every output nullable at run time; 1 = no compact outputs (eq_out / dec_out ignored); 2 = compact outputs, q not written.
// The specialisations only drop dead code: fewer live scalars, fewer SGPR spills in the step loop.
// NW = wavefronts per run: 1 (B <= 128, no barriers at all) or 2 / 4 / 8 (B <= 256 / 512 / 1024): thread gl = 64 wv + lane owns the symbol pair
// (2 gl, 2 gl + 1), the tap-gradient sums are split 2 NW ways, wave 0 owns the taps and their Adam moments; phases are separated
// by s_barrier after an LDS-only wait (sync_lds), so the in-flight q / y stores still never stall a phase.
template <int M, int NLEV, int BT, bool PAIR, int OUT, int NW = 1, int BL = 0>
__global__ __launch_bounds__(64 * NW, VAEQ_WPS) void dp_wave_kernel(const vaeq_dp_args a)
{
    constexpr int mh = M / 2, Mh = 2 * mh, MP = M + 1;
    constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;
    extern __shared__ float4 smem4[];
    char *sm = reinterpret_cast<char *>(smem4);
    const int gl = threadIdx.x, lane = NW > 1 ? (gl & 63) : gl, wv = NW > 1 ? (gl >> 6) : 0, run = blockIdx.x;
    constexpr int NT = 64 * NW, NP = 2 * NW;              // threads per run; parts a tap-gradient sum is split into
    // baked shape whose tap-gradient sums split into NP equal, non-empty parts: their loops run on a scalar trip count and start from the first term
    constexpr bool UNI = BT > 0 && uniform_parts(BT, M, NP);
    // BL > 0 (with BT == 0): the LDS LAYOUT of minibatch length BL (all offsets and strides immediate) for any run-time B <= BL of BL's parity class
    // (M = 13 / 17 on a fixed layout: the pipelined form unrolls into 27-117 spilled registers and loses 25-38 %: they keep the lean loops; so
    //  does M = 31 at one wavefront per run, where it costs 2-5 %)
    constexpr bool FIXL = BT > 0 || (BL > 0 && M != 13 && M != 17 && !(M == 31 && NW == 1));
    constexpr bool PIPE = VAEQ_PIPE && FIXL;               // run-time layouts keep more addresses live: there one operand set,
    constexpr bool WIDE = FIXL;                            // ... 8 accumulator chains and one chi at a time in dL/dU (fits the register file)
    // B100: the baked B = 100 kernel on one wave, the shape that is measured step by step and whose bits are pinned (tests/test_dp_wave_bits_gpu.py).
    // It alone takes eight forms; every other instantiation keeps the plain one, instruction for instruction:
    //  * the halves of the two tap gradients meet on v_permlane32_swap (half_sum2: one swap per kept value, one packed add per pair) instead of 16 ds_bpermute_b32
    //    through __shfl_xor(., 32) per step: the same two addends per sum, bitwise the same taps; 8.09 -> 7.91 ms (profiles/r04/kernel_variants_ab.txt)
    //  * the next window's prefetch is issued without a branch around it (the launch's very last step fetches with every lane out of range: zeros, no
    //    memory access).  Behind the branch the four loads fed a phi: the backend copied their results right after the issue, behind
    //    s_waitcnt vmcnt(3..0) -- every step stood there for the loads' HBM latency and, vmcnt retiring in order, for every q / y store still in
    //    flight.  Now the first wait for them is P0 of the next step (profiles/r05/kernel_variants_ab.txt)
    //  * the q stores leave with the streaming ("nt") cache policy: 32 rows x 400 B per wave-step that nothing reads back before the launch ends
    //    (profiles/r05/kernel_variants_ab.txt; what the stores cost in total: profiles/r05/q_store_bound.txt)
    //  * (M = 25) the D convolution of P3 runs three tau of one chi per lane on 60 lanes (D3Map) instead of two tau of both chi on 44: 300 instead of 416
    //    packed FMAs per lane, every output's chain of FMAs in its old order; the residual's energy sum reads e back from LDS on its old lanes
    //    (profiles/r06/kernel_variants_ab.txt)
    //  * (M = 25) the two tap gradients run on tap-pair lanes (TapPairMap, TP below): a lane sums two neighbouring taps of one parity for one chi resp. o
    //    and takes the second tap's operands from the registers of the first: 12 instead of 16 per-lane LDS reads per 32 packed FMAs, every output's
    //    chain in its old order; the lane that ends up with a tap's sum owns the tap and its Adam moments
    //    (profiles/r07/tapgrad_lds_bound.txt, profiles/r07/kernel_variants_ab.txt)
    //  * (M = 25) the FIR, dL/dU and the D convolution carry the cells that consecutive stages share in registers (CellCarry, pipe2_carry): 12 instead of
    //    14, 24 instead of 28 and 6 instead of 8 per-lane LDS reads per stage, every output's chain in its old order
    //    (profiles/r08/cell_carry_bound.txt, profiles/r08/kernel_variants_ab.txt)
    //  * the step's five wave sums and two variance scans run as interleaved DPP chains whose masked steps are one instruction each (vaeq_wave.h: *_dpp_keep),
    //    the half combines and both Adam updates work on (re, im) register pairs (half_sum2, adam_update_fast2), and every lane runs the updates, only what
    //    leaves the lane being masked: 101 of the step's 1621 straight-line vector instructions were moves, selects and zeros for this
    //    (profiles/r09/kernel_variants_ab.txt)
    //  * (M = 25) the taps of the FIR and dL/dU loops arrive as 16-byte reads, two neighbouring taps each (lds4, Tap16: the float4 of a FIR tap, an aligned pair
    //    of an Ht row), and the MACs on a read's high pair (FIR: on both pairs) are the two v_pk_fma_f32 the backend emits for them anyway, written out with their op_sel (cmac16), so
    //    that no dword is copied on the way: 100 instead of 200 tap reads per wave-step for the same LDS cycles, every output's chain in its old order
    //    (profiles/r10/kernel_variants_ab.txt)
    constexpr bool B100 = BT == 100 && NW == 1;
    constexpr bool CARRY = B100 && M == 25 && PIPE && WIDE;
    constexpr int QAUX = B100 ? 2 : 0;                         // cache policy of the q stores
    const int B = BT ? BT : a.B;
    const int BS = BT ? BT : BL ? BL : B;                      // the minibatch length the LDS layout (offsets, row strides) is made for
    // ODDB: on a class layout (BL) the minibatch length may be odd -- the last lane's pair is (B - 1, phantom): the phantom symbol is computed like
    // any other (from zero-padded cells) and masked wherever it would be stored or summed (v1 below); baked shapes are even and unchanged
    constexpr bool ODDB = BT == 0 && BL > 0;
    const int L = 2 * B, nm = L - Mh, P2 = ODDB ? (B + 1) / 2 : B / 2;
    const float rnm = 1.0f / (float)nm;
    const WaveLayout lay = wave_layout(BS, M, NW);
    const int Lph = lay.Lph, Uph = lay.Uph;
    float2 *Xs = reinterpret_cast<float2 *>(sm + lay.X), *Es = reinterpret_cast<float2 *>(sm + lay.E);
    float2 *Us = reinterpret_cast<float2 *>(sm + lay.U), *GY = Us;
    float4 *Wt = reinterpret_cast<float4 *>(sm + lay.W);       // [p][k] = (wr[o0], wi[o0], wr[o1], wi[o1])
    float2 *Ht = reinterpret_cast<float2 *>(sm + lay.H);       // [chi][nu][j] = (re, im), j = 0..M (j = M: zero pad)
    float *PSv = reinterpret_cast<float *>(sm + lay.PSv);      // [nu][B+1] exclusive prefix sums of v_I + v_Q
    float *PSh = reinterpret_cast<float *>(sm + lay.PSh);      // [nu][M+1] exclusive prefix sums of sum_chi gC |h|^2
    float *VS = reinterpret_cast<float *>(sm + lay.VS);        // [nu][M]
    float *RED = reinterpret_cast<float *>(sm + lay.RED), *XG = reinterpret_cast<float *>(sm + lay.XG);   // NW > 1 only

    // ---- per-run constants (uniform)
    float amp[NLEV], b2[NLEV], nlogP[NLEV];
    const float nusc = a.nu_sc[run];
#pragma unroll
    for (int i = 0; i < NLEV; i++) {
        amp[i] = a.amp[i];
        b2[i] = nusc * amp[i] * amp[i] * LOG2E;
        nlogP[i] = -logf(a.P[(size_t)run * NLEV + i]);
    }
    const float var0 = a.var[run * 2 + 0], var1 = a.var[run * 2 + 1];
    const float lrW = a.lr_W[run], lrH = a.lr_h[run];

    // ---- zero the halo'd buffers once; load taps; owner lanes load their Adam moments
    for (int i = gl; i < (lay.W - lay.X) / 8; i += NT) Xs[i] = make_float2(0.f, 0.f);     // X, E, U, PSv
    for (int i = gl; i < (lay.PSh - lay.H) / 8; i += NT) Ht[i] = make_float2(0.f, 0.f);   // incl. the pad taps
    __syncthreads();
    const int tk = lane & 31, half = lane >> 5;                // tap index / which half this lane owns (o resp. chi)
    const bool worker = tk < M, owner = worker && wv == 0;     // worker: sums a part of a tap's gradient; owner: holds the tap
    const int part = wv * 2 + half;
    const size_t gbase = (size_t)run * 8 * M;
    // which taps a lane owns (state in / out, Adam moments, the tap's write to LDS): W[o = oc][.][k = tj] and h[chi = oc][.][j = tj].  Plain form: the
    // lane that summed tap tk keeps half's part (oc = half, tj = tk); TP: the tap-pair lanes of TapPairMap
    constexpr bool TP = BT == 100 && NW == 1 && M == 25;
    int oc = half, tj = tk;
    bool ownr = owner;
    if constexpr (TP) {
        oc = TapPairMap::c(lane, M);
        tj = TapPairMap::kept(lane, M);
        ownr = TapPairMap::owns(lane, M);
    }
    // Adam moments of the taps this lane owns live in LDS, one 64-lane row per quantity (touched twice per step; 16 VGPRs freed):
    // rows 0-7: m, v of W[o=oc][p][k=tj] (re, im); rows 8-15: m, v of h[chi=oc][nu][.][j=tj]; within each block of four rows [im][p]
    float *MOM = reinterpret_cast<float *>(sm + lay.MOM) + lane;
    // (B = 100: the rows of a (re, im) pair are neighbours -- rows 2 p, 2 p + 1 of each block of four -- so that the two reads the backend fuses into one
    //  ds_read2st64_b32 are the pair the update works on, adam_update_fast2)
#define VAEQ_MOM(base, im, p) MOM[((base) + (BT == 100 && NW == 1 ? 2 * (p) + (im) : 2 * (im) + (p))) * 64]
#define mWr(p) VAEQ_MOM(0, 0, p)
#define mWi(p) VAEQ_MOM(0, 1, p)
#define vWr(p) VAEQ_MOM(4, 0, p)
#define vWi(p) VAEQ_MOM(4, 1, p)
#define mHr(p) VAEQ_MOM(8, 0, p)
#define mHi(p) VAEQ_MOM(8, 1, p)
#define vHr(p) VAEQ_MOM(12, 0, p)
#define vHi(p) VAEQ_MOM(12, 1, p)
    if (ownr) {
#pragma unroll
        for (int p = 0; p < 2; p++) {
            const size_t ir = gbase + (oc * 4 + p) * M + tj, ii = gbase + (oc * 4 + 2 + p) * M + tj;
            float *wq = reinterpret_cast<float *>(&Wt[p * M + tj]);
            wq[oc * 2 + 0] = a.W[ir];
            wq[oc * 2 + 1] = a.W[ii];
            mWr(p) = a.adam_mW[ir]; mWi(p) = a.adam_mW[ii];
            vWr(p) = a.adam_vW[ir]; vWi(p) = a.adam_vW[ii];
            const size_t hr = gbase + ((oc * 2 + p) * 2 + 0) * M + tj, hi = hr + M;
            Ht[(oc * 2 + p) * MP + tj] = make_float2(a.h[hr], a.h[hi]);
            mHr(p) = a.adam_mh[hr]; mHi(p) = a.adam_mh[hi];
            vHr(p) = a.adam_vh[hr]; vHi(p) = a.adam_vh[hi];
        }
    }
    int step = a.step[run];
    // beta^t at the start of each of the launch's first VAEQ_BT_FRAMES frames, evaluated here, where no register is under pressure yet (one pow call
    // site, a lane per frame), and picked up at the frame heads; inside a frame it is a running product in double
    __shared__ double BTW[2][VAEQ_BT_FRAMES];
    if (gl < VAEQ_BT_FRAMES && gl < a.n_frames) {
        const double t = (double)(step + gl * a.steps);
        BTW[0][gl] = pow(0.9, t);
        BTW[1][gl] = pow(0.999, t);
    }
    __syncthreads();
    double b1t = BTW[0][0], b2t = BTW[1][0];

    const int klen = a.keep_len, k0 = a.keep_off;
    const size_t No = (size_t)a.steps * klen;
    constexpr bool pairst = PAIR;                              // keep_off, keep_len even: both symbols of a lane kept together -> 8-byte stores
    const bool act = gl < P2;                                  // thread owns symbols 2*gl, 2*gl+1
    const int nq = (nm + 3) / 4;                               // residual quads t = 4l' .. 4l'+3
    const int n0 = 2 * gl;
    const bool v1 = ODDB ? act && (n0 + 1 < B) : act;       // the lane's second symbol exists
    const float2 *Xl = Xs + gl, *El = Es + gl, *Ul = Us + gl;
    const float2 *Xa = Xs + (act ? gl : 0), *Ea = Es + (act ? gl : 0);   // symbol-pair phases: idle lanes shadow lane 0 (results unused)

    // The window of the NEXT step is fetched into registers while the current step computes (one 16-byte load per lane and
    // row: B <= 128 means L/4 <= 64 lanes), so a step never waits for HBM after the first.
    const bool ldl = gl < (ODDB ? (L + 3) / 4 : L / 4);         // odd B: L = 2 (mod 4), the last lane's upper two samples belong to the next minibatch
    float4 pf[4];
    const uint32_t S4 = (uint32_t)a.S * 4u;                    // bytes per received row; a frame of a run = 4 rows
    auto frame_rsrc = [&](int f) { return make_rsrc(a.rx + ((size_t)run * a.n_frames + f) * 4 * (size_t)a.S, 4u * S4); };
    auto fetch = [&](const __amdgpu_buffer_rsrc_t xr, int s) {
        const uint32_t vo = ldl ? ((uint32_t)s * (uint32_t)a.stride_sym * 2u + 4u * gl) * 4u : OOB;   // lanes beyond the window read zeros
#pragma unroll
        for (int r = 0; r < 4; r++) pf[r] = bld128(xr, vo, (uint32_t)r * S4);
    };
#ifdef VAEQ_PHASE_STAMPS
    long long tst[VAEQ_NSTAMP], tsx[8];
#endif
    fetch(frame_rsrc(0), 0);
    for (int f = 0; f < a.n_frames; f++) {
        const __amdgpu_buffer_rsrc_t xr = frame_rsrc(f), xn = frame_rsrc(f + 1 < a.n_frames ? f + 1 : f);   // this frame's rows, the next frame's
        if (f && f < VAEQ_BT_FRAMES) {                         // beta^t restarts from pow() at every frame, as it does at a launch: how many frames a
            b1t = BTW[0][f];                                    // launch holds is a scheduling choice, the results are bit-identical either way
            b2t = BTW[1][f];                                    // (dp_runs.run_dp_batch groups the frames of small sweeps)
        }
        // one buffer descriptor per output array and frame; rows are addressed by scalar offsets (row * No4) folded into the stores
        const bool qf = OUT != 2 && a.q_out, yf = a.y_out, ef = OUT != 1 && a.eq_out, df = OUT != 1 && a.dec_out;
        const uint32_t No4 = (uint32_t)No * 4u;
        const size_t fr = (size_t)run * a.n_frames + f;
        const __amdgpu_buffer_rsrc_t qr = make_rsrc(qf ? a.q_out + fr * (4 * NLEV) * No : nullptr, qf ? 4u * NLEV * No4 : 0u);
        const __amdgpu_buffer_rsrc_t yr = make_rsrc(yf ? a.y_out + fr * 4 * No : nullptr, yf ? 4u * No4 : 0u);
        const __amdgpu_buffer_rsrc_t er = make_rsrc(ef ? a.eq_out + fr * 2 * No : nullptr, ef ? 2u * No4 : 0u);
        const __amdgpu_buffer_rsrc_t dr = make_rsrc(df ? a.dec_out + fr * 4 * No : nullptr, df ? (uint32_t)(4 * No) : 0u);
        const __amdgpu_buffer_rsrc_t lr_ = make_rsrc(a.loss ? a.loss + fr * a.steps : nullptr, a.loss ? (uint32_t)a.steps * 4u : 0u);
        const __amdgpu_buffer_rsrc_t vr_ = make_rsrc(a.var_est ? a.var_est + fr * 2 * a.steps : nullptr, a.var_est ? (uint32_t)a.steps * 8u : 0u);
#pragma unroll 1
        for (int s = 0; s < a.steps; s++) {
            VAEQ_STAMP(0);
            // ============ P0: prefetched window -> LDS (polyphase scatter; halo stays zero)
            if (ldl) {
#pragma unroll
                for (int p = 0; p < 2; p++) {
                    const float4 I4 = pf[p * 2 + 0], Q4 = pf[p * 2 + 1];
                    const float xi[4] = {I4.x, I4.y, I4.z, I4.w}, xq[4] = {Q4.x, Q4.y, Q4.z, Q4.w};
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const int c = mh + i;                  // + 4*lane: phase (c & 3) is lane independent
                        const bool in = !ODDB || 4 * gl + i < L;
                        Xs[(p * 4 + (c & 3)) * Lph + gl + (c >> 2)] = in ? make_float2(xi[i], xq[i]) : make_float2(0.f, 0.f);
                    }
                }
            }
            sync_lds<NW>();

            VAEQ_STAMP(1);
            // ============ P1: FIR for the lane's symbol pair, both output polarisations
            float2 y[2][2];                                    // [sym][o]
            {
                cacc ya[2][2], yb[2][2];                       // lanes without a symbol pair recompute lane 0's (Xa): no divergence, nothing to zero
                pair_fir<M, true, PIPE, WIDE, CARRY>(ya, yb, Xa, Lph, Wt);   // (CARRY: per p -- the carry restarts where the array changes)
                pair_fir<M, false, PIPE, WIDE, CARRY>(ya, yb, Xa + 4 * Lph, Lph, Wt + M);
#pragma unroll
                for (int sy = 0; sy < 2; sy++)
#pragma unroll
                    for (int o = 0; o < 2; o++) {
                        if constexpr (WIDE) {
                            ya[sy][o].a += yb[sy][o].a;
                            ya[sy][o].b += yb[sy][o].b;
                        }
                        y[sy][o] = cfin(ya[sy][o]);
                    }
            }
            // pin: hipcc otherwise sinks whole FMA chains to their (much later) use and keeps their inputs alive instead
            asm volatile("" : "+v"(y[0][0].x), "+v"(y[0][0].y), "+v"(y[0][1].x), "+v"(y[0][1].y), "+v"(y[1][0].x), "+v"(y[1][0].y),
                         "+v"(y[1][1].x), "+v"(y[1][1].y));
            VAEQ_STAMP(2);
            const bool kept0 = act && (n0 >= k0) && (n0 < k0 + klen), kept1 = act && (n0 + 1 >= k0) && (n0 + 1 < k0 + klen);
            const uint32_t col = (uint32_t)(s * klen + (n0 - k0));
            const uint32_t vo0 = kept0 ? col * 4u : OOB, vo1 = kept1 ? col * 4u + 4u : OOB;     // byte offsets inside a row; OOB = not stored
            if (yf) {
                uint32_t yrow = 0u;                            // rows (o, re / im) in ascending order: a running scalar offset (see qrow below)
                auto next_row = [&]() {
                    yrow += No4;
                    asm volatile("" : "+s"(yrow));
                };
#pragma unroll
                for (int o = 0; o < 2; o++) {
                    const uint32_t r0 = yrow;
                    next_row();
                    const uint32_t r1 = yrow;
                    next_row();
                    if (pairst) {
                        bst64(v2f{y[0][o].x, y[1][o].x}, yr, vo0, r0);
                        bst64(v2f{y[0][o].y, y[1][o].y}, yr, vo0, r1);
                    } else {
                        bst32(y[0][o].x, yr, vo0, r0); bst32(y[0][o].y, yr, vo0, r1);
                        bst32(y[1][o].x, yr, vo1, r0); bst32(y[1][o].y, yr, vo1, r1);
                    }
                }
            }

            VAEQ_STAMP(3);
            // ============ P2: soft demap + moments (registers), mu -> LDS, prefix sums of the variances
            float mv[2][2][2], mt3[2][2][2], mkc[2][2][2];     // [sym][o][c]: Var_q, 3rd central moment, KL-gradient moment
            // the 4 n rows of q leave in ascending order: their byte offset is ONE running scalar (an s_add per row) -- as 32 products row * No4 they
            // were 32 live scalars, spilled and fetched back with v_readlane + hazard s_nops in front of every store
            uint32_t qrow = 0u;
            float klsum = 0.f, vv[2][2];                       // vv[o][sym] = v_I + v_Q
#pragma unroll
            for (int o = 0; o < 2; o++) {
                const float c2 = 0.5f / (o ? var1 : var0) * LOG2E;
                float2 muv[2];                                 // per sym: (mu_I, mu_Q)
#pragma unroll
                for (int c = 0; c < 2; c++) {
                    // both symbols of the lane at once: every add/mul/fma below is one packed instruction (v_pk_*_f32)
                    const v2f yy = c ? v2f{y[0][o].y, y[1][o].y} : v2f{y[0][o].x, y[1][o].x};
                    v2f z[NLEV], q[NLEV];
                    v2f ssum = {0.f, 0.f};
                    float zm0 = -3.0e38f, zm1 = -3.0e38f;
#pragma unroll
                    for (int i = 0; i < NLEV; i++) {
                        const v2f d = yy - amp[i];
                        z[i] = -(d * d * c2 + b2[i]);
                        zm0 = fmaxf(zm0, z[i].x);
                        zm1 = fmaxf(zm1, z[i].y);
                    }
                    const v2f zmax = {zm0, zm1};
#pragma unroll
                    for (int i = 0; i < NLEV; i++) {
                        z[i] -= zmax;
                        q[i] = v2f{__builtin_amdgcn_exp2f(z[i].x), __builtin_amdgcn_exp2f(z[i].y)};
                        ssum += q[i];
                    }
                    const v2f rs = {__builtin_amdgcn_rcpf(ssum.x), __builtin_amdgcn_rcpf(ssum.y)};
                    v2f m1 = {0.f, 0.f};
#pragma unroll
                    for (int i = 0; i < NLEV; i++) {
                        q[i] *= rs;
                        m1 += q[i] * amp[i];
                    }
                    // compact stand-ins for q in the epilogue: E_q[x_I] and the first maximum of q, exactly as it would derive them
                    if (ef && c == 0) {
                        if (pairst) bst64(m1, er, vo0, (uint32_t)o * No4);
                        else { bst32(m1.x, er, vo0, (uint32_t)o * No4); bst32(m1.y, er, vo1, (uint32_t)o * No4); }
                    }
                    if (df) {
                        float v0 = q[0].x, v1 = q[0].y;
                        int b0 = 0, b1 = 0;
#pragma unroll
                        for (int i = 1; i < NLEV; i++) {
                            if (q[i].x > v0) { v0 = q[i].x; b0 = i; }
                            if (q[i].y > v1) { v1 = q[i].y; b1 = i; }
                        }
                        const uint32_t ro = (uint32_t)(o * 2 + c) * (uint32_t)No;                 // one byte per decision
                        if (pairst) bst16((unsigned short)(b0 | (b1 << 8)), dr, kept0 ? col : OOB, ro);
                        else { bst8((unsigned char)b0, dr, kept0 ? col : OOB, ro); bst8((unsigned char)b1, dr, kept1 ? col + 1u : OOB, ro); }
                    }
                    // log(q_i/P_i) = z_i ln2 - log(ssum) - log P_i: the softmax's own logits; the +1e-12 inside the reference's
                    // log and the q/(q+eps P) factor of its derivative change q*log(.) by < 1e-12, and the terms
                    // common to all levels cancel in the centred sum
                    v2f m2 = {0.f, 0.f}, m3 = {0.f, 0.f}, kk = {0.f, 0.f}, kl = {0.f, 0.f};
#pragma unroll
                    for (int i = 0; i < NLEV; i++) {
                        const v2f d = amp[i] - m1, qd = q[i] * d, g = z[i] * LN2 + nlogP[i];
                        m2 += qd * d;
                        m3 += qd * d * d;
                        kk += qd * g;
                        kl += q[i] * g;
                    }
                    const bool inr0 = (n0 >= mh) && (n0 < B - mh) && act;             // KL slice, symbol index (:132)
                    const bool inr1 = (n0 + 1 >= mh) && (n0 + 1 < B - mh) && act;
                    if (inr0) klsum += kl.x - __builtin_amdgcn_logf(ssum.x) * LN2;
                    if (inr1) klsum += kl.y - __builtin_amdgcn_logf(ssum.y) * LN2;
                    asm volatile("" : "+v"(m2), "+v"(m3), "+v"(kk), "+v"(klsum));   // pin (see P1)
                    mv[0][o][c] = m2.x; mv[1][o][c] = m2.y;
                    mt3[0][o][c] = m3.x; mt3[1][o][c] = m3.y;
                    mkc[0][o][c] = inr0 ? kk.x : 0.f;
                    mkc[1][o][c] = inr1 ? kk.y : 0.f;
                    if (c) { muv[0].y = m1.x; muv[1].y = m1.y; } else { muv[0].x = m1.x; muv[1].x = m1.y; }
                    if (qf) {
#pragma unroll
                        for (int i = 0; i < NLEV; i++) {
                            const uint32_t ro = qrow;
                            if (pairst) bst64<QAUX>(q[i], qr, vo0, ro);
                            else { bst32<QAUX>(q[i].x, qr, vo0, ro); bst32<QAUX>(q[i].y, qr, vo1, ro); }
                            qrow += No4;
                            asm volatile("" : "+s"(qrow));     // keeps it a running value (the optimiser would turn it back into products)
                        }
                    }
                }
                vv[o][0] = act ? mv[0][o][0] + mv[0][o][1] : 0.f;
                vv[o][1] = v1 ? mv[1][o][0] + mv[1][o][1] : 0.f;
                if (act) {                                     // U[nu=o][n]: even symbols in phase 0, odd in phase 1
                    Us[(o * 2 + 0) * Uph + gl] = muv[0];
                    Us[(o * 2 + 1) * Uph + gl] = v1 ? muv[1] : make_float2(0.f, 0.f);
                }
            }
            VAEQ_STAMP(4);
            // exclusive prefix sums PSv[nu][n], n = 0..B  (VS[nu][j] = PSv[hi+1] - PSv[lo])
            {
                float inc[2];
                if constexpr (B100) {
                    // both scans at once, their masked steps one instruction each (wave_incl_scan2_dpp_keep).  No input is -0, so no partial sum is: vv is
                    // +0 on a lane without the symbol and elsewhere the sum of two m2 = sum_i (q_i d_i) d_i, every term of which is >= +0 (q_i = exp2(.) rcp(.)
                    // of positives is >= +0, (q d) d carries d's sign twice) added from +0 -- a sum of values >= +0 is >= +0
                    inc[0] = vv[0][0] + vv[0][1];
                    inc[1] = vv[1][0] + vv[1][1];
                    wave_incl_scan2_dpp_keep(inc[0], inc[1]);
                } else {
#pragma unroll
                    for (int o = 0; o < 2; o++) inc[o] = wave_incl_scan_dpp(vv[o][0] + vv[o][1]);
                }
                if constexpr (NW > 1) {                        // add the totals of the waves below (fixed order)
                    if (lane == 63) { RED[wv] = inc[0]; RED[NW + wv] = inc[1]; }
                    sync_lds<NW>();
#pragma unroll
                    for (int w = 0; w < NW - 1; w++)
                        if (w < wv) { inc[0] += RED[w]; inc[1] += RED[NW + w]; }
                }
#pragma unroll
                for (int o = 0; o < 2; o++) {
                    if (act) {
                        PSv[o * (BS + 1) + n0 + 1] = inc[o] - vv[o][1];
                        PSv[o * (BS + 1) + n0 + 2] = inc[o];
                    }
                    if (gl == 0) PSv[o * (BS + 1)] = 0.f;
                }
            }
            sync_lds<NW>();
            if (owner) {                                       // VS[nu][j]: lane = (j = tk, nu = half)
                const int lo = (Mh - tk + 1) >> 1, hi_ = (nm - 1 + Mh - tk) >> 1;
                VS[half * M + tk] = PSv[half * (BS + 1) + hi_ + 1] - PSv[half * (BS + 1) + lo];
            }
            sync_lds<NW>();

            VAEQ_STAMP(5);
            // ============ P3: residual e = x - D for the quad t = 4l'..4l'+3, both chi.
            //   D[chi, 2 tau + par] = sum_nu sum_a h[chi,nu,2a+par] U[nu, tau + mh - a],   tau in {2l', 2l'+1}, a = 0..mh
            float se0 = 0.f, se1 = 0.f;
            // |h|^2 and VS of this lane's (j, nu) for C and the G_V prefix sums: read now, so that their LDS latency hides behind the D loop
            float hq0 = 0.f, hq1 = 0.f;
            if (worker) {
                const float2 h0 = Ht[(0 * 2 + half) * MP + tk], h1 = Ht[(1 * 2 + half) * MP + tk];
                hq0 = h0.x * h0.x + h0.y * h0.y;
                hq1 = h1.x * h1.x + h1.y * h1.y;
            }
            const float vsl = worker ? VS[half * M + tk] : 0.f;
            if constexpr (B100 && M == 25) {
                // B = 100: three tau of ONE chi per lane (D3Map) instead of two tau of both: 6 chains and 150 complex MACs per lane instead of 8 and 208.
                // Every output keeps its chain: nu = 0: a = mh, 0, 1, .. mh - 1, then nu = 1 the same, the first term starting the accumulator.  Only the
                // a = mh term of the odd parity is gone: it multiplies the zero pad tap (j = M), a +-0 that starts the chain or is added to it, which can
                // change at most the sign of a D that is zero -- and x - (+-0) = x for every received sample x other than -0 (all pinned bits equal).
                constexpr int T = 100 - mh, NB = (mh + 1) / 2;
                static_assert((mh & 1) == 0 && (Mh & 3) == 0 && D3Map::exact(100, M), "D3Map: mh even (a = mh stands alone, its odd tap is the pad)");
                // the per-lane pointers below depend on the lane alone: nothing pins them inside the step, so they are derived once, ahead of the frame
                // loop (about ten registers live through every phase -- since the tap loops carry their shared cells the register peak has room for
                // them: 252 VGPRs in the bench kernel, 256 at most over the 18 baked kernels, no scratch; profiles/r08/kernel_variants_ab.txt)
                const int l3 = lane;
                const int m3 = D3Map::m(l3, T), modd = m3 & 1, m3h = (3 * m3) >> 1;
                cacc D3[3][2];                                 // [i][par]: D[chi, 2 (3 m + i) + par]
                // the lane's six cells are the consecutive samples c = Mh + 6 m + k of its chi; 6 m = 2 (mod 4) for odd m: two pointer cases.
                // x is read here, so that its LDS latency hides behind the tap loop
                const int xo = D3Map::chi(l3) * 4 * Lph + (Mh >> 2) + m3h;
                const int o0 = xo + (modd ? 2 * Lph : 0), o2 = xo + (modd ? 1 : 2 * Lph);
                const int off[6] = {o0, o0 + Lph, o2, o2 + Lph, o0 + 1, o0 + Lph + 1};
                v2f x6[6];
#pragma unroll
                for (int k = 0; k < 6; k++) x6[k] = lds2(Xs + off[k]);
                {
                    // U[nu][3 m + k] = (k even ? uE[k / 2] : uO[(k - 1) / 2]) + nu * 2 Uph: the polyphase component is a per-lane constant
                    const float2 *uE = Us + modd * Uph + m3h, *uO = Us + (modd ^ 1) * Uph + m3h + modd;
                    const float2 *hc = Ht + D3Map::chi(l3) * 2 * MP;
                    v2f am[2][4];                              // a = mh of both nu: its reads never stand between two tap loops
#pragma unroll
                    for (int v = 0; v < 2; v++) {
                        am[v][0] = lds2(hc + v * MP + Mh);
                        am[v][1] = lds2(uE + v * 2 * Uph); am[v][2] = lds2(uO + v * 2 * Uph); am[v][3] = lds2(uE + v * 2 * Uph + 1);
                    }
#pragma unroll
                    for (int v = 0; v < 2; v++) {
                        const float2 *hv = hc + v * MP, *ue = uE + v * 2 * Uph, *uo = uO + v * 2 * Uph;
                        {                                      // a = mh: U[3 m + i], even tap h[2 mh] (read ahead of the loops, below)
                            const v2f t = am[v][0], u0 = am[v][1], u1 = am[v][2], u2 = am[v][3];
                            if (v == 0) { cmul(D3[0][0], t, u0); cmul(D3[1][0], t, u1); cmul(D3[2][0], t, u2); }
                            else { cmac(D3[0][0], t, u0); cmac(D3[1][0], t, u1); cmac(D3[2][0], t, u2); }
                        }
                        // stage b: a = 2b, 2b + 1: cells U[3 m + mh - 2b + d], d = -1..2, and taps h[4b .. 4b + 3]: 8 LDS reads feeding 24 packed FMAs
                        auto load = [&](int b, v2f (&r)[8]) {
                            const int sl = (mh >> 1) - b;      // 3 m + mh - 2b = even index 2 sl past the lane's base
                            r[0] = lds2(uo + sl - 1); r[1] = lds2(ue + sl); r[2] = lds2(uo + sl); r[3] = lds2(ue + sl + 1);
#pragma unroll
                            for (int t = 0; t < 4; t++) r[4 + t] = lds2(hv + 4 * b + t);           // (even, odd) tap of a = 2b, of a = 2b + 1
                        };
                        auto fma = [&](int, const v2f (&r)[8], auto first) {
                            constexpr bool F = decltype(first)::value;     // nu = 0, b = 0 starts the odd-parity chains
                            // pin: the taps stay 8-byte registers up to here (the optimiser otherwise splits the set that lives across the loop's back edge
                            // into halves at its loads: four copies behind s_waitcnt lgkmcnt(3..0) at the end of every trip)
                            v2f t0 = r[4], t1 = r[5], t2 = r[6], t3 = r[7];
                            asm volatile("" : "+v"(t0), "+v"(t1));         // (volatile: stays behind the next stage's loads)
#pragma unroll
                            for (int i = 0; i < 3; i++) {
                                cmac(D3[i][0], t0, r[i + 1]);
                                cmacf<F>(D3[i][1], t1, r[i + 1]);
                                // the chain's first product is rounded on its own, as it is where the pad term starts the chain (0 * u + h U): pinned, or the
                                // next term's multiply would be the one left unfused
                                if constexpr (F) asm volatile("" : "+v"(D3[i][1].a), "+v"(D3[i][1].b));
                            }
                            asm volatile("" : "+v"(t2), "+v"(t3));
#pragma unroll
                            for (int i = 0; i < 3; i++) { cmac(D3[i][0], t2, r[i]); cmac(D3[i][1], t3, r[i]); }
                        };
                        if constexpr (CARRY) {
                            // stage b >= 1 takes its cells d = 1, 2 from the registers of stage b - 1 (its d = -1, 0): 6 reads per 24 packed FMAs.  Stage 0
                            // is the plain one, statement for statement; per nu -- the carry restarts where the array changes
                            static_assert(CellCarry::d3_exact(100, M) && CellCarry::D3Map_nm_lanes(T) == D3Map::nm_lanes(T), "CellCarry");
                            auto loadF = [&](v2f (&r)[8]) { load(0, r); };
                            auto loadM = [&](int b, v2f (&r)[8]) {
#pragma unroll
                                for (int t = 0; t < 4; t++) r[4 + t] = lds2(hv + 4 * b + t);
                            };
                            auto loadL = [&](int b, v2f (&r)[8]) { const int sl = (mh >> 1) - b; r[0] = lds2(uo + sl - 1); r[1] = lds2(ue + sl); };
                            auto stage = [&](const v2f (&r)[8], const v2f (&p)[8], auto mid) {   // p[0], p[1]: this stage's cells d = 1, 2
                                v2f t0 = r[4], t1 = r[5], t2 = r[6], t3 = r[7];
                                asm volatile("" : "+v"(t0), "+v"(t1), "+v"(t2), "+v"(t3));     // pin: see fma
                                cmac(D3[2][0], t0, p[1]); cmac(D3[2][1], t1, p[1]); cmac(D3[1][0], t0, p[0]); cmac(D3[1][1], t1, p[0]);
                                cmac(D3[2][0], t2, p[0]); cmac(D3[2][1], t3, p[0]);
                                // (volatile: stays in front of the loads into p[0], p[1])
                                asm volatile("" : "+v"(D3[1][0].a), "+v"(D3[1][0].b), "+v"(D3[1][1].a), "+v"(D3[1][1].b), "+v"(D3[2][0].a), "+v"(D3[2][0].b),
                                             "+v"(D3[2][1].a), "+v"(D3[2][1].b));
                                mid();
                                cmac(D3[0][0], t0, r[1]); cmac(D3[0][1], t1, r[1]); cmac(D3[1][0], t2, r[1]); cmac(D3[1][1], t3, r[1]);
                                cmac(D3[0][0], t2, r[0]); cmac(D3[0][1], t3, r[0]);
                            };
                            auto none = [&]() {};
                            auto done = [&](const v2f (&)[8]) {};
                            if (v == 0) pipe2_carry<8>(NB, loadF, loadM, loadL, [&](const v2f (&r)[8]) { fma(0, r, std::true_type{}); }, stage, none, done);
                            else pipe2_carry<8>(NB, loadF, loadM, loadL, [&](const v2f (&r)[8]) { fma(0, r, std::false_type{}); }, stage, none, done);
                        } else if (v == 0) pipe2<8, true, PIPE>(NB, load, fma);
                        else pipe2<8, false, PIPE>(NB, load, fma);
                    }
                }
                VAEQ_STAMP(6);
                {
                    float2 e[6];
#pragma unroll
                    for (int k = 0; k < 6; k++) {
                        const float2 x = f2(x6[k]);
                        const float2 Dv = cfin(D3[k >> 1][k & 1]);
                        e[k] = make_float2(x.x - Dv.x, x.y - Dv.y);
                        if (6 * (D3Map::nm_lanes(T) - 1) + k >= 2 * T && 6 * m3 + k >= nm) e[k] = make_float2(0.f, 0.f);   // past nm: the pad stays zero
                    }
                    if (D3Map::works(l3, T)) {
#pragma unroll
                        for (int k = 0; k < 6; k++) Es[off[k]] = e[k];
                    }
                }
                // sum |e|^2 keeps its lanes and its order (they set the bits of C and of the loss): lanes l' < nq read their quad back (one wave: LDS
                // executes in issue order) and add exactly as the plain form below does
                sync_lds<NW>();
                {
                    const float2 *Eq = Es + (gl < nq ? gl : 0);   // lanes without a quad read lane 0's and add nothing (no branch)
                    v2f eq[2][4];                              // all eight reads in flight at once (lds2: one round trip, not four)
#pragma unroll
                    for (int chi = 0; chi < 2; chi++)
#pragma unroll
                        for (int i = 0; i < 4; i++) eq[chi][i] = lds2(Eq + (chi * 4 + ((Mh + i) & 3)) * Lph + ((Mh + i) >> 2));
#pragma unroll
                    for (int chi = 0; chi < 2; chi++)
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            const float2 e = f2(eq[chi][i]);
                            const float e2 = __builtin_fmaf(e.x, e.x, e.y * e.y);   // the contraction the plain form's e.x * e.x + e.y * e.y compiles to, spelled out
                            if (chi) se1 += e2; else se0 += e2;
                        }
                    if (gl >= nq) se0 = se1 = 0.f;
                }
            } else {
                cacc D[2][4];                                  // [chi][i], i = 2*dl + par; lanes without a quad shadow lane 0 (no divergence, unused)
                constexpr int NA = mh + 1, NB = NA / 2;        // a = 0..mh; pairs (2b, 2b+1)
#pragma unroll
                for (int v = 0; v < 2; v++) {
                    const float2 *h0 = Ht + (0 * 2 + v) * MP, *h1 = Ht + (1 * 2 + v) * MP;
                    const float2 *up = Us + (gl < nq ? gl : 0) + v * 2 * Uph;       // U[nu][2l' + d] = up[(d & 1) * Uph + (d >> 1)]
                    auto step_a = [&](int aa, v2f ulo, v2f uhi, auto first) {        // ulo = U[2l' + mh - a], uhi = U[2l' + mh - a + 1]
                        constexpr bool F = decltype(first)::value;
                        const v2f e0 = lds2(h0 + 2 * aa), o0 = lds2(h0 + 2 * aa + 1), e1 = lds2(h1 + 2 * aa), o1 = lds2(h1 + 2 * aa + 1);
                        cmacf<F>(D[0][0], e0, ulo); cmacf<F>(D[0][1], o0, ulo);
                        cmacf<F>(D[0][2], e0, uhi); cmacf<F>(D[0][3], o0, uhi);
                        cmacf<F>(D[1][0], e1, ulo); cmacf<F>(D[1][1], o1, ulo);
                        cmacf<F>(D[1][2], e1, uhi); cmacf<F>(D[1][3], o1, uhi);
                    };
                    // a = mh first (d = 0 -> U[2l'], U[2l'+1]; its odd tap is the zero pad when mh is even); for nu = 0 it starts the accumulators
                    if (NA & 1) {
                        if (v == 0) step_a(mh, lds2(up), lds2(up + Uph), std::true_type{});
                        else step_a(mh, lds2(up), lds2(up + Uph), std::false_type{});
                    } else if (v == 0) {
#pragma unroll
                        for (int chi = 0; chi < 2; chi++)
#pragma unroll
                            for (int i = 0; i < 4; i++) D[chi][i] = cacc0();
                    }
                    // stage b: a = 2b, 2b+1 (d = mh - 2b: samples d+1, d, d-1): 3 + 8 independent LDS reads feeding 32 packed FMAs
                    constexpr int ph = mh & 1;                 // phase of d (d and mh have equal parity)
                    auto load = [&](int b, v2f (&r)[11]) {
                        const int sl = (mh >> 1) - b;          // slot of d   (d >> 1)
                        r[0] = lds2(up + ph * Uph + sl);                            // d
                        r[1] = lds2(up + (ph ^ 1) * Uph + sl + ph);                 // d + 1
                        r[2] = lds2(up + (ph ^ 1) * Uph + sl + ph - 1);             // d - 1
#pragma unroll
                        for (int t = 0; t < 4; t++) { r[3 + t] = lds2(h0 + 4 * b + t); r[7 + t] = lds2(h1 + 4 * b + t); }   // (e, o) of a = 2b, 2b+1
                    };
                    auto fma = [&](int, const v2f (&r)[11], auto) {
                        cmac(D[0][0], r[3], r[0]); cmac(D[0][1], r[4], r[0]); cmac(D[0][2], r[3], r[1]); cmac(D[0][3], r[4], r[1]);
                        cmac(D[1][0], r[7], r[0]); cmac(D[1][1], r[8], r[0]); cmac(D[1][2], r[7], r[1]); cmac(D[1][3], r[8], r[1]);
                        cmac(D[0][0], r[5], r[2]); cmac(D[0][1], r[6], r[2]); cmac(D[0][2], r[5], r[0]); cmac(D[0][3], r[6], r[0]);
                        cmac(D[1][0], r[9], r[2]); cmac(D[1][1], r[10], r[2]); cmac(D[1][2], r[9], r[0]); cmac(D[1][3], r[10], r[0]);
                    };
                    pipe2<11, false, PIPE>(NB, load, fma);
                }
                VAEQ_STAMP(6);
                if (gl < nq) {
#pragma unroll
                    for (int chi = 0; chi < 2; chi++)
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            const int ce = Mh + i;             // + 4*lane: same (phase, slot) arithmetic as x
                            const float2 x = Xl[(chi * 4 + (ce & 3)) * Lph + (ce >> 2)];
                            const float2 Dv = cfin(D[chi][i]);
                            float2 e = make_float2(x.x - Dv.x, x.y - Dv.y);
                            if (4 * gl + i >= nm) e = make_float2(0.f, 0.f);
                            Es[(chi * 4 + (ce & 3)) * Lph + gl + (ce >> 2)] = e;
                            const float e2 = e.x * e.x + e.y * e.y;
                            if (chi) se1 += e2; else se0 += e2;
                        }
                }
            }
            float hv0 = 0.f, hv1 = 0.f;                        // B = 100: sum_{nu,j} |h[chi]|^2 VS
            if constexpr (B100) {
                // the step's five wave sums as interleaved chains, their masked steps one instruction each (wave_sum5_dpp_keep): the same additions in
                // the same order as wave_sum_dpp, for every input
                float ws[5] = {wave_sum_first(se0), wave_sum_first(se1), wave_sum_first(klsum), wave_sum_first(hq0, vsl), wave_sum_first(hq1, vsl)};
                wave_sum5_dpp_keep(ws);
                se0 = ws[0]; se1 = ws[1]; klsum = ws[2]; hv0 = ws[3]; hv1 = ws[4];
            } else {
                se0 = wave_sum_dpp(se0);
                se1 = wave_sum_dpp(se1);
                klsum = wave_sum_dpp(klsum);
            }
            if constexpr (NW > 1) {                          // totals over the run's waves, same order in every wave
                if (lane == 0) { RED[16 + wv] = se0; RED[16 + NW + wv] = se1; RED[16 + 2 * NW + wv] = klsum; }
                sync_lds<NW>();
                se0 = RED[16]; se1 = RED[16 + NW]; klsum = RED[16 + 2 * NW];
#pragma unroll
                for (int w = 1; w < NW; w++) { se0 += RED[16 + w]; se1 += RED[16 + NW + w]; klsum += RED[16 + 2 * NW + w]; }
            }
            // C[chi] = sum|e|^2 + sum_{nu,j} |h|^2 VS   (lanes (j, nu) hold one term each for both chi; hq, vsl were read before the D loop)
            float C0, C1;
            if constexpr (B100) {
                C0 = se0 + hv0;
                C1 = se1 + hv1;
            } else {
                C0 = se0 + wave_sum_dpp(hq0 * vsl);
                C1 = se1 + wave_sum_dpp(hq1 * vsl);
            }
            // C is uniform: hardware reciprocal / log2 (1 ulp: 6e-8 on the gradients' common scale, 1e-7 relative on the ELBO) instead of the IEEE
            // division and logf expansions (~60 instructions per step that every lane would execute for lane 0's two stores)
            const float gC0 = (float)nm * __builtin_amdgcn_rcpf(C0), gC1 = (float)nm * __builtin_amdgcn_rcpf(C1);
            {
                const uint32_t vo = gl == 0 ? 0u : OOB;        // lane 0 stores; row offsets ride in the scalar offset
                if (a.loss) bst32((float)nm * LN2 * (__builtin_amdgcn_logf(C0) + __builtin_amdgcn_logf(C1)) + klsum, lr_, vo, (uint32_t)s * 4u);
                if (a.var_est) {
                    bst32(C0 * rnm, vr_, vo, (uint32_t)s * 4u);
                    bst32(C1 * rnm, vr_, vo, ((uint32_t)a.steps + (uint32_t)s) * 4u);
                }
            }
            // prefix sums over j of H2[nu][j] = sum_chi gC[chi] |h[chi,nu,j]|^2  -> G_V by two lookups per symbol
            {
                // (this scan keeps the form that adds a masked zero, at B = 100 too: gC = nm / C has the sign of C = sum |e|^2 + sum |h|^2 VS, and VS is a
                //  DIFFERENCE of two scanned prefix sums -- nothing in the code rules out a C < 0, whose gC |h|^2 is -0 for a tap that is 0)
                const float inc = half_incl_scan_dpp(gC0 * hq0 + gC1 * hq1);   // inclusive scan within each 32-lane half
                if (owner) PSh[half * MP + tk + 1] = inc;
                if (tk == 0) PSh[half * MP] = 0.f;
            }
            sync_lds<NW>();

            VAEQ_STAMP(7);
            // ============ P4a: dL/dh partial sums, lane = (j = tk, half of the tau range); acc[chi][nu]
            step += 1;
            b1t *= 0.9;
            b2t *= 0.999;
            const float rbc1 = __builtin_amdgcn_rcpf((float)(1.0 - b1t));                 // bias corrections: beta^t in double,
            const float bc2s = __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf((float)(1.0 - b2t)));   // the rest in float
            const float ssW = lrW * rbc1, ssH = lrH * rbc1;
            float2 hnew[2];
            hnew[0] = hnew[1] = make_float2(0.f, 0.f);
            float ghr[2] = {0, 0}, ghi[2] = {0, 0};
            float2 hacc[2];                                    // NW > 1: this wave's part of sum e conj(U) for (chi = half, nu)
            {
                // what the owner lane's Adam(h) update reads of the taps and VS is fetched from LDS BEFORE the tap loop, so that the
                // update after the loop starts with fewer exposed LDS round trips (wave 0 only)
                float2 ph_h[2] = {make_float2(0.f, 0.f), make_float2(0.f, 0.f)};
                float ph_vs[2] = {0.f, 0.f};                   // (the moments stay in LDS until the update: this phase cannot spare eight more registers)
                // B = 100: EVERY lane reads and updates the cells its (oc, tj) names, and only what leaves the lane is masked (the tap's write to LDS, the
                // state and debug stores): values defined on all lanes need no zeros for the lanes that own no tap (a v_mov 0 per value and step in front
                // of the exec-masked update).  A lane without a tap reads cells inside the LDS allocation (tj <= M + 1: at most two cells past a row) and
                // updates the moments of its OWN column of MOM, which nothing else reads: that column is never initialised, so such a lane runs Adam on
                // whatever the LDS holds (NaN included) and the result is discarded with it.  The bound on tj is TapPairMap's: M = 25 only
                static_assert(!B100 || TP, "B = 100: every lane updates -- the cells a lane without a tap names are inside the LDS allocation for TapPairMap (M = 25) only");
                if (B100 || (NW == 1 && ownr)) {
#pragma unroll
                    for (int v = 0; v < 2; v++) {
                        ph_h[v] = Ht[(oc * 2 + v) * MP + tj];
                        ph_vs[v] = VS[v * M + tj];
                    }
                }
                cacc ca[2][2];
                if constexpr (TP) {
                    // tap pairs (TapPairMap): ca[tap of the pair][nu] of the lane's chi over its half of the tau range; read tap a = 2 slot (mh even: its U
                    // cells tau + mh - a of even tau are the even phase), the other tap a + 1 from registers.  The pointers are derived once, ahead of the frame loop (see P3)
                    static_assert(TapPairMap::exact(100, M) && UNI, "TapPairMap");
                    const int lt = lane;
                    constexpr int NH = TapPairMap::dh_pairs(100, M);
                    const int par = TapPairMap::par(lt, M), sl = TapPairMap::alo(lt, M) >> 1, ma = TapPairMap::part_h(lt, M) * NH;
                    const int ceA = par + Mh, ceB = par + Mh + 2;
                    const float2 *ec = Es + TapPairMap::c(lt, M) * 4 * Lph + ma;
                    const float2 *uA = Us + (mh >> 1) - sl + ma, *uB = uA + Uph;
                    const float2 *uC = TapPairMap::tap(lt, M, 1) < M ? uB - 1 : uA;   // U of tap a + 1 at the first tau (the slot of a = 12 alone has no such tap)
                    VAEQ_XSTAMP(0);
                    tap_pair_sum<NH, 1>(ca, ec + (ceA & 3) * Lph + (ceA >> 2), ec + (ceB & 3) * Lph + (ceB >> 2), uA, uB, 2 * Uph, uC);
                } else {
                    // sum over tau of e[chi, 2 tau + par] conj(U[nu, tau + mh - a]); tau runs in pairs (2m, 2m+1) so that the
                    // polyphase component of every operand is a per-lane constant and only the slot advances (by one per m).
                    // Past the last valid tau the residual cells are zero (pad), so the pair loop may overrun by one.
                    // Lanes beyond the M taps shadow tap 0 (no divergence; their sums are never read).
                    const int tkc = worker ? tk : 0, par = tkc & 1, aa = tkc >> 1;
                    const int T = (nm - par + 1) >> 1, Th = ((T + 2 * NP - 1) / (2 * NP)) << 1;   // even split points
                    const int ma = (part * Th) >> 1, mb = (min(T, part * Th + Th) + 1) >> 1;
                    const int ceA = par + Mh, ceB = par + Mh + 2, npA = mh - aa, npB = mh - aa + 1;
                    const float2 *eA = Es + (ceA & 3) * Lph + (ceA >> 2) + ma, *eB = Es + (ceB & 3) * Lph + (ceB >> 2) + ma;
                    const float2 *uA = Us + (npA & 1) * Uph + (npA >> 1) + ma, *uB = Us + (npB & 1) * Uph + (npB >> 1) + ma;
                    // stage = two pairs (m = 2i, 2i+1): 16 independent LDS reads feeding 32 packed FMAs (a one-pair stage's 16 FMAs are too short
                    // to cover the next stage's LDS latency); an odd last pair is handled after the pipeline
                    auto load1 = [&](int m, v2f *r) {
                        r[0] = lds2(eA + m); r[1] = lds2(eA + 4 * Lph + m); r[2] = lds2(uA + m); r[3] = lds2(uA + 2 * Uph + m);
                        r[4] = lds2(eB + m); r[5] = lds2(eB + 4 * Lph + m); r[6] = lds2(uB + m); r[7] = lds2(uB + 2 * Uph + m);
                    };
                    cacc cbx[2][2];                            // the odd tau of every pair sum here: 16 independent chains (see pair_fir) (WIDE)
                    cacc (&cb)[2][2] = WIDE ? cbx : ca;
                    auto fma1 = [&](const v2f *r, auto first) {
                        constexpr bool F = decltype(first)::value;
                        cmacf<F>(ca[0][0], r[2], r[0]); cmacf<F>(ca[0][1], r[3], r[0]); cmacf<F>(ca[1][0], r[2], r[1]); cmacf<F>(ca[1][1], r[3], r[1]);
                        cmacf<F && WIDE>(cb[0][0], r[6], r[4]); cmacf<F && WIDE>(cb[0][1], r[7], r[4]); cmacf<F && WIDE>(cb[1][0], r[6], r[5]); cmacf<F && WIDE>(cb[1][1], r[7], r[5]);
                    };
                    auto load = [&](int i, v2f (&r)[16]) { load1(2 * i, r); load1(2 * i + 1, r + 8); };
                    auto fma = [&](int, const v2f (&r)[16], auto first) { fma1(r, first); fma1(r + 8, std::false_type{}); };
                    int n = mb - ma;
                    VAEQ_XSTAMP(0);
                    if constexpr (UNI) {                       // baked shape: every part has the same number (>= 2) of pairs
                        n = __builtin_amdgcn_readfirstlane(n);
                        pipe2<16, true, PIPE>(n >> 1, load, fma);
                    } else {
                        ca[0][0] = ca[0][1] = ca[1][0] = ca[1][1] = cbx[0][0] = cbx[0][1] = cbx[1][0] = cbx[1][1] = cacc0();
                        pipe2<16, false, PIPE>(n >> 1, load, fma);
                    }
                    if (n & 1) {
                        v2f r[8];
                        load1(n - 1, r);
                        fma1(r, std::false_type{});
                    }
                    if constexpr (WIDE) {
#pragma unroll
                        for (int i = 0; i < 2; i++)
#pragma unroll
                            for (int j = 0; j < 2; j++) { ca[i][j].a += cbx[i][j].a; ca[i][j].b += cbx[i][j].b; }
                    }
                }
                VAEQ_XSTAMP(1);
                if constexpr (B100) {
                    // the halves meet as (re, im) pairs and the update stays on pairs (half_sum2, adam_update_fast2); every lane (see ph_h above)
                    v2f sum[2];
#pragma unroll
                    for (int v = 0; v < 2; v++) sum[v] = half_sum2(cfinc2(ca[0][v]), cfinc2(ca[1][v]));   // e * conj(U) of the kept chi
                    VAEQ_XSTAMP(2);
                    const float g = oc ? gC1 : gC0;
#pragma unroll
                    for (int v = 0; v < 2; v++) {
                        v2f hh = {ph_h[v].x, ph_h[v].y};
                        const v2f gh = g * __builtin_elementwise_fma(2.0f * hh, v2f{ph_vs[v], ph_vs[v]}, -2.0f * sum[v]);
                        if (!a.no_update) {
                            v2f mo = {mHr(v), mHi(v)}, vo = {vHr(v), vHi(v)};
                            adam_update_fast2(hh, mo, vo, gh, ssH, bc2s);
                            mHr(v) = mo.x; mHi(v) = mo.y;
                            vHr(v) = vo.x; vHi(v) = vo.y;
                        }
                        hnew[v] = f2(hh);
                        // the last step's gradient leaves here (not behind P5, next to dL/dw's): four registers less through P4b, the kernel's register peak
                        if (a.dbg_gW && ownr && f == a.n_frames - 1 && s == a.steps - 1) {
                            a.dbg_gh[gbase + ((oc * 2 + v) * 2 + 0) * M + tj] = gh.x;
                            a.dbg_gh[gbase + ((oc * 2 + v) * 2 + 1) * M + tj] = gh.y;
                        }
                    }
                } else {
                    float2 acc[2][2];
#pragma unroll
                    for (int chi = 0; chi < 2; chi++)
#pragma unroll
                        for (int v = 0; v < 2; v++) acc[chi][v] = cfinc(ca[chi][v]);             // e * conj(U)
                    // combine the two halves; lane (j, half) keeps chi = half
#pragma unroll
                    for (int chi = 0; chi < 2; chi++)
#pragma unroll
                        for (int v = 0; v < 2; v++) {
                            acc[chi][v].x += __shfl_xor(acc[chi][v].x, 32, 64);
                            acc[chi][v].y += __shfl_xor(acc[chi][v].y, 32, 64);
                        }
                    if constexpr (NW > 1) {                        // waves 1.. hand their partial sums to wave 0 (read after the next barrier)
#pragma unroll
                        for (int v = 0; v < 2; v++) {
                            hacc[v] = half ? acc[1][v] : acc[0][v];
                            if (wv > 0) {
                                XG[((wv - 1) * 4 + 2 * v + 0) * 64 + lane] = hacc[v].x;
                                XG[((wv - 1) * 4 + 2 * v + 1) * 64 + lane] = hacc[v].y;
                            }
                        }
                    }
                    VAEQ_XSTAMP(2);
                    if (NW == 1 && ownr) {
                        const float g = oc ? gC1 : gC0;
#pragma unroll
                        for (int v = 0; v < 2; v++) {
                            const float2 ac = half ? acc[1][v] : acc[0][v];
                            const float2 hh = ph_h[v];
                            const float vs = ph_vs[v];
                            ghr[v] = g * (-2.0f * ac.x + 2.0f * hh.x * vs);
                            ghi[v] = g * (-2.0f * ac.y + 2.0f * hh.y * vs);
                            hnew[v] = hh;
                            if (!a.no_update) {
                                adam_update_fast(hnew[v].x, mHr(v), vHr(v), ghr[v], ssH, bc2s);
                                adam_update_fast(hnew[v].y, mHi(v), vHi(v), ghi[v], ssH, bc2s);
                            }
                        }
                    }
                }
            }

            if constexpr (B100) asm volatile("" : "+v"(hnew[0].x), "+v"(hnew[0].y), "+v"(hnew[1].x), "+v"(hnew[1].y));   // pin (see P1)
            else asm volatile("" : "+v"(hnew[0].x), "+v"(hnew[0].y), "+v"(hnew[1].x), "+v"(hnew[1].y), "+v"(ghr[0]), "+v"(ghr[1]), "+v"(ghi[0]),
                              "+v"(ghi[1]));
            // prefetch the next window now: the q/y stores of this step were issued half a step ago and have drained, so the wait
            // for these loads at the top of the next step does not also wait for fresh stores (vmcnt retires in order)
            {
                const bool last_s = s + 1 == a.steps;
                if constexpr (B100) {                         // no branch: the loads' results are not copied (and waited for) here
                    const bool more = !(last_s && f + 1 == a.n_frames);
                    const uint32_t vo = ldl && more ? ((uint32_t)(last_s ? 0 : s + 1) * (uint32_t)a.stride_sym * 2u + 4u * gl) * 4u : OOB;   // the launch's last step: nothing is read
#pragma unroll
                    for (int r = 0; r < 4; r++) pf[r] = bld128(last_s ? xn : xr, vo, (uint32_t)r * S4);
                } else if (!(last_s && f + 1 == a.n_frames)) fetch(last_s ? xn : xr, last_s ? 0 : s + 1);
            }
            VAEQ_XSTAMP(3);
            VAEQ_STAMP(8);
            // ============ P4b: dL/dU for the lane's symbol pair (same shape as the FIR, on e with conj(h)), then dL/dy
            float2 gy[2][2];                                   // [sym][nu]
            {
                float2 au0[2][2], au1[2][2];                   // chi = 0 / 1: [sym][nu]
                {
                    cacc cu[2][2][2];                          // [chi][sym][nu]
                    pair_du<M, WIDE, CARRY>(cu, Ea, Lph, Ht, MP);
#pragma unroll
                    for (int sy = 0; sy < 2; sy++)
#pragma unroll
                        for (int v = 0; v < 2; v++) { au0[sy][v] = cfinc(cu[0][sy][v]); au1[sy][v] = cfinc(cu[1][sy][v]); }   // e * conj(h)
                }
#pragma unroll
                for (int sy = 0; sy < 2; sy++) {
                    const int sx = 2 * (n0 + sy);
                    const int jlo = max(0, Mh - sx), jhi = max(jlo - 1, min(Mh, nm - 1 + Mh - sx));
#pragma unroll
                    for (int v = 0; v < 2; v++) {
                        const float ur = -2.0f * (gC0 * au0[sy][v].x + gC1 * au1[sy][v].x);
                        const float ui = -2.0f * (gC0 * au0[sy][v].y + gC1 * au1[sy][v].y);
                        const float gv = PSh[v * MP + jhi + 1] - PSh[v * MP + jlo];
                        const float iv = 1.0f / (v ? var1 : var0);
                        gy[sy][v].x = iv * (ur * mv[sy][v][0] + gv * mt3[sy][v][0] + mkc[sy][v][0]);
                        gy[sy][v].y = iv * (ui * mv[sy][v][1] + gv * mt3[sy][v][1] + mkc[sy][v][1]);
                    }
                }
            }
            VAEQ_STAMP(9);
            sync_lds<NW>();                                   // every read of U / old h is done (GY aliases U)
            if constexpr (NW > 1) {
                if (owner) {
                    const float g = half ? gC1 : gC0;
#pragma unroll
                    for (int v = 0; v < 2; v++) {
                        float2 ac = hacc[v];
#pragma unroll
                        for (int w = 0; w < NW - 1; w++) {
                            ac.x += XG[(w * 4 + 2 * v + 0) * 64 + lane];
                            ac.y += XG[(w * 4 + 2 * v + 1) * 64 + lane];
                        }
                        const float2 hh = Ht[(half * 2 + v) * MP + tk];
                        const float vs = VS[v * M + tk];
                        ghr[v] = g * (-2.0f * ac.x + 2.0f * hh.x * vs);
                        ghi[v] = g * (-2.0f * ac.y + 2.0f * hh.y * vs);
                        hnew[v] = hh;
                        if (!a.no_update) {
                            adam_update_fast(hnew[v].x, mHr(v), vHr(v), ghr[v], ssH, bc2s);
                            adam_update_fast(hnew[v].y, mHi(v), vHi(v), ghi[v], ssH, bc2s);
                        }
                    }
                }
            }
            if (act) {
#pragma unroll
                for (int v = 0; v < 2; v++) {
                    GY[v * BS + n0] = gy[0][v];
                    GY[v * BS + n0 + 1] = v1 ? gy[1][v] : make_float2(0.f, 0.f);
                }
            }
            if (ownr && !a.no_update) {
                Ht[(oc * 2 + 0) * MP + tj] = hnew[0];
                Ht[(oc * 2 + 1) * MP + tj] = hnew[1];
            }
            sync_lds<NW>();

            VAEQ_STAMP(10);
            // ============ P5: dL/dw partial sums, lane = (k = tk, half of the symbol range); acc[o][p]
            float gwr[2] = {0, 0}, gwi[2] = {0, 0};
            {
                float pw_w[2][2] = {{0.f, 0.f}, {0.f, 0.f}}, pw_m[2][2] = {{0.f, 0.f}, {0.f, 0.f}}, pw_v[2][2] = {{0.f, 0.f}, {0.f, 0.f}};   // as for Adam(h)
                if (B100 || ownr) {                          // (B = 100: every lane, see Adam(h))
#pragma unroll
                    for (int p = 0; p < 2; p++) {
                        const float *wq = reinterpret_cast<const float *>(&Wt[p * M + tj]) + oc * 2;
                        pw_w[p][0] = wq[0]; pw_w[p][1] = wq[1];
                        pw_m[p][0] = mWr(p); pw_m[p][1] = mWi(p);
                        pw_v[p][0] = vWr(p); pw_v[p][1] = vWi(p);
                    }
                }
                cacc ca[2][2];
                if constexpr (TP) {
                    // tap pairs (TapPairMap): read tap k + 2 = 2 (a + 1) + par, the pair's lower tap k from registers; ca[o-half order][p]: [0] = the lower
                    // tap, which the lower half keeps
                    const int lt = lane;
                    constexpr int NQ = TapPairMap::dw_pairs(100);
                    const int cA = TapPairMap::tap(lt, M, 1), cB = cA + 2, ma = TapPairMap::part_w(lt) * NQ;
                    const float2 *gA = GY + TapPairMap::c(lt, M) * BS + 2 * ma;
                    const float2 *xA = Xs + (cA & 3) * Lph + (cA >> 2) + ma, *xB = Xs + (cB & 3) * Lph + (cB >> 2) + ma;
                    cacc cr[2][2];                             // [0] = the read (upper) tap
                    VAEQ_XSTAMP(4);
                    tap_pair_sum<NQ, 2>(cr, gA, gA + 1, xA, xB, 4 * Lph, xB - 1);
#pragma unroll
                    for (int p = 0; p < 2; p++) { ca[0][p] = cr[1][p]; ca[1][p] = cr[0][p]; }
                } else {
                    // sum over n of gy[o, n] conj(x[p, 2n + k]); n runs in pairs (2m, 2m+1): x phase fixed per lane, gy pair = 16 bytes
                    const int tkc = worker ? tk : 0;           // lanes beyond the M taps shadow tap 0
                    const int Be = ODDB ? B + (B & 1) : B;     // odd B: the last pair's second symbol has dL/dy = 0
                    const int Bq = ((Be + 2 * NP - 1) / (2 * NP)) << 1;                  // even split points
                    const int ma = (part * Bq) >> 1, mb = min(Be, part * Bq + Bq) >> 1;
                    const int cA = tkc, cB = tkc + 2;
                    const float2 *xA = Xs + (cA & 3) * Lph + (cA >> 2) + ma, *xB = Xs + (cB & 3) * Lph + (cB >> 2) + ma;
                    const float2 *G0 = GY + 2 * ma, *G1 = GY + BS + 2 * ma;
                    auto load1 = [&](int m, v2f *r) {
                        r[0] = lds2(G0 + 2 * m); r[1] = lds2(G0 + 2 * m + 1); r[2] = lds2(G1 + 2 * m); r[3] = lds2(G1 + 2 * m + 1);   // gy[o][2m], gy[o][2m+1]
                        r[4] = lds2(xA + m); r[5] = lds2(xA + 4 * Lph + m); r[6] = lds2(xB + m); r[7] = lds2(xB + 4 * Lph + m);
                    };
                    cacc cbx[2][2];                            // the odd symbols of every pair sum here: 16 independent chains (WIDE)
                    cacc (&cb)[2][2] = WIDE ? cbx : ca;
                    auto fma1 = [&](const v2f *r, auto first) {
                        constexpr bool F = decltype(first)::value;
                        cmacf<F>(ca[0][0], r[4], r[0]); cmacf<F>(ca[0][1], r[5], r[0]); cmacf<F>(ca[1][0], r[4], r[2]); cmacf<F>(ca[1][1], r[5], r[2]);
                        cmacf<F && WIDE>(cb[0][0], r[6], r[1]); cmacf<F && WIDE>(cb[0][1], r[7], r[1]); cmacf<F && WIDE>(cb[1][0], r[6], r[3]); cmacf<F && WIDE>(cb[1][1], r[7], r[3]);
                    };
                    auto load = [&](int i, v2f (&r)[16]) { load1(2 * i, r); load1(2 * i + 1, r + 8); };       // stage = two symbol pairs (see dL/dh)
                    auto fma = [&](int, const v2f (&r)[16], auto first) { fma1(r, first); fma1(r + 8, std::false_type{}); };
                    int n = mb - ma;
                    VAEQ_XSTAMP(4);
                    if constexpr (UNI) {
                        n = __builtin_amdgcn_readfirstlane(n);
                        pipe2<16, true, PIPE>(n >> 1, load, fma);
                    } else {
                        ca[0][0] = ca[0][1] = ca[1][0] = ca[1][1] = cbx[0][0] = cbx[0][1] = cbx[1][0] = cbx[1][1] = cacc0();
                        pipe2<16, false, PIPE>(n >> 1, load, fma);
                    }
                    if (n & 1) {
                        v2f r[8];
                        load1(n - 1, r);
                        fma1(r, std::false_type{});
                    }
                    if constexpr (WIDE) {
#pragma unroll
                        for (int i = 0; i < 2; i++)
#pragma unroll
                            for (int j = 0; j < 2; j++) { ca[i][j].a += cbx[i][j].a; ca[i][j].b += cbx[i][j].b; }
                    }
                }
                VAEQ_XSTAMP(5);
                if constexpr (B100) {
                    // as for dL/dh: the halves meet as (re, im) pairs, lane (k, half) keeps o = half, and every lane runs the update on pairs; the tap's and
                    // the moments' writes to LDS are the owner's alone (a lane without a tap names a cell that another lane owns)
                    v2f sum[2];
#pragma unroll
                    for (int p = 0; p < 2; p++) sum[p] = half_sum2(cfinc2(ca[0][p]), cfinc2(ca[1][p]));   // gy * conj(x)
                    VAEQ_XSTAMP(6);
#pragma unroll
                    for (int p = 0; p < 2; p++) {
                        gwr[p] = sum[p].x;
                        gwi[p] = sum[p].y;
                        if (!a.no_update) {
                            v2f w = {pw_w[p][0], pw_w[p][1]}, mo = {pw_m[p][0], pw_m[p][1]}, vo = {pw_v[p][0], pw_v[p][1]};
                            adam_update_fast2(w, mo, vo, sum[p], ssW, bc2s);
                            if (ownr) {
                                float *wq = reinterpret_cast<float *>(&Wt[p * M + tj]) + oc * 2;
                                wq[0] = w.x;
                                wq[1] = w.y;
                                mWr(p) = mo.x; mWi(p) = mo.y;
                                vWr(p) = vo.x; vWi(p) = vo.y;
                            }
                        }
                    }
                } else {
                    float2 acc[2][2];
#pragma unroll
                    for (int o = 0; o < 2; o++)
#pragma unroll
                        for (int pp = 0; pp < 2; pp++) acc[o][pp] = cfinc(ca[o][pp]);            // gy * conj(x)
#pragma unroll
                    for (int o = 0; o < 2; o++)
#pragma unroll
                        for (int p = 0; p < 2; p++) {
                            acc[o][p].x += __shfl_xor(acc[o][p].x, 32, 64);
                            acc[o][p].y += __shfl_xor(acc[o][p].y, 32, 64);
                        }
                    if constexpr (NW > 1) {                        // as for dL/dh: wave 0 adds the other waves' parts after the barrier
#pragma unroll
                        for (int p = 0; p < 2; p++) {
                            const float2 ac = half ? acc[1][p] : acc[0][p];
                            if (wv > 0) {
                                XG[((wv - 1) * 4 + 2 * p + 0) * 64 + lane] = ac.x;
                                XG[((wv - 1) * 4 + 2 * p + 1) * 64 + lane] = ac.y;
                            }
                        }
                        sync_lds<NW>();
                    }
                    VAEQ_XSTAMP(6);
                    if (ownr) {
#pragma unroll
                        for (int p = 0; p < 2; p++) {
                            float2 ac = half ? acc[1][p] : acc[0][p];
                            if constexpr (NW > 1) {
#pragma unroll
                                for (int w = 0; w < NW - 1; w++) {
                                    ac.x += XG[(w * 4 + 2 * p + 0) * 64 + lane];
                                    ac.y += XG[(w * 4 + 2 * p + 1) * 64 + lane];
                                }
                            }
                            gwr[p] = ac.x;
                            gwi[p] = ac.y;
                            if (!a.no_update) {
                                float *wq = reinterpret_cast<float *>(&Wt[p * M + tj]) + oc * 2;
                                float wr = pw_w[p][0], wi = pw_w[p][1];
                                adam_update_fast(wr, pw_m[p][0], pw_v[p][0], gwr[p], ssW, bc2s);
                                adam_update_fast(wi, pw_m[p][1], pw_v[p][1], gwi[p], ssW, bc2s);
                                wq[0] = wr;
                                wq[1] = wi;
                                mWr(p) = pw_m[p][0]; mWi(p) = pw_m[p][1];
                                vWr(p) = pw_v[p][0]; vWi(p) = pw_v[p][1];
                            }
                        }
                    }
                }
            }
            if (a.dbg_gW && ownr && f == a.n_frames - 1 && s == a.steps - 1) {
#pragma unroll
                for (int p = 0; p < 2; p++) {
                    a.dbg_gW[gbase + (oc * 4 + p) * M + tj] = gwr[p];
                    a.dbg_gW[gbase + (oc * 4 + 2 + p) * M + tj] = gwi[p];
                    if constexpr (!B100) {                     // (B = 100: stored in P4a)
                        a.dbg_gh[gbase + ((oc * 2 + p) * 2 + 0) * M + tj] = ghr[p];
                        a.dbg_gh[gbase + ((oc * 2 + p) * 2 + 1) * M + tj] = ghi[p];
                    }
                }
            }
            sync_lds<NW>();
            VAEQ_XSTAMP(7);
            VAEQ_STAMP(11);
        }
    }
#ifdef VAEQ_PHASE_STAMPS
    if (gl == 0 && run == (int)gridDim.x / 2 && a.loss)
        for (int i = 0; i + 1 < VAEQ_NSTAMP; i++) a.loss[i] = (float)(tst[i + 1] - tst[i]);
    if (gl == 0 && run == (int)gridDim.x / 2 && a.loss)
        for (int i = 0; i < 7; i++) a.loss[16 + i] = (float)(tsx[i + 1] - tsx[i]);
#endif

    // ---- state out
    if (ownr && !a.no_update) {
#pragma unroll
        for (int p = 0; p < 2; p++) {
            const size_t ir = gbase + (oc * 4 + p) * M + tj, ii = gbase + (oc * 4 + 2 + p) * M + tj;
            const float *wq = reinterpret_cast<const float *>(&Wt[p * M + tj]) + oc * 2;
            a.W[ir] = wq[0]; a.W[ii] = wq[1];
            a.adam_mW[ir] = mWr(p); a.adam_mW[ii] = mWi(p);
            a.adam_vW[ir] = vWr(p); a.adam_vW[ii] = vWi(p);
            const size_t hr = gbase + ((oc * 2 + p) * 2 + 0) * M + tj, hi = hr + M;
            const float2 hh = Ht[(oc * 2 + p) * MP + tj];
            a.h[hr] = hh.x; a.h[hi] = hh.y;
            a.adam_mh[hr] = mHr(p); a.adam_mh[hi] = mHi(p);
            a.adam_vh[hr] = vHr(p); a.adam_vh[hi] = vHi(p);
        }
    }
    if (gl == 0 && !a.no_update) a.step[run] = step;
#undef VAEQ_MOM
#undef mWr
#undef mWi
#undef vWr
#undef vWi
#undef mHr
#undef mHi
#undef vHr
#undef vHi
}


// Launch of dp_wave_kernel<M, NLEV, BT, PAIR, OUT, NW, BL>: PAIR from the parity of the keep window, OUT from the outputs the call asks for.
// BT > 0: the baked shape (a.B == BT); BL > 0 (BT == 0): run-time B <= BL on the fixed LDS layout of BL; both 0: the layout follows a.B.
// SPEC = false: only the all-outputs-nullable instantiation (OUT = 0) exists -- the run-time layouts and the tap counts that are not the reference's default.
template <int M, int NLEV, int BT, int NW, int BL, bool SPEC>
static int launch_wave(const vaeq_dp_args &a, hipStream_t st)
{
    const size_t lds = (size_t)wave_layout(BL ? BL : a.B, M, NW).total;
    const bool pair = ((a.keep_len | a.keep_off) & 1) == 0;
    const int out = !SPEC ? 0 : (!a.eq_out && !a.dec_out) ? 1 : !a.q_out ? 2 : 0;
    constexpr int O1 = SPEC ? 1 : 0, O2 = SPEC ? 2 : 0;
    void (*const k[2][3])(const vaeq_dp_args) = {
        {dp_wave_kernel<M, NLEV, BT, false, 0, NW, BL>, dp_wave_kernel<M, NLEV, BT, false, O1, NW, BL>, dp_wave_kernel<M, NLEV, BT, false, O2, NW, BL>},
        {dp_wave_kernel<M, NLEV, BT, true, 0, NW, BL>, dp_wave_kernel<M, NLEV, BT, true, O1, NW, BL>, dp_wave_kernel<M, NLEV, BT, true, O2, NW, BL>}};
    note_kernel("vaeq::dp_wave_kernel<%d, %d, %d, %s, %d, %d, %d>", M, NLEV, BT, pair ? "true" : "false", out, NW, BL);   // every template argument, as rocprofv3 prints the name
    return launch(k[pair][out], dim3(a.R), dim3(64 * NW), lds, st, a);
}

// Runs of that shape resident on the device at once (B: the minibatch length the layout follows when neither BT nor BL fixes it)
template <int M, int NLEV, int BT, int NW, int BL>
static int64_t wave_resident(int B)
{
    int nb = 0, dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return VAEQ_ERR_DEVICE;
    auto k = dp_wave_kernel<M, NLEV, BT, true, 0, NW, BL>;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k, 64 * NW, (size_t)wave_layout(BL ? BL : B, M, NW).total) != hipSuccess) return VAEQ_ERR_DEVICE;
    return (int64_t)nb * prop.multiProcessorCount;
}

// ... with NLEV from the call: the baked shapes and M = 25's run-time layout (BT = 0) ...
template <int M, int BT, int NW>
static int launch_wave_lev(const vaeq_dp_args &a, hipStream_t st)
{
    return dispatch_nlev(a.n_lev, [&](auto nl) { return launch_wave<M, decltype(nl)::value, BT, NW, 0, (BT > 0)>(a, st); });
}
template <int M, int BT, int NW>
static int64_t wave_resident_lev(int B, int n_lev)
{
    return dispatch_nlev(n_lev, [&](auto nl) { return wave_resident<M, decltype(nl)::value, BT, NW, 0>(B); });
}
// ... and run-time B <= BL on the fixed layout of BL (immediate offsets and strides, pipelined tap loops)
template <int M, int BL, int NW, bool SPEC>
static int launch_wave_fixl_lev(const vaeq_dp_args &a, hipStream_t st)
{
    return dispatch_nlev(a.n_lev, [&](auto nl) { return launch_wave<M, decltype(nl)::value, 0, NW, BL, SPEC>(a, st); });
}
template <int M, int BL, int NW>
static int64_t wave_resident_fixl_lev(int n_lev)
{
    return dispatch_nlev(n_lev, [&](auto nl) { return wave_resident<M, decltype(nl)::value, 0, NW, BL>(BL); });
}

// every supported M for a given NW (the per-NW translation units instantiate these): M = 25 on the run-time layout (its fixed-layout and baked forms
// are dispatched before; this is their A/B counterpart), every other tap count on the fixed layout of the NW class's largest minibatch
template <int NW>
static int launch_wave_any(const vaeq_dp_args &a, hipStream_t st)
{
    switch (a.M) {
    case 25: return launch_wave_lev<25, 0, NW>(a, st);
    case 31: return launch_wave_fixl_lev<31, 128 * NW, NW, false>(a, st);
    case 21: return launch_wave_fixl_lev<21, 128 * NW, NW, false>(a, st);
    case 17: return launch_wave_fixl_lev<17, 128 * NW, NW, false>(a, st);
    case 13: return launch_wave_fixl_lev<13, 128 * NW, NW, false>(a, st);
    case 9: return launch_wave_fixl_lev<9, 128 * NW, NW, false>(a, st);
    }
    return VAEQ_ERR_SHAPE;
}

template <int NW>
static int64_t wave_resident_any(int B, int M, int n_lev)
{
    switch (M) {
    case 25: return wave_resident_lev<25, 0, NW>(B, n_lev);
    case 31: return wave_resident_fixl_lev<31, 128 * NW, NW>(n_lev);
    case 21: return wave_resident_fixl_lev<21, 128 * NW, NW>(n_lev);
    case 17: return wave_resident_fixl_lev<17, 128 * NW, NW>(n_lev);
    case 13: return wave_resident_fixl_lev<13, 128 * NW, NW>(n_lev);
    case 9: return wave_resident_fixl_lev<9, 128 * NW, NW>(n_lev);
    }
    return VAEQ_ERR_SHAPE;
}

}  // namespace vaeq
