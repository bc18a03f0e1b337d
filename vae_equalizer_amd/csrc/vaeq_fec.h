// vaeq_fec.h -- what the algebraic and the Chase decoders (vaeq_bch.hip, vaeq_staircase.hip, vaeq_chase.hip, vaeq_tpc.hip) share: the product
// in GF(2^m) over the exp / log tables, the wave reduction, the Chase front end of a single-error-correcting code over its table of columns, and
// on the host the field's polynomial and generator degree, the packer of a column table and the frame rules of every decoder's entry point
// (vaeq_ldpc.h's ldpc_shape_ok calls them too); and for the (extended) t = 2 BCH words of vaeq_chase_bch_decode and vaeq_tpc_bch_decode their
// envelope, the builder of their field tables and their Chase front end, ebch_front, beside chase_front.  The builder of the large fields'
// tables and the odd-syndrome step stay with vaeq_bch.hip and vaeq_staircase.hip, and vaeq_chase.hip keeps the text of chase_front in place:
// behind a call they compile to other code.
//
// Floating point: vaeq_tpc.hip rounds every operation of its rule on its own and switches contraction off behind its includes, so nothing here is
// under that pragma.  No float multiplication that feeds an addition may stand in this file: the Chase front end adds non-negative floats and
// nothing else, and every product stays with its decoder.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vaeq {

constexpr int FEC_W = 64;                                      // the bit planes of a frame at most
constexpr int GF_M_MIN = 4, GF_M_MAX = 13;
constexpr int CHASE_N = 256, CHASE_R = 10, CHASE_P = 6, CHASE_SLOTS = CHASE_N / 64;   // the envelope of the Chase front end: n, r, p; slots of a lane
constexpr uint32_t CHASE_NONE = 0xffffu;

// The columns of a parity-check matrix, column j the syndrome of an error at position j.
struct fec_cols {
    uint16_t col[CHASE_N];
};
static_assert(sizeof(fec_cols) <= 512, "the table travels in the kernel arguments");

// a b in GF(2^m): both table reads are issued, the select discards them where a factor is zero
__device__ __forceinline__ uint32_t gf_mul(const uint16_t *EXP, const uint16_t *LOG, uint32_t q, uint32_t a, uint32_t b)
{
    uint32_t s = (uint32_t)LOG[a] + (uint32_t)LOG[b];
    s = s >= q ? s - q : s;
    const uint32_t v = EXP[s];
    return a && b ? v : 0u;
}

// op over the 64 lanes, the same value in every lane (and in a scalar register): inside a row of 16 lanes four DPP steps -- the neighbour in the
// quad, the other pair, the other quad of the half row (row_half_mirror), the other half (row_mirror) -- then the four rows by readlane.  No
// LDS round trip: a butterfly of __shfl_xor is six dependent ds_bpermute, and a codeword needs up to nine reductions one after another.
template <class Op>
__device__ __forceinline__ uint32_t fec_wave_reduce(uint32_t x, Op op)
{
    x = op(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1, 0xf, 0xf, false));    // quad_perm [1, 0, 3, 2]
    x = op(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x4E, 0xf, 0xf, false));    // quad_perm [2, 3, 0, 1]
    x = op(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x141, 0xf, 0xf, false));   // row_half_mirror
    x = op(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x140, 0xf, 0xf, false));   // row_mirror
    const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)x, 0), r1 = (uint32_t)__builtin_amdgcn_readlane((int)x, 16);
    const uint32_t r2 = (uint32_t)__builtin_amdgcn_readlane((int)x, 32), r3 = (uint32_t)__builtin_amdgcn_readlane((int)x, 48);
    return op(op(r0, r1), op(r2, r3));
}
__device__ __forceinline__ uint32_t fec_wave_min(uint32_t x) { return fec_wave_reduce(x, [](uint32_t a, uint32_t b) { return a < b ? a : b; }); }
__device__ __forceinline__ uint32_t fec_wave_xor(uint32_t x) { return fec_wave_reduce(x, [](uint32_t a, uint32_t b) { return a ^ b; }); }
__device__ __forceinline__ uint32_t fec_wave_add(uint32_t x) { return fec_wave_reduce(x, [](uint32_t a, uint32_t b) { return a + b; }); }

// What the Chase front end found, wave-uniform but for T, v, cand, mine and flip.
struct chase_pick {
    uint32_t lp[CHASE_P];                                      // the p least reliable positions, CHASE_NONE behind them
    uint32_t T, v;                                             // this lane's test pattern and its syndrome position, CHASE_NONE where it has none
    bool cand;                                                 // the pattern leads to a codeword
    uint32_t mine, best;                                       // the bits of this lane's metric and of the wave's smallest; all ones: no candidate
    uint32_t Tw, vw;                                           // the winner's T and v (where best is a metric)
    uint32_t flip;                                             // bit k: slot k of this lane is flipped
    int nflip;
};

// The Chase front end of one word in one wave; lane l holds the positions l, l + 64, ... of the n.  key: the bits of |x| of the lane's positions,
// all ones past the word (taken positions turn to all ones here); s0: the syndrome of the hard decisions; COL, POS: the columns and the
// syndrome -> position table; abs_at(v): |x_v| as the lane that owns v formed it, for any v (CHASE_NONE included: the value is then discarded).
// The p least reliable positions come from p wave-wide minima, lane T evaluates test pattern T -- one table lookup and at most seven predicated
// additions -- and one more minimum over the metric bits picks the winner by (metric, T).
template <class A>
__device__ __forceinline__ chase_pick chase_front(uint32_t (&key)[CHASE_SLOTS], const uint32_t s0, const int n, const int p, const int lane,
                                                  const uint16_t *COL, const uint16_t *POS, A &&abs_at)
{
    chase_pick c;
    // the p least reliable positions: wave-uniform position, column and |x|
    uint32_t lc[CHASE_P];
    float la[CHASE_P];
#pragma unroll
    for (int i = 0; i < CHASE_P; i++) {
        c.lp[i] = CHASE_NONE;
        lc[i] = 0;
        la[i] = 0.0f;
        if (i < p) {                                           // wave-uniform; p <= n: a position is left
            uint32_t m = key[0];                               // by (|x|, j): the smallest |x| (its bits order as it does: it is never
#pragma unroll
            for (int k = 1; k < CHASE_SLOTS; k++) m = min(m, key[k]);   // negative), then the smallest position that has it
            m = fec_wave_min(m);
            uint32_t at = CHASE_NONE;
#pragma unroll
            for (int k = CHASE_SLOTS - 1; k >= 0; k--) at = key[k] == m ? (uint32_t)(64 * k + lane) : at;
            c.lp[i] = fec_wave_min(at);
            la[i] = __uint_as_float(m);
            lc[i] = COL[c.lp[i]];
#pragma unroll
            for (int k = 0; k < CHASE_SLOTS; k++) key[k] = (uint32_t)(64 * k + lane) == c.lp[i] ? ~0u : key[k];
        }
    }

    // lane T: test pattern T
    c.T = (uint32_t)lane;
    uint32_t s = s0;
#pragma unroll
    for (int i = 0; i < CHASE_P; i++) s ^= (c.T >> i) & 1u ? lc[i] : 0u;
    c.v = s ? (uint32_t)POS[s] : CHASE_NONE;                   // s < 2^r: a xor of columns
    c.cand = c.T < (1u << p) && (s == 0 || c.v != CHASE_NONE);
    float metric = 0.0f;
    bool cancelled = false;
#pragma unroll
    for (int i = 0; i < CHASE_P; i++) {                        // x + (+0) = x for x >= 0: the predicated add is the specified sum
        const bool in = (c.T >> i) & 1u, hit = in && c.lp[i] == c.v;
        metric = metric + (in && !hit ? la[i] : 0.0f);
        cancelled |= hit;
    }
    const float av = abs_at(c.v);
    metric = metric + (c.v != CHASE_NONE && !cancelled ? av : 0.0f);
    c.mine = c.cand ? __float_as_uint(metric) : ~0u;
    c.best = fec_wave_min(c.mine);                             // by (metric, T)

    c.Tw = c.vw = CHASE_NONE;
    c.flip = 0;
    c.nflip = 0;
    if (c.best != ~0u) {                                       // wave-uniform
        c.Tw = fec_wave_min(c.mine == c.best ? c.T : CHASE_NONE);
        c.vw = (uint32_t)__builtin_amdgcn_readlane((int)c.v, (int)c.Tw);
#pragma unroll
        for (int k = 0; k < CHASE_SLOTS; k++) {
            if (64 * k >= n) break;                            // wave-uniform: a slot no position falls into
            const uint32_t j = (uint32_t)(64 * k + lane);
            uint32_t f = c.vw == j;                            // the symmetric difference of the winner's flips and {vw}
#pragma unroll
            for (int i = 0; i < CHASE_P; i++) f ^= (uint32_t)(((c.Tw >> i) & 1u) && c.lp[i] == j);
            c.flip |= f << k;
            c.nflip += __popcll(__ballot(f != 0));
        }
    }
    return c;
}

// ---- the (extended) double-error-correcting BCH component of vaeq_chase_bch_decode and vaeq_tpc_bch_decode ----

constexpr int EBCH_M_MIN = 4, EBCH_M_MAX = 8;                  // n_i <= 2^m - 1 <= 255: with the parity bit a word fills the front end's CHASE_N
constexpr uint32_t EBCH_NOPOS = 0xfffeu;                       // no located position; differs from CHASE_NONE, which pads the list
constexpr uint32_t EBCH_PAR = 0x10000u;                        // the overall-parity bit of a packed column

// The code as it travels in the kernel arguments, and as a wave reads it: the exp, log and half-solve tables of GF(2^m) in LDS, 2^m uint16 each.
struct ebch_code {
    int m, n_i, ext;
    uint32_t poly;
};
struct ebch_tables {
    const uint16_t *EXP, *LOG, *HS;                            // HS[c]: the even y with y^2 + y = c, 0xffff where there is none
    uint32_t q;                                                // 2^m - 1
    int n_i, ext;
};

// The tables of GF(2^m) at TAB[3 2^m], by all nt threads of the workgroup; the caller puts a __syncthreads behind.  Every thread steps to its
// own exponents (at most 254 doublings, once per workgroup); y and y + 1 have the same y^2 + y, so only the even y writes it.
__device__ __forceinline__ void ebch_build(uint16_t *TAB, const int m, const uint32_t poly, const int tid, const int nt)
{
    const uint32_t q = (1u << m) - 1u;
    uint16_t *EXP = TAB, *LOG = TAB + (1u << m), *HS = LOG + (1u << m);
    for (uint32_t e = (uint32_t)tid; e <= q; e += (uint32_t)nt) {
        uint32_t x = 1;
        for (uint32_t k = 0; k < (1u << EBCH_M_MAX) - 1u; k++) {
            if (k >= e) break;
            x <<= 1;
            x ^= (x >> m) ? poly : 0u;
        }
        EXP[e] = (uint16_t)x;                                  // EXP[q] = 1 is never read: every exponent is reduced below q
        if (e < q) LOG[x] = (uint16_t)e;                       // x runs over 1 .. q once
        HS[e] = (uint16_t)0xffffu;
    }
    if (tid == 0) LOG[0] = 0;                                  // never used as a logarithm; a defined value for the reads that a select discards
    __syncthreads();
    for (uint32_t y = 2u * (uint32_t)tid; y <= q; y += 2u * (uint32_t)nt) HS[gf_mul(EXP, LOG, q, y, y) ^ y] = (uint16_t)y;
}

__device__ __forceinline__ ebch_tables ebch_view(const uint16_t *TAB, const ebch_code c)
{
    return {TAB, TAB + (1u << c.m), TAB + (2u << c.m), (1u << c.m) - 1u, c.n_i, c.ext};
}

// The packed column of position j < n: alpha^j | alpha^(3 j) << 8 | EBCH_PAR, the parity position u = n_i has the parity bit alone.  The xor of
// the columns of a word is S_1 | S_3 << 8 | its weight's parity << 16 in one reduction.
__device__ __forceinline__ uint32_t ebch_col(const ebch_tables tb, const uint32_t j)
{
    const uint32_t ji = min(j, tb.q - 1u);                     // u (and nothing else) may lie past the tables
    uint32_t j3 = 3u * ji;
    j3 = j3 >= tb.q ? j3 - tb.q : j3;
    j3 = j3 >= tb.q ? j3 - tb.q : j3;
    const uint32_t inner = (uint32_t)tb.EXP[ji] | (uint32_t)tb.EXP[j3] << 8;
    return (j < (uint32_t)tb.n_i ? inner : 0u) | EBCH_PAR;
}
// a word of decisions with this packed syndrome is no codeword
__device__ __forceinline__ bool ebch_bad(const ebch_tables tb, const uint32_t syn) { return (syn & (0xffffu | (tb.ext ? EBCH_PAR : 0u))) != 0; }

// What the front end of such a word found.  The flip set of a lane's pattern is { lp[i] : bit i of in } with va (bit 6), vb (bit 7) and the parity
// position (bit 8) where those are flipped and not in the list: disjoint parts, so two sets are compared part by part.
struct ebch_pick {
    uint32_t lp[CHASE_P];
    uint32_t T, va, vb, in;                                    // va < vb: the located positions, EBCH_NOPOS where there is none
    bool cand;
    uint32_t mine, best;                                       // as chase_pick's
    uint32_t Tw, vaw, vbw, inw;                                // the winner's
    uint32_t flip;
    int nflip;
};

// chase_front for a double-error-correcting word: the same list and the same two minima; lane T decides its pattern by the closed form of the
// locator of two errors.  S_1 = S_3 = 0: no position.  S_1 = 0 alone: no candidate.  S_3 = S_1^3: the position log S_1.  Otherwise the roots of
// x^2 + S_1 x + (S_3 + S_1^3) / S_1 are S_1 y and S_1 (y + 1) with y^2 + y = (S_3 + S_1^3) / S_1^3, which the half-solve table answers.  A
// position is compared with n_i before anything is read at it.  Every table read is issued at an index below 2^m whatever the lane holds; the
// selects discard what does not apply.
template <class A>
__device__ __forceinline__ ebch_pick ebch_front(uint32_t (&key)[CHASE_SLOTS], const uint32_t s0, const int n, const int p, const int lane,
                                                const ebch_tables tb, A &&abs_at)
{
    ebch_pick c;
    const uint32_t u = (uint32_t)tb.n_i;                       // the parity position (where ext)
    uint32_t lc[CHASE_P];
    float la[CHASE_P];
#pragma unroll
    for (int i = 0; i < CHASE_P; i++) {
        c.lp[i] = CHASE_NONE;
        lc[i] = 0;
        la[i] = 0.0f;
        if (i < p) {                                           // wave-uniform; p <= n: a position is left
            uint32_t m = key[0];
#pragma unroll
            for (int k = 1; k < CHASE_SLOTS; k++) m = min(m, key[k]);
            m = fec_wave_min(m);
            uint32_t at = CHASE_NONE;
#pragma unroll
            for (int k = CHASE_SLOTS - 1; k >= 0; k--) at = key[k] == m ? (uint32_t)(64 * k + lane) : at;
            c.lp[i] = fec_wave_min(at);
            la[i] = __uint_as_float(m);
            lc[i] = ebch_col(tb, c.lp[i]);
#pragma unroll
            for (int k = 0; k < CHASE_SLOTS; k++) key[k] = (uint32_t)(64 * k + lane) == c.lp[i] ? ~0u : key[k];
        }
    }

    // lane T: the syndromes and the parity of e xor F_T, then the locator
    c.T = (uint32_t)lane;
    uint32_t s = s0;
#pragma unroll
    for (int i = 0; i < CHASE_P; i++) s ^= (c.T >> i) & 1u ? lc[i] : 0u;
    const uint32_t S1 = s & 0xffu, S3 = (s >> 8) & 0xffu;
    const uint32_t S1c = gf_mul(tb.EXP, tb.LOG, tb.q, gf_mul(tb.EXP, tb.LOG, tb.q, S1, S1), S1), D = S3 ^ S1c;
    uint32_t lq = (uint32_t)tb.LOG[D] + tb.q - (uint32_t)tb.LOG[S1c];   // D / S_1^3 (both logarithms are below q)
    lq = lq >= tb.q ? lq - tb.q : lq;
    const uint32_t y = tb.HS[tb.EXP[lq]], ys = y == 0xffffu ? 0u : y;
    const uint32_t x0 = gf_mul(tb.EXP, tb.LOG, tb.q, S1, ys), x1 = x0 ^ S1;
    const uint32_t p0 = tb.LOG[x0], p1 = tb.LOG[x1], ps = tb.LOG[S1];
    const bool two = S1 != 0 && D != 0, one = S1 != 0 && D == 0;
    c.va = two ? min(p0, p1) : one ? ps : EBCH_NOPOS;
    c.vb = two ? max(p0, p1) : EBCH_NOPOS;
    const bool located = S1 == 0 ? S3 == 0 : one ? c.va < u : y != 0xffffu && c.vb < u;
    const uint32_t nv = two ? 2u : one ? 1u : 0u;
    const bool fu = tb.ext && (((s >> 16) + nv) & 1u);         // the parity bit restores an even weight
    c.cand = c.T < (1u << p) && located;
    c.va = c.cand ? c.va : EBCH_NOPOS;                         // a lane without a candidate holds no position
    c.vb = c.cand ? c.vb : EBCH_NOPOS;

    // the flip set and its metric: the listed members in the order of the list, then va, vb and the parity position
    c.in = 0;
    bool la_listed = false, lb_listed = false, lu_listed = false;
    float metric = 0.0f;
#pragma unroll
    for (int i = 0; i < CHASE_P; i++) {                        // x + (+0) = x for x >= 0: the predicated add is the specified sum
        const bool ha = c.lp[i] == c.va, hb = c.lp[i] == c.vb, hu = fu && c.lp[i] == u;   // lp pads with CHASE_NONE, which is no position
        const uint32_t member = ((c.T >> i) & 1u) ^ (uint32_t)ha ^ (uint32_t)hb ^ (uint32_t)hu;
        c.in |= member << i;
        metric = metric + (member ? la[i] : 0.0f);
        la_listed |= ha;
        lb_listed |= hb;
        lu_listed |= hu;
    }
    const bool fa = c.va != EBCH_NOPOS && !la_listed, fb = c.vb != EBCH_NOPOS && !lb_listed, fp = c.cand && fu && !lu_listed;
    c.in |= (uint32_t)fa << 6 | (uint32_t)fb << 7 | (uint32_t)fp << 8;
    const float aa = abs_at(c.va), ab = abs_at(c.vb), au = abs_at(u);
    metric = metric + (fa ? aa : 0.0f);
    metric = metric + (fb ? ab : 0.0f);
    metric = metric + (fp ? au : 0.0f);
    c.mine = c.cand ? __float_as_uint(metric) : ~0u;
    c.best = fec_wave_min(c.mine);                             // by (metric, T)

    c.Tw = CHASE_NONE;
    c.vaw = c.vbw = EBCH_NOPOS;
    c.inw = 0;
    c.flip = 0;
    c.nflip = 0;
    if (c.best != ~0u) {                                       // wave-uniform
        c.Tw = fec_wave_min(c.mine == c.best ? c.T : CHASE_NONE);
        c.vaw = (uint32_t)__builtin_amdgcn_readlane((int)c.va, (int)c.Tw);
        c.vbw = (uint32_t)__builtin_amdgcn_readlane((int)c.vb, (int)c.Tw);
        c.inw = (uint32_t)__builtin_amdgcn_readlane((int)c.in, (int)c.Tw);
#pragma unroll
        for (int k = 0; k < CHASE_SLOTS; k++) {
            if (64 * k >= n) break;                            // wave-uniform: a slot no position falls into
            const uint32_t j = (uint32_t)(64 * k + lane);
            uint32_t f = (uint32_t)(((c.inw >> 6) & 1u) && c.vaw == j) | (uint32_t)(((c.inw >> 7) & 1u) && c.vbw == j) |
                         (uint32_t)(((c.inw >> 8) & 1u) && u == j);
#pragma unroll
            for (int i = 0; i < CHASE_P; i++) f |= (uint32_t)(((c.inw >> i) & 1u) && c.lp[i] == j);
            c.flip |= f << k;
            c.nflip += __popcll(__ballot(f != 0));
        }
    }
    return c;
}

// the primitive polynomial of GF(2^m), m = 4 .. 13, as a bit mask (include/vaeq.h)
static inline uint32_t gf_poly(int m)
{
    static const uint32_t poly[GF_M_MAX - GF_M_MIN + 1] = {0x13, 0x25, 0x43, 0x89, 0x11D, 0x211, 0x409, 0x805, 0x1053, 0x201B};
    return poly[m - GF_M_MIN];
}

// the size of the union of the cyclotomic cosets of 1 .. 2t modulo 2^m - 1: the degree of the generator
static inline int bch_parity(int m, int t)
{
    const int q = (1 << m) - 1;
    bool seen[1 << GF_M_MAX] = {};
    int count = 0;
    for (int j = 1; j <= 2 * t; j++)
        for (int x = j % q; !seen[x]; x = 2 * x % q) {
            seen[x] = true;
            count++;
        }
    return count;
}

// the envelope of an (extended) t = 2 BCH component: n = n_i + ext bits, more inner bits than the generator's degree (2 m for these m)
static inline bool ebch_ok(int64_t m, int64_t n, int64_t ext)
{
    return m >= EBCH_M_MIN && m <= EBCH_M_MAX && ext >= 0 && ext <= 1 && n - ext > bch_parity((int)m, 2) && n - ext <= (1ll << m) - 1;
}
static inline ebch_code ebch_make(int m, int n, int ext) { return {m, n - ext, ext, gf_poly(m)}; }
static inline int64_t ebch_table_bytes(int m) { return 6ll << m; }   // exp, log and half-solve, uint16

// cols_host[n] -> the kernel's table; false unless the columns are distinct, non-zero and below 2^r (n <= CHASE_N, r <= CHASE_R)
static inline bool fec_cols_pack(const int32_t *cols_host, int n, int r, fec_cols *tab)
{
    bool seen[1 << CHASE_R] = {};
    *tab = {};
    for (int j = 0; j < n; j++) {
        const int32_t c = cols_host[j];
        if (c < 1 || c >= (1 << r) || seen[c]) return false;
        seen[c] = true;
        tab->col[j] = (uint16_t)c;
    }
    return true;
}

// The frame of every decoder, behind the empty batch and the NULL pointers: R runs of C codewords in w planes of N symbols from symbol t0 on.
static inline bool fec_frame_ok(int64_t R, int64_t C, int64_t N, int64_t w, int64_t t0)
{
    return R >= 0 && C >= 1 && N >= 1 && N <= 0x3fffffff && w >= 1 && w <= FEC_W && t0 >= 0 && t0 <= N;
}

// C codewords of n bits fit behind t0: il = the interleaver's rule t0 + C ceil(n / w) <= N, else the bit-packed one t0 w + C n <= N w.  The
// caller keeps C n below 2^63.
static inline bool fec_fit_ok(bool il, int64_t C, int64_t n, int64_t w, int64_t t0, int64_t N)
{
    return il ? t0 + C * ((n + w - 1) / w) <= N : t0 * w + C * n <= N * w;
}

}  // namespace vaeq
