// vaeq_staircase.hip -- hard-decision FEC behind the demappers: a sliding-window iterative decoder of a staircase code over shortened BCH
// components (vaeq_staircase_decode, include/vaeq.h).  Integer throughout.  Every component code is linear and bounded-distance decoding depends
// on the error pattern alone, so the decoder works on e = received xor transmitted and there is no encoder; a numpy model gives the same bits.
//
// One chain per workgroup, one lane per component of the pair in flight.  LDS holds the exp / log tables of GF(2^m), built as vaeq_bch.hip
// builds them, and a ring of W + 1 blocks of the error pattern, block i in slot i mod (W + 1).  A block is kept twice: row-major (row a in
// ceil(s / 32) words) and transposed, so that component j of pair i reads its column of block i - 1 (row j of that block's transposed copy) and
// its row of block i (row j of the row-major copy) as whole words, and these words are read and written by lane j alone during the pair step.
// A flip goes to the lane's own word with a plain store and to the other copy, whose words belong to many components, with an LDS atomic xor;
// nobody reads that other copy before the barrier that ends the pair step.  The components of a pair own disjoint bits, so a lane applies its
// flips as soon as it has decided: what it decided on is the state before the step.
// A lane accumulates the t odd syndromes of the set bits of its words; a clean component stops there.  A dirty one runs Berlekamp-Massey and
// the root search in its own registers (t <= 8 is a template argument: t + 1 coefficients, every index a constant after unrolling).  A locator of degree L over
// GF(2^m) has at most L roots, so "exactly L roots, none of them shortened" is "L roots among the positions below 2 s", and the block-0 rule
// of pair 1 is "L roots among the positions s .. 2 s - 1": the search never leaves the word.  L = 1 needs no search, its root is log Lambda_1.
// A block enters through vaeq_ldpc.h's gather (consecutive lanes on consecutive symbols of a plane): its slot is cleared and every error bit
// is an LDS atomic or into both copies -- errors are a percent of the bits.  A block's final state leaves when the window moves past it.
// The table code and the syndrome step repeat vaeq_bch.hip's: from one shared function both kernels compile to other code.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vaeq.h"
#include "vaeq_fec.h"
#include "vaeq_launch.h"
#include "vaeq_ldpc.h"

namespace vaeq {

constexpr int STC_M_MIN = GF_M_MIN, STC_M_MAX = 10, STC_T = 8, STC_S = 511, STC_L = 65535, STC_W = 32;
static_assert(STC_M_MAX <= GF_M_MAX, "the field comes from vaeq_fec.h");

static inline bool stc_dims_ok(int64_t m, int64_t s, int64_t W)
{
    return m >= STC_M_MIN && m <= STC_M_MAX && s >= 2 && s <= STC_S && 2 * s <= (1 << m) - 1 && W >= 1 && W <= STC_W;
}

// the tables (2 x 2^m uint16) and W + 1 blocks, each row-major and transposed, s rows of ceil(s / 32) words
static inline int64_t stc_state_bytes(int64_t m, int64_t s, int64_t W) { return ((int64_t)4 << m) + (W + 1) * 2 * s * ((s + 31) / 32) * 4; }

struct stc_args {
    long long N, t0;
    int C, w, m, s, L, W, iters, P;
    uint32_t poly;
};

template <int T>
__global__ __launch_bounds__(512) void staircase_kernel(const stc_args A, const float *__restrict__ llr, const int8_t *__restrict__ bits,
                                                        int32_t *__restrict__ out, int8_t *__restrict__ hard, int32_t *__restrict__ pos_err,
                                                        int32_t *__restrict__ pos_iters)
{
    extern __shared__ __align__(16) unsigned char stc_lds[];
    __shared__ unsigned cnt[4];                                // pre_err, erased, nflip, bad_flips: unsigned, a count past 2^32 wraps (vaeq.h)
    __shared__ int blkerr[STC_W + 1];                          // the errors of the block that leaves a slot
    const int tid = threadIdx.x, NT = blockDim.x;
    const int m = A.m, s = A.s, L = A.L, W = min(A.W, STC_W), ring = W + 1, RW = (s + 31) >> 5, blk = s * RW;
    const int max_iter = min(A.iters, LDPC_ITER), w = A.w;
    const uint32_t q = (1u << m) - 1u;
    uint16_t *EXP = reinterpret_cast<uint16_t *>(stc_lds), *LOG = EXP + (1u << m);
    uint32_t *ROWS = reinterpret_cast<uint32_t *>(LOG + (1u << m)), *COLS = ROWS + ring * blk;   // slot k: ROWS + k blk, its transpose COLS + k blk
    const size_t run = blockIdx.x / (unsigned)A.C;
    const int chain = (int)(blockIdx.x % (unsigned)A.C);
    const size_t rc = run * (size_t)A.C + chain;
    const long long s2 = (long long)s * s, chain0 = (long long)chain * L * s2;                  // the chain's first global bit

    {   // the tables: thread tid owns the exponents tid ch .. tid ch + ch - 1 (vaeq_bch.hip)
        const uint32_t ch = (q + (uint32_t)NT - 1u) / (uint32_t)NT, lo = (uint32_t)tid * ch;
        uint32_t x = 1, base = 2;                              // x = alpha^lo by squaring; a product is m shift-and-add steps
        for (int b = 0; b <= STC_M_MAX; b++) {
            uint32_t y = 0, z = 0;                             // y = x base, z = base^2
            for (int k = STC_M_MAX - 1; k >= 0; k--) {
                y <<= 1; z <<= 1;
                y ^= (y >> m) ? A.poly : 0u;
                z ^= (z >> m) ? A.poly : 0u;
                if ((base >> k) & 1u) { y ^= x; z ^= base; }
            }
            x = ((lo >> b) & 1u) ? y : x;
            base = z;
        }
        if (tid == 0) LOG[0] = 0;                              // never used as a logarithm; a defined value for the reads that a select discards
        for (uint32_t k = 0; k < ch; k++) {
            const uint32_t e = lo + k;
            if (e < q) { EXP[e] = (uint16_t)x; LOG[x] = (uint16_t)e; }
            if (e == q) EXP[q] = 1;
            x <<= 1;
            x ^= (x >> m) ? A.poly : 0u;
        }
    }
    if (tid < 4) cnt[tid] = 0;
    for (int k = tid; k < STC_W + 1; k += NT) blkerr[k] = 0;
    for (int k = tid; k < 2 * ring * blk; k += NT) ROWS[k] = 0u;                                 // block 0 is all zero and stays so
    __syncthreads();

    auto mul = [&](uint32_t a, uint32_t b) { return gf_mul(EXP, LOG, q, a, b); };

    unsigned pre = 0, era = 0, nflip = 0, bad = 0;
    // block i (1 .. L) enters a cleared slot: the gather of the s^2 bits behind global bit chain0 + (i - 1) s^2
    auto enter = [&](int i, int slot) {
        const long long g0 = chain0 + (long long)(i - 1) * s2, s_lo = g0 / w;
        const ldpc_window win = {A.t0 + s_lo, s_lo * w - g0, (int)((g0 + s2 - 1) / w - s_lo) + 1, 1};
        uint32_t *Rs = ROWS + slot * blk, *Cs = COLS + slot * blk;
        ldpc_gather(win, run, A.N, w, (int)s2, tid, NT, llr, bits, [&](long long j, float x, uint32_t b) {
            era += x == 0.f;
            if ((uint32_t)(x < 0.f) != b) {                    // a NaN and +-0 are bit 0
                const int a = (int)j / s, c = (int)j - a * s;
                pre++;
                atomicOr(&Rs[a * RW + (c >> 5)], 1u << (c & 31));
                atomicOr(&Cs[c * RW + (a >> 5)], 1u << (a & 31));
            }
        });
    };
    // block i leaves: its errors to the slot's counter, its decisions (the TX bit xor the error bit) to hard
    auto leave = [&](int i, int slot) {
        const uint32_t *Rs = ROWS + slot * blk;
        int err = 0;
        for (int k = tid; k < blk; k += NT) err += __popc(Rs[k]);
        if (err) atomicAdd(&blkerr[slot], err);
        if (hard) {
            const long long g0 = chain0 + (long long)(i - 1) * s2;
            int8_t *dst = hard + rc * (size_t)L * (size_t)s2 + (size_t)(i - 1) * (size_t)s2;
            for (int j = tid; j < (int)s2; j += NT) {
                const int a = j / s, c = j - a * s;
                const long long g = g0 + j, sym = g / w;
                const int8_t tx = bits[(run * (size_t)w + (size_t)(g - sym * w)) * (size_t)A.N + (size_t)(A.t0 + sym)];
                dst[j] = (int8_t)((tx & 1) ^ (int)((Rs[a * RW + (c >> 5)] >> (c & 31)) & 1u));
            }
        }
    };
    // the block's counter to pos_err and the chain's sum (thread 0, behind a barrier)
    unsigned perr = 0;
    auto file = [&](int i, int slot) {
        const int e = blkerr[slot];
        blkerr[slot] = 0;
        perr += (unsigned)e;
        if (pos_err) pos_err[rc * (size_t)L + (size_t)(i - 1)] = e;
    };

    // component tid of pair i: -> its status; the flips are applied
    auto component = [&](int i, int sp, int sc) -> int {
        uint32_t *own_col = COLS + sp * blk + tid * RW, *own_row = ROWS + sc * blk + tid * RW;   // column tid of block i - 1, row tid of block i
        uint32_t syn[T];
#pragma unroll
        for (int k = 0; k < T; k++) syn[k] = 0;
        for (int half = 0; half < 2; half++) {
            const uint32_t *src = half ? own_row : own_col;
            for (int wd = 0; wd < (STC_S + 31) / 32; wd++) {
                if (wd >= RW) break;
                uint32_t word = src[wd];
                for (int k = 0; k < 32; k++) {
                    if (!word) break;
                    const uint32_t p = (uint32_t)(half * s + wd * 32 + __ffs((int)word) - 1);   // p < 2 s <= q
                    word &= word - 1u;
                    uint32_t y = p, d = 2u * p;                // S_j += alpha^(j p) for the odd j: the exponent advances by 2 p
                    d = d >= q ? d - q : d;
#pragma unroll
                    for (int j = 0; j < T; j++) {
                        syn[j] ^= EXP[y];
                        y += d;
                        y = y >= q ? y - q : y;
                    }
                }
            }
        }
        uint32_t any = 0;
#pragma unroll
        for (int k = 0; k < T; k++) any |= syn[k];
        if (!any) return 0;

        uint32_t S[2 * T + 1];                             // S[j], j = 1 .. 2t; S_2j = S_j^2
        S[0] = 0;
#pragma unroll
        for (int j = 1; j <= 2 * T; j++) {
            if (j & 1) S[j] = syn[j >> 1];
            else {
                uint32_t lg = 2u * (uint32_t)LOG[S[j >> 1]];
                lg = lg >= q ? lg - q : lg;
                const uint32_t v = EXP[lg];
                S[j] = S[j >> 1] ? v : 0u;
            }
        }
        // Berlekamp-Massey: B <- x B every step; on a discrepancy d, Lambda <- Lambda + (d / b) B, and where 2 L <= r the old Lambda becomes
        // B, b <- d, L <- r + 1 - L.  Coefficients above x^t are dropped: they matter only where L ends above t, which is status 2.
        uint32_t lam[T + 1], Bp[T + 1], bb = 1;
        int Ld = 0;
#pragma unroll
        for (int k = 0; k <= T; k++) lam[k] = Bp[k] = k == 0;
#pragma unroll
        for (int r = 0; r < 2 * T; r++) {
            if (Ld <= T) {
#pragma unroll
                for (int k = T; k >= 1; k--) Bp[k] = Bp[k - 1];
                Bp[0] = 0;
                uint32_t d = S[r + 1];
#pragma unroll
                for (int k = 1; k <= T; k++)
                    if (k <= r && k <= Ld) d ^= mul(lam[k], S[r + 1 - k > 0 ? r + 1 - k : 0]);
                if (d) {
                    uint32_t ib = q - (uint32_t)LOG[bb];
                    ib = ib >= q ? ib - q : ib;
                    const uint32_t coef = mul(d, EXP[ib]);
                    const bool grow = 2 * Ld <= r;
#pragma unroll
                    for (int k = 0; k <= T; k++) {
                        const uint32_t old = lam[k];
                        lam[k] = old ^ mul(coef, Bp[k]);
                        Bp[k] = grow ? old : Bp[k];
                    }
                    if (grow) {
                        Ld = r + 1 - Ld;
                        bb = d;
                    }
                }
            }
        }
        if (Ld > T) return 2;
        // the roots alpha^(-p) of Lambda among the positions lo .. 2 s - 1, packed ten bits each; pair 1 has no block 0 to flip
        const uint32_t lo = i == 1 ? (uint32_t)s : 0u, hi = 2u * (uint32_t)s;
        unsigned long long r0 = 0, r1 = 0;
        int nroot = 0;
        if (Ld == 1) {
            const uint32_t p = LOG[lam[1]];                    // Lambda = 1 + Lambda_1 x, and Lambda_1 != 0 where L = 1
            if (lam[1] && p >= lo && p < hi) { r0 = p; nroot = 1; }
        } else {
            uint32_t ll[T + 1];                            // log Lambda_k, and 0 with nz clear for a zero coefficient (every k > L is one)
            bool nz[T + 1];
#pragma unroll
            for (int k = 1; k <= T; k++) {
                nz[k] = lam[k] != 0;
                ll[k] = nz[k] ? (uint32_t)LOG[lam[k]] : 0u;
            }
            for (uint32_t p0 = lo; p0 < 2u * STC_S; p0 += 4) {  // four positions a trip, their table reads in flight together
                if (p0 >= hi) break;
                uint32_t v[4][T];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const uint32_t pp = min(p0 + u, hi - 1u), g = pp == 0 ? 0u : q - pp;   // alpha^(-pp); a clamped position: pp < 2 s <= q
                    uint32_t acc = 0;                          // Lambda(alpha^(-pp)) = 1 + sum_k Lambda_k alpha^(-k pp)
#pragma unroll
                    for (int k = 1; k <= T; k++) {
                        acc += g;
                        acc = acc >= q ? acc - q : acc;
                        uint32_t x = ll[k] + acc;
                        x = x >= q ? x - q : x;
                        v[u][k - 1] = EXP[x];
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    uint32_t val = 1;
#pragma unroll
                    for (int k = 1; k <= T; k++)
                        val ^= nz[k] ? v[u][k - 1] : 0u;
                    if (val == 0 && p0 + u < hi && nroot < T) {
                        const uint32_t pp = p0 + u;
                        if (nroot < 6) r0 |= (unsigned long long)pp << (10 * nroot);
                        else r1 |= (unsigned long long)pp << (10 * (nroot - 6));
                        nroot++;
                    }
                }
            }
        }
        if (nroot != Ld) return 2;
        for (int k = 0; k < T; k++) {
            if (k >= nroot) break;
            const int p = (int)((k < 6 ? r0 >> (10 * k) : r1 >> (10 * (k - 6))) & 1023u);
            uint32_t *own, *other;                             // bit (p, tid) of block i - 1 or bit (tid, p - s) of block i, in both copies
            int ob;
            if (p < s) {
                own = own_col + (p >> 5);
                ob = p & 31;
                other = ROWS + sp * blk + p * RW + (tid >> 5);
            } else {
                own = own_row + ((p - s) >> 5);
                ob = (p - s) & 31;
                other = COLS + sc * blk + (p - s) * RW + (tid >> 5);
            }
            const uint32_t old = *own;
            bad += !((old >> ob) & 1u);
            *own = old ^ (1u << ob);
            atomicXor(other, 1u << (tid & 31));
        }
        nflip += (unsigned)nroot;
        return 1;
    };

    for (int i = 1; i <= STC_W; i++) {                         // the first window: blocks 1 .. min(W, L); block 0 is slot 0
        if (i > W || i > L) break;
        enter(i, i);
    }
    __syncthreads();

    int total = 0, most = 0, all_ok = 1;
    int sq = 0;                                                // q mod ring: the slot of block q
    for (int pos = 0; pos < STC_L; pos++) {
        if (pos >= A.P) break;
        int iters = 0, dirty = 0;
        for (int it = 0; it < LDPC_ITER; it++) {
            if (it >= max_iter) break;
            int flipped = 0, bad_status = 0, sp = sq;
            for (int k = 0; k < STC_W; k++) {
                const int i = pos + 1 + k;
                if (k >= W || i > L) break;
                const int sc = sp + 1 == ring ? 0 : sp + 1;
                if (tid < s) {
                    const int st = component(i, sp, sc);
                    flipped |= st == 1;
                    bad_status |= st != 0;
                }
                __syncthreads();
                sp = sc;
            }
            iters = it + 1;
            dirty = __syncthreads_or(bad_status);              // workgroup-uniform, behind a barrier
            if (!__syncthreads_or(flipped)) break;
        }
        total += iters;
        most = max(most, iters);
        all_ok &= !dirty;
        if (pos_iters && tid == 0) pos_iters[rc * (size_t)A.P + pos] = iters;
        if (pos == A.P - 1) break;

        // the window moves: block pos leaves the slot that block pos + W + 1 enters
        if (pos >= 1) leave(pos, sq);
        __syncthreads();
        if (tid == 0 && pos >= 1) file(pos, sq);
        for (int k = tid; k < blk; k += NT) ROWS[sq * blk + k] = COLS[sq * blk + k] = 0u;
        __syncthreads();
        enter(pos + W + 1, sq);                                // pos < P - 1 = L - W: the block exists
        __syncthreads();
        sq = sq + 1 == ring ? 0 : sq + 1;
    }

    {                                                          // the blocks still resident, final with the last position
        const int first = max(A.P - 1, 1);
        int slot = first % ring;
        for (int i = first; i <= L; i++) {
            leave(i, slot);
            slot = slot + 1 == ring ? 0 : slot + 1;
        }
        if (pre) atomicAdd(&cnt[0], pre);
        if (era) atomicAdd(&cnt[1], era);
        if (nflip) atomicAdd(&cnt[2], nflip);
        if (bad) atomicAdd(&cnt[3], bad);
        __syncthreads();
        if (tid == 0) {
            slot = first % ring;
            for (int i = first; i <= L; i++) {
                file(i, slot);
                slot = slot + 1 == ring ? 0 : slot + 1;
            }
            int32_t *dst = out + rc * 8;
            dst[0] = total;
            dst[1] = all_ok;
            dst[2] = (int32_t)perr;
            dst[3] = (int32_t)cnt[0];
            dst[4] = (int32_t)cnt[1];
            dst[5] = most;
            dst[6] = (int32_t)cnt[2];
            dst[7] = (int32_t)cnt[3];
        }
    }
}

}  // namespace vaeq

extern "C" int64_t vaeq_staircase_lds_bytes(int32_t m, int32_t s, int32_t W)
{
    return vaeq::stc_dims_ok(m, s, W) ? vaeq::stc_state_bytes(m, s, W) : (int64_t)VAEQ_ERR_SHAPE;
}

extern "C" int vaeq_staircase_decode(int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0, int32_t m, int32_t t, int32_t s, int32_t L,
                                     const float *llr, const int8_t *bits, int32_t W, int32_t iters, int32_t *out, int8_t *hard,
                                     int32_t *pos_err, int32_t *pos_iters, void *stream)
{
    using namespace vaeq;
    if (R == 0) return VAEQ_OK;                                // an empty batch owns no memory: its pointers may be NULL
    if (!llr || !bits || !out) return VAEQ_ERR_NULL;
    if (!fec_frame_ok(R, C, N, w, t0) || iters < 1 || iters > LDPC_ITER) return VAEQ_ERR_SHAPE;
    if (t < 1 || t > STC_T || !stc_dims_ok(m, s, W) || bch_parity(m, t) >= 2 * s || L < 1 || L > STC_L) return VAEQ_ERR_SHAPE;
    // the bit-packed fit rule t0 w + C n_chain <= N w without the product, so not fec_fit_ok: C n_chain passes 2^63 (n_chain reaches 1.7e10,
    // C 2^31 - 1); (N - t0) w < 2^36
    const int64_t n_chain = (int64_t)L * s * s, room = (N - t0) * w;
    if (stc_state_bytes(m, s, W) > LDPC_STATE_MAX || C > room / n_chain || (int64_t)R * C > 0x7fffffff) return VAEQ_ERR_SHAPE;
    const int P = L - W + 1 > 1 ? L - W + 1 : 1;
    const stc_args A = {(long long)N, (long long)t0, (int)C, (int)w, (int)m, (int)s, (int)L, (int)W, (int)iters, P, gf_poly(m)};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((int64_t)R * C)), block((unsigned)((s + 63) / 64 * 64));
    const size_t lds = (size_t)stc_state_bytes(m, s, W);
    switch (t) {                                               // t is a template argument: every coefficient index is a constant
    case 1: return launch(staircase_kernel<1>, grid, block, lds, st, A, llr, bits, out, hard, pos_err, pos_iters);
    case 2: return launch(staircase_kernel<2>, grid, block, lds, st, A, llr, bits, out, hard, pos_err, pos_iters);
    case 3: return launch(staircase_kernel<3>, grid, block, lds, st, A, llr, bits, out, hard, pos_err, pos_iters);
    case 4: return launch(staircase_kernel<4>, grid, block, lds, st, A, llr, bits, out, hard, pos_err, pos_iters);
    case 5: return launch(staircase_kernel<5>, grid, block, lds, st, A, llr, bits, out, hard, pos_err, pos_iters);
    case 6: return launch(staircase_kernel<6>, grid, block, lds, st, A, llr, bits, out, hard, pos_err, pos_iters);
    case 7: return launch(staircase_kernel<7>, grid, block, lds, st, A, llr, bits, out, hard, pos_err, pos_iters);
    }
    return launch(staircase_kernel<8>, grid, block, lds, st, A, llr, bits, out, hard, pos_err, pos_iters);
}
