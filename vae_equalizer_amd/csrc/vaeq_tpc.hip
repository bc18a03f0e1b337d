// vaeq_tpc.hip -- the soft-in / soft-out decoder of include/vaeq.h (vaeq_tpc_decode): Chase-Pyndiah decoding of a product code whose rows and
// columns are words of two single-error-correcting codes given by the columns of their parity-check matrices, over the demappers' LLRs under the
// LDPC decoder's bit-packed map, against the TX bits.  The rule is stated on r, the LLR towards the transmitted bit, so there is no encoder;
// integers and float32 operations in a fixed order, so a numpy model gives the same bits.
//
// The mapping: one workgroup per block in flight, grid-stride over the R C blocks.  All threads gather the block once through ldpc_gather and
// file r (clamped) and W (float32 each, row stride n2 | 1: a column walk changes bank at every step) and a byte TX bit | d << 1 per bit in LDS,
// where they stay for all half-iterations.  In a half-iteration one wave decodes one word, lanes on positions (base + j stride: stride 1 along a
// row, n2 | 1 along a column).  vaeq_fec.h's chase_front does the Chase part: the p least reliable positions from p wave-wide minima of the key
// |R| bits, lane T evaluates test pattern T, one more minimum over the metric bits picks the winner D.  The competitor search: every lane that
// holds a candidate walks the at most p + 2 positions where its flips can differ from D's -- the p least reliable ones, its own syndrome position
// and D's -- and, where they do differ, files its metric's bits with an LDS atomic minimum (non-negative floats order as unsigned integers) into a
// per-wave array of n' words that started at all ones.  A minimum is order-free, so the bits are deterministic.  Each lane then reads the
// entries of its positions and forms W'.  The stop test is one pass over the decision bytes in the other direction, a wave per word, and the
// workgroup decides with __syncthreads_or, so every thread reaches every barrier.  Counters are ballots and popcounts, joined across the waves by
// integer LDS atomics.  Everything leaves as plain vector stores.  Every loop has a static bound.
//
// The kernel and the word are templates on the component: tpc_ham, two single-error-correcting codes by their columns (vaeq_tpc_decode), and
// tpc_bch, two (extended) t = 2 BCH codes by their fields (vaeq_tpc_bch_decode).  A component says what the packed column of a position is, what
// its front end is (chase_front / ebch_front of vaeq_fec.h), where a candidate competes and when a word of decisions is a codeword; the block
// state, the gather, the schedule, W', the counters and the outputs are written once.  For tpc_bch the columns and positions give way to the exp,
// log and half-solve tables of GF(2^m), built in LDS by the workgroup (one set where m1 == m2), and a lane's competitor walk has p + 5 places.
//
// Two wave counts per component: 16 waves where a block has more than 4096 bits (such a block's state leaves room for one or two workgroups on a CU: the
// waves have to come from inside it), 4 waves below (several workgroups share a CU).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vaeq.h"
#include "vaeq_fec.h"
#include "vaeq_launch.h"
#include "vaeq_ldpc.h"

// Every float32 operation of the rule is rounded on its own.  The build contracts a * b + c into one fma by default, and HIP's __fmul_rn /
// __fadd_rn are plain operators inside a header, which contract like any other: the rule's arithmetic is written with the operators of the
// language behind this line, where nothing is fused.  vaeq_fec.h stands before it and holds no product.
#pragma clang fp contract(off)

namespace vaeq {

constexpr int TPC_ITERS = 16, TPC_HALF = 2 * TPC_ITERS;        // the words are the Chase front end's: n <= CHASE_N, r <= CHASE_R, p <= CHASE_P
constexpr int TPC_WAVES_BIG = 16, TPC_WAVES_SMALL = 4, TPC_BIG_ABOVE = 4096;
constexpr int64_t TPC_GRID = 1024, TPC_LDS_MAX = 156 * 1024;   // the dynamic block; the static counters below take under 1 KiB of the rest

struct tpc_args {
    long long N, t0, blocks;                                   // blocks = R C
    int C, w, n1, r1, n2, r2, p, iters, K1, K2;
    float clip;
    float alpha[TPC_HALF], beta[TPC_HALF];
};

static inline int tpc_waves(int n1, int n2) { return n1 * n2 > TPC_BIG_ABOVE ? TPC_WAVES_BIG : TPC_WAVES_SMALL; }
// r and W (float32) and the byte TX bit | d << 1 of every bit at the odd row stride, the competitor array of every wave, the two tables of
// columns and the two syndrome -> position tables (uint16)
static inline int64_t tpc_state_bytes(int n1, int r1, int n2, int r2)
{
    const int64_t cells = (int64_t)n1 * (n2 | 1), nmax = n1 > n2 ? n1 : n2;
    return 8 * cells + (cells + 3) / 4 * 4 + 4 * tpc_waves(n1, n2) * nmax + (2 * ((int64_t)n1 + n2) + 3) / 4 * 4 + 2 * ((1ll << r1) + (1ll << r2));
}
// the same state with the field tables (exp, log, half-solve; one set where m1 == m2) in the place of the columns and positions
static inline int64_t tpc_bch_state_bytes(int m1, int n1, int m2, int n2)
{
    const int64_t cells = (int64_t)n1 * (n2 | 1), nmax = n1 > n2 ? n1 : n2;
    return 8 * cells + (cells + 3) / 4 * 4 + 4 * tpc_waves(n1, n2) * nmax + ebch_table_bytes(m1) + (m1 == m2 ? 0 : ebch_table_bytes(m2));
}
static inline bool tpc_dims_ok(int64_t n1, int64_t r1, int64_t n2, int64_t r2)
{
    return n1 >= 3 && n1 <= CHASE_N && n2 >= 3 && n2 <= CHASE_N && r1 >= 2 && r1 <= CHASE_R && r2 >= 2 && r2 <= CHASE_R;
}

// The two kinds of component as a wave reads them, one view per direction: the packed column of a position, what its front end is, whether a
// syndrome of decisions is a codeword's, and the view of a half-iteration.  tpc_ham / tpc_bch are the codes as the kernel arguments carry them.
struct tpc_ham_word {
    const uint16_t *COL, *POS;
    __device__ __forceinline__ uint32_t col(int j) const { return COL[j]; }
    __device__ __forceinline__ bool bad(uint32_t syn) const { return syn != 0; }
    template <class A>
    __device__ __forceinline__ chase_pick front(uint32_t (&key)[CHASE_SLOTS], uint32_t s0, int n, int p, int lane, A &&abs_at) const
    {
        return chase_front(key, s0, n, p, lane, COL, POS, abs_at);
    }
    static __device__ __forceinline__ tpc_ham_word pick(bool first, const tpc_ham_word a, const tpc_ham_word b)
    {
        return {first ? a.COL : b.COL, first ? a.POS : b.POS};
    }
};
struct tpc_bch_word {
    ebch_tables tb;
    __device__ __forceinline__ uint32_t col(int j) const { return ebch_col(tb, (uint32_t)j); }
    __device__ __forceinline__ bool bad(uint32_t syn) const { return ebch_bad(tb, syn); }
    template <class A>
    __device__ __forceinline__ ebch_pick front(uint32_t (&key)[CHASE_SLOTS], uint32_t s0, int n, int p, int lane, A &&abs_at) const
    {
        return ebch_front(key, s0, n, p, lane, tb, abs_at);
    }
    static __device__ __forceinline__ tpc_bch_word pick(bool first, const tpc_bch_word a, const tpc_bch_word b)
    {
        return {{first ? a.tb.EXP : b.tb.EXP, first ? a.tb.LOG : b.tb.LOG, first ? a.tb.HS : b.tb.HS, first ? a.tb.q : b.tb.q,
                 first ? a.tb.n_i : b.tb.n_i, first ? a.tb.ext : b.tb.ext}};
    }
};

// The tables of the two codes behind the block's state, by all NT threads; the block loop's first barrier stands behind them.
struct tpc_ham {
    fec_cols tab1, tab2;
    using word = tpc_ham_word;
    __device__ __forceinline__ void tables(const tpc_args &A, unsigned char *mem, int tid, int NT, word &w1, word &w2) const
    {
        const int n1 = A.n1, n2 = A.n2;
        uint16_t *COL1 = reinterpret_cast<uint16_t *>(mem), *COL2 = COL1 + n1;
        uint16_t *POS1 = COL1 + (n1 + n2 + 1) / 2 * 2, *POS2 = POS1 + (1 << A.r1);
        for (int s = tid; s < (1 << A.r1) + (1 << A.r2); s += NT) POS1[s] = (uint16_t)CHASE_NONE;
        __syncthreads();
        for (int j = tid; j < n1; j += NT) {                   // the columns are distinct: no two threads write one entry
            COL1[j] = tab1.col[j];
            POS1[tab1.col[j]] = (uint16_t)j;
        }
        for (int j = tid; j < n2; j += NT) {
            COL2[j] = tab2.col[j];
            POS2[tab2.col[j]] = (uint16_t)j;
        }
        w1 = {COL1, POS1};
        w2 = {COL2, POS2};
    }
};
struct tpc_bch {
    ebch_code c1, c2;
    using word = tpc_bch_word;
    __device__ __forceinline__ void tables(const tpc_args &, unsigned char *mem, int tid, int NT, word &w1, word &w2) const
    {
        uint16_t *TAB1 = reinterpret_cast<uint16_t *>(mem), *TAB2 = c1.m == c2.m ? TAB1 : TAB1 + (3u << c1.m);   // one field, one set of tables
        ebch_build(TAB1, c1.m, c1.poly, tid, NT);
        if (c1.m != c2.m) {                                    // uniform: a kernel argument
            __syncthreads();
            ebch_build(TAB2, c2.m, c2.poly, tid, NT);
        }
        w1 = {ebch_view(TAB1, c1)};
        w2 = {ebch_view(TAB2, c2)};
    }
};
static_assert(sizeof(tpc_args) + sizeof(tpc_ham) <= 2048 && sizeof(tpc_bch) <= sizeof(tpc_ham), "the codes and the schedules travel in the kernel arguments");

// The competitors of a word with a winner: every lane that holds a candidate files its metric's bits at the positions where its flips and D's
// differ.  Single-error-correcting: position lp[i] is flipped by T iff bit i of T xor (v == lp[i]); a v outside the list is flipped by its own
// candidate alone.
__device__ __forceinline__ void tpc_compete(const chase_pick &c, const int p, uint32_t *MC)
{
    const uint32_t T = c.T, v = c.v, Tw = c.Tw, vw = c.vw, mine = c.mine;
    bool v_listed = v == CHASE_NONE, vw_listed = vw == CHASE_NONE;
#pragma unroll
    for (int i = 0; i < CHASE_P; i++) {
        if (i < p) {
            const uint32_t mt = ((T >> i) & 1u) ^ (uint32_t)(v == c.lp[i]), md = ((Tw >> i) & 1u) ^ (uint32_t)(vw == c.lp[i]);
            if (mt != md) atomicMin(&MC[c.lp[i]], mine);
            v_listed |= v == c.lp[i];
            vw_listed |= vw == c.lp[i];
        }
    }
    if (v != vw) {
        if (!v_listed) atomicMin(&MC[v], mine);
        if (!vw_listed) atomicMin(&MC[vw], mine);
    }
}

// Double-error-correcting: the flip sets are compared part by part (ebch_pick): the p listed positions, this lane's at most two unlisted located
// positions, the winner's, and the parity position -- p + 5 places.  A position is an address only where its bit of `in` says it was located
// below n_i (or is the parity position of an extended word).
__device__ __forceinline__ void tpc_compete(const ebch_pick &c, const int p, uint32_t *MC, const uint32_t u)
{
    const uint32_t diff = c.in ^ c.inw, mine = c.mine;
#pragma unroll
    for (int i = 0; i < CHASE_P; i++) {
        if (i < p && ((diff >> i) & 1u)) atomicMin(&MC[c.lp[i]], mine);
    }
    const bool fa = (c.in >> 6) & 1u, fb = (c.in >> 7) & 1u, faw = (c.inw >> 6) & 1u, fbw = (c.inw >> 7) & 1u;
    if (fa && !((faw && c.vaw == c.va) || (fbw && c.vbw == c.va))) atomicMin(&MC[c.va], mine);
    if (fb && !((faw && c.vaw == c.vb) || (fbw && c.vbw == c.vb))) atomicMin(&MC[c.vb], mine);
    if (faw && !((fa && c.va == c.vaw) || (fb && c.vb == c.vaw))) atomicMin(&MC[c.vaw], mine);
    if (fbw && !((fa && c.va == c.vbw) || (fb && c.vb == c.vbw))) atomicMin(&MC[c.vbw], mine);
    if ((diff >> 8) & 1u) atomicMin(&MC[u], mine);
}
__device__ __forceinline__ void tpc_compete(const tpc_ham_word &, const chase_pick &c, const int p, uint32_t *MC) { tpc_compete(c, p, MC); }
__device__ __forceinline__ void tpc_compete(const tpc_bch_word &w, const ebch_pick &c, const int p, uint32_t *MC)
{
    tpc_compete(c, p, MC, (uint32_t)w.tb.n_i);
}

// the soft input of a cell: one multiplication, one addition, never fused
__device__ __forceinline__ float tpc_soft(float r, float alpha, float W)
{
    const float scaled = alpha * W;
    return r + scaled;
}

// One word, one wave: the n positions at base + j stride, the code in cw.  W' and the decision bytes are written in place; the result is
// the status, the weight of d and the positions without a competitor (wave-uniform).
struct tpc_word_result {
    int status, weight, nbeta;
};

template <class W>
__device__ __forceinline__ tpc_word_result tpc_word(const int lane, const int n, const int p, const int base, const int stride, const float alpha,
                                                    const float beta, const float clip, const W cw, const float *RR, float *WW, uint8_t *DB,
                                                    uint32_t *MC)
{
    uint32_t key[CHASE_SLOTS];                                 // the bits of |R| of the positions not yet taken, all ones otherwise
    float Rv[CHASE_SLOTS];
    uint32_t err = 0, s0 = 0;                                  // bit k: slot k of this lane
#pragma unroll
    for (int k = 0; k < CHASE_SLOTS; k++) {
        key[k] = ~0u;
        Rv[k] = 0.0f;
    }
#pragma unroll
    for (int k = 0; k < CHASE_SLOTS; k++) {
        if (64 * k >= n) break;                                // wave-uniform: a slot no position falls into
        const int j = 64 * k + lane;
        const bool in = j < n;
        const int jj = in ? j : 0, at = base + jj * stride;    // a lane past the word reads position 0 and keeps nothing of it
        Rv[k] = tpc_soft(RR[at], alpha, WW[at]);
        const uint32_t e = in && Rv[k] < 0.0f;
        key[k] = in ? __float_as_uint(Rv[k]) & 0x7fffffffu : ~0u;
        err |= e << k;
        s0 ^= e ? cw.col(jj) : 0u;
        if (in) MC[j] = ~0u;                                   // no competitor yet
    }
    s0 = fec_wave_xor(s0);

    // the winner D; |R_v| of a syndrome position as the lane that owns v formed it
    const auto c = cw.front(key, s0, n, p, lane, [&](uint32_t v) {
        const int at = base + (int)min(v, (uint32_t)n - 1u) * stride;
        return fabsf(tpc_soft(RR[at], alpha, WW[at]));
    });
    const uint32_t best = c.best;

    tpc_word_result res = {2, 0, 0};
    if (best != ~0u) {                                         // wave-uniform
        res.status = c.nflip ? 1 : 0;
        __builtin_amdgcn_wave_barrier();                       // the competitors: where a candidate's flips and D's differ
        if (c.cand) tpc_compete(cw, c, p, MC);
        __builtin_amdgcn_wave_barrier();
    }
    err ^= c.flip;                                             // d
    const float mD = __uint_as_float(best);
#pragma unroll
    for (int k = 0; k < CHASE_SLOTS; k++) {
        if (64 * k >= n) break;
        const int j = 64 * k + lane;
        const bool in = j < n, d = (err >> k) & 1u;
        const uint32_t mc = in ? MC[j] : 0u;
        const bool none = mc == ~0u;
        float Wn = 0.0f;                                       // status 2: +0 for the whole word
        if (res.status != 2) {
            const float delta = __uint_as_float(none ? best : mc) - mD;
            Wn = none ? (d ? -beta : beta) : (d ? -delta : delta) - Rv[k];
            Wn = fminf(fmaxf(Wn, -clip), clip);
            res.nbeta += __popcll(__ballot(in && none));
        }
        res.weight += __popcll(__ballot(in && d));
        if (in) {
            const int at = base + j * stride;
            WW[at] = Wn;
            DB[at] = (uint8_t)((DB[at] & 1u) | (uint32_t)d << 1);
        }
    }
    return res;
}

template <int WAVES, class CODE>
__global__ __launch_bounds__(64 * WAVES) void tpc_kernel(const tpc_args A, const CODE code, const float *__restrict__ llr,
                                                         const int8_t *__restrict__ bits, const float *__restrict__ scale,
                                                         int32_t *__restrict__ out, float *__restrict__ llr_out, int8_t *__restrict__ bits_out,
                                                         float *__restrict__ ext, int32_t *__restrict__ half_err)
{
    constexpr int NT = 64 * WAVES;
    extern __shared__ __align__(16) unsigned char tpc_lds[];
    __shared__ int CNT[8];                                     // pre_err, erased, pay_err, nstat2, nbeta, the weight of d (two slots)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n1 = A.n1, n2 = A.n2, ns = n2 | 1, cells = n1 * ns, n = n1 * n2, nmax = max(n1, n2), p = A.p;
    float *RR = reinterpret_cast<float *>(tpc_lds), *WW = RR + cells;
    uint32_t *MC = reinterpret_cast<uint32_t *>(WW + cells) + wave * nmax;     // this wave's competitor array
    uint8_t *DB = reinterpret_cast<uint8_t *>(WW + cells) + 4 * (size_t)WAVES * nmax;
    typename CODE::word w1, w2;                                // the column code and the row code
    code.tables(A, DB + (cells + 3) / 4 * 4, tid, NT, w1, w2);

    for (long long g = blockIdx.x; g < A.blocks; g += gridDim.x) {
        const size_t run = (size_t)(g / A.C);
        const int c = (int)(g - (long long)run * A.C);
        if (tid < 8) CNT[tid] = 0;
        __syncthreads();                                       // the tables, the counters; the last block's readers are through
        int pre = 0, erased = 0;
        ldpc_gather(ldpc_window_of<false>(c, A.C, A.w, A.t0, 0, n), run, A.N, A.w, n, tid, NT, llr, bits, [&](long long j, float x, uint32_t b) {
            x = x != x ? 0.0f : x;                             // a NaN is +0
            pre += (int)((uint32_t)(x < 0.0f) ^ b);
            erased += x == 0.0f;
            const int a = (int)j / n2, at = a * ns + ((int)j - a * n2);
            RR[at] = fminf(fmaxf(b ? -x : x, -A.clip), A.clip);
            WW[at] = 0.0f;
            DB[at] = (uint8_t)b;
        });
        pre = (int)fec_wave_add((uint32_t)pre);
        erased = (int)fec_wave_add((uint32_t)erased);
        if (lane == 0) {
            atomicAdd(&CNT[0], pre);
            atomicAdd(&CNT[1], erased);
        }
        float bs = scale ? scale[run] : 1.0f;
        __syncthreads();

        int executed = 0, ok = 0, weight = 0;
#pragma unroll 1
        for (int h = 0; h < TPC_HALF; h++) {
            if (h >= 2 * A.iters) break;                       // uniform
            const bool colwise = h & 1;
            const int words = colwise ? n2 : n1, len = colwise ? n1 : n2, others = colwise ? n1 : n2, olen = colwise ? n2 : n1;
            const typename CODE::word cw = CODE::word::pick(colwise, w1, w2), ow = CODE::word::pick(colwise, w2, w1);
            const float prod = A.beta[h] * bs, beta = prod > 0.0f ? fminf(prod, A.clip) : 0.0f;   // a NaN product is +0
            int stat2 = 0, nbeta = 0, wsum = 0;
            for (int wd = wave; wd < words; wd += WAVES) {     // one wave, one word
                const tpc_word_result res = tpc_word(lane, len, p, colwise ? wd : wd * ns, colwise ? ns : 1, A.alpha[h], beta, A.clip, cw, RR,
                                                     WW, DB, MC);
                stat2 += res.status == 2;
                nbeta += res.nbeta;
                wsum += res.weight;
            }
            int *WT = &CNT[5 + (h & 1)];                       // two slots in turn: the one of h - 1 may still be being read
            if (tid == 0) *WT = 0;
            __syncthreads();
            if (lane == 0) {
                atomicAdd(&CNT[3], stat2);
                atomicAdd(&CNT[4], nbeta);
                atomicAdd(WT, wsum);
            }
            int bad = stat2;                                   // the other direction's syndromes on d
            for (int wd = wave; wd < others; wd += WAVES) {
                const int base = colwise ? wd * ns : wd, stride = colwise ? 1 : ns;
                uint32_t syn = 0;
#pragma unroll
                for (int k = 0; k < CHASE_SLOTS; k++) {
                    if (64 * k >= olen) break;
                    const int j = 64 * k + lane;
                    const bool in = j < olen;
                    const int jj = in ? j : 0;
                    const uint32_t d = in ? (uint32_t)DB[base + jj * stride] >> 1 : 0u;
                    syn ^= d ? ow.col(jj) : 0u;
                }
                bad |= ow.bad(fec_wave_xor(syn));
            }
            const int go_on = __syncthreads_or(bad);
            weight = *WT;
            executed = h + 1;
            if (half_err && tid == 0) half_err[(size_t)g * (size_t)(2 * A.iters) + h] = weight;
            if (!go_on) {
                ok = 1;
                break;
            }
        }
        if (half_err) {
            for (int h = executed + tid; h < 2 * A.iters; h += NT) half_err[(size_t)g * (size_t)(2 * A.iters) + h] = -1;
        }

        int pay = 0;
        const size_t sbase = (run * (size_t)A.C + (size_t)c) * (size_t)n;
        for (int j = tid; j < n; j += NT) {                    // consecutive lanes, consecutive entries
            const int a = j / n2, b = j - a * n2, at = a * ns + b;
            const uint32_t db = DB[at];
            pay += (db >> 1) && a < A.K1 && b < A.K2;
            if (llr_out) {
                llr_out[sbase + j] = ((db >> 1) ^ (db & 1u)) ? -1.0f : 1.0f;
                bits_out[sbase + j] = (int8_t)(db & 1u);
            }
            if (ext) ext[sbase + j] = WW[at];
        }
        pay = (int)fec_wave_add((uint32_t)pay);
        if (lane == 0) atomicAdd(&CNT[2], pay);
        __syncthreads();
        if (tid < 8) {
            const int val = tid == 0 ? executed : tid == 1 ? ok : tid == 2 ? weight : tid == 3 ? CNT[0] : tid == 4 ? CNT[1] : tid == 5 ? CNT[2]
                          : tid == 6 ? CNT[3] : CNT[4];
            out[(size_t)g * 8 + tid] = val;
        }
        __syncthreads();                                       // the state and the counters are the next block's
    }
}

// The rules both entry points share behind the frame's and the codes' own: p, iters, clip, the payload, the schedules, the fit and the counts;
// VAEQ_OK fills the kernel's arguments (r1, r2: the columns' width of a single-error-correcting code, m of a BCH one).
static inline int tpc_frame(int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0, int32_t n1, int32_t r1, int32_t n2, int32_t r2, int32_t p,
                            int32_t iters, const float *alpha_host, const float *beta_host, float clip, int32_t K1, int32_t K2, bool want_stream,
                            tpc_args *out)
{
    if (p < 0 || p > CHASE_P || p > n1 || p > n2 || iters < 1 || iters > TPC_ITERS || !(clip > 0.0f) || !(clip <= 0x1p96f) || K1 < 1 || K1 > n1 ||
        K2 < 1 || K2 > n2)
        return VAEQ_ERR_SHAPE;
    tpc_args A = {(long long)N, (long long)t0, (long long)R * C, (int)C, (int)w, (int)n1, (int)r1, (int)n2, (int)r2, (int)p, (int)iters, (int)K1,
                  (int)K2, clip, {}, {}};
    for (int h = 0; h < 2 * iters; h++) {                      // finite, alpha in [0, 16], beta >= 0 (a NaN fails every comparison)
        A.alpha[h] = alpha_host[h];
        A.beta[h] = beta_host[h];
        if (!(A.alpha[h] >= 0.0f && A.alpha[h] <= 16.0f) || !(A.beta[h] >= 0.0f && A.beta[h] <= 3.402823466e38f)) return VAEQ_ERR_SHAPE;
    }
    const int64_t n = (int64_t)n1 * n2;                        // at most 2^16: C n stays below 2^47
    if (!fec_fit_ok(false, C, n, w, t0, N) || (int64_t)R * C > 0x7fffffff || (want_stream && (int64_t)C * n > 0x3fffffff)) return VAEQ_ERR_SHAPE;
    *out = A;
    return VAEQ_OK;
}

template <class CODE>
static inline int tpc_launch(const tpc_args &A, const CODE &code, int64_t lds, const float *llr, const int8_t *bits, const float *scale, int32_t *out,
                             float *llr_out, int8_t *bits_out, float *ext, int32_t *half_err, void *stream)
{
    const dim3 grid((unsigned)(A.blocks < TPC_GRID ? A.blocks : TPC_GRID));
    const bool big = tpc_waves(A.n1, A.n2) == TPC_WAVES_BIG;
    return launch(big ? tpc_kernel<TPC_WAVES_BIG, CODE> : tpc_kernel<TPC_WAVES_SMALL, CODE>, grid,
                  dim3(64 * (big ? TPC_WAVES_BIG : TPC_WAVES_SMALL)), (size_t)lds, reinterpret_cast<hipStream_t>(stream), A, code, llr, bits, scale,
                  out, llr_out, bits_out, ext, half_err);
}

}  // namespace vaeq

extern "C" int64_t vaeq_tpc_lds_bytes(int32_t n1, int32_t r1, int32_t n2, int32_t r2)
{
    using namespace vaeq;
    if (!tpc_dims_ok(n1, r1, n2, r2)) return (int64_t)VAEQ_ERR_SHAPE;
    const int64_t bytes = tpc_state_bytes(n1, r1, n2, r2);
    return bytes <= TPC_LDS_MAX ? bytes : (int64_t)VAEQ_ERR_LDS;
}

extern "C" int vaeq_tpc_decode(int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0, int32_t n1, int32_t r1, const int32_t *cols1_host, int32_t n2,
                               int32_t r2, const int32_t *cols2_host, const float *llr, const int8_t *bits, int32_t p, int32_t iters,
                               const float *alpha_host, const float *beta_host, const float *scale, float clip, int32_t K1, int32_t K2,
                               int32_t *out, float *llr_out, int8_t *bits_out, float *ext, int32_t *half_err, void *stream)
{
    using namespace vaeq;
    if (R == 0) return VAEQ_OK;                                // an empty batch owns no memory: its pointers may be NULL
    if (!cols1_host || !cols2_host || !llr || !bits || !alpha_host || !beta_host || !out || !llr_out != !bits_out) return VAEQ_ERR_NULL;
    if (!fec_frame_ok(R, C, N, w, t0) || !tpc_dims_ok(n1, r1, n2, r2)) return VAEQ_ERR_SHAPE;
    tpc_args A;
    const int rc = tpc_frame(R, C, N, w, t0, n1, r1, n2, r2, p, iters, alpha_host, beta_host, clip, K1, K2, llr_out != nullptr, &A);
    if (rc != VAEQ_OK) return rc;
    const int64_t lds = tpc_state_bytes(n1, r1, n2, r2);
    if (lds > TPC_LDS_MAX) return VAEQ_ERR_LDS;
    tpc_ham code;
    if (!fec_cols_pack(cols1_host, n1, r1, &code.tab1) || !fec_cols_pack(cols2_host, n2, r2, &code.tab2)) return VAEQ_ERR_SHAPE;
    return tpc_launch(A, code, lds, llr, bits, scale, out, llr_out, bits_out, ext, half_err, stream);
}

extern "C" int64_t vaeq_tpc_bch_lds_bytes(int32_t m1, int32_t n1, int32_t ext1, int32_t m2, int32_t n2, int32_t ext2)
{
    using namespace vaeq;
    if (!ebch_ok(m1, n1, ext1) || !ebch_ok(m2, n2, ext2)) return (int64_t)VAEQ_ERR_SHAPE;
    const int64_t bytes = tpc_bch_state_bytes(m1, n1, m2, n2);
    return bytes <= TPC_LDS_MAX ? bytes : (int64_t)VAEQ_ERR_LDS;
}

extern "C" int vaeq_tpc_bch_decode(int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0, int32_t m1, int32_t n1, int32_t ext1, int32_t m2, int32_t n2,
                                   int32_t ext2, const float *llr, const int8_t *bits, int32_t p, int32_t iters, const float *alpha_host,
                                   const float *beta_host, const float *scale, float clip, int32_t K1, int32_t K2, int32_t *out, float *llr_out,
                                   int8_t *bits_out, float *ext, int32_t *half_err, void *stream)
{
    using namespace vaeq;
    if (R == 0) return VAEQ_OK;                                // an empty batch owns no memory: its pointers may be NULL
    if (!llr || !bits || !alpha_host || !beta_host || !out || !llr_out != !bits_out) return VAEQ_ERR_NULL;
    if (!fec_frame_ok(R, C, N, w, t0) || !ebch_ok(m1, n1, ext1) || !ebch_ok(m2, n2, ext2)) return VAEQ_ERR_SHAPE;
    tpc_args A;
    const int rc = tpc_frame(R, C, N, w, t0, n1, m1, n2, m2, p, iters, alpha_host, beta_host, clip, K1, K2, llr_out != nullptr, &A);
    if (rc != VAEQ_OK) return rc;
    const int64_t lds = tpc_bch_state_bytes(m1, n1, m2, n2);
    if (lds > TPC_LDS_MAX) return VAEQ_ERR_LDS;
    const tpc_bch code = {ebch_make(m1, n1, ext1), ebch_make(m2, n2, ext2)};
    return tpc_launch(A, code, lds, llr, bits, scale, out, llr_out, bits_out, ext, half_err, stream);
}
