// vaeq_chase.hip -- the soft-in / hard-out inner decoder of include/vaeq.h (vaeq_chase_decode): Chase decoding of a single-error-correcting
// code given by the columns of its parity-check matrix, over the demappers' LLRs under the LDPC decoders' bit maps, against the TX bits.  The rule
// acts on e = received xor transmitted, so there is no encoder; integers and float32 additions in a fixed order, so a numpy model gives the same bits.
//
// The mapping: workgroups of four waves; the columns and the syndrome -> position table (2^r uint16) built once per workgroup in LDS from the
// by-value columns; then a workgroup takes tiles of up to 32 consecutive codewords of a run (at most 2048 bits), grid-stride over the tiles.
// All 256 threads gather the tile through ldpc_gather, one (codeword, symbol) each -- lanes on consecutive symbols of a plane in the bit-packed
// map, on consecutive codewords (which are consecutive symbols) behind the interleaver -- and file |x| (with the error bit on top) and the TX bit
// of every position in LDS.  One wave then decodes one codeword: lane l holds the positions l, l + 64, l + 128, l + 192.  The p least reliable
// positions come from p wave-wide minima of the key |x| bits << 16 | j, after which their (position, column, |x|) are wave-uniform; lane T
// evaluates test pattern T -- one table lookup and at most seven predicated additions -- and one more minimum over metric bits << 8 | T picks
// the winner.  That span is the text of vaeq_fec.h's chase_front, which vaeq_tpc.hip calls; it stands here in place because this kernel measured
// 4 to 8 % slower through the call: a fix to one goes to the other.  Counters are ballots and popcounts.
// vaeq_chase_bch_decode is the same kernel with CODE = ebch_code: the exp, log and half-solve tables of GF(2^m) in the place of the columns and
// positions, and that span replaced by a call of vaeq_fec.h's ebch_front; the gather, the tiles, the counters and the stream are written once.
// The payload stream leaves through a transposed byte tile in LDS (rows of 33 bytes: no bank
// conflict on either side), so that under either spread a wave's stores are runs of consecutive stream entries.  Everything leaves as plain
// vector stores.  Every loop has a static bound.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vaeq.h"
#include "vaeq_fec.h"
#include "vaeq_launch.h"
#include "vaeq_ldpc.h"

namespace vaeq {

constexpr int CHASE_WAVES = 4, CHASE_NT = 64 * CHASE_WAVES;
constexpr int CHASE_TILE = 2048, CHASE_TW = 32, CHASE_ROW = 33;   // a tile: bits, codewords; a row of the stream tile in bytes (TW padded by one)
constexpr int64_t CHASE_GRID = 2048;
static_assert(CHASE_NT == CHASE_N, "thread j of a workgroup files column j");

struct chase_args {
    long long N, t0, tiles;                                    // tiles = R tiles_run
    int C, w, depth, n, r, p, K, spread, tw, tiles_run;        // tw: the codewords of a full tile, tiles_run = ceil(C / tw)
};

// the codewords of a full tile and the dynamic LDS of a workgroup: |x| with the error bit (uint32) and the TX bit (uint8) of every position of a
// tile, each with CHASE_N entries of slack behind (a wave's four slots reach that far past the start of its codeword), and the stream tile
static inline int chase_tile_words(int n) { return CHASE_TILE / n < CHASE_TW ? CHASE_TILE / n : CHASE_TW; }
static inline size_t chase_lds_bytes(int n, int K, bool want_stream)
{
    const size_t pos = (size_t)chase_tile_words(n) * (n | 1) + CHASE_N;   // a codeword every n | 1 entries: an odd stride, the codewords on different banks
    return 4 * pos + (want_stream ? ((size_t)K * CHASE_ROW + 3) / 4 * 4 : 0) + pos;
}

// CODE: fec_cols, a single-error-correcting code by its columns, or ebch_code, an (extended) t = 2 BCH code by its field (vaeq_chase_bch_decode).
// The two share everything but the tables and the span from the list to the flips.
template <bool IL, class CODE>
__global__ __launch_bounds__(CHASE_NT) void chase_kernel(const chase_args A, const CODE tab, const float *__restrict__ llr,
                                                         const int8_t *__restrict__ bits, int32_t *__restrict__ out,
                                                         float *__restrict__ llr_out, int8_t *__restrict__ bits_out)
{
    extern __shared__ __align__(16) unsigned char chase_lds[];
    constexpr bool BCH = std::is_same<CODE, ebch_code>::value;
    __shared__ uint16_t COL[CHASE_N], POS[1 << CHASE_R];       // (not referenced, and so not allocated, where BCH)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = A.n, p = A.p, K = A.K, C = A.C, w = A.w;
    const int ns = n | 1, npos = A.tw * ns + CHASE_N;
    uint32_t *TA = reinterpret_cast<uint32_t *>(chase_lds);    // the bits of |x|, the error bit in bit 31
    uint8_t *ST = chase_lds + 4 * (size_t)npos;                // the stream tile: row i, CHASE_ROW bytes, holds TX bit | decided bit << 1 of payload bit i
    uint8_t *TT = ST + (llr_out ? ((size_t)K * CHASE_ROW + 3) / 4 * 4 : 0);

    ebch_tables tb = {};
    if constexpr (BCH) {
        __shared__ uint16_t TABLES[3 << EBCH_M_MAX];           // exp, log and half-solve of GF(2^m)
        ebch_build(TABLES, tab.m, tab.poly, tid, CHASE_NT);
        tb = ebch_view(TABLES, tab);
    } else {
        for (int s = tid; s < (1 << CHASE_R); s += CHASE_NT) POS[s] = (uint16_t)CHASE_NONE;
        __syncthreads();
        {   // CHASE_NT == CHASE_N: thread j owns column j; the columns are distinct, so no two threads write one entry
            const uint32_t c = tid < n ? tab.col[tid] : 0u;
            COL[tid] = (uint16_t)c;
            if (tid < n) POS[c] = (uint16_t)tid;
        }
    }
    __syncthreads();

    const int SM = IL ? (n + w - 1) / w : (n + w - 2) / w + 1;  // the most symbols a codeword touches
    for (long long tile = blockIdx.x; tile < A.tiles; tile += gridDim.x) {
        const size_t run = (size_t)(tile / A.tiles_run);
        const int cw0 = (int)(tile - (long long)run * A.tiles_run) * A.tw, TW = min(A.tw, C - cw0);
        for (int item = tid; item < TW * SM; item += CHASE_NT) {   // one (codeword, symbol) per thread: ldpc_gather's loop runs once, for s
            int wd, sy;
            if constexpr (IL) { sy = item / TW; wd = item - sy * TW; }
            else { wd = item / SM; sy = item - wd * SM; }
            const int base = wd * ns;
            ldpc_gather(ldpc_window_of<IL>(cw0 + wd, C, w, A.t0, A.depth, n), run, A.N, w, n, sy, SM, llr, bits, [&](long long j, float x, uint32_t b) {
                x = x != x ? 0.0f : x;                         // a NaN is +0
                const uint32_t e = (uint32_t)(x < 0) ^ b;
                TA[base + (int)j] = (__float_as_uint(x) & 0x7fffffffu) | e << 31;
                TT[base + (int)j] = (uint8_t)b;
            });
        }
        __syncthreads();
        for (int wd = wave; wd < TW; wd += CHASE_WAVES) {      // one wave, one codeword
            const int base = wd * ns;
            const size_t g = run * (size_t)C + (size_t)(cw0 + wd);

            uint32_t key[CHASE_SLOTS];                             // the bits of |x| of the positions not yet taken, all ones otherwise
            uint32_t err = 0, txb = 0, s0 = 0;                     // bit k: slot k of this lane
            int pre = 0, erased = 0;
#pragma unroll
            for (int k = 0; k < CHASE_SLOTS; k++) key[k] = ~0u;
#pragma unroll
            for (int k = 0; k < CHASE_SLOTS; k++) {
                if (64 * k >= n) break;                            // wave-uniform: a slot no position falls into
                const int j = 64 * k + lane;
                const bool in = j < n;
                const uint32_t word = TA[base + j], a = word & 0x7fffffffu, e = in ? word >> 31 : 0u;
                key[k] = in ? a : ~0u;
                err |= e << k;
                txb |= (in ? (uint32_t)TT[base + j] : 0u) << k;
                if constexpr (BCH) s0 ^= e ? ebch_col(tb, (uint32_t)(in ? j : 0)) : 0u;
                else s0 ^= e ? (uint32_t)COL[j] : 0u;
                pre += __popcll(__ballot(e != 0));
                erased += __popcll(__ballot(in && a == 0));
            }
            s0 = fec_wave_xor(s0);

            int status = 2, nflip = 0;
            uint32_t flip = 0;                                     // bit k: slot k of this lane is flipped
            if constexpr (BCH) {
                const ebch_pick c = ebch_front(key, s0, n, p, lane, tb, [&](uint32_t v) {
                    return __uint_as_float(TA[base + (int)min(v, (uint32_t)n - 1u)] & 0x7fffffffu);
                });
                flip = c.flip;
                nflip = c.nflip;
                status = c.best == ~0u ? 2 : nflip ? 1 : 0;
            } else {
                // the p least reliable positions: wave-uniform position, column and |x|
                uint32_t lp[CHASE_P], lc[CHASE_P];
                float la[CHASE_P];
#pragma unroll
                for (int i = 0; i < CHASE_P; i++) {
                    lp[i] = CHASE_NONE;
                    lc[i] = 0;
                    la[i] = 0.0f;
                    if (i < p) {                                       // wave-uniform; p <= n: a position is left
                        uint32_t m = key[0];                               // by (|x|, j): the smallest |x| (its bits order as it does: it is never
#pragma unroll
                        for (int k = 1; k < CHASE_SLOTS; k++) m = min(m, key[k]);   // negative), then the smallest position that has it
                        m = fec_wave_min(m);
                        uint32_t at = CHASE_NONE;
#pragma unroll
                        for (int k = CHASE_SLOTS - 1; k >= 0; k--) at = key[k] == m ? (uint32_t)(64 * k + lane) : at;
                        lp[i] = fec_wave_min(at);
                        la[i] = __uint_as_float(m);
                        lc[i] = COL[lp[i]];
#pragma unroll
                        for (int k = 0; k < CHASE_SLOTS; k++) key[k] = (uint32_t)(64 * k + lane) == lp[i] ? ~0u : key[k];
                    }
                }

                // lane T: test pattern T
                const uint32_t T = (uint32_t)lane;
                uint32_t s = s0;
#pragma unroll
                for (int i = 0; i < CHASE_P; i++) s ^= (T >> i) & 1u ? lc[i] : 0u;
                const uint32_t v = s ? (uint32_t)POS[s] : CHASE_NONE;  // s < 2^r: a xor of columns
                const bool cand = T < (1u << p) && (s == 0 || v != CHASE_NONE);
                float metric = 0.0f;
                bool cancelled = false;
#pragma unroll
                for (int i = 0; i < CHASE_P; i++) {                    // x + (+0) = x for x >= 0: the predicated add is the specified sum
                    const bool in = (T >> i) & 1u, hit = in && lp[i] == v;
                    metric += in && !hit ? la[i] : 0.0f;
                    cancelled |= hit;
                }
                const uint32_t av = TA[base + (int)min(v, (uint32_t)CHASE_N - 1u)] & 0x7fffffffu;
                metric += v != CHASE_NONE && !cancelled ? __uint_as_float(av) : 0.0f;
                const uint32_t mine = cand ? __float_as_uint(metric) : ~0u, best = fec_wave_min(mine);   // by (metric, T)

                if (best != ~0u) {                                     // wave-uniform
                    const uint32_t Tw = fec_wave_min(mine == best ? T : CHASE_NONE), vw = (uint32_t)__builtin_amdgcn_readlane((int)v, (int)Tw);
#pragma unroll
                    for (int k = 0; k < CHASE_SLOTS; k++) {
                        if (64 * k >= n) break;
                        const uint32_t j = (uint32_t)(64 * k + lane);
                        uint32_t f = vw == j;                          // the symmetric difference of F_T and {v}
#pragma unroll
                        for (int i = 0; i < CHASE_P; i++) f ^= (uint32_t)(((Tw >> i) & 1u) && lp[i] == j);
                        flip |= f << k;
                        nflip += __popcll(__ballot(f != 0));
                    }
                    status = nflip ? 1 : 0;
                }
            }
            err ^= flip;
            int post = 0, pay_post = 0;
#pragma unroll
            for (int k = 0; k < CHASE_SLOTS; k++) {
                if (64 * k >= n) break;
                const int j = 64 * k + lane;
                const bool e = (err >> k) & 1u;
                post += __popcll(__ballot(e));
                pay_post += __popcll(__ballot(e && j < K));
                if (llr_out && j < K) ST[j * CHASE_ROW + wd] = (uint8_t)(((txb >> k) & 1u) | (((txb >> k) & 1u) ^ (uint32_t)e) << 1);
            }
            if (lane < 6) {
                const int val = lane == 0 ? status : lane == 1 ? pre : lane == 2 ? post : lane == 3 ? nflip : lane == 4 ? erased : pay_post;
                out[(size_t)g * 6 + lane] = val;
            }
        }
        if (llr_out) {                                         // (uniform: a kernel argument)
            __syncthreads();
            const size_t sbase = run * (size_t)C * (size_t)K;
            for (int item = tid; item < TW * K; item += CHASE_NT) {   // consecutive lanes, consecutive stream entries: along the codewords under
                int wd, i;                                            // the spread, along the payload bits without
                if (A.spread) { i = item / TW; wd = item - i * TW; }
                else { wd = item / K; i = item - wd * K; }
                const size_t u = sbase + (A.spread ? (size_t)i * (size_t)C + (size_t)(cw0 + wd) : (size_t)(cw0 + wd) * (size_t)K + (size_t)i);
                const uint32_t d = ST[i * CHASE_ROW + wd];
                llr_out[u] = d & 2u ? -1.0f : 1.0f;
                bits_out[u] = (int8_t)(d & 1u);
            }
        }
        __syncthreads();                                       // the tiles are the next iteration's
    }
}

// The rules both entry points share behind the code's own: the frame, depth, p, K, spread, that depth's fit rule and the counts.
static inline bool chase_rules_ok(int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0, int32_t depth, int32_t n, int32_t p, int32_t K, int32_t spread,
                                  bool want_stream)
{
    return fec_frame_ok(R, C, N, w, t0) && depth >= 0 && depth <= C && p >= 0 && p <= CHASE_P && p <= n && K >= 1 && K <= n && spread >= 0 &&
           spread <= 1 && fec_fit_ok(depth >= 1, C, n, w, t0, N) && (int64_t)R * C <= 0x7fffffff && !(want_stream && (int64_t)C * K > 0x3fffffff);
}

// r: the columns' width of a single-error-correcting code, m of a BCH one
template <class CODE>
static inline int chase_launch(const CODE &code, int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0, int32_t depth, int32_t n, int32_t r, int32_t p,
                               int32_t K, int32_t spread, const float *llr, const int8_t *bits, int32_t *out, float *llr_out, int8_t *bits_out,
                               void *stream)
{
    const int tw = chase_tile_words(n), tiles_run = (C + tw - 1) / tw;
    const chase_args A = {(long long)N, (long long)t0, (long long)R * tiles_run, (int)C, (int)w, (int)depth, (int)n, (int)r, (int)p, (int)K, (int)spread,
                          tw, tiles_run};
    const dim3 grid((unsigned)(A.tiles < CHASE_GRID ? A.tiles : CHASE_GRID)), block(CHASE_NT);
    return launch(depth >= 1 ? chase_kernel<true, CODE> : chase_kernel<false, CODE>, grid, block, chase_lds_bytes(n, K, llr_out != nullptr),
                  reinterpret_cast<hipStream_t>(stream), A, code, llr, bits, out, llr_out, bits_out);
}

}  // namespace vaeq

extern "C" int vaeq_chase_decode(int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0, int32_t depth, int32_t n, int32_t r,
                                 const int32_t *cols_host, const float *llr, const int8_t *bits, int32_t p, int32_t K, int32_t spread,
                                 int32_t *out, float *llr_out, int8_t *bits_out, void *stream)
{
    using namespace vaeq;
    if (R == 0) return VAEQ_OK;                                // an empty batch owns no memory: its pointers may be NULL
    if (!cols_host || !llr || !bits || !out || !llr_out != !bits_out) return VAEQ_ERR_NULL;
    if (n < 3 || n > CHASE_N || r < 2 || r > CHASE_R || !chase_rules_ok(R, C, N, w, t0, depth, n, p, K, spread, llr_out != nullptr))
        return VAEQ_ERR_SHAPE;
    fec_cols tab;
    if (!fec_cols_pack(cols_host, n, r, &tab)) return VAEQ_ERR_SHAPE;
    return chase_launch(tab, R, C, N, w, t0, depth, n, r, p, K, spread, llr, bits, out, llr_out, bits_out, stream);
}

extern "C" int vaeq_chase_bch_decode(int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0, int32_t depth, int32_t m, int32_t n, int32_t ext,
                                     const float *llr, const int8_t *bits, int32_t p, int32_t K, int32_t spread, int32_t *out, float *llr_out,
                                     int8_t *bits_out, void *stream)
{
    using namespace vaeq;
    if (R == 0) return VAEQ_OK;                                // an empty batch owns no memory: its pointers may be NULL
    if (!llr || !bits || !out || !llr_out != !bits_out) return VAEQ_ERR_NULL;
    if (!ebch_ok(m, n, ext) || !chase_rules_ok(R, C, N, w, t0, depth, n, p, K, spread, llr_out != nullptr)) return VAEQ_ERR_SHAPE;
    return chase_launch(ebch_make(m, n, ext), R, C, N, w, t0, depth, n, m, p, K, spread, llr, bits, out, llr_out, bits_out, stream);
}
