// vaeq_bch.hip -- the outer hard-decision decoder of include/vaeq.h (vaeq_bch_outer): a bounded-distance decoder of a shortened narrow-sense
// binary BCH code over the payload bits of the LDPC decoders' `post`, against the TX bits under the decoders' own map.  Integer throughout; the
// result is a function of the error pattern alone, so there is no encoder (the TX bits need not be a codeword) and a numpy model gives the same
// bits.
//
// The mapping: workgroups of four waves; the exp / log tables of GF(2^m) built once per workgroup in LDS (2 x 2^m uint16), each thread raising
// alpha to the start of its chunk and stepping by alpha; then one wave per outer codeword, the waves of a workgroup on neighbouring codewords of a
// run, so that under the bit interleaver (positions C_o stream bits apart) the lines one wave touches are the lines its neighbours need.  The
// lanes walk the positions with clamped addresses -- no branch around a load, four iterations' loads in flight -- file each iteration's error
// ballot in LDS (the Chien search counts its flips against it) and accumulate the t odd syndromes of their error positions in registers;
// S_2j = S_j^2.  A clean codeword leaves behind the ballots; one with errors reduces the syndromes with an XOR butterfly, runs Berlekamp-Massey
// with one coefficient per lane and the discrepancy as a wave reduction, and the Chien search with the lanes over all 2^m - 1 positions, the
// shortened ones included: the rule wants L roots, none of them shortened.  Every loop has a static bound (2 t <= 32, 2^m - 1 <= 8191 positions).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vaeq.h"
#include "vaeq_fec.h"
#include "vaeq_launch.h"
#include "vaeq_ldpc.h"

namespace vaeq {

#ifndef VAEQ_BCH_WAVES
#define VAEQ_BCH_WAVES 4                                       // waves per workgroup: 8 and 16 measured, DESIGN.md
#endif
constexpr int BCH_M_MIN = GF_M_MIN, BCH_M_MAX = GF_M_MAX, BCH_T = 16, BCH_WAVES = VAEQ_BCH_WAVES, BCH_NT = 64 * BCH_WAVES, BCH_IT = (1 << BCH_M_MAX) / 64;
constexpr int64_t BCH_GRID = 8192 / BCH_WAVES;

struct bch_args {
    long long N, t0, total;                                    // total = R C_o outer codewords
    int C, w, depth, n, K, m, t, n_o, C_o, spread, post_i16;
    uint32_t poly;
};

struct bch_scratch {                                           // of one wave
    unsigned long long err[BCH_IT];                            // the error ballot of positions 64 it .. 64 it + 63
    uint16_t S[2 * BCH_T + 2];                                 // S[j], j = 1 .. 2t
    uint16_t lam[BCH_T + 2];                                   // log Lambda_k, 0xffff for a zero coefficient
    int16_t loc[BCH_T];
};

// what one lane wrote to its wave's scratch, visible to the others: the wave runs in lockstep, this keeps the compiler from reordering
__device__ __forceinline__ void bch_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t bch_wave_xor(uint32_t x)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x ^= (uint32_t)__shfl_xor((int)x, o);
    return x;
}

// I: the type of a stream bit index and of an offset inside a run's tensors, uint32_t where C n < 2^31 and w N < 2^32
template <bool IL, class I>
__global__ __launch_bounds__(BCH_NT) void bch_outer_kernel(const bch_args A, const void *__restrict__ post, const int8_t *__restrict__ bits,
                                                           int32_t *__restrict__ out, int16_t *__restrict__ loc)
{
    extern __shared__ __align__(16) unsigned char bch_lds[];
    __shared__ bch_scratch scratch[BCH_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = A.m, t = min(A.t, BCH_T), n_o = A.n_o, C_o = A.C_o;
    const uint32_t q = (1u << m) - 1u;
    uint16_t *EXP = reinterpret_cast<uint16_t *>(bch_lds), *LOG = EXP + (1u << m);

    {   // the tables: thread tid owns the exponents tid ch .. tid ch + ch - 1
        const uint32_t ch = (q + BCH_NT - 1) / BCH_NT, lo = (uint32_t)tid * ch;
        uint32_t x = 1, base = 2;                              // x = alpha^lo by squaring; a product is m shift-and-add steps
        for (int b = 0; b <= BCH_M_MAX; b++) {
            uint32_t y = 0, z = 0;                             // y = x base, z = base^2
            for (int k = BCH_M_MAX - 1; k >= 0; k--) {
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
    __syncthreads();

    auto mul = [&](uint32_t a, uint32_t b) { return gf_mul(EXP, LOG, q, a, b); };

    bch_scratch &sc = scratch[wave];
    const int nit = (n_o + 63) >> 6;
    const long long stride = (long long)gridDim.x * BCH_WAVES;
    for (long long a = (long long)blockIdx.x * BCH_WAVES + wave; a < A.total; a += stride) {
        const size_t run = (size_t)(a / C_o);
        const uint32_t ao = (uint32_t)(a - (long long)run * C_o);
        const size_t post_run = run * (size_t)A.C * (size_t)A.n, bits_run = run * (size_t)A.w * (size_t)A.N;
        uint32_t syn[BCH_T];
#pragma unroll
        for (int k = 0; k < BCH_T; k++) syn[k] = 0;
        int pre = 0;
        auto walk = [&](auto *__restrict__ rxp) {                // float or int16: negative is bit 1; a NaN and +-0 are bit 0
            const auto *__restrict__ rxr = rxp + post_run;     // the run's tensors: the offsets inside them are of type I
            const int8_t *__restrict__ txr = bits + bits_run;
            for (int it0 = 0; it0 < nit; it0 += 4) {           // four iterations' loads in flight; nit <= 128, a multiple of 4 where it is 128
                decltype(*rxp + 0) x[4];
                int b[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int pc = min((it0 + k) * 64 + lane, n_o - 1);   // a clamped address: no branch around the loads
                    const I u = A.spread ? (I)pc * (I)C_o + (I)ao : (I)ao * (I)n_o + (I)pc;
                    const I c = u / (I)A.K;
                    const uint32_t i = (uint32_t)(u - c * (I)A.K);
                    x[k] = rxr[c * (I)A.n + (I)i];
                    b[k] = txr[ldpc_bit_at<IL, I>(c, i, A.C, A.w, A.N, A.t0, A.depth, A.n)];
                }
#pragma unroll
                for (int k = 0; k < 4; k++) { ldpc_pin(x[k]); ldpc_pin(b[k]); }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int it = it0 + k, p = it * 64 + lane;
                    const bool e = p < n_o && (x[k] < 0) != (bool)(b[k] & 1);
                    const unsigned long long mask = __ballot(e);
                    if (lane == 0) sc.err[it] = mask;
                    pre += __popcll(mask);
                    if (e) {                                   // S_j += alpha^(j p) for the odd j: the exponent advances by 2 p
                        uint32_t y = (uint32_t)p, d = 2u * (uint32_t)p;   // p < n_o <= q
                        d = d >= q ? d - q : d;
#pragma unroll
                        for (int j = 0; j < BCH_T; j++)
                            if (j < t) {
                                syn[j] ^= EXP[y];
                                y += d;
                                y = y >= q ? y - q : y;
                            }
                    }
                }
            }
        };
        if (A.post_i16) walk(static_cast<const int16_t *>(post));
        else walk(static_cast<const float *>(post));
        int status = 0, post_err = pre, nflip = 0;
        uint32_t any = 0;
        if (pre) {
#pragma unroll
            for (int k = 0; k < BCH_T; k++)
                if (k < t) {
                    syn[k] = bch_wave_xor(syn[k]);
                    any |= syn[k];
                }
        }
        if (any) {                                             // wave-uniform from here on
            status = 2;
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < BCH_T; k++)
                    if (k < t) sc.S[2 * k + 1] = (uint16_t)syn[k];
            }
            bch_wave_sync();
            if (lane >= 2 && lane <= 2 * t && !(lane & 1)) {   // S_j = S_o^(2^s) for j = o 2^s, o odd
                const int s = __ffs(lane) - 1;
                const uint32_t x = sc.S[lane >> s];
                uint32_t lg = LOG[x];
                for (int k = 0; k < 5; k++)
                    if (k < s) {
                        lg += lg;
                        lg = lg >= q ? lg - q : lg;
                    }
                sc.S[lane] = x ? EXP[lg] : (uint16_t)0;
            }
            bch_wave_sync();

            // Berlekamp-Massey, Lambda_k and B_k in lane k: B <- x B every step; on a discrepancy d, Lambda <- Lambda + (d / b) B, and where
            // 2 L <= r the old Lambda becomes B, b <- d, L <- r + 1 - L.  Lambda_0 stays 1.  L <= 2 t <= 32 < 64 lanes.
            uint32_t lam = lane == 0, B = lane == 0, b = 1;
            int L = 0;
            for (int r = 0; r < 2 * BCH_T; r++) {
                if (r >= 2 * t) break;
                const uint32_t up = (uint32_t)__shfl_up((int)B, 1);
                B = lane == 0 ? 0u : up;
                const int si = r + 1 - lane;
                const uint32_t s = sc.S[min(max(si, 1), 2 * t)];
                const uint32_t d = bch_wave_xor(lane <= L && si >= 1 ? mul(lam, s) : 0u);
                if (d) {
                    uint32_t ib = q - (uint32_t)LOG[b];
                    ib = ib >= q ? ib - q : ib;
                    const uint32_t coef = mul(d, EXP[ib]), old = lam;
                    lam ^= mul(coef, B);
                    if (2 * L <= r) {
                        L = r + 1 - L;
                        B = old;
                        b = d;
                    }
                }
            }
            if (L <= t) {
                if (lane <= L) sc.lam[lane] = lam ? LOG[lam] : (uint16_t)0xffff;
                bch_wave_sync();
                const int nq = (int)(q + 63u) >> 6;
                int total = 0, nin = 0, hit = 0, miss = 0;
                for (int it = 0; it < BCH_IT; it++) {
                    if (it >= nq) break;
                    const uint32_t p = (uint32_t)(it * 64 + lane), g = p == 0 || p >= q ? 0u : q - p;   // alpha^(-p)
                    uint32_t val = 1, acc = 0;                 // Lambda(alpha^(-p)) = 1 + sum_k Lambda_k alpha^(-k p)
#pragma unroll
                    for (int k = 1; k <= BCH_T; k++)
                        if (k <= L) {
                            acc += g;
                            acc = acc >= q ? acc - q : acc;
                            const uint32_t ll = sc.lam[k];
                            uint32_t x = (ll == 0xffffu ? 0u : ll) + acc;
                            x = x >= q ? x - q : x;
                            const uint32_t v = EXP[x];
                            val ^= ll == 0xffffu ? 0u : v;
                        }
                    const bool root = p < q && val == 0, inr = root && p < (uint32_t)n_o;
                    const unsigned long long all = __ballot(root), inm = __ballot(inr), em = it < nit ? sc.err[it] : 0ull;
                    if (inr) {
                        const int slot = nin + __popcll(inm & ((1ull << lane) - 1ull));
                        if (slot < BCH_T) sc.loc[slot] = (int16_t)p;
                    }
                    total += __popcll(all);
                    nin += __popcll(inm);
                    hit += __popcll(inm & em);
                    miss += __popcll(inm & ~em);
                }
                bch_wave_sync();
                if (total == L && nin == L) {                  // L roots, none of them at a shortened position
                    status = 1;
                    nflip = L;
                    post_err = pre - hit + miss;
                }
            }
        }
        if (lane == 0) {
            int32_t *dst = out + (size_t)a * 4;
            dst[0] = status;
            dst[1] = pre;
            dst[2] = post_err;
            dst[3] = nflip;
        }
        if (loc && lane < t) loc[(size_t)a * (size_t)t + lane] = status == 1 && lane < nflip ? sc.loc[lane] : (int16_t)-1;
        bch_wave_sync();                                       // the scratch is the next codeword's
    }
}

}  // namespace vaeq

extern "C" int vaeq_bch_outer(int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0, int32_t depth, int32_t n, int32_t K, int32_t m, int32_t t,
                              int32_t n_o, int32_t C_o, int32_t spread, const void *post, int32_t post_i16, const int8_t *bits, int32_t *out,
                              int16_t *loc, void *stream)
{
    using namespace vaeq;
    if (R == 0) return VAEQ_OK;                                // an empty batch owns no memory: its pointers may be NULL
    if (!post || !bits || !out) return VAEQ_ERR_NULL;
    if (!fec_frame_ok(R, C, N, w, t0) || (int64_t)R * C > 0x7fffffff || depth < 0 || depth > C || n < 2 || n > LDPC_NB * LDPC_Z) return VAEQ_ERR_SHAPE;
    const bool il = depth >= 1;
    if (!fec_fit_ok(il, C, n, w, t0, N)) return VAEQ_ERR_SHAPE;
    if (K < 1 || K > n || m < BCH_M_MIN || m > BCH_M_MAX || t < 1 || t > BCH_T || n_o > (1 << m) - 1 || n_o <= bch_parity(m, t) || spread < 0 ||
        spread > 1 || post_i16 < 0 || post_i16 > 1 || C_o < 1 || (int64_t)R * C_o > 0x7fffffff)
        return VAEQ_ERR_SHAPE;
    if ((int64_t)C_o * n_o > (int64_t)C * K) return VAEQ_ERR_SHAPE;
    const bch_args A = {(long long)N, (long long)t0, (long long)R * C_o, (int)C, (int)w, (int)depth, (int)n, (int)K, (int)m, (int)t, (int)n_o, (int)C_o,
                        (int)spread, (int)post_i16, gf_poly(m)};
    const bool wide = (int64_t)C * n > 0x7fffffff || (int64_t)w * N > 0xffffffffll;
    const int64_t blocks = (A.total + BCH_WAVES - 1) / BCH_WAVES;
    const dim3 grid((unsigned)(blocks < BCH_GRID ? blocks : BCH_GRID)), block(BCH_NT);
    const size_t lds = (size_t)4 << m;                         // exp and log, 2^m uint16 each
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (wide) return launch(il ? bch_outer_kernel<true, uint64_t> : bch_outer_kernel<false, uint64_t>, grid, block, lds, st, A, post, bits, out, loc);
    return launch(il ? bch_outer_kernel<true, uint32_t> : bch_outer_kernel<false, uint32_t>, grid, block, lds, st, A, post, bits, out, loc);
}
