// vaeq_ldpc.hip -- post-FEC figures on the device: the batched decoders of quasi-cyclic LDPC codes over the per-bit LLRs of the demappers
// (vaeq_dp_epilogue_llr, vaeq_awgn_llr, vaeq_cma_epilogue_llr, vaeq_awgn_track_llr).  Layered normalized min-sum in one of two arithmetics
// (vaeq_ldpc_rule.h): float32, every operation rounded on its own in the order include/vaeq.h fixes, so that a numpy float32 model gives the same
// bits; and fixed point as a hardware decoder holds it, where the header fixes every rounding, clamp and tie, so that an integer numpy model gives
// the same bits.  Float32 min-sum is positively homogeneous -- a common factor on all LLRs changes no decision -- and the fixed-point decoder is
// not: its clamps and its rounding to zero make the scale of an equalizer's LLRs (its noise-variance estimate) visible in the post-FEC figures.
// No encoder: the transmitted bits are the sweep's random symbols, so the decoders work towards their syndrome (coset decoding).
// Three entry points: vaeq_ldpc_decode maps bit-packed contiguous codewords onto the frame, vaeq_ldpc_decode_il puts a symbol interleaver over
// groups of `depth` codewords in front, vaeq_ldpc_decode_q is the fixed-point decoder with either gather (depth == 0: contiguous).  The gather
// is a template argument of the kernels and touches nothing else.  The two arithmetics are two kernels, ldpc_decode_kernel and ldpc_q_kernel,
// written out side by side: the same mapping and control code, twins line for line but for the type of L, the state's layout, the quantiser
// in the gather and the layer update (DESIGN.md section 5 says why they are not one body).
// The envelope, the table and its packer, the edge walker and the gather are in vaeq_ldpc.h.
//
// One codeword per workgroup, one thread per check of the layer in flight (Z checks, blockDim = Z rounded up to whole waves).  The whole state lives
// in LDS (vaeq_ldpc_rule.h describes both layouts).  A layer's checks own disjoint variables (a block is a cyclic permutation), so a layer needs no
// barrier inside; one barrier separates two layers.  Check i of a block with shift s reads L[c Z + (i + s) mod Z]: consecutive lanes, consecutive
// addresses, one wrap.  The table of shifts comes by value in the kernel arguments, row by row as (column, shift) pairs of its non-zero blocks, and is
// read eight edges at a time with scalar loads.  The kernels are bound by instruction issue, not by LDS: a check reads its eight
// L values of a group together, keeps t_e and the addresses of its up to 32 edges in registers between the minimum search and the write-back (float:
// 124 VGPRs, four waves per SIMD, what the LDS of four workgroups per CU fills anyway; fixed point: 94 and five), and tracks (m1, m2) with one min
// and one median-of-three.
// The decision to go on is made by __syncthreads_or over the per-thread syndrome tests: every thread of the workgroup gets the same answer
// behind the same barrier, and every loop has a static bound.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vaeq.h"
#include "vaeq_launch.h"
#include "vaeq_ldpc_rule.h"

namespace vaeq {

// IL: the symbol interleaver of vaeq_ldpc_decode_il over groups of `depth` codewords (include/vaeq.h); false: vaeq_ldpc_decode's bit-packed
// contiguous codewords, `depth` unused.  Only the gather differs.
template <bool IL>
__global__ __launch_bounds__(LDPC_Z) void ldpc_decode_kernel(const ldpc_table tab, int C, long long N, int w, long long t0, int mb, int nb, int Z,
                                                             const float *__restrict__ llr, const int8_t *__restrict__ bits, float alpha,
                                                             int max_iter, int32_t *__restrict__ out, float *__restrict__ post, int depth)
{
    extern __shared__ __align__(16) unsigned char ldpc_lds[];
    __shared__ int cnt[3];                                     // post_err, pre_err, erased
    const int tid = threadIdx.x, NT = blockDim.x, n = nb * Z, m = mb * Z;
    float *L = reinterpret_cast<float *>(ldpc_lds);
    float *M1 = L + n, *M2 = M1 + m;
    uint32_t *META = reinterpret_cast<uint32_t *>(M2 + m), *SG = META + m;
    uint8_t *B = reinterpret_cast<uint8_t *>(SG + m);
    const size_t run = blockIdx.x / (unsigned)C;
    const int cw = (int)(blockIdx.x % (unsigned)C);
    mb = min(mb, LDPC_MB);
    max_iter = min(max_iter, LDPC_ITER);

    const ldpc_window win = ldpc_window_of<IL>(cw, C, w, t0, depth, n);
    if (tid < 3) cnt[tid] = 0;
    int pre = 0, era = 0;
    ldpc_gather(win, run, N, w, n, tid, NT, llr, bits, [&](long long j, float x, uint32_t b) {
        L[j] = x;
        B[j] = (uint8_t)b;
        pre += (uint32_t)(x < 0.f) != b;
        era += x == 0.f;
    });
    __syncthreads();
    if (pre) atomicAdd(&cnt[1], pre);
    if (era) atomicAdd(&cnt[2], era);
    auto ldL = [&](int v) -> float { return L[v]; };
    auto ldB = [&](int v) -> uint32_t { return B[v]; };
    if (tid < Z)
        for (int l = 0; l < mb; l++) {                         // sigma of the TX bits; all messages zero
            uint32_t par = 0;
            ldpc_edges(tab.row[l], (int)(tab.wt >> (8 * l)) & 0xff, Z, tid, ldB, [&](int, bool valid, int, uint32_t b) { par ^= valid ? b : 0u; });
            const int c = l * Z + tid;
            M1[c] = 0.f;
            M2[c] = 0.f;
            META[c] = par << 8;
            SG[c] = 0u;
        }

    // the syndrome test of this thread's mb checks on the hard decisions L < 0
    auto unsatisfied = [&]() -> int {
        uint32_t bad = 0;
        if (tid < Z)
            for (int l = 0; l < mb; l++) {
                uint32_t par = META[l * Z + tid] >> 8;
                ldpc_edges(tab.row[l], (int)(tab.wt >> (8 * l)) & 0xff, Z, tid, ldL, [&](int, bool valid, int, float x) { par ^= (uint32_t)(valid && x < 0.f); });
                bad |= par;
            }
        return (int)bad;
    };

    int iters = 0;
    int fail = __syncthreads_or(unsatisfied());                // workgroup-uniform, behind a barrier
    for (int it = 0; it < LDPC_ITER; it++) {
        if (!fail || it >= max_iter) break;                    // uniform: fail and max_iter are the same in every thread
        for (int l = 0; l < mb; l++) {
            if (tid < Z) {
                const int c = l * Z + tid, wt = (int)(tab.wt >> (8 * l)) & 0xff;
                const uint4 *row = tab.row[l];
                const uint32_t meta = META[c], sg = SG[c];
                const int idx = (int)(meta & 0xffu);
                const float a1 = __fmul_rn(alpha, M1[c]), a2 = __fmul_rn(alpha, M2[c]);
                float m1 = __builtin_inff(), m2 = __builtin_inff();
                int nidx = 0;
                uint32_t s = 0, S = meta >> 8;
                float t[LDPC_ROW];
                int va[LDPC_ROW];
                ldpc_edges(row, wt, Z, tid, ldL, [&](int e, bool valid, int v, float x) {
                    t[e] = __fsub_rn(x, ldpc_signed(e == idx ? a2 : a1, sg, e));
                    va[e] = v;
                    const float a = valid ? fabsf(t[e]) : __builtin_inff();    // an edge past wt: never below m1 or m2, no sign
                    nidx = a < m1 ? e : nidx;                                  // the first edge that attains the minimum
                    m2 = __builtin_amdgcn_fmed3f(m1, m2, a);                   // m1 <= m2: the median is the second smallest of the three
                    m1 = fminf(m1, a);
                    const uint32_t neg = (uint32_t)(valid && t[e] < 0.f);
                    s |= neg << e;
                    S ^= neg;
                });
                const float b1 = __fmul_rn(alpha, m1), b2 = __fmul_rn(alpha, m2);
                const uint32_t nsg = S ? ~s : s;               // the new message of edge e is negative iff S ^ s_e (bits past wt are never read)
#pragma unroll
                for (int e = 0; e < LDPC_ROW; e++)             // t and the addresses are still in registers: no second read of L
                    if (e < wt) L[va[e]] = __fadd_rn(t[e], ldpc_signed(e == nidx ? b2 : b1, nsg, e));
                M1[c] = m1;
                M2[c] = m2;
                META[c] = (meta & ~0xffu) | (uint32_t)nidx;
                SG[c] = nsg;
            }
            __syncthreads();
        }
        iters = it + 1;
        fail = __syncthreads_or(unsatisfied());
    }

    int err = 0;
    const size_t o = (run * (size_t)C + cw) * (size_t)n;
    for (int j = tid; j < n; j += NT) {
        const float x = L[j];
        err += (int)(x < 0.f) != (int)B[j];
        if (post) post[o + j] = x;
    }
    if (err) atomicAdd(&cnt[0], err);
    __syncthreads();
    if (tid == 0) {
        int32_t *dst = out + (run * (size_t)C + cw) * 5;
        dst[0] = iters;
        dst[1] = !fail;
        dst[2] = cnt[0];
        dst[3] = cnt[1];
        dst[4] = cnt[2];
    }
}

// The fixed-point twin of ldpc_decode_kernel: the same control code over int16 L, the quantiser in the gather, the packed state and the integer
// layer update.  Kept as a kernel of its own: DESIGN.md section 5, "The LDPC decoders: what is shared and what is not".
template <bool IL>
__global__ __launch_bounds__(LDPC_Z) void ldpc_q_kernel(const ldpc_table tab, int C, long long N, int w, long long t0, int mb, int nb, int Z,
                                                        const float *__restrict__ llr, const int8_t *__restrict__ bits, const ldpc_q_rule q,
                                                        int max_iter, int32_t *__restrict__ out, int16_t *__restrict__ post, int depth)
{
    extern __shared__ __align__(16) unsigned char ldpc_q_lds[];
    __shared__ int cnt[3];                                     // post_err, pre_err, erased
    const int tid = threadIdx.x, NT = blockDim.x, n = nb * Z, m = mb * Z;
    int16_t *L = reinterpret_cast<int16_t *>(ldpc_q_lds);
    uint8_t *B = ldpc_q_lds + ((2 * n + 3) & ~3);
    uint32_t *META = reinterpret_cast<uint32_t *>(B + ((n + 3) & ~3)), *SG = META + m;
    const size_t run = blockIdx.x / (unsigned)C;
    const int cw = (int)(blockIdx.x % (unsigned)C);
    mb = min(mb, LDPC_MB);
    max_iter = min(max_iter, LDPC_ITER);
    const int Mmax = q.cmax, Lmax = q.lmax, num = q.num, beta = q.beta;
    const float cmax = (float)q.cmax;
    auto norm = [&](int a) -> int { return max(((num * a + 4) >> 3) - beta, 0); };

    const ldpc_window win = ldpc_window_of<IL>(cw, C, w, t0, depth, n);
    if (tid < 3) cnt[tid] = 0;
    int pre = 0, era = 0;
    ldpc_gather(win, run, N, w, n, tid, NT, llr, bits, [&](long long j, float x, uint32_t b) {
        float y = __fmul_rn(x, q.scale);
        y = y != y ? 0.f : y;                                  // a NaN is +0
        y = fminf(fmaxf(y, -cmax), cmax);
        const int Q = (int)rintf(y);                           // ties to even
        L[j] = (int16_t)Q;
        B[j] = (uint8_t)b;
        pre += (uint32_t)(x < 0.f) != b;                       // of the raw input: the float decoder's count
        era += Q == 0;
    });
    __syncthreads();
    if (pre) atomicAdd(&cnt[1], pre);
    if (era) atomicAdd(&cnt[2], era);
    auto ldL = [&](int v) -> int { return L[v]; };
    auto ldB = [&](int v) -> uint32_t { return B[v]; };
    if (tid < Z)
        for (int l = 0; l < mb; l++) {                         // sigma of the TX bits; all messages zero
            uint32_t par = 0;
            ldpc_edges(tab.row[l], (int)(tab.wt >> (8 * l)) & 0xff, Z, tid, ldB, [&](int, bool valid, int, uint32_t b) { par ^= valid ? b : 0u; });
            const int c = l * Z + tid;
            META[c] = par << 24;
            SG[c] = 0u;
        }

    // the syndrome test of this thread's mb checks on the hard decisions L < 0
    auto unsatisfied = [&]() -> int {
        uint32_t bad = 0;
        if (tid < Z)
            for (int l = 0; l < mb; l++) {
                uint32_t par = META[l * Z + tid] >> 24;
                ldpc_edges(tab.row[l], (int)(tab.wt >> (8 * l)) & 0xff, Z, tid, ldL, [&](int, bool valid, int, int x) { par ^= (uint32_t)(valid && x < 0); });
                bad |= par;
            }
        return (int)bad;
    };

    int lo = -Lmax, hi = Lmax;                                 // the clamp's bounds in vector registers, once: v_med3_i32 takes one scalar at most
    ldpc_pin(lo);
    ldpc_pin(hi);
    int iters = 0;
    int fail = __syncthreads_or(unsatisfied());                // workgroup-uniform, behind a barrier
    for (int it = 0; it < LDPC_ITER; it++) {
        if (!fail || it >= max_iter) break;                    // uniform: fail and max_iter are the same in every thread
        for (int l = 0; l < mb; l++) {
            if (tid < Z) {
                const int c = l * Z + tid, wt = (int)(tab.wt >> (8 * l)) & 0xff;
                const uint4 *row = tab.row[l];
                const uint32_t meta = META[c], sg = SG[c];
                int idx = (int)((meta >> 16) & 0xffu);
                ldpc_pin(idx);                                 // extracted once, not per comparison
                const int a1 = norm((int)(meta & 0xffu)), a2 = norm((int)((meta >> 8) & 0xffu));
                int m1 = 0x7fff, m2 = 0x7fff;                  // above every Mmax
                int nidx = 0;
                uint32_t s = 0, S = meta >> 24;
                int t[LDPC_ROW];
                int va[LDPC_ROW];
                ldpc_edges(row, wt, Z, tid, ldL, [&](int e, bool valid, int v, int x) {
                    // an edge past wt takes part as a large positive value (vaeq_ldpc_rule.h, absent edges)
                    t[e] = (valid ? x : 0x3fff) - ldpc_q_signed(e == idx ? a2 : a1, sg, e);
                    va[e] = v;
                    const int a = min(abs(t[e]), Mmax);
                    nidx = a < m1 ? e : nidx;                                  // the first edge that attains the minimum
                    m2 = ldpc_med3(m1, m2, a);                                 // m1 <= m2: the median is the second smallest of the three
                    m1 = min(m1, a);
                    const uint32_t neg = (uint32_t)(t[e] < 0);
                    s |= neg << e;
                    S ^= neg;
                });
                int b1 = norm(m1), b2 = norm(m2);
                ldpc_pin(b1);                                  // or the backend moves f() behind the select below and evaluates it once per edge
                ldpc_pin(b2);
                const uint32_t nsg = S ? ~s : s;               // the new message of edge e is negative iff S ^ s_e (bits past wt are never read)
#pragma unroll
                for (int e = 0; e < LDPC_ROW; e++)             // t and the addresses are still in registers: no second read of L
                    if (e < wt) L[va[e]] = (int16_t)ldpc_med3(t[e] + ldpc_q_signed(e == nidx ? b2 : b1, nsg, e), lo, hi);
                META[c] = (meta & 0xff000000u) | (uint32_t)nidx << 16 | (uint32_t)m2 << 8 | (uint32_t)m1;
                SG[c] = nsg;
            }
            __syncthreads();
        }
        iters = it + 1;
        fail = __syncthreads_or(unsatisfied());
    }

    int err = 0;
    const size_t o = (run * (size_t)C + cw) * (size_t)n;
    for (int j = tid; j < n; j += NT) {
        const int x = L[j];
        err += (int)(x < 0) != (int)B[j];
        if (post) post[o + j] = (int16_t)x;
    }
    if (err) atomicAdd(&cnt[0], err);
    __syncthreads();
    if (tid == 0) {
        int32_t *dst = out + (run * (size_t)C + cw) * 5;
        dst[0] = iters;
        dst[1] = !fail;
        dst[2] = cnt[0];
        dst[3] = cnt[1];
        dst[4] = cnt[2];
    }
}

// What the three entry points share behind their own refusals.  depth >= 1: the interleaver's gather; rule_ok: the arithmetic's own rules,
// behind the fit rule and ahead of the table's.
template <class Launch>
static int ldpc_decode_any(int64_t (*bytes)(int64_t, int64_t), int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0, int32_t depth, int32_t mb,
                           int32_t nb, int32_t Z, const int32_t *shifts_host, const void *llr, const void *bits, int32_t max_iter, const void *out,
                           bool il, bool rule_ok, Launch &&go)
{
    if (R == 0) return VAEQ_OK;                                // an empty batch owns no memory: its pointers may be NULL
    if (!shifts_host || !llr || !bits || !out) return VAEQ_ERR_NULL;
    const int64_t lds = bytes((int64_t)nb * Z, (int64_t)mb * Z);
    if (!ldpc_shape_ok(R, C, N, w, t0, depth, mb, nb, Z, max_iter, lds, il) || !rule_ok) return VAEQ_ERR_SHAPE;
    ldpc_table tab;
    if (!ldpc_pack(mb, nb, Z, shifts_host, &tab)) return VAEQ_ERR_SHAPE;
    return go(tab, dim3((unsigned)((int64_t)R * C)), dim3((unsigned)((Z + 63) / 64 * 64)), (size_t)lds);
}

// il: vaeq_ldpc_decode_il's interleaver of `depth`; otherwise vaeq_ldpc_decode's contiguous codewords, depth unused
static int ldpc_decode_float(int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0, int32_t depth, int32_t mb, int32_t nb, int32_t Z,
                             const int32_t *shifts_host, const float *llr, const int8_t *bits, float alpha, int32_t max_iter, int32_t *out, float *post,
                             void *stream, bool il)
{
    return ldpc_decode_any(ldpc_float_bytes, R, C, N, w, t0, depth, mb, nb, Z, shifts_host, llr, bits, max_iter, out, il, true,
                                       [&](const ldpc_table &tab, dim3 grid, dim3 block, size_t lds) {
        return launch(il ? ldpc_decode_kernel<true> : ldpc_decode_kernel<false>, grid, block, lds, reinterpret_cast<hipStream_t>(stream), tab, (int)C,
                      (long long)N, (int)w, (long long)t0, (int)mb, (int)nb, (int)Z, llr, bits, alpha, (int)max_iter, out, post, (int)depth);
    });
}

}  // namespace vaeq

extern "C" int64_t vaeq_ldpc_lds_bytes(int32_t mb, int32_t nb, int32_t Z)
{
    return vaeq::ldpc_dims_ok(mb, nb, Z) ? vaeq::ldpc_float_bytes((int64_t)nb * Z, (int64_t)mb * Z) : (int64_t)VAEQ_ERR_SHAPE;
}

extern "C" int64_t vaeq_ldpc_q_lds_bytes(int32_t mb, int32_t nb, int32_t Z)
{
    return vaeq::ldpc_dims_ok(mb, nb, Z) ? vaeq::ldpc_fixed_bytes((int64_t)nb * Z, (int64_t)mb * Z) : (int64_t)VAEQ_ERR_SHAPE;
}

extern "C" int vaeq_ldpc_decode(int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0, int32_t mb, int32_t nb, int32_t Z,
                                const int32_t *shifts_host, const float *llr, const int8_t *bits, float alpha, int32_t max_iter, int32_t *out,
                                float *post, void *stream)
{
    return vaeq::ldpc_decode_float(R, C, N, w, t0, 0, mb, nb, Z, shifts_host, llr, bits, alpha, max_iter, out, post, stream, false);
}

extern "C" int vaeq_ldpc_decode_il(int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0, int32_t depth, int32_t mb, int32_t nb, int32_t Z,
                                   const int32_t *shifts_host, const float *llr, const int8_t *bits, float alpha, int32_t max_iter, int32_t *out,
                                   float *post, void *stream)
{
    return vaeq::ldpc_decode_float(R, C, N, w, t0, depth, mb, nb, Z, shifts_host, llr, bits, alpha, max_iter, out, post, stream, true);
}

extern "C" int vaeq_ldpc_decode_q(int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0, int32_t depth, int32_t mb, int32_t nb, int32_t Z,
                                  const int32_t *shifts_host, const float *llr, const int8_t *bits, int32_t qbits, int32_t abits, float scale,
                                  int32_t num, int32_t beta, int32_t max_iter, int32_t *out, int16_t *post, void *stream)
{
    using namespace vaeq;
    const bool il = depth >= 1;
    return ldpc_decode_any(ldpc_fixed_bytes, R, C, N, w, t0, depth, mb, nb, Z, shifts_host, llr, bits, max_iter, out, il,
                                              depth >= 0 && depth <= C && ldpc_q_rule_ok(qbits, abits, scale, num, beta),
                                              [&](const ldpc_table &tab, dim3 grid, dim3 block, size_t lds) {
        return launch(il ? ldpc_q_kernel<true> : ldpc_q_kernel<false>, grid, block, lds, reinterpret_cast<hipStream_t>(stream), tab, (int)C, (long long)N,
                      (int)w, (long long)t0, (int)mb, (int)nb, (int)Z, llr, bits, ldpc_q_rule_of(qbits, abits, scale, num, beta), (int)max_iter, out, post,
                      (int)depth);
    });
}
