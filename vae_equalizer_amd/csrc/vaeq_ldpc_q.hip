// vaeq_ldpc_q.hip -- the fixed-point decoder of include/vaeq.h (vaeq_ldpc_decode_q): vaeq_ldpc.hip's layered min-sum with q-bit channel LLRs,
// q-bit check messages and saturating a-posteriori values, as a hardware decoder holds them.  The quantiser is the only float arithmetic; from
// there on every value is an integer and the header fixes every rounding, clamp and tie, so that an integer numpy model gives the same bits.
// Float32 min-sum is positively homogeneous -- a common factor on all LLRs changes no decision -- and this decoder is not: its clamps and its
// rounding to zero make the scale of an equalizer's LLRs (its noise-variance estimate) visible in the post-FEC figures.
//
// The mapping is the float kernel's, for the reasons measured there: one codeword per workgroup, one thread per check of
// the layer in flight, the table by value in the arguments, eight reads in flight and pinned, t_e and the addresses of the up to 32 edges kept
// in registers between the minimum search and the write-back, one barrier per layer, __syncthreads_or for the stop decision, static loop
// bounds; both gather forms (depth == 0: bit-packed contiguous codewords, depth >= 1: the symbol interleaver) from vaeq_ldpc.h.  The state is
// smaller: L[n] as int16, the TX bits [n] as bytes, and per check two dwords -- m1 | m2 << 8 | idx << 16 | sigma << 24, and the signs -- 3 n + 8 m
// bytes against 5 n + 16 m.  A layer's checks own disjoint variables, and a 16-bit store touches its own two bytes alone, so a layer still
// needs no barrier inside.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "vaeq.h"
#include "vaeq_launch.h"
#include "vaeq_ldpc_sc.h"

namespace vaeq {

inline int64_t ldpc_q_state_bytes(int64_t mb, int64_t nb, int64_t Z) { return ((2 * nb * Z + 3) & ~(int64_t)3) + ((nb * Z + 3) & ~(int64_t)3) + 8 * mb * Z; }

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
                    // An edge past wt takes part as a large positive value: t_e > 0 and a_e = Mmax, which changes neither m1, m2 and idx (the
                    // two or more real edges before it have brought both minima to Mmax or below; an equal value is not "first") nor a sign.
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

}  // namespace vaeq

extern "C" int64_t vaeq_ldpc_q_lds_bytes(int32_t mb, int32_t nb, int32_t Z)
{
    return vaeq::ldpc_dims_ok(mb, nb, Z) ? vaeq::ldpc_q_state_bytes(mb, nb, Z) : (int64_t)VAEQ_ERR_SHAPE;
}

extern "C" int vaeq_ldpc_decode_q(int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0, int32_t depth, int32_t mb, int32_t nb, int32_t Z,
                                  const int32_t *shifts_host, const float *llr, const int8_t *bits, int32_t qbits, int32_t abits, float scale,
                                  int32_t num, int32_t beta, int32_t max_iter, int32_t *out, int16_t *post, void *stream)
{
    using namespace vaeq;
    if (R == 0) return VAEQ_OK;                                // an empty batch owns no memory: its pointers may be NULL
    if (!shifts_host || !llr || !bits || !out) return VAEQ_ERR_NULL;
    if (depth < 0 || depth > C) return VAEQ_ERR_SHAPE;
    const bool il = depth >= 1;
    const int64_t lds = ldpc_q_state_bytes(mb, nb, Z);
    if (!ldpc_shape_ok(R, C, N, w, t0, depth, mb, nb, Z, max_iter, lds, il)) return VAEQ_ERR_SHAPE;
    if (!ldpc_q_rule_ok(qbits, abits, scale, num, beta)) return VAEQ_ERR_SHAPE;
    ldpc_table tab;
    if (!ldpc_pack(mb, nb, Z, shifts_host, &tab)) return VAEQ_ERR_SHAPE;
    const ldpc_q_rule q = {scale, (1 << (qbits - 1)) - 1, (1 << (abits - 1)) - 1, (int)num, (int)beta};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return launch(il ? ldpc_q_kernel<true> : ldpc_q_kernel<false>, dim3((unsigned)((int64_t)R * C)), dim3((unsigned)((Z + 63) / 64 * 64)), (size_t)lds,
                  st, tab, (int)C, (long long)N, (int)w, (long long)t0, (int)mb, (int)nb, (int)Z, llr, bits, q, (int)max_iter, out, post, (int)depth);
}
