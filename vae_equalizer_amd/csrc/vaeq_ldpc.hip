// vaeq_ldpc.hip -- post-FEC figures on the device: a batched decoder of quasi-cyclic LDPC codes over the per-bit LLRs of the demappers
// (vaeq_dp_epilogue_llr, vaeq_awgn_llr, vaeq_cma_epilogue_llr, vaeq_awgn_track_llr).  Layered normalized min-sum, float32, every operation
// rounded on its own in the order include/vaeq.h fixes, so that a numpy float32 model gives the same bits.  No encoder: the transmitted bits are
// the sweep's random symbols, so the decoder works towards their syndrome (coset decoding).  Two entry points, one kernel: vaeq_ldpc_decode maps
// bit-packed contiguous codewords onto the frame, vaeq_ldpc_decode_il puts a symbol interleaver over groups of `depth` codewords in front; the
// choice is a template argument of the kernel and touches its input gather alone.
// The envelope, the table and its packer, the edge walker and the gather are in vaeq_ldpc.h, shared with the fixed-point decoder (vaeq_ldpc_q.hip).
//
// One codeword per workgroup, one thread per check of the layer in flight (Z checks, blockDim = Z rounded up to whole waves).  The whole state
// lives in LDS: L[n] f32, the TX bits [n] as bytes, and per check the compressed message (m1, m2, idx | sigma << 8, signs), 16 bytes, as four
// arrays so that consecutive checks touch consecutive banks.  A layer's checks own disjoint variables (a block is a cyclic permutation), so
// a layer needs no barrier inside; one barrier separates two layers.  Check i of a block with shift s reads L[c Z + (i + s) mod Z]:
// consecutive lanes, consecutive addresses, one wrap.  The table of shifts comes by value in the kernel arguments, row by row as (column, shift)
// pairs of its non-zero blocks, and is read eight edges at a time with scalar loads.  The kernel is bound by instruction issue, not by LDS
// (DESIGN.md section 5): a check reads its eight L values of a group together, keeps t_e and the addresses of its up to 32 edges in registers
// between the minimum search and the write-back (124 VGPRs: four waves per SIMD, what the LDS of four workgroups per CU fills anyway), and
// tracks (m1, m2) with one min and one median-of-three.
// The decision to go on is made by __syncthreads_or over the per-thread syndrome tests: every thread of the workgroup gets the same answer
// behind the same barrier, and every loop has a static bound.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vaeq.h"
#include "vaeq_launch.h"
#include "vaeq_ldpc.h"

namespace vaeq {

inline int64_t ldpc_state_bytes(int64_t mb, int64_t nb, int64_t Z) { return 4 * nb * Z + ((nb * Z + 3) & ~(int64_t)3) + 16 * mb * Z; }

// x with its sign flipped when bit e of sg is set (an exact negation, of zero too)
__device__ __forceinline__ float ldpc_signed(float x, uint32_t sg, int e) { return __uint_as_float(__float_as_uint(x) ^ ((sg >> e) << 31)); }

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

}  // namespace vaeq

extern "C" int64_t vaeq_ldpc_lds_bytes(int32_t mb, int32_t nb, int32_t Z)
{
    return vaeq::ldpc_dims_ok(mb, nb, Z) ? vaeq::ldpc_state_bytes(mb, nb, Z) : (int64_t)VAEQ_ERR_SHAPE;
}

namespace vaeq {

// il: vaeq_ldpc_decode_il's interleaver of `depth`; otherwise vaeq_ldpc_decode's contiguous codewords, depth unused
static int ldpc_decode_any(int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0, int32_t depth, int32_t mb, int32_t nb, int32_t Z,
                           const int32_t *shifts_host, const float *llr, const int8_t *bits, float alpha, int32_t max_iter, int32_t *out, float *post,
                           void *stream, bool il)
{
    if (R == 0) return VAEQ_OK;                                // an empty batch owns no memory: its pointers may be NULL
    if (!shifts_host || !llr || !bits || !out) return VAEQ_ERR_NULL;
    const int64_t lds = ldpc_state_bytes(mb, nb, Z);
    if (!ldpc_shape_ok(R, C, N, w, t0, depth, mb, nb, Z, max_iter, lds, il)) return VAEQ_ERR_SHAPE;
    ldpc_table tab;
    if (!ldpc_pack(mb, nb, Z, shifts_host, &tab)) return VAEQ_ERR_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return launch(il ? ldpc_decode_kernel<true> : ldpc_decode_kernel<false>, dim3((unsigned)((int64_t)R * C)), dim3((unsigned)((Z + 63) / 64 * 64)),
                  (size_t)lds, st, tab, (int)C, (long long)N, (int)w, (long long)t0, (int)mb, (int)nb, (int)Z, llr, bits, alpha, (int)max_iter, out, post,
                  (int)depth);
}

}  // namespace vaeq

extern "C" int vaeq_ldpc_decode(int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0, int32_t mb, int32_t nb, int32_t Z,
                                const int32_t *shifts_host, const float *llr, const int8_t *bits, float alpha, int32_t max_iter, int32_t *out,
                                float *post, void *stream)
{
    return vaeq::ldpc_decode_any(R, C, N, w, t0, 0, mb, nb, Z, shifts_host, llr, bits, alpha, max_iter, out, post, stream, false);
}

extern "C" int vaeq_ldpc_decode_il(int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0, int32_t depth, int32_t mb, int32_t nb, int32_t Z,
                                   const int32_t *shifts_host, const float *llr, const int8_t *bits, float alpha, int32_t max_iter, int32_t *out,
                                   float *post, void *stream)
{
    return vaeq::ldpc_decode_any(R, C, N, w, t0, depth, mb, nb, Z, shifts_host, llr, bits, alpha, max_iter, out, post, stream, true);
}
