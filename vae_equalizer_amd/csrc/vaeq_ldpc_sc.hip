// vaeq_ldpc_sc.hip -- spatially coupled LDPC codes behind the demappers: a sliding-window decoder over a terminated chain of Lc positions that is
// far larger than LDS (vaeq_ldpc_sc_decode, include/vaeq.h).  The code is a set of ms + 1 component tables [mb][nb] of circulants; block row
// (t, l) of the coupled matrix holds components[t - i][l][c] in block column (i, c) for 0 <= t - i <= ms.  The layer update is vaeq_ldpc.hip's,
// operation for operation (layered normalized min-sum in float32, coset decoding, every operation rounded on its own), so a window that covers
// the whole chain gives what vaeq_ldpc_decode gives on the coupled table.  The gather and its bit map are vaeq_ldpc.h's: column block i of
// chain c is codeword c Lc + i of nb Z bits.
//
// One chain per workgroup, one thread per check of the layer in flight.  The window is a ring in LDS: column block i (L as float32 and the TX
// bits as bytes) lives in slot i mod (W + ms), the compressed state (m1, m2, idx | sigma << 8, signs) of row block t in slot t mod W.  All slot
// arithmetic is on wave-uniform values.  When the window moves from p to p + 1, column block p - ms is counted and stored, column block p + W
// is gathered into the slot it leaves, and row block p + W starts from zeros, with its sigma from the TX bits then resident, in the slot of
// row block p.  Nothing else is touched: the rows and columns that stay keep their state.
// The table travels by value: per l the up to 32 non-zero blocks of a full row in ascending coupled column (d = t - i descending, then c), one
// dword each (d << 23 | c Z << 9 | shift), and per l two sets of masks that tell which of these edges a truncated row at the head (d <= t) or
// at the tail (d > t - Lc) of the chain really has.  An edge keeps its number e in the full row wherever the row is, so idx and the sign bits
// of a check mean the same thing for as long as it lives.
// The entering block's loads are not issued ahead of the position's iterations: the layer update keeps 32 t_e and 32 addresses in registers
// (vaeq_ldpc.hip), and a block of up to nb values and bits per thread held across it does not fit beside them without scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vaeq.h"
#include "vaeq_launch.h"
#include "vaeq_ldpc_sc.h"

namespace vaeq {

inline int64_t sc_state_bytes(int64_t ms, int64_t mb, int64_t nb, int64_t Z, int64_t W)
{
    const int64_t ring = (W + ms) * nb * Z;
    return 4 * ring + ((ring + 3) & ~(int64_t)3) + 16 * W * mb * Z;
}

// x with its sign flipped when bit e of sg is set (an exact negation, of zero too)
__device__ __forceinline__ float sc_signed(float x, uint32_t sg, int e) { return __uint_as_float(__float_as_uint(x) ^ ((sg >> e) << 31)); }

__global__ __launch_bounds__(LDPC_Z) void ldpc_sc_kernel(const sc_table tab, int C, long long N, int w, long long t0, int ms, int mb, int nb, int Z,
                                                         int Lc, int W, int T, int P, const float *__restrict__ llr,
                                                         const int8_t *__restrict__ bits, float alpha, int max_iter, int32_t *__restrict__ out,
                                                         float *__restrict__ post, int32_t *__restrict__ pos_err, int32_t *__restrict__ pos_iters)
{
    extern __shared__ __align__(16) unsigned char sc_lds[];
    __shared__ int cnt[2];                                     // pre_err, erased
    __shared__ int colerr[SC_W + SC_MS];                       // the errors of the column block that leaves a slot
    const int tid = threadIdx.x, NT = blockDim.x;
    mb = min(mb, SC_MB);
    ms = min(ms, SC_MS);
    W = min(W, SC_W);
    max_iter = min(max_iter, LDPC_ITER);
    const int nbZ = nb * Z, mZ = mb * Z, ring = W + ms, rows = Lc + ms;
    float *L = reinterpret_cast<float *>(sc_lds);
    float *M1 = L + ring * nbZ, *M2 = M1 + W * mZ;
    uint32_t *META = reinterpret_cast<uint32_t *>(M2 + W * mZ), *SG = META + W * mZ;
    uint8_t *B = reinterpret_cast<uint8_t *>(SG + W * mZ);
    const size_t run = blockIdx.x / (unsigned)C;
    const int chain = (int)(blockIdx.x % (unsigned)C);
    const size_t rc = run * (size_t)C + chain;

    if (tid < 2) cnt[tid] = 0;
    for (int k = tid; k < SC_W + SC_MS; k += NT) colerr[k] = 0;
    int pre = 0, era = 0;
    auto ldL = [&](int v) -> float { return L[v]; };
    auto ldB = [&](int v) -> uint32_t { return B[v]; };

    // column block i enters its slot: the gather of codeword chain Lc + i of nb Z bits
    auto enter_col = [&](int i, int slot) {
        const ldpc_window win = ldpc_window_of<false>(chain * Lc + i, C, w, t0, 0, nbZ);
        float *Ls = L + slot * nbZ;
        uint8_t *Bs = B + slot * nbZ;
        ldpc_gather(win, run, N, w, nbZ, tid, NT, llr, bits, [&](long long j, float x, uint32_t b) {
            Ls[j] = x;
            Bs[j] = (uint8_t)b;
            pre += (uint32_t)(x < 0.f) != b;
            era += x == 0.f;
        });
    };
    // column block i leaves: its final values to post, its errors to the slot's counter
    auto leave_col = [&](int i, int slot) {
        const float *Ls = L + slot * nbZ;
        const uint8_t *Bs = B + slot * nbZ;
        const size_t o = rc * (size_t)Lc * (size_t)nbZ + (size_t)i * (size_t)nbZ;
        int err = 0;
        for (int j = tid; j < nbZ; j += NT) {
            const float x = Ls[j];
            err += (int)(x < 0.f) != (int)Bs[j];
            if (post) post[o + j] = x;
        }
        if (err) atomicAdd(&colerr[slot], err);
    };
    // row block t enters its slot: sigma of the TX bits now resident, all messages zero
    auto enter_row = [&](int t, int rslot, int tslot) {
        if (tid < Z)
            for (int l = 0; l < mb; l++) {
                uint32_t par = 0;
                sc_edges(tab.row[l], (int)(tab.wt >> (8 * l)) & 0xff, sc_mask(tab, l, t, ms, Lc), Z, tid, tslot, ring, nbZ, ldB,
                         [&](int, bool valid, int, uint32_t b) { par ^= valid ? b : 0u; });
                const int c = (rslot * mb + l) * Z + tid;
                M1[c] = 0.f;
                M2[c] = 0.f;
                META[c] = par << 8;
                SG[c] = 0u;
            }
    };
    // the syndrome test of this thread's checks of the row blocks t_lo .. t_hi - 1 on the hard decisions L < 0
    auto unsatisfied = [&](int t_lo, int t_hi, int rslot, int tslot) -> int {
        uint32_t bad = 0;
        if (tid < Z)
            for (int t = t_lo; t < t_hi; t++) {
                for (int l = 0; l < mb; l++) {
                    uint32_t par = META[(rslot * mb + l) * Z + tid] >> 8;
                    sc_edges(tab.row[l], (int)(tab.wt >> (8 * l)) & 0xff, sc_mask(tab, l, t, ms, Lc), Z, tid, tslot, ring, nbZ, ldL,
                             [&](int, bool valid, int, float x) { par ^= (uint32_t)(valid && x < 0.f); });
                    bad |= par;
                }
                rslot = rslot + 1 == W ? 0 : rslot + 1;
                tslot = tslot + 1 == ring ? 0 : tslot + 1;
            }
        return (int)bad;
    };

    {                                                          // the first window: column blocks 0 .. min(Lc, W) - 1, row blocks 0 .. min(W, rows) - 1
        const int nc = min(Lc, W), nr = min(W, rows);
        for (int i = 0; i < nc; i++) enter_col(i, i);
        __syncthreads();
        for (int t = 0; t < nr; t++) enter_row(t, t, t);
    }

    int total = 0, most = 0, all_ok = 1, perr = 0;
    int pW = 0, pR = 0;                                        // p mod W, p mod ring
    for (int p = 0; p < P; p++) {
        const int t_hi = min(p + W, rows), t_test = p < P - 1 ? min(p + T, rows) : t_hi;
        int iters = 0;
        int fail = __syncthreads_or(unsatisfied(p, t_test, pW, pR));           // workgroup-uniform, behind a barrier
        for (int it = 0; it < LDPC_ITER; it++) {
            if (!fail || it >= max_iter) break;                // uniform: fail and max_iter are the same in every thread
            int rslot = pW, tslot = pR;
            for (int t = p; t < t_hi; t++) {
                for (int l = 0; l < mb; l++) {
                    if (tid < Z) {
                        const int c = (rslot * mb + l) * Z + tid, wt = (int)(tab.wt >> (8 * l)) & 0xff;
                        const uint32_t mask = sc_mask(tab, l, t, ms, Lc);
                        const uint32_t meta = META[c], sg = SG[c];
                        const int idx = (int)(meta & 0xffu);
                        const float a1 = __fmul_rn(alpha, M1[c]), a2 = __fmul_rn(alpha, M2[c]);
                        float m1 = __builtin_inff(), m2 = __builtin_inff();
                        int nidx = 0;
                        uint32_t s = 0, S = meta >> 8;
                        float te[LDPC_ROW];
                        int va[LDPC_ROW];
                        sc_edges(tab.row[l], wt, mask, Z, tid, tslot, ring, nbZ, ldL, [&](int e, bool valid, int v, float x) {
                            te[e] = __fsub_rn(x, sc_signed(e == idx ? a2 : a1, sg, e));
                            va[e] = v;
                            const float a = valid ? fabsf(te[e]) : __builtin_inff();   // an edge that is not there: never below m1 or m2, no sign
                            nidx = a < m1 ? e : nidx;                                  // the first edge that attains the minimum
                            m2 = __builtin_amdgcn_fmed3f(m1, m2, a);                   // m1 <= m2: the median is the second smallest of the three
                            m1 = fminf(m1, a);
                            const uint32_t neg = (uint32_t)(valid && te[e] < 0.f);
                            s |= neg << e;
                            S ^= neg;
                        });
                        const float b1 = __fmul_rn(alpha, m1), b2 = __fmul_rn(alpha, m2);
                        const uint32_t nsg = S ? ~s : s;       // the new message of edge e is negative iff S ^ s_e (bits of absent edges are never read)
#pragma unroll
                        for (int e = 0; e < LDPC_ROW; e++)     // t and the addresses are still in registers: no second read of L
                            if ((mask >> e) & 1u) L[va[e]] = __fadd_rn(te[e], sc_signed(e == nidx ? b2 : b1, nsg, e));
                        M1[c] = m1;
                        M2[c] = m2;
                        META[c] = (meta & ~0xffu) | (uint32_t)nidx;
                        SG[c] = nsg;
                    }
                    __syncthreads();
                }
                rslot = rslot + 1 == W ? 0 : rslot + 1;
                tslot = tslot + 1 == ring ? 0 : tslot + 1;
            }
            iters = it + 1;
            fail = __syncthreads_or(unsatisfied(p, t_test, pW, pR));
        }
        total += iters;
        most = max(most, iters);
        all_ok &= !fail;
        if (pos_iters && tid == 0) pos_iters[rc * (size_t)P + p] = iters;
        if (p == P - 1) break;

        // the window moves: column block p - ms leaves the slot that column block p + W enters, row block p + W takes the slot of row block p
        const int cslot = pR - ms < 0 ? pR - ms + ring : pR - ms;              // (p - ms) mod ring = (p + W) mod ring
        if (p >= ms) leave_col(p - ms, cslot);
        __syncthreads();
        if (tid == 0 && p >= ms) {
            const int e = colerr[cslot];
            colerr[cslot] = 0;
            perr += e;
            if (pos_err) pos_err[rc * (size_t)Lc + (p - ms)] = e;
        }
        if (p + W < Lc) enter_col(p + W, cslot);
        __syncthreads();
        if (p + W < rows) enter_row(p + W, pW, cslot);
        pW = pW + 1 == W ? 0 : pW + 1;
        pR = pR + 1 == ring ? 0 : pR + 1;
    }

    {                                                          // the column blocks still resident, final with the last position
        const int first = max(P - 1 - ms, 0);
        int slot = first % ring;
        for (int i = first; i < Lc; i++) {
            leave_col(i, slot);
            slot = slot + 1 == ring ? 0 : slot + 1;
        }
        if (pre) atomicAdd(&cnt[0], pre);
        if (era) atomicAdd(&cnt[1], era);
        __syncthreads();
        if (tid == 0) {
            slot = first % ring;
            for (int i = first; i < Lc; i++) {
                const int e = colerr[slot];
                perr += e;
                if (pos_err) pos_err[rc * (size_t)Lc + i] = e;
                slot = slot + 1 == ring ? 0 : slot + 1;
            }
            int32_t *dst = out + rc * 6;
            dst[0] = total;
            dst[1] = all_ok;
            dst[2] = perr;
            dst[3] = cnt[0];
            dst[4] = cnt[1];
            dst[5] = most;
        }
    }
}

}  // namespace vaeq

extern "C" int64_t vaeq_ldpc_sc_lds_bytes(int32_t ms, int32_t mb, int32_t nb, int32_t Z, int32_t W)
{
    return vaeq::sc_dims_ok(ms, mb, nb, Z, W) ? vaeq::sc_state_bytes(ms, mb, nb, Z, W) : (int64_t)VAEQ_ERR_SHAPE;
}

extern "C" int vaeq_ldpc_sc_decode(int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0, int32_t ms, int32_t mb, int32_t nb, int32_t Z, int32_t Lc,
                                   const int32_t *components_host, const float *llr, const int8_t *bits, int32_t W, int32_t T, float alpha,
                                   int32_t iters, int32_t *out, float *post, int32_t *pos_err, int32_t *pos_iters, void *stream)
{
    using namespace vaeq;
    if (R == 0) return VAEQ_OK;                                // an empty batch owns no memory: its pointers may be NULL
    if (!components_host || !llr || !bits || !out) return VAEQ_ERR_NULL;
    if (!fec_frame_ok(R, C, N, w, t0) || iters < 1 || iters > LDPC_ITER || !sc_dims_ok(ms, mb, nb, Z, W) || Lc < 1 || Lc > SC_LC || T < 1 || T > W)
        return VAEQ_ERR_SHAPE;
    const int64_t n_chain = (int64_t)Lc * nb * Z;
    if (sc_state_bytes(ms, mb, nb, Z, W) > LDPC_STATE_MAX || !fec_fit_ok(false, C, n_chain, w, t0, N) || (int64_t)R * C > 0x7fffffff ||
        (int64_t)C * Lc > 0x7fffffff)
        return VAEQ_ERR_SHAPE;
    sc_table tab;
    if (!sc_pack(ms, mb, nb, Z, Lc, components_host, &tab)) return VAEQ_ERR_SHAPE;
    const int P = Lc + ms - W + 1 > 1 ? Lc + ms - W + 1 : 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return launch(ldpc_sc_kernel, dim3((unsigned)((int64_t)R * C)), dim3((unsigned)((Z + 63) / 64 * 64)),
                  (size_t)sc_state_bytes(ms, mb, nb, Z, W), st, tab, (int)C, (long long)N, (int)w, (long long)t0, (int)ms, (int)mb, (int)nb, (int)Z,
                  (int)Lc, (int)W, (int)T, P, llr, bits, alpha, (int)iters, out, post, pos_err, pos_iters);
}
