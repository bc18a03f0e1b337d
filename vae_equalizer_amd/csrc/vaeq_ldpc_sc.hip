// vaeq_ldpc_sc.hip -- spatially coupled LDPC codes behind the demappers: the sliding-window decoders over a terminated chain of Lc positions that
// is far larger than LDS (vaeq_ldpc_sc_decode and, in fixed point, vaeq_ldpc_sc_decode_q; include/vaeq.h).  The code is a set of ms + 1
// component tables [mb][nb] of circulants; block row (t, l) of the coupled matrix holds components[t - i][l][c] in block column (i, c) for
// 0 <= t - i <= ms.  The layer update is the block decoders' (vaeq_ldpc_rule.h: layered normalized min-sum, coset decoding, in float32 or in
// fixed point), so a window that covers the whole chain gives what vaeq_ldpc_decode and vaeq_ldpc_decode_q give on the coupled table.  Unlike
// the float window decoder the fixed-point one sees the scale of the LLRs, so BER_post behind an ScLdpcCode shows what an equalizer's
// noise-variance estimate costs after FEC.  The gather and its bit map are vaeq_ldpc.h's: column block i of chain c is codeword c Lc + i of
// nb Z bits.
//
// One chain per workgroup, one thread per check of the layer in flight.  The window is a ring in LDS, the state of either arithmetic
// (vaeq_ldpc_rule.h) over (W + ms) nb Z values and W mb Z checks: column block i (L and the TX bits) lives in slot i mod (W + ms), the compressed
// state of row block t in slot t mod W.  All slot arithmetic is on wave-uniform values.  When the window moves from p to p + 1, column block p - ms is
// counted and stored, column block p + W is gathered into the slot it leaves, and row block p + W starts from zeros, with its sigma from the TX bits
// then resident, in the slot of row block p.  Nothing else is touched: the rows and columns that stay keep their state.
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
#include "vaeq_ldpc_rule.h"
#include "vaeq_ldpc_sc.h"

namespace vaeq {

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
                            te[e] = __fsub_rn(x, ldpc_signed(e == idx ? a2 : a1, sg, e));
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
                            if ((mask >> e) & 1u) L[va[e]] = __fadd_rn(te[e], ldpc_signed(e == nidx ? b2 : b1, nsg, e));
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

// The fixed-point twin of ldpc_sc_kernel, kept as a kernel of its own ("The LDPC decoders: what is shared and what is not").
// One thing differs from both parents: t_e and the address of L[v_e] share one register per edge between the minimum search and the write-back.
// |t_e| <= Lmax + Mmax < 2^15, and an index into at most 64 KiB of int16 is below 2^15.  32 registers instead of 64 bring the kernel from 178
// VGPRs to 142, from two waves per SIMD to three, for 36 instructions more in 7500 (vaeq::ldpc_sc_q_kernel).
__global__ __launch_bounds__(LDPC_Z) void ldpc_sc_q_kernel(const sc_table tab, int C, long long N, int w, long long t0, int ms, int mb, int nb,
                                                           int Z, int Lc, int W, int T, int P, const float *__restrict__ llr,
                                                           const int8_t *__restrict__ bits, const ldpc_q_rule q, int max_iter,
                                                           int32_t *__restrict__ out, int16_t *__restrict__ post, int32_t *__restrict__ pos_err,
                                                           int32_t *__restrict__ pos_iters)
{
    extern __shared__ __align__(16) unsigned char sc_q_lds[];
    __shared__ int cnt[2];                                     // pre_err, erased
    __shared__ int colerr[SC_W + SC_MS];                       // the errors of the column block that leaves a slot
    const int tid = threadIdx.x, NT = blockDim.x;
    mb = min(mb, SC_MB);
    ms = min(ms, SC_MS);
    W = min(W, SC_W);
    max_iter = min(max_iter, LDPC_ITER);
    const int nbZ = nb * Z, mZ = mb * Z, ring = W + ms, rows = Lc + ms;
    int16_t *L = reinterpret_cast<int16_t *>(sc_q_lds);
    uint8_t *B = sc_q_lds + ((2 * ring * nbZ + 3) & ~3);
    uint32_t *META = reinterpret_cast<uint32_t *>(B + ((ring * nbZ + 3) & ~3)), *SG = META + W * mZ;
    const size_t run = blockIdx.x / (unsigned)C;
    const int chain = (int)(blockIdx.x % (unsigned)C);
    const size_t rc = run * (size_t)C + chain;
    const int Mmax = q.cmax, Lmax = q.lmax, num = q.num, beta = q.beta;
    const float cmax = (float)q.cmax;
    auto norm = [&](int a) -> int { return max(((num * a + 4) >> 3) - beta, 0); };

    if (tid < 2) cnt[tid] = 0;
    for (int k = tid; k < SC_W + SC_MS; k += NT) colerr[k] = 0;
    int pre = 0, era = 0;
    auto ldL = [&](int v) -> int { return L[v]; };
    auto ldB = [&](int v) -> uint32_t { return B[v]; };

    // column block i enters its slot: the gather of codeword chain Lc + i of nb Z bits, through vaeq_ldpc_decode_q's quantiser
    auto enter_col = [&](int i, int slot) {
        const ldpc_window win = ldpc_window_of<false>(chain * Lc + i, C, w, t0, 0, nbZ);
        int16_t *Ls = L + slot * nbZ;
        uint8_t *Bs = B + slot * nbZ;
        ldpc_gather(win, run, N, w, nbZ, tid, NT, llr, bits, [&](long long j, float x, uint32_t b) {
            float y = __fmul_rn(x, q.scale);
            y = y != y ? 0.f : y;                              // a NaN is +0
            y = fminf(fmaxf(y, -cmax), cmax);
            const int Q = (int)rintf(y);                       // ties to even
            Ls[j] = (int16_t)Q;
            Bs[j] = (uint8_t)b;
            pre += (uint32_t)(x < 0.f) != b;                   // of the raw input: the float decoder's count
            era += Q == 0;
        });
    };
    // column block i leaves: its final values to post, its errors to the slot's counter
    auto leave_col = [&](int i, int slot) {
        const int16_t *Ls = L + slot * nbZ;
        const uint8_t *Bs = B + slot * nbZ;
        const size_t o = rc * (size_t)Lc * (size_t)nbZ + (size_t)i * (size_t)nbZ;
        int err = 0;
        for (int j = tid; j < nbZ; j += NT) {
            const int x = Ls[j];
            err += (int)(x < 0) != (int)Bs[j];
            if (post) post[o + j] = (int16_t)x;
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
                META[c] = par << 24;
                SG[c] = 0u;
            }
    };
    // the syndrome test of this thread's checks of the row blocks t_lo .. t_hi - 1 on the hard decisions L < 0
    auto unsatisfied = [&](int t_lo, int t_hi, int rslot, int tslot) -> int {
        uint32_t bad = 0;
        if (tid < Z)
            for (int t = t_lo; t < t_hi; t++) {
                for (int l = 0; l < mb; l++) {
                    uint32_t par = META[(rslot * mb + l) * Z + tid] >> 24;
                    sc_edges(tab.row[l], (int)(tab.wt >> (8 * l)) & 0xff, sc_mask(tab, l, t, ms, Lc), Z, tid, tslot, ring, nbZ, ldL,
                             [&](int, bool valid, int, int x) { par ^= (uint32_t)(valid && x < 0); });
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

    int lo = -Lmax, hi = Lmax;                                 // the clamp's bounds in vector registers, once: v_med3_i32 takes one scalar at most
    ldpc_pin(lo);
    ldpc_pin(hi);
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
                        int idx = (int)((meta >> 16) & 0xffu);
                        ldpc_pin(idx);                         // extracted once, not per comparison
                        const int a1 = norm((int)(meta & 0xffu)), a2 = norm((int)((meta >> 8) & 0xffu));
                        int m1 = 0x7fff, m2 = 0x7fff;          // above every Mmax
                        int nidx = 0;
                        uint32_t s = 0, S = meta >> 24;
                        uint32_t tv[LDPC_ROW];                 // t_e in the low half (|t_e| <= Lmax + Mmax < 2^15), the address of L[v_e] in the high one
                        sc_edges(tab.row[l], wt, mask, Z, tid, tslot, ring, nbZ, ldL, [&](int e, bool valid, int v, int x) {
                            // an edge that is not there takes part as a large positive value (vaeq_ldpc_rule.h, absent edges)
                            const int te = (valid ? x : 0x3fff) - ldpc_q_signed(e == idx ? a2 : a1, sg, e);
                            tv[e] = (uint32_t)v << 16 | ((uint32_t)te & 0xffffu);
                            const int a = min(abs(te), Mmax);
                            nidx = a < m1 ? e : nidx;                                  // the first edge that attains the minimum
                            m2 = ldpc_med3(m1, m2, a);                                 // m1 <= m2: the median is the second smallest of the three
                            m1 = min(m1, a);
                            const uint32_t neg = (uint32_t)(te < 0);
                            s |= neg << e;
                            S ^= neg;
                        });
                        int b1 = norm(m1), b2 = norm(m2);
                        ldpc_pin(b1);                          // or the backend moves f() behind the select below and evaluates it once per edge
                        ldpc_pin(b2);
                        const uint32_t nsg = S ? ~s : s;       // the new message of edge e is negative iff S ^ s_e
#pragma unroll
                        for (int e = 0; e < LDPC_ROW; e++)     // t and the addresses are still in registers: no second read of L
                            if ((mask >> e) & 1u)
                                L[tv[e] >> 16] = (int16_t)ldpc_med3((int)(int16_t)tv[e] + ldpc_q_signed(e == nidx ? b2 : b1, nsg, e), lo, hi);
                        META[c] = (meta & 0xff000000u) | (uint32_t)nidx << 16 | (uint32_t)m2 << 8 | (uint32_t)m1;
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

// What the two entry points share.  bytes: the arithmetic's state size (vaeq_ldpc_rule.h); rule_ok: its own rules, behind the fit rule and
// ahead of the table's; go(tab, grid, block, lds, P) launches.
template <class Launch>
static int sc_decode_any(int64_t (*bytes)(int64_t, int64_t), int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0, int32_t ms, int32_t mb,
                         int32_t nb, int32_t Z, int32_t Lc, const int32_t *components_host, const void *llr, const void *bits, int32_t W, int32_t T,
                         int32_t iters, const void *out, bool rule_ok, Launch &&go)
{
    if (R == 0) return VAEQ_OK;                                // an empty batch owns no memory: its pointers may be NULL
    if (!components_host || !llr || !bits || !out) return VAEQ_ERR_NULL;
    if (!sc_shape_ok(R, C, N, w, t0, ms, mb, nb, Z, Lc, W, T, iters, bytes) || !rule_ok) return VAEQ_ERR_SHAPE;
    sc_table tab;
    if (!sc_pack(ms, mb, nb, Z, Lc, components_host, &tab)) return VAEQ_ERR_SHAPE;
    const int P = Lc + ms - W + 1 > 1 ? Lc + ms - W + 1 : 1;
    return go(tab, dim3((unsigned)((int64_t)R * C)), dim3((unsigned)((Z + 63) / 64 * 64)), (size_t)sc_ring_bytes(bytes, ms, mb, nb, Z, W), P);
}

}  // namespace vaeq

extern "C" int64_t vaeq_ldpc_sc_lds_bytes(int32_t ms, int32_t mb, int32_t nb, int32_t Z, int32_t W)
{
    return vaeq::sc_dims_ok(ms, mb, nb, Z, W) ? vaeq::sc_ring_bytes(vaeq::ldpc_float_bytes, ms, mb, nb, Z, W) : (int64_t)VAEQ_ERR_SHAPE;
}

extern "C" int64_t vaeq_ldpc_sc_q_lds_bytes(int32_t ms, int32_t mb, int32_t nb, int32_t Z, int32_t W)
{
    return vaeq::sc_dims_ok(ms, mb, nb, Z, W) ? vaeq::sc_ring_bytes(vaeq::ldpc_fixed_bytes, ms, mb, nb, Z, W) : (int64_t)VAEQ_ERR_SHAPE;
}

extern "C" int vaeq_ldpc_sc_decode(int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0, int32_t ms, int32_t mb, int32_t nb, int32_t Z, int32_t Lc,
                                   const int32_t *components_host, const float *llr, const int8_t *bits, int32_t W, int32_t T, float alpha,
                                   int32_t iters, int32_t *out, float *post, int32_t *pos_err, int32_t *pos_iters, void *stream)
{
    using namespace vaeq;
    return sc_decode_any(ldpc_float_bytes, R, C, N, w, t0, ms, mb, nb, Z, Lc, components_host, llr, bits, W, T, iters, out, true,
                                     [&](const sc_table &tab, dim3 grid, dim3 block, size_t lds, int P) {
        return launch(ldpc_sc_kernel, grid, block, lds, reinterpret_cast<hipStream_t>(stream), tab, (int)C, (long long)N, (int)w, (long long)t0, (int)ms,
                      (int)mb, (int)nb, (int)Z, (int)Lc, (int)W, (int)T, P, llr, bits, alpha, (int)iters, out, post, pos_err, pos_iters);
    });
}

extern "C" int vaeq_ldpc_sc_decode_q(int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0, int32_t ms, int32_t mb, int32_t nb, int32_t Z, int32_t Lc,
                                     const int32_t *components_host, const float *llr, const int8_t *bits, int32_t W, int32_t T, int32_t qbits,
                                     int32_t abits, float scale, int32_t num, int32_t beta, int32_t iters, int32_t *out, int16_t *post,
                                     int32_t *pos_err, int32_t *pos_iters, void *stream)
{
    using namespace vaeq;
    return sc_decode_any(ldpc_fixed_bytes, R, C, N, w, t0, ms, mb, nb, Z, Lc, components_host, llr, bits, W, T, iters, out,
                                           ldpc_q_rule_ok(qbits, abits, scale, num, beta),
                                           [&](const sc_table &tab, dim3 grid, dim3 block, size_t lds, int P) {
        return launch(ldpc_sc_q_kernel, grid, block, lds, reinterpret_cast<hipStream_t>(stream), tab, (int)C, (long long)N, (int)w, (long long)t0,
                      (int)ms, (int)mb, (int)nb, (int)Z, (int)Lc, (int)W, (int)T, P, llr, bits, ldpc_q_rule_of(qbits, abits, scale, num, beta), (int)iters,
                      out, post, pos_err, pos_iters);
    });
}
