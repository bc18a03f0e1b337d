// vaeq_ldpc.h -- what belongs to a quasi-cyclic block code (vaeq_ldpc.hip), whichever arithmetic decodes it (vaeq_ldpc_rule.h): the envelope, the
// table of shifts as it travels in the kernel arguments, its packer, the edge walker of a check and the gather of a codeword from the frame
// (both forms; the window decoders and the outer BCH decoder use the gather's map too).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vaeq_fec.h"

namespace vaeq {

constexpr int LDPC_MB = 8, LDPC_NB = 64, LDPC_ROW = 32, LDPC_Z = 512, LDPC_ITER = 100, LDPC_W = FEC_W;
constexpr int64_t LDPC_STATE_MAX = 64 * 1024;

// Row l: edges e < wt[l] in ascending block column, two per dword, edge e in bits 16 (e & 1) .. of dword e / 2 as column << 9 | shift.
struct ldpc_table {
    uint4 row[LDPC_MB][LDPC_ROW / 8];
    uint64_t wt;                                               // byte l: the edges of row l
};
static_assert(sizeof(ldpc_table) <= 1024, "the table travels in the kernel arguments");

// A loaded value stays where it is: without this the backend sinks each read into the branch that uses it, and every read waits alone.
__device__ __forceinline__ void ldpc_pin(float &x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ void ldpc_pin(uint32_t &x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ void ldpc_pin(int &x) { asm volatile("" : "+v"(x)); }

// f(e, valid, v, x) for the edges of check i of a layer, eight at a time: v the variable of edge e, x = ld(v), all eight reads in flight
// before the first use.  The four groups are unrolled, so e is a constant in f and arrays indexed by it stay in registers.  The last group of a
// row may hold edges past wt (valid = false, wave-uniform): their table entry is 0, so they read variable i, an address inside L, and f must
// leave no trace of them.
template <class LD, class F>
__device__ __forceinline__ void ldpc_edges(const uint4 *row, int wt, int Z, int i, LD &&ld, F &&f)
{
#pragma unroll
    for (int g = 0; g < LDPC_ROW / 8; g++) {
        if (8 * g >= wt) break;
        const uint4 pk = row[g];
        const uint32_t d[4] = {pk.x, pk.y, pk.z, pk.w};
        int v[8];
        decltype(ld(0)) x[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint32_t h = (d[k >> 1] >> (16 * (k & 1))) & 0xffffu;
            const uint32_t j = (uint32_t)i + (h & 511u);       // (i + s) mod Z: j - Z wraps past j exactly when j < Z
            v[k] = (int)((h >> 9) * (uint32_t)Z + min(j, j - (uint32_t)Z));
        }
#pragma unroll
        for (int k = 0; k < 8; k++) x[k] = ld(v[k]);
#pragma unroll
        for (int k = 0; k < 8; k++) ldpc_pin(x[k]);
#pragma unroll
        for (int k = 0; k < 8; k++) f(8 * g + k, 8 * g + k < wt, v[k], x[k]);
    }
}

// f(j, x, b) for every bit j of codeword cw of a run: x its LLR, b its TX bit, each exactly once, four planes of a symbol at a time with their
// loads in flight together.  IL: the symbol interleaver of vaeq_ldpc_decode_il over groups of `depth` codewords (include/vaeq.h); false:
// vaeq_ldpc_decode's bit-packed contiguous codewords, `depth` unused.
// Contiguous: bit j of this codeword is global bit g = cw n + j of the run: symbol t0 + g / w, plane g % w.  Consecutive lanes on consecutive
// symbols of one plane.  Interleaved: symbol u of the codeword is symbol base + u D + d of the frame, its plane p is bit u w + p; consecutive
// lanes on consecutive u, D symbols apart -- the D workgroups of a group have adjacent block indices and read the same lines between them,
// and L2 hides it: +0.36 ms on 6.68 ms where the call is almost all gather (lanes on consecutive frame symbols, each keeping its
// own residue, run the loop body D times as often and take 28.6 ms).
struct ldpc_window {
    long long first, j_lo;                                     // the frame's symbol and the codeword's bit (of plane 0) at s = 0
    int nsym, step;
};

template <bool IL>
__device__ __forceinline__ ldpc_window ldpc_window_of(int cw, int C, int w, long long t0, int depth, int n)
{
    const long long g0 = (long long)cw * n;
    long long first, j_lo;
    int nsym, step;
    if constexpr (IL) {
        const int S = (n + w - 1) / w, k0 = cw / depth * depth;
        step = min(depth, C - k0);
        first = t0 + (long long)k0 * S + (cw - k0);
        j_lo = 0;
        nsym = S;
    } else {
        const long long s_lo = g0 / w;
        step = 1;
        first = t0 + s_lo;
        j_lo = s_lo * w - g0;
        nsym = (int)((g0 + n - 1) / w - s_lo) + 1;
    }
    return {first, j_lo, nsym, step};
}

template <class F>
__device__ __forceinline__ void ldpc_gather(const ldpc_window win, size_t run, long long N, int w, int n, int tid, int NT,
                                            const float *__restrict__ llr, const int8_t *__restrict__ bits, F &&f)
{
    const long long first = win.first, j_lo = win.j_lo;
    const int nsym = win.nsym, step = win.step;
    for (int s = tid; s < nsym; s += NT) {
        const size_t sym = (size_t)first + (size_t)s * (size_t)step;
        for (int p0 = 0; p0 < w; p0 += 4) {
            float x[4];
            uint32_t b[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const size_t at = (run * (size_t)w + min(p0 + k, w - 1)) * (size_t)N + sym;
                x[k] = llr[at];
                b[k] = (uint32_t)bits[at] & 1u;
            }
#pragma unroll
            for (int k = 0; k < 4; k++) { ldpc_pin(x[k]); ldpc_pin(b[k]); }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const long long j = j_lo + (long long)s * w + (p0 + k);
                if (p0 + k < w && j >= 0 && j < n) f(j, x[k], b[k]);
            }
        }
    }
}

// The same map for one bit (vaeq_bch.hip, which visits the payload bits of a codeword in its own order): where bit j of codeword cw lies in a
// run's [w][N] tensors, as ldpc_window_of and ldpc_gather above walk it.  I, the type of every index and of the result: uint32_t where C n < 2^31
// and w N < 2^32 (no 64-bit multiply per bit), else uint64_t.
template <bool IL, class I>
__device__ __forceinline__ I ldpc_bit_at(I cw, uint32_t j, int C, int w, long long N, long long t0, int depth, int n)
{
    if constexpr (IL) {
        const uint32_t S = ((uint32_t)n + (uint32_t)w - 1u) / (uint32_t)w, u = j / (uint32_t)w;
        const I k0 = cw / (I)depth * (I)depth;
        const I D = (I)C - k0 < (I)depth ? (I)C - k0 : (I)depth;
        return (I)(j - u * (uint32_t)w) * (I)N + (I)t0 + k0 * (I)S + (I)u * D + (cw - k0);
    } else {
        const I g = cw * (I)n + (I)j, s = g / (I)w;
        return (g - s * (I)w) * (I)N + (I)t0 + s;
    }
}

// shifts[mb][nb] -> the kernel's table; false when the table leaves the envelope
static inline bool ldpc_pack(int mb, int nb, int Z, const int32_t *shifts, ldpc_table *tab)
{
    uint32_t d[LDPC_MB][LDPC_ROW / 2] = {};
    tab->wt = 0;
    for (int l = 0; l < mb; l++) {
        int wt = 0;
        for (int c = 0; c < nb; c++) {
            const int32_t s = shifts[l * nb + c];
            if (s < -1 || s >= Z) return false;
            if (s < 0) continue;
            if (wt == LDPC_ROW) return false;
            d[l][wt >> 1] |= ((uint32_t)c << 9 | (uint32_t)s) << (16 * (wt & 1));
            wt++;
        }
        if (wt < 2) return false;
        tab->wt |= (uint64_t)wt << (8 * l);
    }
    for (int l = 0; l < LDPC_MB; l++) {
        for (int k = 0; k < LDPC_ROW / 8; k++) tab->row[l][k] = make_uint4(d[l][4 * k], d[l][4 * k + 1], d[l][4 * k + 2], d[l][4 * k + 3]);
    }
    return true;
}

static inline bool ldpc_dims_ok(int64_t mb, int64_t nb, int64_t Z)
{
    return mb >= 1 && mb <= LDPC_MB && nb >= 2 && nb <= LDPC_NB && Z >= 2 && Z <= LDPC_Z;
}

// The shape rules the block decoders share, behind the empty batch and the NULL pointers: the frame and fit rules of vaeq_fec.h (il = the
// interleaver's); lds = the state of a codeword in bytes.
static inline bool ldpc_shape_ok(int64_t R, int64_t C, int64_t N, int64_t w, int64_t t0, int64_t depth, int64_t mb, int64_t nb, int64_t Z,
                                 int64_t max_iter, int64_t lds, bool il)
{
    if (!fec_frame_ok(R, C, N, w, t0) || max_iter < 1 || max_iter > LDPC_ITER || !ldpc_dims_ok(mb, nb, Z) || (il && (depth < 1 || depth > C)))
        return false;
    return lds <= LDPC_STATE_MAX && fec_fit_ok(il, C, nb * Z, w, t0, N) && R * C <= 0x7fffffff;
}

}  // namespace vaeq
