// vaeq_ldpc_sc.h -- what belongs to a spatially coupled chain (vaeq_ldpc_sc.hip), whichever arithmetic decodes it: the envelope, the host's
// shape rules, the table as it travels in the kernel arguments, the packer, the mask of the edges a truncated row really has and the edge
// walker over the ring of column blocks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "vaeq_ldpc.h"

namespace vaeq {

constexpr int SC_MS = 7, SC_MB = 4, SC_NB = 32, SC_W = 32, SC_LC = 65535;

struct sc_table {
    uint4 row[SC_MB][LDPC_ROW / 4];                            // edge e of row l: dword e
    uint32_t le[SC_MB][SC_MS + 1];                             // bit e: edge e has d <= k
    uint32_t ge[SC_MB][SC_MS + 1];                             // bit e: edge e has d >= k
    uint32_t wt;                                               // byte l: the edges of a full row l
};
static_assert(sizeof(sc_table) <= 1024, "the table travels in the kernel arguments");

inline bool sc_dims_ok(int64_t ms, int64_t mb, int64_t nb, int64_t Z, int64_t W)
{
    return ms >= 1 && ms <= SC_MS && mb >= 1 && mb <= SC_MB && nb >= 2 && nb <= SC_NB && Z >= 2 && Z <= LDPC_Z && W >= ms + 1 && W <= SC_W;
}

// the edges row block (t, l) really has, as a mask over the edges of a full row: 0 <= t - d < Lc
__device__ __forceinline__ uint32_t sc_mask(const sc_table &tab, int l, int t, int ms, int Lc)
{
    return tab.le[l][min(t, ms)] & tab.ge[l][min(max(t - Lc + 1, 0), ms)];
}

// ldpc_edges for row block t of the chain: f(e, valid, v, x) for the edges of check i, eight at a time with their reads in flight together.
// tslot = t mod ring; the column block of an edge with offset d is in slot (t - d) mod ring, a wave-uniform value.  An edge that does not exist
// (past wt, or outside the chain: valid = false, wave-uniform) reads an address inside L and f must leave no trace of it.
template <class LD, class F>
__device__ __forceinline__ void sc_edges(const uint4 *row, int wt, uint32_t mask, int Z, int i, int tslot, int ring, int nbZ, LD &&ld, F &&f)
{
#pragma unroll
    for (int g = 0; g < LDPC_ROW / 8; g++) {
        if (8 * g >= wt) break;
        const uint4 pa = row[2 * g], pb = row[2 * g + 1];
        const uint32_t h[8] = {pa.x, pa.y, pa.z, pa.w, pb.x, pb.y, pb.z, pb.w};
        int v[8];
        decltype(ld(0)) x[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint32_t j = (uint32_t)i + (h[k] & 511u);    // (i + s) mod Z: j - Z wraps past j exactly when j < Z
            int slot = tslot - (int)(h[k] >> 23);
            slot += slot < 0 ? ring : 0;
            v[k] = slot * nbZ + (int)((h[k] >> 9) & 0x3fffu) + (int)min(j, j - (uint32_t)Z);
        }
#pragma unroll
        for (int k = 0; k < 8; k++) x[k] = ld(v[k]);
#pragma unroll
        for (int k = 0; k < 8; k++) ldpc_pin(x[k]);
#pragma unroll
        for (int k = 0; k < 8; k++) f(8 * g + k, (bool)((mask >> (8 * g + k)) & 1u), v[k], x[k]);
    }
}

// components[ms + 1][mb][nb] -> the kernel's table; false when the table leaves the envelope: a shift outside -1 .. Z - 1, more than 32 non-zero
// blocks in a full row, or a block row (t, l) of the coupled matrix, truncated ones included, with fewer than 2
static inline bool sc_pack(int ms, int mb, int nb, int Z, int Lc, const int32_t *comp, sc_table *tab)
{
    uint32_t d[SC_MB][LDPC_ROW] = {};
    memset(tab, 0, sizeof(*tab));
    for (int l = 0; l < mb; l++) {
        int wt = 0;
        for (int dd = ms; dd >= 0; dd--)
            for (int c = 0; c < nb; c++) {
                const int32_t s = comp[(dd * mb + l) * nb + c];
                if (s < -1 || s >= Z) return false;
                if (s < 0) continue;
                if (wt == LDPC_ROW) return false;
                d[l][wt] = (uint32_t)dd << 23 | (uint32_t)(c * Z) << 9 | (uint32_t)s;
                for (int k = 0; k <= SC_MS; k++) {
                    if (dd <= k) tab->le[l][k] |= 1u << wt;
                    if (dd >= k) tab->ge[l][k] |= 1u << wt;
                }
                wt++;
            }
        tab->wt |= (uint32_t)wt << (8 * l);
        for (int k = 0; k < LDPC_ROW / 4; k++) tab->row[l][k] = make_uint4(d[l][4 * k], d[l][4 * k + 1], d[l][4 * k + 2], d[l][4 * k + 3]);
    }
    for (int l = 0; l < mb; l++)
        for (int t = 0; t < Lc + ms; t++) {
            if (t == ms && Lc - 1 > ms) t = Lc - 1;            // the full rows ms .. Lc - 1 are all alike
            const int lo = t - Lc + 1 < 0 ? 0 : t - Lc + 1, hi = t < ms ? t : ms;
            if (__builtin_popcount(tab->le[l][hi] & tab->ge[l][lo > ms ? ms : lo]) < 2) return false;
        }
    return true;
}

// the ring of a window in bytes: bytes(n_values, n_checks) is the arithmetic's state size (vaeq_ldpc_rule.h); call it behind sc_dims_ok
static inline int64_t sc_ring_bytes(int64_t (*bytes)(int64_t, int64_t), int64_t ms, int64_t mb, int64_t nb, int64_t Z, int64_t W)
{
    return bytes((W + ms) * nb * Z, W * mb * Z);
}

// The shape rules the two window decoders share, behind the empty batch and the NULL pointers: the frame rule of vaeq_fec.h and the chain's
// own, then the state, the fit of C chains of Lc nb Z bits each, bit-packed, and the index ranges.
static inline bool sc_shape_ok(int64_t R, int64_t C, int64_t N, int64_t w, int64_t t0, int64_t ms, int64_t mb, int64_t nb, int64_t Z, int64_t Lc,
                               int64_t W, int64_t T, int64_t iters, int64_t (*bytes)(int64_t, int64_t))
{
    if (!fec_frame_ok(R, C, N, w, t0) || iters < 1 || iters > LDPC_ITER || !sc_dims_ok(ms, mb, nb, Z, W) || Lc < 1 || Lc > SC_LC || T < 1 || T > W)
        return false;
    return sc_ring_bytes(bytes, ms, mb, nb, Z, W) <= LDPC_STATE_MAX && fec_fit_ok(false, C, Lc * nb * Z, w, t0, N) && R * C <= 0x7fffffff &&
           C * Lc <= 0x7fffffff;
}

}  // namespace vaeq
