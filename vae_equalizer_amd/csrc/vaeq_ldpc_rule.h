// vaeq_ldpc_rule.h -- what the two arithmetics of the layered min-sum decoders are made of, for the block kernels (vaeq_ldpc.hip) and the window
// kernels (vaeq_ldpc_sc.hip) alike: the float sign flip; the integer rule with its median of three, its conditional negation and the host's
// check of it; the size of each arithmetic's state in LDS, which the four *_lds_bytes exports and the five entry points call; and the argument
// about absent edges in the integer update, in the form that covers every row of either shape.
// The kernels themselves are written out four times ("The LDPC decoders: what is shared and what is not", says what
// was tried and measured): every form that shared a body or the layer update between them changed their instruction streams and cost time.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "vaeq_ldpc.h"

namespace vaeq {

// x with its sign flipped when bit e of sg is set (an exact negation, of zero too)
__device__ __forceinline__ float ldpc_signed(float x, uint32_t sg, int e) { return __uint_as_float(__float_as_uint(x) ^ ((sg >> e) << 31)); }

// the median of three: the clamp to [lo, hi] of x, and the second smallest of (m1, m2, a) when m1 <= m2
__device__ __forceinline__ int ldpc_med3(int a, int b, int c)
{
    int r;
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// x negated when bit e of sg is set
__device__ __forceinline__ int ldpc_q_signed(int x, uint32_t sg, int e)
{
    const int mask = -(int)((sg >> e) & 1u);
    return (x ^ mask) - mask;
}

struct ldpc_q_rule {
    float scale;
    int cmax, lmax, num, beta;                                 // Cmax = Mmax = 2^(qbits-1) - 1, Lmax = 2^(abits-1) - 1
};

// the quantiser's rules of vaeq_ldpc_decode_q and vaeq_ldpc_sc_decode_q (include/vaeq.h)
inline bool ldpc_q_rule_ok(int64_t qbits, int64_t abits, float scale, int64_t num, int64_t beta)
{
    return !(qbits < 2 || qbits > 8 || abits < qbits || abits > 15 || !(scale > 0.f) || !isfinite(scale) || num < 1 || num > 8 || beta < 0 || beta > 127);
}

inline ldpc_q_rule ldpc_q_rule_of(int qbits, int abits, float scale, int num, int beta)
{
    return {scale, (1 << (qbits - 1)) - 1, (1 << (abits - 1)) - 1, num, beta};
}

// The float32 state: L[n_values] f32, the TX bits [n_values] as bytes, and per check the compressed message (m1, m2, idx | sigma << 8, signs),
// 16 bytes, as four arrays so that consecutive checks touch consecutive banks.  A block code has n values and m checks, a window
// (W + ms) nb Z and W mb Z.
static inline int64_t ldpc_float_bytes(int64_t n_values, int64_t n_checks) { return 4 * n_values + ((n_values + 3) & ~(int64_t)3) + 16 * n_checks; }

// The fixed-point state: L[n_values] as int16, the TX bits [n_values] as bytes (each array padded to a word), and per check two dwords --
// m1 | m2 << 8 | idx << 16 | sigma << 24, and the signs: 3 n + 8 m bytes against the float state's 5 n + 16 m.  A 16-bit store touches its own
// two bytes alone, so the checks of a layer, which own disjoint variables, still need no barrier between them.
static inline int64_t ldpc_fixed_bytes(int64_t n_values, int64_t n_checks)
{
    return ((2 * n_values + 3) & ~(int64_t)3) + ((n_values + 3) & ~(int64_t)3) + 8 * n_checks;
}

// Absent edges in the integer layer update (ldpc_q_kernel, ldpc_sc_q_kernel).  An edge that is not there (past wt, or outside the chain) takes part as
// a large positive value: whatever its stale sign bit says, t_e >= 0x3fff - f(Mmax) > 0 and a_e = Mmax, so it adds no sign.  Every row has two or more
// real edges (ldpc_pack, sc_pack), each with a_e <= Mmax, so at the end m1 and m2 are the two smallest of the real a_e: an extra Mmax lowers
// neither.  Where the absent edges come behind the real ones (a block code's rows, the tail rows of a chain) they never take nidx either: the first
// real edge has brought m1 to Mmax or below, and an equal value is not "first".  In a head row of a chain (t < ms) the absent edges come first
// instead, and one of them may take nidx.  A real edge with a_e < Mmax behind it takes nidx over (a < m1), the first such one, as specified.  When
// every real a_e equals Mmax, nidx stays on the absent edge: then m1 = m2 = Mmax, every real edge receives f(Mmax) whichever edge idx names, now and
// when this state is read back, so L, the signs and (m1, m2) are the specified ones and idx, which leaves the kernel nowhere, is the only value that
// differs from the specification's.

}  // namespace vaeq
