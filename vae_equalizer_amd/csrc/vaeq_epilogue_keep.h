// vaeq_epilogue_keep.h -- which symbols of a frame the per-frame epilogues keep: the per-minibatch cut and the frame-edge slice of
// func_VAELE_DP_MQAM_shaping.py:73-79 (batch_len > 0) resp. func_VAEflex_DP_MQAM_shaping.py:72-84 (batch_len = 0) as index arithmetic.
// Shared by vaeq_epilogue.hip (SER), vaeq_epilogue_info.hip (GMI / achievable rate / BER) and vaeq_epilogue_llr.hip: all see exactly the same window.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vaeq {

constexpr int EPI_NT = 256, N_SHIFT = 21, HALF_SHIFT = 10, N_CUT = 10, EDGE = 11;

// the frames the information-rate and LLR entry points of the DP and CMA epilogues take: long enough for both edges and the shift search, indices
// in int32, and whole minibatches where there is a per-minibatch cut (the CMA frames have none: batch_len = 0)
inline bool epi_frame_shape_ok(int32_t R, int64_t N, int32_t batch_len)
{
    return R >= 0 && N >= 2 * EDGE + N_SHIFT && N <= 0x3fffffff && batch_len >= 0 && (batch_len == 0 || N % batch_len == 0);
}

// symbols kept of every minibatch by the reference's slice [: batch_len - shift[0] - 10] (:73-77), with Python's slice semantics: an end past the
// minibatch keeps all of it, an end of 0 keeps nothing, and a NEGATIVE end e (batch_len < shift[0] + 10, so only for batch_len < 20) counts from the
// minibatch's end and keeps batch_len + e symbols (none when that is negative, too)
__device__ __forceinline__ int epi_lk(int batch_len, int shift0)
{
    const int e = batch_len - shift0 - N_CUT;
    return e < 0 ? max(batch_len + e, 0) : min(e, batch_len);
}

// symbols that survive the per-minibatch cut (:73-77) and the frame-edge slice (:79)
__device__ __forceinline__ bool epi_keep(int n, int N, int batch_len, int shift0, int ms)
{
    if (batch_len <= 0) return n >= EDGE && n < N - EDGE - ms;
    const int Lk = epi_lk(batch_len, shift0);
    const int mb = n / batch_len, j = n - mb * batch_len, k = mb * Lk + j, K = (N / batch_len) * Lk;
    return j < Lk && k >= EDGE && k < K - EDGE - ms;
}

// epi_keep for the symbols n = tid, tid + 256, ... of one thread without an integer division per symbol: (minibatch, offset) advance by
// (256 / batch_len, 256 % batch_len) with one carry
struct KeepWalk {
    int N, batch_len, ms, Lk, K, mb, j, dq, dr;
    __device__ __forceinline__ KeepWalk(int n0, int N_, int batch_len_, int shift0, int ms_) : N(N_), batch_len(batch_len_), ms(ms_)
    {
        Lk = K = mb = j = dq = dr = 0;
        if (batch_len > 0) {
            Lk = epi_lk(batch_len, shift0);
            K = (N / batch_len) * Lk;
            mb = n0 / batch_len; j = n0 - mb * batch_len;
            dq = EPI_NT / batch_len; dr = EPI_NT - dq * batch_len;
        }
    }
    __device__ __forceinline__ bool keep(int n) const
    {
        if (batch_len <= 0) return n >= EDGE && n < N - EDGE - ms;
        const int k = mb * Lk + j;
        return j < Lk && k >= EDGE && k < K - EDGE - ms;
    }
    __device__ __forceinline__ void next()
    {
        mb += dq; j += dr;
        if (j >= batch_len) { j -= batch_len; mb++; }
    }
};

}  // namespace vaeq
