// vaeq_info.h -- the small helpers the information-rate kernels share (vaeq_epilogue_info.hip: a DP frame; vaeq_awgn_info.hip: an AWGN
// validation frame): the Gray label of a level, the floored log2 of a stored posterior, an integer wave sum and a register-array pick.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>

namespace vaeq {

__device__ __forceinline__ int info_gray(int i) { return i ^ (i >> 1); }
__device__ __forceinline__ float info_log2(float x) { return __log2f(fmaxf(x, FLT_MIN)); }       // l(x) of q-mode: an exact 0 costs 126 bit, not infinity
__device__ __forceinline__ int info_wave_sum(int v)
{
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
template <int NL>
__device__ __forceinline__ float info_pick(const float (&v)[NL], int l)     // v[l] without a register array indexed at run time
{
    float r = v[0];
#pragma unroll
    for (int i = 1; i < NL; i++) r = l == i ? v[i] : r;
    return r;
}

}  // namespace vaeq
