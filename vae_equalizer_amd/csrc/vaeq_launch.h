// vaeq_launch.h -- host side of the extern "C" entry points: shape predicates, the n_lev dispatch and the kernel launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "vaeq.h"

namespace vaeq {

// A CU of gfx950 has 160 KiB of LDS.  A kernel whose only LDS is its dynamic block may ask for all of it; one that also owns static
// __shared__ arrays (taps, window sums, reduction scratch: a few KiB) has to leave them room, so its dynamic block is held to 150 KiB.
constexpr size_t LDS_MAX = 160 * 1024;
constexpr size_t LDS_MAX_BESIDE_STATIC = 150 * 1024;
// Dynamic LDS above this needs hipFuncAttributeMaxDynamicSharedMemorySize raised first; raising it for a request that would have fitted anyway is harmless.
constexpr size_t LDS_RAISE_ABOVE = 32 * 1024;

// an odd FIR of at most 63 taps at a positive oversampling
inline bool fir_shape_ok(int64_t sps, int64_t M) { return sps > 0 && M > 0 && (M & 1) == 1 && M <= 63; }

// ... and a minibatch of B symbols that is longer than the FIR (loss family: the residual keeps B * sps - 2 (M / 2) samples)
inline bool loss_shape_ok(int64_t B, int64_t sps, int64_t M)
{
    return B > 0 && fir_shape_ok(sps, M) && B * sps - 2 * (M / 2) > 0 && B > 2 * (M / 2);
}

// a batch of AWGN validation frames of N symbols (vaeq_awgn_info, vaeq_awgn_llr): indices in int32 with room for a shift
inline bool awgn_frame_shape_ok(int32_t R, int64_t N) { return R >= 0 && N >= 1 && N <= 0x3fffffff; }

// ... and of soft sequences of Nz samples against Nd TX symbols (vaeq_awgn_track_info, vaeq_awgn_track_llr): the LMMSE output is one sample longer
inline bool track_shape_ok(int32_t R, int64_t Nz, int64_t Nd, int32_t edge, int32_t interleaved)
{
    return awgn_frame_shape_ok(R, Nz) && Nd >= 1 && (Nz == Nd || Nz == Nd + 1) && edge >= 0 && (interleaved == 0 || interleaved == 1);
}

// f(std::integral_constant<int, n_lev>{}) for the three supported level counts (4-/16-/64-QAM), VAEQ_ERR_SHAPE otherwise; the result has f's type
// (int for a launch, int64_t for an occupancy query)
template <class F>
inline auto dispatch_nlev(int n_lev, F &&f) -> decltype(f(std::integral_constant<int, 2>{}))
{
    switch (n_lev) {
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    }
    return VAEQ_ERR_SHAPE;
}

// Launch `kernel` with lds_bytes of dynamic LDS: VAEQ_ERR_LDS when the device refuses that much, VAEQ_ERR_LAUNCH when the launch fails.
template <class... Params, class... Args>
inline int launch(void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, Args... args)
{
    if (lds_bytes > LDS_RAISE_ABOVE &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess)
        return VAEQ_ERR_LDS;
    hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, args...);
    return hipGetLastError() == hipSuccess ? VAEQ_OK : VAEQ_ERR_LAUNCH;
}

}  // namespace vaeq
