// vaeq_misc.hip -- what belongs to no kernel family: version / error strings, the last-launched-kernel record, the HBM copy probe.
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <stdint.h>

#include "vaeq.h"
#include "vaeq_common.h"

namespace vaeq {
static thread_local char g_last_kernel[160] = "";
void note_kernel(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_last_kernel, sizeof g_last_kernel, fmt, ap);
    va_end(ap);
}

// grid-stride 16-byte copy: the measured HBM copy bandwidth next to the spec peak
__global__ __launch_bounds__(256) void stream_copy_kernel(float4 *__restrict__ dst, const float4 *__restrict__ src, size_t n16)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) dst[i] = src[i];
}
}  // namespace vaeq

extern "C" int vaeq_last_kernel(char *buf, int32_t len)
{
    if (!buf || len <= 0) return VAEQ_ERR_NULL;
    snprintf(buf, (size_t)len, "%s", vaeq::g_last_kernel);
    return VAEQ_OK;
}

extern "C" int vaeq_stream_copy(void *dst, const void *src, int64_t bytes, void *stream)
{
    if (!dst || !src) return VAEQ_ERR_NULL;
    if (bytes < 0 || (bytes & 15) || (reinterpret_cast<uintptr_t>(dst) & 15) || (reinterpret_cast<uintptr_t>(src) & 15)) return VAEQ_ERR_SHAPE;
    if (bytes == 0) return VAEQ_OK;
    hipLaunchKernelGGL(vaeq::stream_copy_kernel, dim3(256 * 16), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<float4 *>(dst), reinterpret_cast<const float4 *>(src), (size_t)bytes / 16);
    return hipGetLastError() == hipSuccess ? VAEQ_OK : VAEQ_ERR_LAUNCH;
}

extern "C" int vaeq_version(void) { return VAEQ_VERSION; }

extern "C" const char *vaeq_strerror(int code)
{
    switch (code) {
    case VAEQ_OK: return "ok";
    case VAEQ_ERR_NULL: return "required pointer is NULL";
    case VAEQ_ERR_SHAPE: return "inconsistent or unsupported sizes";
    case VAEQ_ERR_LDS: return "per-run working set exceeds the 160 KiB LDS of a CU";
    case VAEQ_ERR_LAUNCH: return "HIP kernel launch failed";
    case VAEQ_ERR_DEVICE: return "no gfx950 device";
    }
    return "unknown vaeq error";
}
