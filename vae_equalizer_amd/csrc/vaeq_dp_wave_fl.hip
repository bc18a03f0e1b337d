// vaeq_dp_wave_fl.hip -- M = 25, multi-wave shapes of the wave-per-run DP kernel (vaeq_dp_wave_kernel.h) on FIXED LDS layouts (template parameter BL):
// two wavefronts per run on the layout of B = 256 for 128 < B <= 256, four on that of 512 for B <= 512, eight on that of 1024 for B <= 1024 (B = 200 / 400
// stay baked, vaeq_dp_wave_mw.hip).  Offsets and row strides are immediate, the tap loops pipelined; B itself stays a run-time value.
// The layouts fit the residency the register file allows anyway (2 waves per SIMD): 4 x 35 KB, 2 x 66 KB, 1 x 130 KB per CU.
#include "vaeq_dp_wave_kernel.h"

namespace vaeq {

int launch_dp_wave_fl(const vaeq_dp_args &a, hipStream_t st)
{
    return a.B <= 256 ? launch_wave_fixl_lev<25, 256, 2, true>(a, st) : a.B <= 512 ? launch_wave_fixl_lev<25, 512, 4, true>(a, st) : launch_wave_fixl_lev<25, 1024, 8, true>(a, st);
}
int64_t dp_wave_fl_resident(int B, int n_lev) { return B <= 256 ? wave_resident_fixl_lev<25, 256, 2>(n_lev) : B <= 512 ? wave_resident_fixl_lev<25, 512, 4>(n_lev) : wave_resident_fixl_lev<25, 1024, 8>(n_lev); }

}  // namespace vaeq
