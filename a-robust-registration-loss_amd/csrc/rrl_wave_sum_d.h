// rrl_wave_sum_d.h -- the deterministic double sum over a wavefront, shared by the units whose sums are fixed-order double
// sums of float32 terms (rrl_newton.hip: the normal equations; rrl_kabsch.hip: the moments of the closed-form fit).
#pragma once

// sum over the 64 lanes of a double, valid in every lane: wave_sum's DPP sequence (rrl_common.h) on both halves of the value
// -- a fixed association, deterministic
__device__ __forceinline__ double wave_sum_d(double v) {
#define RRL_DPP_ADD_D(ctrl, rm)                                                                             \
    {                                                                                                       \
        const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), ctrl, rm, 0xf, false);             \
        const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), ctrl, rm, 0xf, false);             \
        v += __hiloint2double(hi, lo);                                                                      \
    }
    RRL_DPP_ADD_D(0x111, 0xf) RRL_DPP_ADD_D(0x112, 0xf) RRL_DPP_ADD_D(0x114, 0xf) RRL_DPP_ADD_D(0x118, 0xf)
    RRL_DPP_ADD_D(0x142, 0xa) RRL_DPP_ADD_D(0x143, 0xc)
#undef RRL_DPP_ADD_D
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}
