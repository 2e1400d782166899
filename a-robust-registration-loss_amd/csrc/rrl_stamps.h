// rrl_stamps.h -- in-kernel time stamps of the stages behind the scan (the rrl_stage_*.h kernels; tools/stamps*.py read them
// through rrl_sparse.hip's rrl_debug_*stamps entries).  Default builds: the macros are empty.  Experiments only
// (RRL_HIPCC_FLAGS=-DRRL_STAMPS -> lib_exp): 100 MHz time stamps, and this header then DEFINES the device tables -- it is
// included by rrl_sparse.hip's translation unit only.
#pragma once
#include "rrl_common.h"

#ifdef RRL_STAMPS
__device__ unsigned long long g_stamps[32];  // workgroup 0's lane 0
#define STAMP(i) do { if (threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) g_stamps[i] = wall_clock64(); } while (0)
__device__ unsigned long long g_wstamps[12 * 2048];  // [stamp][workgroup]: per-workgroup stamps of the tail kernel
#define STAMPW(i) do { if ((threadIdx.x & 63) == 0) { const unsigned wg_ = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z); \
    if (wg_ < 2048u) g_wstamps[(i) * 2048 + wg_] = wall_clock64(); } } while (0)
__device__ unsigned long long g_pstamps[8 * 2048];  // ... of the per-line stage
#define STAMPP(i) do { if ((threadIdx.x & 63) == 0) { const unsigned wg_ = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z); \
    if (wg_ < 2048u) g_pstamps[(i) * 2048 + wg_] = wall_clock64(); } } while (0)
#define STAMPC(i) STAMPP(i)  // (the sampler's count pass, rrl_sampler.h: stamps 6, 7 of the same table)
#else
#define STAMP(i)
#define STAMPW(i)
#define STAMPP(i)
#define STAMPC(i)
#endif
