// sg_launch.h -- host-side helpers of the launch wrappers (every .hip of csrc; sg_tiles also for the .cpp files).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sg_common.h"

// after a kernel launch: a launch error ends the wrapper with the hipError_t as its (positive) return value
#define SG_CHECK_LAUNCH()                                  \
    do {                                                   \
        hipError_t e__ = hipGetLastError();                \
        if (e__ != hipSuccess) return (int)e__;            \
    } while (0)

// 1024-row tiles of the longest frame: the grid's x of every kernel that walks frames by tile (at least one)
static inline int64_t sg_tiles(int64_t max_frame)
{
    const int64_t t = (max_frame + SG_TILE - 1) / SG_TILE;
    return t > 0 ? t : 1;
}

// compute units of the current device
static inline int sg_cu_count()
{
    int dev_id = 0, cus = 256;
    (void)hipGetDevice(&dev_id);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev_id);
    return cus > 0 ? cus : 256;
}

template <typename K>
static int sg_set_lds(K kernel, size_t lds, bool *attr_set)
{
    int dev_id = 0;
    (void)hipGetDevice(&dev_id);
    if (dev_id < 0 || dev_id >= 64 || !attr_set[dev_id]) {          // per device: several contexts may live in one process
        hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
        if (dev_id >= 0 && dev_id < 64) attr_set[dev_id] = true;
    }
    return 0;
}

// The row type of a launch from the C ABI's dtype (0: float32, else float64): f is a generic lambda that takes a value of the type,
//     sg_by_dtype(dtype, [&](auto t) { using T = decltype(t); ... (const T *)rows ... return 0; })
// so the float and the double launch are ONE text (both are instantiated, as by a written-out if / else).
template <class F>
static inline int sg_by_dtype(int dtype, F &&f)
{
    return dtype == 0 ? f(float{}) : f(double{});
}
