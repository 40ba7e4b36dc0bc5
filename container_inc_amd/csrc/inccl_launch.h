// inccl_launch.h -- the host side of every kernel launch, once: pointer
// alignment, the cached CU count, the grid arithmetic, the SrcPtrs fill and the
// dispatch on the fan-in R.  Included by all seven .hip files.
#ifndef INCCL_LAUNCH_H
#define INCCL_LAUNCH_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "inccl_kernels.h"
#include "inccl_stream.h"

namespace inccl_dev {

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// compute units of the current device, asked once (256 when it cannot be asked)
inline int num_cus()
{
    static int cus = 0;
    if (cus == 0) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) == hipSuccess &&
            hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
            cus = v;
        else
            cus = 256;
    }
    return cus;
}

// workgroups for `items` at `per_group` a workgroup: at least 1, at most `cap`.
// kNoCap: one workgroup per group (the vector stream kernels' default).
constexpr int64_t kNoCap = 0x7fffffff;
inline int grid_capped(int64_t items, int64_t per_group, int64_t cap)
{
    const int64_t g = (items + per_group - 1) / per_group;
    return (int)(g < 1 ? 1 : (g < cap ? g : cap));
}
// ... at most per_cu_cap workgroups per CU (a grid-stride loop covers the rest)
inline int grid_of(int64_t items, int64_t per_group, int per_cu_cap)
{
    return grid_capped(items, per_group, (int64_t)num_cus() * per_cu_cap);
}

// s = the R pointers of srcs, none NULL; *vec stays true while all are 16-B
// aligned (PTRS: SrcPtrs, or the ResPtrs of inccl_block.h for fp32 residuals)
template <class T, class PTRS>
inline int fill_srcs(T* const* srcs, int R, PTRS* s, bool* vec)
{
    if (srcs == nullptr || R < 1 || R > kMaxR) return INCCL_ERR_ARG;
    *s = PTRS{};
    for (int r = 0; r < R; ++r) {
        if (srcs[r] == nullptr) return INCCL_ERR_ARG;
        s->p[r] = srcs[r];
        *vec = *vec && aligned16(srcs[r]);
    }
    return 0;
}

// CALL(R) with R a constant 1..8 (callers have checked the range)
#define INCCL_R_SWITCH(R, CALL) \
    switch (R) {                \
        case 1: CALL(1); break; \
        case 2: CALL(2); break; \
        case 3: CALL(3); break; \
        case 4: CALL(4); break; \
        case 5: CALL(5); break; \
        case 6: CALL(6); break; \
        case 7: CALL(7); break; \
        default: CALL(8); break; \
    }

}  // namespace inccl_dev

#endif
