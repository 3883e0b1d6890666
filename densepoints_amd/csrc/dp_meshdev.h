// dp_meshdev.h -- what the mesh stages (dp_meshclean.hip, dp_meshsmooth.hip, dp_meshdecimate.hip, dp_meshrender.hip,
// dp_meshcolour.hip) share: the block shape of their one-lane-per-item kernels, the guarded load
// of a triangle, the launch over so many blocks, and the host checks of the
// counts and pointers both sections of include/densepoints.h list.  The
// count / scan / emit pieces themselves (block_sum, block_exclusive,
// wave_count) are dp_mapdev.h's.
#pragma once

#include "dp_ctx.h"
#include "dp_mapdev.h"

#include <initializer_list>

namespace dpk {

constexpr int kMeshLanes = 256;

// the item (triangle, vertex, key) of this lane
__device__ __forceinline__ int64_t mesh_item() { return (int64_t)blockIdx.x * kMeshLanes + threadIdx.x; }

inline int64_t mesh_blocks(int64_t items) { return (items + kMeshLanes - 1) / kMeshLanes; }

// the triangle's indices; false (and nothing else read) unless t is a triangle
// and all three are vertices: no index is used as an address before this
__device__ __forceinline__ bool load_valid_triangle(const int32_t *tris, int64_t nt, int64_t nv, int64_t t, int32_t v[3])
{
    if (t >= nt)
        return false;
    v[0] = tris[3 * t];
    v[1] = tris[3 * t + 1];
    v[2] = tris[3 * t + 2];
    const uint64_t n = (uint64_t)nv;
    return (uint64_t)(uint32_t)v[0] < n && (uint64_t)(uint32_t)v[1] < n && (uint64_t)(uint32_t)v[2] < n;
}

template <typename K, typename A> hipError_t launch_over(K kernel, int64_t blocks, const A &a, hipStream_t s)
{
    if (blocks <= 0)
        return hipSuccess;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kMeshLanes), 0, s, a);
    return hipGetLastError();
}

} // namespace dpk

// ---- host checks shared by the mesh stages' C-ABI halves ------------------------

static inline int mesh_check_counts(dp_ctx *c, const std::string &w, const void *tris, int64_t nt, int64_t nv)
{
    if (nt < 0 || nv < 0 || nt > 0x7FFFFFFFll || nv > 0x7FFFFFFFll)
        return fail(c, DP_E_ARG, w + ": the counts must be in 0..2^31 - 1");
    if (nt > 0 && !tris)
        return fail(c, DP_E_ARG, w + ": triangles must be given");
    return DP_OK;
}

static inline int mesh_check_cap(dp_ctx *c, const std::string &w, const void *buf, int64_t cap)
{
    if (cap < 0 || (cap > 0 && !buf))
        return fail(c, DP_E_ARG, w + ": a cap must be >= 0, with its buffer given when > 0");
    return DP_OK;
}

// an output may not be an input
static inline int mesh_check_alias(dp_ctx *c, const std::string &w, std::initializer_list<const void *> outs,
                                   std::initializer_list<const void *> ins)
{
    for (const void *o : outs)
        for (const void *i : ins)
            if (o && o == i)
                return fail(c, DP_E_ARG, w + ": an output pointer equals an input pointer");
    return DP_OK;
}
