// dp_partition.hip -- multi-GPU partition of a generation's items:
// super-tile keys, the statistics of a cut of the key-sorted order, and the
// gather of the items a rank refines.
#include "dp_internal.h"

namespace dpk {

// Super-tile key of each item (spec in include/densepoints.h): the
// centre projected into its reference view, ty = floor(v / tile) and tx =
// floor(u / tile) clamped to [-1, TY] / [-1, TX] (NaN and |q| >= 2e9 count as
// 0), key = (ref (TY + 2) + ty + 1) (TX + 2) + tx + 1: dense, so the sort
// covers only the key's ceil(log2(V (TY + 2) (TX + 2))) low bits.  Sorting by
// key orders the items by (reference view, tile row, tile column); the
// partition cuts that order into `world` contiguous equal shares.
__device__ __forceinline__ uint64_t tile_coord(double q, int64_t tmax)
{
    int64_t t = 0;
    if (q > -2.0e9 && q < 2.0e9)
        t = (int64_t)floor(q);
    t = t < -1 ? -1 : t > tmax ? tmax : t;
    return (uint64_t)(t + 1);
}

__global__ void tile_keys_kernel(const dpg::ViewDev *views, const dp_patch *items, int64_t n, double tile, int64_t tx_max,
                                 int64_t ty_max, uint64_t *key, int64_t *iota, unsigned long long *stats)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) // the partition statistics' counters (partition_stats_kernel adds to them)
        stats[0] = stats[1] = 0ull;
    if (i >= n)
        return;
    iota[i] = i; // the sort's values: item indices
    const dp_patch &p = items[i];
    const dpg::ViewDev &v = views[p.ref];
    double u, w;
    dpg::project(v.P, (double)p.pos[0], (double)p.pos[1], (double)p.pos[2], u, w);
    key[i] = ((uint64_t)p.ref * (uint64_t)(ty_max + 2) + tile_coord(w / tile, ty_max)) * (uint64_t)(tx_max + 2) +
             tile_coord(u / tile, tx_max);
}

// partition statistics over the key-sorted items: stats[0] = distinct tiles,
// stats[1] = items of the tiles a cut lo[r] (0 < lo[r] < n) splits between ranks
__global__ void partition_stats_kernel(const uint64_t *key, int64_t n, int world, unsigned long long *stats)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long heads = 0, split = 0;
    if (j < n) {
        const uint64_t k = key[j];
        heads = (j == 0 || key[j - 1] != k) ? 1ull : 0ull;
        for (int r = 1; r < world; ++r) {
            // the cut lo_r = floor(r n / world) (n < 2^31, world <= 64: no overflow)
            const int64_t c = ((int64_t)r * n) / world;
            if (c > 0 && c < n && key[c - 1] == key[c] && key[c] == k) {
                split = 1;
                break;
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        heads += __shfl_xor(heads, o);
        split += __shfl_xor(split, o);
    }
    if ((threadIdx.x & 63) == 0 && (heads | split)) {
        atomicAdd(&stats[0], heads);
        atomicAdd(&stats[1], split);
    }
}

hipError_t launch_tile_keys(const dpg::ViewDev *views, const dp_patch *items, int64_t n, double tile, int64_t tx_max,
                            int64_t ty_max, uint64_t *key, int64_t *iota, unsigned long long *stats, hipStream_t s)
{
    if (n <= 0)
        return hipSuccess;
    hipLaunchKernelGGL(tile_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, views, items, n, tile,
                       tx_max, ty_max, key, iota, stats);
    return hipGetLastError();
}

// (the counters were zeroed by tile_keys_kernel)
hipError_t launch_partition_stats(const uint64_t *key, int64_t n, int world, unsigned long long *stats, hipStream_t s)
{
    if (n <= 0)
        return hipSuccess;
    hipLaunchKernelGGL(partition_stats_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, key, n, world,
                       stats);
    return hipGetLastError();
}

__global__ void gather_patches_kernel(const dp_patch *src, const int64_t *idx, int64_t n, dp_patch *dst)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        dst[i] = src[idx[i]];
}

hipError_t launch_gather_patches(const dp_patch *src, const int64_t *idx, int64_t n, dp_patch *dst, hipStream_t s)
{
    if (n <= 0)
        return hipSuccess;
    hipLaunchKernelGGL(gather_patches_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, idx, n, dst);
    return hipGetLastError();
}

} // namespace dpk
