// dp_mapdev.h -- device helpers shared by the map stages (dp_render.hip,
// dp_fuse.hip, dp_mapref.hip, dp_tsdf.hip, dp_meshclean.hip).  Their CPU
// references are matched bit for bit: every fp64 expression here keeps its
// shape, parentheses included.
#pragma once

#include "dp_internal.h"

namespace dpk {

// a pixel holds a depth: positive and finite (host and device)
DP_HD bool is_depth(float z) { return z > 0.0f && z <= 3.402823466e+38f; }

// the set bits of m below this lane
__device__ __forceinline__ uint32_t lanes_below(uint64_t m)
{
    const uint32_t lo = __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u);
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), lo);
}

// one add per wave and counter, spread over Stripes copies of the Counters
// (summed by the host, dpk::StripedCounters); every lane of the wave calls
template <int Stripes, int Counters>
__device__ __forceinline__ void wave_count(unsigned long long *count, int counter, unsigned long long v, uint32_t stripe)
{
    for (int o = 32; o > 0; o >>= 1)
        v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0 && v)
        atomicAdd(&count[(stripe & (Stripes - 1)) * Counters + counter], v);
}

// the sum of v over a block of Block threads, in every thread (every thread
// calls; wsum holds Block / 64 words of LDS)
template <int Block> __device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t *wsum)
{
    for (int o = 32; o > 0; o >>= 1)
        v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0)
        wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t t = 0;
    for (int w = 0; w < Block / 64; ++w)
        t += wsum[w];
    return t;
}

// the sum of v over the block's threads below this one (every thread calls)
__device__ __forceinline__ uint32_t block_exclusive(uint32_t v, uint32_t *wsum)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o);
        if (lane >= o)
            x += y;
    }
    if (lane == 63)
        wsum[wv] = x;
    __syncthreads();
    uint32_t base = 0;
    for (int w = 0; w < wv; ++w)
        base += wsum[w];
    return base + x - v;
}

// row r of the 3 x 4 projection P applied to the point X
__device__ __forceinline__ double row_of(const double *P, int r, const double *X)
{
    return ((P[4 * r] * X[0] + P[4 * r + 1] * X[1]) + P[4 * r + 2] * X[2]) + P[4 * r + 3];
}

// the point of pixel (x, y) at the depth zd
__device__ __forceinline__ void backproject(const ViewInv &v, double x, double y, double zd, double *X)
{
    const double b0 = zd * x - v.P[3];
    const double b1 = zd * y - v.P[7];
    const double b2 = zd - v.P[11];
    for (int j = 0; j < 3; ++j)
        X[j] = ((v.A[3 * j] * b0 + v.A[3 * j + 1] * b1) + v.A[3 * j + 2] * b2) / v.det;
}

// X projected through P and rounded to the nearest pixel (xi, yi) of a W x H
// plane; d is its depth.  False behind the camera, out of range or outside.
__device__ __forceinline__ bool nearest_pixel(const double *P, int32_t W, int32_t H, const double *X, double &d,
                                              int32_t &xi, int32_t &yi)
{
    d = row_of(P, 2, X);
    if (!(d > 0.0))
        return false;
    const double h0 = row_of(P, 0, X);
    const double h1 = row_of(P, 1, X);
    double u, v;
    dpg::div2(h0, h1, d, u, v);
    if (!(fabs(u) < 2.0e9) || !(fabs(v) < 2.0e9))
        return false;
    xi = (int32_t)rint(u);
    yi = (int32_t)rint(v);
    return xi >= 0 && xi < W && yi >= 0 && yi < H;
}

} // namespace dpk
