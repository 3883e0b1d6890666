// dp_wave.h -- wave-level primitives shared by the two refine kernels
// (dp_refine.hip, dp_fast_kernel.hip): each keeps one wavefront per patch and
// its uniform state in LDS.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dpk {

__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// wave-uniform copy of a double (lane 0's), so comparisons on it are scalar branches
__device__ __forceinline__ double uni_f64(double v)
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readfirstlane((int)(b & 0xffffffff));
    const int hi = __builtin_amdgcn_readfirstlane((int)(b >> 32));
    return __longlong_as_double(((long long)(unsigned)hi << 32) | (unsigned)lo);
}

__device__ __forceinline__ double readlane_f64(double v, int l)
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffff), l);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
    return __longlong_as_double(((long long)(unsigned)hi << 32) | (unsigned)lo);
}

// Lane id through an opaque (volatile) mbcnt: values derived from it are
// recomputed where they are used instead of being hoisted to kernel scope,
// where dozens of per-lane LDS addresses would stay live in VGPRs across the
// whole refine loop.
__device__ __forceinline__ int lane_id()
{
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

typedef __attribute__((address_space(3))) const double *lds_f64_t;
typedef __attribute__((address_space(3))) uint32_t *lds_u32_t;
typedef __attribute__((address_space(3))) uint16_t *lds_u16_t;

__device__ __forceinline__ uint32_t lds_addr(const void *p)
{
    return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const char *)p;
}

} // namespace dpk

// A field of the kernel's argument struct `Args` read afresh from the
// kernel-argument segment at its use (a volatile scalar load) instead of an
// SGPR kept live across the kernel: both refine kernels run out of SGPRs, and
// the compiler's spills of the option block came back through v_readlane
// (VALU) in the per-evaluation loops.
#define DP_KARG(Args, T, field)                                                                       \
    (*(const volatile __attribute__((address_space(4))) T *)((const __attribute__((address_space(4))) char *) \
                                                                  __builtin_amdgcn_kernarg_segment_ptr() +   \
                                                              offsetof(Args, field)))
