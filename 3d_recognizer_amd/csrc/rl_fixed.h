// Fixed fp32 expressions shared by the kernels whose numpy twins reproduce them bit for bit (scene.hip, lovasz.hip).
#pragma once
#include <hip/hip_runtime.h>

// e^x for x <= 0 as a fixed sequence of fp32 operations, so that the numpy twin (utils/scene.py: exp_fixed) gives the same
// bits: k = rint(x*log2(e)), r = x - k*ln2 in two steps (k*0.693359375 is exact), the degree-5 polynomial of Cephes' expf
// (public domain; 1.7e-7 relative) by Horner in separate multiplies and adds, then the exact product with 2^k.  Below -87
// (the result would leave the normal numbers) and for NaN it is 0.
__device__ __forceinline__ float exp_fixed(float x) {
    if (!(x >= -87.f)) return 0.f;
    const float k = rintf(__fmul_rn(x, 1.44269504088896341f));
    float r = __fsub_rn(x, __fmul_rn(k, 0.693359375f));
    r = __fsub_rn(r, __fmul_rn(k, -2.12194440e-4f));
    float p = 1.9875691500e-4f;
    p = __fadd_rn(__fmul_rn(p, r), 1.3981999507e-3f);
    p = __fadd_rn(__fmul_rn(p, r), 8.3334519073e-3f);
    p = __fadd_rn(__fmul_rn(p, r), 4.1665795894e-2f);
    p = __fadd_rn(__fmul_rn(p, r), 1.6666665459e-1f);
    p = __fadd_rn(__fmul_rn(p, r), 5.0000001201e-1f);
    p = __fadd_rn(__fadd_rn(__fmul_rn(p, __fmul_rn(r, r)), r), 1.f);
    return __fmul_rn(p, __int_as_float(((int)k + 127) << 23));     // k in [-126, 0]: 2^k is a normal number
}
