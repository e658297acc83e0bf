// square_distance (PointNet/models/pointnet_util.py:19-40 of the reference) for one pair of points in the fp32 evaluation
// order pinned in SURVEY.md section 8(a'): explicit rounding intrinsics, so the result does not depend on -ffp-contract.
// Shared by the geometry kernels (psg_geometry.hip), whose integer outputs it decides, and by the coordinate-gradient
// kernels (psg_pn2_geomgrad.cuh), which differentiate the 3-NN weights at the distances the forward computed.
#pragma once
#include <hip/hip_runtime.h>

namespace psg {

__device__ __forceinline__ float sumsq3(float x, float y, float z)
{
    return __fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z));
}

// square_distance(src, dst) for one pair: ((-2*dot) + |src|^2) + |dst|^2, dot = FMA chain over k
__device__ __forceinline__ float sqdist(float sx, float sy, float sz, float ssq, float dx, float dy, float dz,
                                        float dsq)
{
    float dot = __fmaf_rn(sz, dz, __fmaf_rn(sy, dy, __fmul_rn(sx, dx)));
    return __fadd_rn(__fadd_rn(__fmul_rn(-2.0f, dot), ssq), dsq);
}

}  // namespace psg
