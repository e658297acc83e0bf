// torch.optim.Adam's single-tensor update in fp32, torch's operation order, every operation an explicit round-to-nearest
// intrinsic so that no unit's contraction setting can change a bit.  Shared by the NU attacks of the PointNet / PointNet++ /
// ResGCN families: nu_adam_step_kernel (psg_attack.hip), nu_coord_adam_kernel and nu_coord_adam_w_kernel (psg_nu_field.cuh),
// scene_nu_step_kernel (psg_scene_nu.hip).  Not RandLA-Net's TF1 Adam (psg_randla_attack.hip): another expression.
#pragma once
#include <cmath>
#include <hip/hip_runtime.h>

namespace psg {

// the step-dependent constants of step t >= 1, in double: step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t)
struct AdamConsts { float step_size, bc2_sqrt; };
inline AdamConsts adam_consts(float lr, float beta1, float beta2, int step)
{
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    return {(float)((double)lr / bc1), (float)sqrt(bc2)};
}

// m, v <- the moments after gradient g; returns x - step_size * m / (sqrt(v) / bc2_sqrt + eps)
__device__ __forceinline__ float adam_update(float x, float &m, float &v, float g, float beta1, float beta2, float eps,
                                             float step_size, float bc2_sqrt)
{
    const float mm = __fadd_rn(m, __fmul_rn(__fsub_rn(g, m), 1.0f - beta1));
    const float vv = __fadd_rn(__fmul_rn(v, beta2), __fmul_rn(1.0f - beta2, __fmul_rn(g, g)));
    m = mm;
    v = vv;
    const float denom = __fadd_rn(__fdiv_rn(sqrtf(vv), bc2_sqrt), eps);
    return __fadd_rn(x, __fmul_rn(-step_size, __fdiv_rn(mm, denom)));
}

}  // namespace psg
