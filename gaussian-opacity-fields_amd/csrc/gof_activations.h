// gof_activations.h -- the two filtered activations of the reference GaussianModel (scene/gaussian_model.py:157-162, 183-194) as
// device functions: ONE definition for the training path (gaussian_model_ops.hip: gof_act_scaling / gof_act_opacity) and for the
// fused model file (model_io.hip: gof_model_pack in GOF_MODEL_FUSED mode), so the two cannot drift apart by a bit.
// fp32 throughout, in the reference's order of operations; the library is built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

namespace gof {

// get_scaling_with_3D_filter of one component: sqrt(square(exp(raw)) + square(filter_3D)); ff = filter_3D * filter_3D     (:160-161)
__device__ __forceinline__ float act_scaling_value(float raw, float ff)
{
    const float s = expf(raw);
    return sqrtf(s * s + ff);
}

// get_opacity_with_3D_filter: sigmoid(raw_opacity) * sqrt(det(S^2) / det(S^2 + filter_3D^2))                           (:184-194)
__device__ __forceinline__ float act_opacity_value(float raw_opacity, float rs0, float rs1, float rs2, float ff)
{
    const float s0 = expf(rs0), s1 = expf(rs1), s2 = expf(rs2);
    const float q0 = s0 * s0, q1 = s1 * s1, q2 = s2 * s2;       // scales_square (:188)
    const float det1 = q0 * q1 * q2;                            // :189
    const float det2 = (q0 + ff) * (q1 + ff) * (q2 + ff);       // :191-192
    const float coef = sqrtf(det1 / det2);                      // :193
    const float o = 1.0f / (1.0f + expf(-raw_opacity));         // sigmoid
    return o * coef;                                            // :194
}

} // namespace gof
