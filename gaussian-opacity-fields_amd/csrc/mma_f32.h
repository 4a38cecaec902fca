// mma_f32.h -- the exact fp32 matrix step of gfx950 (v_mfma_f32_32x32x2_f32) and its host restatement, shared by the GEMMs that
// are built on it (conv3x3_f32.h: the convolution of lpips.hip and appearance.hip; appearance.hip's weight gradient).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

namespace gof {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// The matrix step, D = A B + C for A [32][2] (lane l holds A[l & 31][l >> 5]), B [2][32] (lane l holds B[l >> 5][l & 31]) and C / D
// [32][32] (register r of lane l holds row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31):
//     D[i][j] = fmaf(A[i][1], B[1][j], fmaf(A[i][0], B[0][j], C[i][j]))
// Under the HIP compiler this is ONE instruction.  The CPU test suite compiles the kernel sources as plain C++ against a host
// stand-in of the HIP runtime that knows no matrix instruction: there (no HIP compiler) the step is restated with cross-lane reads
// and fmaf in the same k order, so the CPU suite runs the kernels that use it and gets the same bits.  The only such conditional in csrc.
__device__ __forceinline__ f32x16 mma_32x32x2(float a, float b, f32x16 c)
{
#if !defined(__HIP__) && !defined(__HIPCC__)
    const int l = (int)(threadIdx.x & 63u);
    const float b0 = __shfl(b, l & 31), b1 = __shfl(b, (l & 31) + 32);
    for (int r = 0; r < 16; r++) {
        const int i = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
        const float a0 = __shfl(a, i), a1 = __shfl(a, i + 32);
        c[r] = fmaf(a1, b1, fmaf(a0, b0, c[r]));
    }
    return c;
#else
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
#endif
}

} // namespace gof
