// conv3x3_f32.h -- the 3x3 convolution with zero padding 1 as an implicit GEMM on the exact fp32 matrix step (mma_f32.h): the one main
// loop of the units that convolve (lpips.hip: a batch of images; appearance.hip: one plane read through an operand view).  A unit
// supplies where a pixel operand comes from and what happens to the accumulators, and keeps its own choice of tile.
//
// GEMM view: M = pixels, N = C_out, K = 9 C_in with k = ci * 9 + ky * 3 + kx (torch's flattening of the weight, so the weight tensor is
// read as it lies).  THE ORDER OF K IS THE CONTRACT: every output is one fmaf chain over k ascending, started from 0.
// A workgroup of 4 waves owns BM pixels x BN output channels and walks K in chunks of 4 input channels (36 terms; the last chunk of a
// C_in that is no multiple of 4 is shorter and padded to an even length with a term 0 * 0).  Per chunk the pixel operand X[k][m] (the
// shifted image values, 0 outside the image: the zero padding) and the weight operand Wt[n][k] (rows behind C_out: zeros) are staged
// in LDS, then every wave runs the chunk's k-steps on its 2 x WN accumulator tiles of 32 x 32.  The instruction takes the WEIGHTS in
// its A slot and the PIXELS in its B slot, i.e. it forms the transposed tile: an accumulator register then holds 32 consecutive pixels
// of one output channel across lanes 0-31, and a planar output is stored in 128-byte rows.
//   LDS: X [36][BM + 32] (the pad makes the two k rows a k-step reads fall into different bank halves), Wt [BN][37].
//   Tiles <WN, WGN>: <2, 2>: BM = 128, BN = 128 (waves 2 x 2);  <2, 1>: BM = 256, BN = 64;  <1, 1>: BM = 256, BN = 32.
#pragma once
#include <hip/hip_runtime.h>
#include "mma_f32.h"

namespace gof {
namespace conv3x3 {

constexpr int KC = 36;          // terms of a full K chunk: 4 input channels x 9 taps
constexpr int KP = 37;          // row pitch of the weight operand in LDS (odd: a wave's 32 rows fall into 32 banks)

// the workgroups of tile <WN, WGN>: BM = 256 / WGN pixels x BN = 32 WN WGN output channels each
template <int WN, int WGN>
inline dim3 grid(int M, int C_out) { return dim3((unsigned)((M + 256 / WGN - 1) / (256 / WGN)), (unsigned)((C_out + 32 * WN * WGN - 1) / (32 * WN * WGN))); }

// Where an accumulator register lies: store = pixel(q) once per pixel q < M this lane holds, then store(co, v) for each of its output
// channels -- register r of tile (i, j) is pixel wm_base + 32 i + (lane & 31) of the workgroup and channel wn_base + 32 j + (r & 3) +
// 8 (r >> 2) + 4 (lane >> 5).
template <int WN, class P>
__device__ __forceinline__ void for_each_output(const f32x16 (&acc)[2][WN], int M, int m0, int n0, int wm_base, int wn_base, int lane, P pixel)
{
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int q = m0 + wm_base + 32 * i + (lane & 31);
        if (q >= M) continue;
        const auto store = pixel(q);
#pragma unroll
        for (int j = 0; j < WN; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) store(n0 + wn_base + 32 * j + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), acc[i][j][r]);
    }
}

// The main loop.  Operand: members W, H (the plane), bool prepare(p) (decodes the pixel this thread stages into its members y, x; false
// behind M) and float load(ci, tap) (its value at input channel ci, tap = ky * 3 + kx, called only for taps inside the plane).  Epilogue:
// epilogue(acc, m0, n0, wm_base, wn_base, lane, Xs), once, after the last barrier -- Xs (KC * BMP floats of LDS) is free as scratch.
// FULL_N: the unit promises C_out % BN == 0, so no weight row lies behind C_out and the staging loop does not test for one (measured on
// MI355X: the test costs the LPIPS layers on the 128-channel tile 3 %, profiles/conv3x3_shared.md).
template <int WN, int WGN, bool FULL_N, class Operand, class Epilogue>
__device__ __forceinline__ void main_loop(int C_in, int C_out, Operand op, const float* __restrict__ w, Epilogue epilogue)
{
    constexpr int WGM = 4 / WGN, BM = 64 * WGM, BN = 32 * WN * WGN, BMP = BM + 32;
    constexpr int RPT = KC * BM / 256;                     // X rows a thread stages per chunk (36 or 18: whole input channels)
    __shared__ float Xs[KC * BMP];
    __shared__ float Ws[BN * KP];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const int m0 = (int)blockIdx.x * BM, n0 = (int)blockIdx.y * BN;
    const int K = 9 * C_in;

    // the pixel this thread stages and which of its 9 taps lie inside the plane
    const int lm = t % BM, lk0 = t / BM;
    unsigned inside = 0;
    if (op.prepare(m0 + lm))
        for (int ky = 0; ky < 3; ky++)
            for (int kx = 0; kx < 3; kx++)
                if (op.y + ky - 1 >= 0 && op.y + ky - 1 < op.H && op.x + kx - 1 >= 0 && op.x + kx - 1 < op.W) inside |= 1u << (ky * 3 + kx);

    const int wm_base = (wave % WGM) * 64, wn_base = (wave / WGM) * 32 * WN;
    f32x16 acc[2][WN];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < WN; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.0f;

    for (int c0 = 0; c0 < C_in; c0 += 4) {
        const int nci = (C_in - c0 < 4) ? C_in - c0 : 4;
        const int klen = 9 * nci, kpad = (klen + 1) & ~1;
        // pixel operand: rows kk = lk0 * RPT + j, all KC of them (rows behind klen are zeros: the pad term, and never NaN)
#pragma unroll
        for (int j = 0; j < RPT; j++) {
            const int kk = lk0 * RPT + j;
            const int ci = lk0 * (RPT / 9) + j / 9, tap = j % 9;
            float v = 0.0f;
            if (kk < klen && ((inside >> tap) & 1u)) v = op.load(c0 + ci, tap);
            Xs[kk * BMP + lm] = v;
        }
        // weight operand: row n = 36 consecutive floats of the weight tensor; rows behind C_out are zeros
        for (int e = t; e < BN * KC; e += 256) {
            const int n = e / KC, kk = e - n * KC;
            Ws[n * KP + kk] = (kk < klen && (FULL_N || n0 + n < C_out)) ? w[(size_t)(n0 + n) * (size_t)K + (size_t)(c0 * 9 + kk)] : 0.0f;
        }
        __syncthreads();
        for (int ks = 0; ks < kpad; ks += 2) {
            const int kk = ks + (lane >> 5);
            float a[WN], b[2];
#pragma unroll
            for (int j = 0; j < WN; j++) a[j] = Ws[(wn_base + 32 * j + (lane & 31)) * KP + kk];
#pragma unroll
            for (int i = 0; i < 2; i++) b[i] = Xs[kk * BMP + wm_base + 32 * i + (lane & 31)];
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < WN; j++) acc[i][j] = mma_32x32x2(a[j], b[i], acc[i][j]);
        }
        __syncthreads();
    }
    epilogue(acc, m0, n0, wm_base, wn_base, lane, Xs);
}

} // namespace conv3x3
} // namespace gof
