/*
 * gof_model_io_hip.h -- C ABI of the model file's row transpose in libgof_hip.so.
 *
 * What the reference's GaussianModel.save_ply / save_fused_ply / load_ply (scene/gaussian_model.py:374-430, 486-530) do on the host
 * with eight device-to-host copies, np.concatenate and one Python tuple per Gaussian: the transpose between the model's seven
 * structure-of-arrays tensors and the rows of its PLY file, on the device, in front of (behind) ONE pinned copy per chunk of rows.
 *
 * Conventions as in gof_hip.h: extern "C", device pointers, caller-owned buffers, launches on `stream`, 0 = ok, negative = GOF_E_*
 * with text in gof_last_error().  No workspace, no atomics; every byte of an output is written by the call (the contents of the
 * output buffers do not matter on entry); nothing is written where the return code is not 0.
 *
 * The model of P Gaussians with K = (D + 1)^2 - 1 higher-order SH coefficients per colour channel (0 <= K <= GOF_MODEL_MAX_K):
 *   xyz [P,3], f_dc [P,1,3], f_rest [P,K,3], opacity [P,1], scaling [P,3], rotation [P,4], filter_3D [P,1], all float32.
 * A row of the file (construct_list_of_attributes, :374-388), float32 each:
 *   x y z | nx ny nz | f_dc_0..2 | f_rest_0..3K-1 | opacity | scale_0..2 | rot_0..3 | filter_3D        C = 18 + 3K floats
 * f_rest_j with j = c * K + k holds f_rest[p, k, c] (transpose(1, 2).flatten(1)); f_dc_c holds f_dc[p, 0, c].
 */
#ifndef GOF_MODEL_IO_HIP_H_INCLUDED
#define GOF_MODEL_IO_HIP_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GOF_MODEL_MAX_K 24                      /* SH degree <= 4 */
#define GOF_MODEL_RAW 0                         /* save_ply: pure data movement, C = 18 + 3K */
#define GOF_MODEL_FUSED 1                       /* save_fused_ply: the 3D filter folded into opacity and scale, C = 17 + 3K */

/* floats per row of the file: 18 + 3K (RAW) or 17 + 3K (FUSED); -1 for a K or mode out of range */
int64_t gof_model_row_floats(int32_t K, int32_t mode);
/* channels of the model per Gaussian, = entries of gof_model_unpack's column table: 15 + 3K; -1 for a K out of range */
int64_t gof_model_channels(int32_t K);

/* ---- pack: rows [first, first + count) of the seven tensors -> count contiguous rows at out_rows ---------------------------------
 * RAW: every column is a copy of its tensor element, bit for bit; nx ny nz are written as +0.0.
 * FUSED: opacity = log(o / (1 - o)) with o = what gof_act_opacity gives for the row, scale_c = log(s_c) with s_c = what
 *   gof_act_scaling gives (the same device functions, csrc/gof_activations.h), fp32; no filter_3D column; the rest as RAW.
 * f_rest may be NULL where K = 0.  0 <= first, first + count <= P < 2^31. */
int gof_model_pack(int64_t P, int32_t K, int64_t first, int64_t count, const float* xyz, const float* f_dc, const float* f_rest,
                   const float* opacity, const float* scaling, const float* rotation, const float* filter_3D, int32_t mode,
                   float* out_rows, void* stream);

/* ---- unpack: count rows of a file's vertex element -> rows [first, first + count) of the seven tensors --------------------------
 * rows: count * pitch bytes in device memory, little-endian, as they lie in the file; pitch in bytes (1 <= pitch < 2^30), neither
 * it nor an offset nor `rows` itself need be a multiple of 4 (a value that is not 4-byte aligned is assembled from bytes).
 * columns (HOST memory, gof_model_channels(K) entries, in the order x y z f_dc_0..2 f_rest_0..3K-1 opacity scale_0..2 rot_0..3
 * filter_3D): where the channel's value lies in a row and its type.  GOF_PLY_FLOAT64 is rounded to the nearest float32 (ties to
 * even), as torch.tensor(float64 array, dtype=torch.float) does.  Any other type is GOF_E_INVALID, as is a column that does not lie
 * inside [0, pitch).  Nothing outside rows[0, count * pitch) is read. */
#define GOF_PLY_FLOAT32 0
#define GOF_PLY_FLOAT64 1
#define GOF_PLY_INT8 2
#define GOF_PLY_UINT8 3
#define GOF_PLY_INT16 4
#define GOF_PLY_UINT16 5
#define GOF_PLY_INT32 6
#define GOF_PLY_UINT32 7
typedef struct GofModelColumn {
    int64_t offset;                             /* byte offset of the value inside a row */
    int32_t type;                               /* GOF_PLY_* */
    int32_t reserved;                           /* 0 */
} GofModelColumn;

int gof_model_unpack(int64_t P, int32_t K, int64_t first, int64_t count, const void* rows, int64_t pitch, const GofModelColumn* columns,
                     float* xyz, float* f_dc, float* f_rest, float* opacity, float* scaling, float* rotation, float* filter_3D,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif
