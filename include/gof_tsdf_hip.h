/*
 * gof_tsdf_hip.h -- C ABI of the TSDF fusion in libgof_hip.so (csrc/tsdf.hip): the rendered depth / colour of every view fused into a
 * sparse volume of voxel blocks, and the triangle mesh of its zero level set (the reference's extract_mesh_tsdf.py, which uses
 * Open3D's VoxelBlockGrid).  The contract -- volume, camera, touch, integrate, extract, capacity -- is in DESIGN.md ("TSDF fusion").
 *
 * Conventions as in gof_hip.h: extern "C", device pointers, caller-owned workspaces, asynchronous on `stream`, 0 = ok, text of an
 * error in gof_last_error().  Camera data lives on the device: `intrinsic` is a 3x3 row-major fp32 matrix (fx = [0], cx = [2],
 * fy = [4], cy = [5]), `extrinsic` a 4x4 row-major fp32 world->camera matrix.  Images are fp32: depth [H][W], colour [3][H][W].
 *
 * Per view:  gof_tsdf_touch (one read-back: the frame's block count and how many of them are new) -> gof_tsdf_grow if the
 * volume's block capacity is too small -> gof_tsdf_integrate (no read-back).
 * Mesh:      gof_tsdf_extract_count (one read-back: the vertex and triangle totals) -> gof_tsdf_extract_emit.
 */
#ifndef GOF_TSDF_HIP_H_INCLUDED
#define GOF_TSDF_HIP_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One volume: caller-owned device buffers.  table_capacity: a power of two >= 2 * block_capacity (open addressing, empty slot =
 * ~0 key).  block_data: block_capacity blocks of 5 planes (tsdf, weight, r, g, b) of R^3 fp32, voxel x fastest.  block_keys: the
 * packed key of every used storage slot.  counter: 4 u32 words, [0] = used storage slots. */
typedef struct GofTsdfVolume {
    float voxel_size;
    float trunc;                 /* truncation distance (world units) */
    int32_t block_resolution;    /* must be 16 */
    int32_t reserved0;
    int64_t table_capacity;
    int64_t block_capacity;
    uint64_t* table_keys;        /* [table_capacity] */
    uint32_t* table_vals;        /* [table_capacity] storage slot of the key */
    uint64_t* block_keys;        /* [block_capacity] */
    float* block_data;           /* [block_capacity][5][R^3] */
    uint32_t* counter;           /* [4] */
} GofTsdfVolume;

/* Workspace of one frame whose block hash set has `set_capacity` slots (a power of two). */
size_t gof_tsdf_frame_ws_bytes(int64_t set_capacity);
/* Workspace of the mesh extraction of a volume with `num_blocks` active blocks. */
size_t gof_tsdf_extract_ws_bytes(int64_t num_blocks);

/* Makes `dst` hold the first `num_blocks` blocks of `src` (NULL: an empty volume): clears dst's table and unused storage, copies the
 * blocks, keys and counter and rebuilds dst's table from the keys on the device.  dst and src must not share buffers. */
int gof_tsdf_grow(const GofTsdfVolume* dst, const GofTsdfVolume* src, int64_t num_blocks, void* stream);

/* The frame's block set (every block a valid pixel's truncation segment passes through), compacted in the frame workspace.
 * Returns GOF_E_CAPACITY if the set needs more than `set_capacity` slots (redo with a larger one), GOF_E_INVALID for a block
 * coordinate outside [-2^20, 2^20).  *num_frame_blocks / *num_new_blocks: the set's size and how many of its blocks the volume
 * does not hold yet (the call's one read-back). */
int gof_tsdf_touch(const GofTsdfVolume* vol, const float* depth, int32_t height, int32_t width, const float* intrinsic,
                   const float* extrinsic, float depth_scale, float depth_max, void* frame_ws, size_t frame_ws_bytes,
                   int64_t set_capacity, int64_t* num_frame_blocks, int64_t* num_new_blocks, void* stream);

/* Activates the new blocks of the last gof_tsdf_touch on the same frame workspace and updates every voxel of the frame's blocks.
 * num_blocks: the volume's active blocks before the call; num_blocks + num_new_blocks must fit block_capacity. */
int gof_tsdf_integrate(const GofTsdfVolume* vol, int64_t num_blocks, const float* depth, const float* color, int32_t height,
                       int32_t width, const float* intrinsic, const float* extrinsic, float depth_scale, float depth_max,
                       void* frame_ws, size_t frame_ws_bytes, int64_t set_capacity, int64_t num_frame_blocks,
                       int64_t num_new_blocks, void* stream);

/* Marching cubes over the volume's num_blocks active blocks (cubes whose 8 corners have weight >= weight_threshold):
 * the vertex and triangle totals (the call's one read-back); the workspace then holds what gof_tsdf_extract_emit writes.
 * GOF_E_INVALID if num_blocks is not the volume's count of used slots, GOF_E_DEVICE if an earlier integrate flagged the volume. */
int gof_tsdf_extract_count(const GofTsdfVolume* vol, int64_t num_blocks, float weight_threshold, void* ws, size_t ws_bytes,
                           int64_t* num_vertices, int64_t* num_triangles, void* stream);

/* vertices / colors / normals [V][3] fp32, triangles [F][3] int32; V, F as gof_tsdf_extract_count returned. */
int gof_tsdf_extract_emit(const GofTsdfVolume* vol, int64_t num_blocks, float weight_threshold, void* ws, size_t ws_bytes,
                          int64_t num_vertices, int64_t num_triangles, float* vertices, int32_t* triangles, float* colors,
                          float* normals, void* stream);

/* Block coordinates [num_blocks][3] int32 of the active blocks, in storage-slot order. */
int gof_tsdf_block_coords(const GofTsdfVolume* vol, int64_t num_blocks, int32_t* coords, void* stream);

#ifdef __cplusplus
}
#endif
#endif
