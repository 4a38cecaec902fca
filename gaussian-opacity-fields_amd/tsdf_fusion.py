"""TSDF fusion on the GPU: the reference's extract_mesh_tsdf.py without Open3D.

The script (extract_mesh_tsdf.py:16-83) renders every training view, fuses depth / alpha / colour into Open3D's
``t.geometry.VoxelBlockGrid`` on a CUDA device and writes the marching-cubes mesh.  Here the volume and the mesh are
``gof_tsdf_*`` of libgof_hip.so (csrc/tsdf.hip, include/gof_tsdf_hip.h); the contract is DESIGN.md "TSDF fusion".

    vol = TSDFVolume(voxel_size=0.002)
    vol.integrate(depth, color, intrinsic, extrinsic)            # device tensors; one small read-back per view
    mesh = vol.extract_triangle_mesh()                            # vertices / triangles / colors / normals on the device
    write_ply(path, *mesh)

``tsdf_fusion`` has the script's signature; ``launch/run_reference_script.py`` binds it in place of the script's own function.
There is no host fallback: every step runs on the device or raises.
"""
import collections
import ctypes as C
import functools
import os

import numpy as np
import torch

from diff_gaussian_rasterization import _backend as B
import gof_native as gn

__all__ = ["TSDFVolume", "TriangleMesh", "fuse_views", "write_ply", "tsdf_fusion"]

TriangleMesh = collections.namedtuple("TriangleMesh", ["vertices", "triangles", "colors", "normals"])

BLOCK_RESOLUTION = 16
_VOXELS = BLOCK_RESOLUTION ** 3


class GofTsdfVolume(C.Structure):
    """Mirror of include/gof_tsdf_hip.h"""
    _fields_ = [("voxel_size", C.c_float), ("trunc", C.c_float), ("block_resolution", C.c_int32), ("reserved0", C.c_int32),
                ("table_capacity", C.c_int64), ("block_capacity", C.c_int64),
                ("table_keys", C.c_void_p), ("table_vals", C.c_void_p), ("block_keys", C.c_void_p), ("block_data", C.c_void_p),
                ("counter", C.c_void_p)]


def bind(lib):
    """ctypes signatures of the gof_tsdf_* entry points on `lib`"""
    vp, sz, i32, i64, f32 = C.c_void_p, C.c_size_t, C.c_int32, C.c_int64, C.c_float
    V = C.POINTER(GofTsdfVolume)
    P = C.POINTER(i64)
    return gn.bind(lib, {"gof_tsdf_frame_ws_bytes": [i64], "gof_tsdf_extract_ws_bytes": [i64]}, {
        "gof_tsdf_grow": [V, V, i64, vp],
        "gof_tsdf_touch": [V, vp, i32, i32, vp, vp, f32, f32, vp, sz, i64, P, P, vp],
        "gof_tsdf_integrate": [V, i64, vp, vp, i32, i32, vp, vp, f32, f32, vp, sz, i64, i64, i64, vp],
        "gof_tsdf_extract_count": [V, i64, f32, vp, sz, P, P, vp],
        "gof_tsdf_extract_emit": [V, i64, f32, vp, sz, i64, i64, vp, vp, vp, vp, vp],
        "gof_tsdf_block_coords": [V, i64, vp, vp],
    })


bind(B.lib)


def _pow2_at_least(n):
    return 1 << max(0, int(n - 1).bit_length())


def _dptr(t):
    return C.c_void_p(t.data_ptr())


# the device seams, by the names the host tests replace per module (tests/test_tsdf_host.py); one definition each: gof_native
_stream, _device_of, _on_device = gn.stream, gn.device_of, gn.on_device
_device = functools.partial(gn.current_device, "TSDFVolume")


def _buffer(role, shape, dtype, device):
    """Every device buffer of a TSDFVolume, by its role: the five arrays of GofTsdfVolume under their field names, "frame ws",
    "extract ws", "block_coords" and the four fields of TriangleMesh.  The one seam of this module alone: the host tests decide here
    what a buffer of each role holds when the library receives it."""
    return torch.empty(shape, dtype=dtype, device=device)


class TSDFVolume:
    """Sparse TSDF volume of 16^3-voxel blocks on a ROCm device (DESIGN.md "TSDF fusion").

    block_count is the initial capacity, a hint: the table and the block storage grow on the device when a view needs more, and no
    block is ever dropped.  80 KB of state per block (tsdf, weight, r, g, b in fp32)."""

    def __init__(self, voxel_size, block_resolution=16, block_count=50000, trunc_voxel_multiplier=8.0, device="cuda"):
        if int(block_resolution) != BLOCK_RESOLUTION:
            raise ValueError("TSDFVolume: block_resolution must be 16 (got %r)" % (block_resolution,))
        if not voxel_size > 0 or not trunc_voxel_multiplier > 0:
            raise ValueError("TSDFVolume: voxel_size and trunc_voxel_multiplier must be > 0")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("TSDFVolume (gfx950 backend) needs a ROCm device, got %s" % dev)
        self.device = dev if dev.index is not None else _device()
        self.voxel_size = float(voxel_size)
        self.trunc = float(trunc_voxel_multiplier) * self.voxel_size
        self._n = 0
        self._set_cap = 1 << 14
        self._frame_ws = None
        self._vol = None
        self._alloc(max(1, int(block_count)))

    # -- storage ------------------------------------------------------------------------------------------------------------
    def _alloc(self, block_capacity):
        dev = self.device
        tcap = _pow2_at_least(2 * block_capacity)
        bufs = {role: _buffer(role, count, dtype, dev) for role, count, dtype in (
            ("table_keys", tcap, torch.int64), ("table_vals", tcap, torch.int32), ("block_keys", block_capacity, torch.int64),
            ("block_data", block_capacity * 5 * _VOXELS, torch.float32), ("counter", 4, torch.int32))}
        vol = GofTsdfVolume(self.voxel_size, self.trunc, BLOCK_RESOLUTION, 0, tcap, block_capacity, *[b.data_ptr() for b in bufs.values()])
        with _device_of(bufs["counter"]):
            B._check(B.lib.gof_tsdf_grow(C.byref(vol), C.byref(self._vol) if self._vol is not None else None, self._n, _stream()))
        self._bufs, self._vol = bufs, vol         # (the old buffers are freed in stream order behind the copy)

    @property
    def block_capacity(self):
        return int(self._vol.block_capacity)

    @property
    def num_blocks(self):
        return self._n

    def block_coords(self):
        """[num_blocks, 3] int32 block coordinates, in storage order (the order of block_data())"""
        out = _buffer("block_coords", (self._n, 3), torch.int32, self.device)
        if self._n:
            with _device_of(out):
                B._check(B.lib.gof_tsdf_block_coords(C.byref(self._vol), self._n, _dptr(out), _stream()))
        return out

    def block_data(self):
        """[num_blocks, 5, 16, 16, 16] fp32 view of the blocks' (tsdf, weight, r, g, b), indexed [block, plane, z, y, x]"""
        return self._bufs["block_data"][:self._n * 5 * _VOXELS].view(self._n, 5, BLOCK_RESOLUTION, BLOCK_RESOLUTION, BLOCK_RESOLUTION)

    # -- integrate ----------------------------------------------------------------------------------------------------------
    def _frame_workspace(self):
        need = int(B.lib.gof_tsdf_frame_ws_bytes(self._set_cap))
        if self._frame_ws is None or self._frame_ws.numel() < need:
            self._frame_ws = _buffer("frame ws", need, torch.uint8, self.device)
        return self._frame_ws

    def _camera(self, m, shape):
        t = torch.as_tensor(m, dtype=torch.float32, device=self.device)
        if tuple(t.shape) != shape:
            raise ValueError("TSDFVolume.integrate: expected a %s matrix, got %s" % ("x".join(map(str, shape)), tuple(t.shape)))
        return t.contiguous()

    @torch.no_grad()
    def integrate(self, depth, color, intrinsic, extrinsic, depth_scale=1.0, depth_max=6.0):
        """depth [H,W] or [1,H,W], color [3,H,W] or [H,W,3] (device tensors); intrinsic 3x3 (fx, fy, cx, cy are used), extrinsic 4x4
        world->camera.  A pixel is valid iff 0 < depth / depth_scale <= depth_max."""
        if not _on_device(depth) or not _on_device(color):
            raise RuntimeError("TSDFVolume.integrate needs device tensors")
        d = depth.detach()
        if d.dim() == 3 and d.shape[0] == 1:
            d = d[0]
        if d.dim() != 2:
            raise ValueError("TSDFVolume.integrate: depth must be [H,W] or [1,H,W], got %s" % (tuple(depth.shape),))
        H, W = int(d.shape[0]), int(d.shape[1])
        c = color.detach()
        if tuple(c.shape) == (3, H, W):
            pass
        elif tuple(c.shape) == (H, W, 3):
            c = c.permute(2, 0, 1)
        else:
            raise ValueError("TSDFVolume.integrate: color must be [3,H,W] or [H,W,3] for a %dx%d depth, got %s" % (H, W, tuple(color.shape)))
        d = d.to(device=self.device, dtype=torch.float32).contiguous()
        c = c.to(device=self.device, dtype=torch.float32).contiguous()
        K = self._camera(intrinsic, (3, 3))
        E = self._camera(extrinsic, (4, 4))
        nf, nn = C.c_int64(0), C.c_int64(0)
        with _device_of(d):
            stream = _stream()
            while True:
                ws = self._frame_workspace()
                rc = B.lib.gof_tsdf_touch(C.byref(self._vol), _dptr(d), H, W, _dptr(K), _dptr(E), float(depth_scale), float(depth_max),
                                          _dptr(ws), ws.numel(), self._set_cap, C.byref(nf), C.byref(nn), stream)
                if rc != B.GOF_E_CAPACITY:
                    B._check(rc)
                    break
                self._set_cap *= 2                   # the frame's block set did not fit: redo with twice the slots
            n_frame, n_new = int(nf.value), int(nn.value)
            if self._n + n_new > self.block_capacity:
                self._alloc(max(2 * self.block_capacity, self._n + n_new))
            B._check(B.lib.gof_tsdf_integrate(C.byref(self._vol), self._n, _dptr(d), _dptr(c), H, W, _dptr(K), _dptr(E), float(depth_scale),
                                              float(depth_max), _dptr(ws), ws.numel(), self._set_cap, n_frame, n_new, stream))
        self._n += n_new
        if 4 * n_frame > self._set_cap:             # keep the next frame's set at most a quarter full
            self._set_cap = _pow2_at_least(4 * n_frame)

    # -- extract ------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def extract_triangle_mesh(self, weight_threshold=3.0):
        """Marching cubes of the zero level set -> TriangleMesh(vertices [V,3] f32, triangles [F,3] i32, colors [V,3] f32,
        normals [V,3] f32), device tensors, bit-reproducible for the same views in the same order."""
        dev = self.device
        n = self._n
        nv, nt = C.c_int64(0), C.c_int64(0)
        with _device_of(self._bufs["counter"]):
            stream = _stream()
            ws = _buffer("extract ws", int(B.lib.gof_tsdf_extract_ws_bytes(n)), torch.uint8, dev)
            B._check(B.lib.gof_tsdf_extract_count(C.byref(self._vol), n, float(weight_threshold), _dptr(ws), ws.numel(), C.byref(nv), C.byref(nt), stream))
            V, F = int(nv.value), int(nt.value)
            verts = _buffer("vertices", (V, 3), torch.float32, dev)
            cols = _buffer("colors", (V, 3), torch.float32, dev)
            nrms = _buffer("normals", (V, 3), torch.float32, dev)
            tris = _buffer("triangles", (F, 3), torch.int32, dev)
            if V or F:
                B._check(B.lib.gof_tsdf_extract_emit(C.byref(self._vol), n, float(weight_threshold), _dptr(ws), ws.numel(), V, F,
                                                     _dptr(verts), _dptr(tris), _dptr(cols), _dptr(nrms), stream))
        return TriangleMesh(verts, tris, cols, nrms)


def intrinsic_of(view):
    """The script's K (extract_mesh_tsdf.py:49-54): (projection_matrix @ ndc2pix)[:3, :3].T, on the device"""
    W, H = view.image_width, view.image_height
    P = view.projection_matrix
    ndc2pix = torch.tensor([[W / 2, 0, 0, (W - 1) / 2], [0, H / 2, 0, (H - 1) / 2], [0, 0, 0, 1]], dtype=torch.float32).to(P.device).T
    return (P.float() @ ndc2pix)[:3, :3].T.contiguous()


@torch.no_grad()
def fuse_views(views, gaussians, pipeline, background, kernel_size, render=None, voxel_size=0.002, alpha_thres=0.5, depth_max=6.0,
               progress=True):
    """The script's view loop (extract_mesh_tsdf.py:34-78): render every view, mask its depth, integrate -> TSDFVolume"""
    if render is None:
        from gaussian_renderer import render
    vol = TSDFVolume(voxel_size, block_resolution=16, block_count=50000)
    it = views
    if progress:
        try:
            from tqdm import tqdm
            it = tqdm(views, desc="Rendering progress")
        except ImportError:
            pass
    for view in it:
        rendering = render(view, gaussians, pipeline, background, kernel_size=kernel_size)["render"]
        depth = rendering[6:7, :, :]
        alpha = rendering[7:8, :, :]
        rgb = rendering[:3, :, :]
        if getattr(view, "gt_alpha_mask", None) is not None:
            depth[(view.gt_alpha_mask < 0.5)] = 0
        depth[(alpha < alpha_thres)] = 0
        vol.integrate(depth, rgb, intrinsic_of(view), view.world_view_transform.T, 1.0, depth_max)
    return vol


def write_ply(path, vertices, triangles, colors, normals):
    """Binary little-endian PLY: vertex x y z nx ny nz (float) red green blue (uchar); face vertex_indices (list uchar int)"""
    v = np.ascontiguousarray(torch.as_tensor(vertices).detach().cpu().numpy(), dtype=np.float32).reshape(-1, 3)
    n = np.ascontiguousarray(torch.as_tensor(normals).detach().cpu().numpy(), dtype=np.float32).reshape(-1, 3)
    c = np.asarray(torch.as_tensor(colors).detach().cpu().numpy(), dtype=np.float64).reshape(-1, 3)
    f = np.ascontiguousarray(torch.as_tensor(triangles).detach().cpu().numpy(), dtype=np.int32).reshape(-1, 3)
    if not (len(v) == len(n) == len(c)):
        raise ValueError("write_ply: vertices, colors and normals must have the same length")
    vrec = np.empty(len(v), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                                   ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    for i, k in enumerate("xyz"):
        vrec[k] = v[:, i]
        vrec["n" + k] = n[:, i]
    rgb = np.round(np.clip(c, 0.0, 1.0) * 255.0).astype(np.uint8)
    for i, k in enumerate(("red", "green", "blue")):
        vrec[k] = rgb[:, i]
    frec = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    frec["n"] = 3
    frec["i"] = f
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\n"
              "property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\n"
              "element face %d\nproperty list uchar int vertex_indices\nend_header\n") % (len(v), len(f))
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())


def tsdf_fusion(model_path, name, iteration, views, gaussians, pipeline, background, kernel_size):
    """extract_mesh_tsdf.py:16-83 -> <model_path>/<name>/ours_<iteration>/tsdf/tsdf.ply"""
    render_path = os.path.join(model_path, name, "ours_{}".format(iteration), "tsdf")
    os.makedirs(render_path, exist_ok=True)
    vol = fuse_views(views, gaussians, pipeline, background, kernel_size)
    mesh = vol.extract_triangle_mesh()
    write_ply(os.path.join(render_path, "tsdf.ply"), *mesh)
