#!/usr/bin/env python3
"""Run an UNCHANGED script of the reference (train.py, render.py, extract_mesh.py, ...) against the
MI355X backend.

    python gaussian-opacity-fields_amd/launch/run_reference_script.py /path/to/gaussian-opacity-fields/train.py -s <scene> ...

What it does, in this order (nothing in the reference checkout is edited):
  1. puts this package first on sys.path so `import diff_gaussian_rasterization` resolves to the gfx950
     backend, and the reference checkout second so its own packages (scene, utils, gaussian_renderer) import;
  2. `simple_knn._C.distCUDA2` resolves to the HIP implementation in this package (simple_knn/, include/gof_knn_hip.h); puts the
     import shim for the out-of-scope native submodule (tetranerf: CGAL Delaunay) on sys.path unless the
     real modules are importable;
  3. rebinds utils.tetmesh.marching_tetrahedra to the HIP implementation BEFORE the script imports it by name
     (extract_mesh.py:14: `from utils.tetmesh import marching_tetrahedra`);
  4. rebinds the per-iteration training epilogue to its HIP implementation (train_epilogue/, include/gof_train_hip.h):
     utils.loss_utils.ssim (train.py:20), utils.depth_utils.depth_to_normal / depths_to_points (train.py:38) and the
     optimizer GaussianModel.training_setup builds (scene/gaussian_model.py:360 -> FusedAdam over the same param groups) and
     GaussianModel.compute_3D_filter (scene/gaussian_model.py:262-311, one launch over points x cameras) and
     GaussianModel.densify_and_prune (:685-707: device index lists + one row gather per tensor; GOF_TORCH_DENSIFY=1 keeps the reference's).
     GOF_TORCH_EPILOGUE=1 keeps the reference's torch implementations; the loss train.py composes inline from these helpers
     (train.py:150-189) is evaluated by ONE fused call at `loss.backward()` (train_epilogue/deferred.py; GOF_EAGER_LOSS=1 keeps the
     helpers eager, one launch pair each); scene.cameras.Camera.world_view_transform becomes a
     train_epilogue.PoseMatrix (train.py:177-179: `.T.inverse()` computed once per camera, `c2w[:3, :3] @ normals` one streaming
     launch instead of a GEMM; GOF_PLAIN_POSE=1 keeps the plain tensor);
  5. wraps gaussian_renderer.integrate (imported by name at extract_mesh.py:5) so that the Gaussian side of the opacity-field
     query (binning + pixel pass) runs once per view for the ~10 point sets extract_mesh.py queries against the unchanged model
     (diff_gaussian_rasterization.integrate_view_key; GOF_INTEGRATE_CACHE_GB bounds the HBM it may keep, 0 disables);
  6. runs the script as __main__ with the remaining argv.  A function the script defines itself cannot be rebound through an
     imported module: for extract_mesh.py's `evaluage_alpha` (:17-34, the loop over all views per point set) the module body is
     executed without its `if __name__ == "__main__":` block, the name is pointed at mesh_extraction.evaluate_alpha (the same loop
     with the min / arg-min reduction over views fused into the point pass), then the block runs (run_script below;
     GOF_TORCH_VIEW_REDUCE=1 keeps the script's own function).  extract_mesh_tsdf.py's `tsdf_fusion` (:16-83, Open3D's
     VoxelBlockGrid on a CUDA device) is rebound the same way to tsdf_fusion.tsdf_fusion (the HIP TSDF fusion); its top-level
     `import open3d` / `import open3d.core` resolve to shims/open3d when open3d is not installed.
  7. evaluate_dtu_mesh.py:190-192 shells out to `python dtu_eval/eval.py ...` (Open3D, scikit-learn): the script's `os` becomes a
     stand-in whose system() runs that one command in-process through mesh_eval's command line (the HIP Chamfer evaluation,
     csrc/cloud.hip) and forwards everything else to the real os; GOF_DTU_EVAL_SUBPROCESS=1 leaves the script alone.  Given
     dtu_eval/eval.py itself, the launcher runs mesh_eval's command line with the same arguments.
  8. given eval_tnt/run.py (Open3D 0.9: the last step of scripts/run_tnt.py), the launcher runs tnt_eval's command line (the HIP
     Tanks-and-Temples F-score evaluation, csrc/cloud_reg.hip) with the same arguments; GOF_TNT_EVAL_SUBPROCESS=1 leaves the script
     alone.
  9. evaluate_dtu_mesh.py:59-131, 172 asks cv2, scikit-image and trimesh for the calibration decomposition, the mask dilation, the
     projection of all vertices into all views and the mesh container: the script's `cull_mesh` becomes mesh_cull.cull_mesh (the HIP
     mesh culling, csrc/mesh_cull.hip), and where cv2 / trimesh are not installed its `load_dtu_camera` becomes
     mesh_cull.load_dtu_camera and its `trimesh` a namespace whose load() is mesh_cull.load; import stand-ins for the packages that
     are missing (shims_dtu/) go LAST on sys.path -- skimage's and cv2's for this script only, trimesh's for every script (10.).
     GOF_DTU_CULL_TORCH=1 leaves the script alone.
 10. extract_mesh.py:36-120 and scene/gaussian_model.py:31-72, 433-463 ask torch einsums over views x points, boolean-mask assignments
     and trimesh for the tetrahedralization's input points, the 8 bisection rounds and the mesh: GaussianModel.get_tetra_points
     becomes mesh_extraction.get_tetra_points and the script's `marching_tetrahedra_with_binary_search` the function of that name in
     mesh_extraction (csrc/extract.hip: one launch over candidates x views, one launch per round, a mesh_cull.DeviceMesh exported from
     the device); the bound function queries the field through whatever `evaluage_alpha` is in the script's namespace when it is
     called, so 6.'s switch still selects the script's own loop.  GOF_TORCH_EXTRACT=1 leaves both names alone.  `import trimesh`
     (scene/gaussian_model.py:23, extract_mesh.py:12) resolves to the stand-in of shims_dtu/ where trimesh is not installed, for
     every script; an installed trimesh wins.
 11. render.py:18,35-36 and metrics.py:16,19,33-34,76,100 ask torchvision for save_image / to_tensor and the lpips package for
     `lpips.LPIPS(net='vgg')`: where they are not installed, `import torchvision` and `import lpips` resolve to the stand-ins of
     shims/ (LAST on sys.path: an installed package wins).  lpips.LPIPS is image_metrics.LPIPS (the HIP VGG16 feature distance,
     csrc/lpips.hip); it reads the user's own weight files (GOF_LPIPS_VGG16, GOF_LPIPS_LIN, torch's hub cache, an installed lpips
     package) and never downloads.  metrics.py's `ssim` is 4.'s.
 12. train.py:67-88 defines L1_loss_appearance (`--use_decoupled_appearance`: the reference's TNT and DTU runs) from torch convolutions,
     pixel-shuffles and bilinear resamplings: with GOF_HIP_APPEARANCE=1 the script's name becomes
     train_epilogue.appearance.L1_loss_appearance (csrc/appearance.hip: the network forward and backward on the exact fp32 matrix
     instruction in fixed orders, bit-reproducible), rebound as 6. rebinds `evaluage_alpha`.  The network module, its optimizer groups
     and checkpoints are the reference's.  GOF_TORCH_APPEARANCE=1 keeps the script's own function whatever else is set.
 13. scene/gaussian_model.py:390-430, 486-530 move the model between its tensors and point_cloud.ply through plyfile: eight
     device-to-host copies, a concatenation and one Python tuple per Gaussian (train.py saves through it, render.py, extract_mesh.py,
     extract_mesh_tsdf.py and create_fused_ply.py load through it): GaussianModel.save_ply / save_fused_ply / load_ply become model_io's
     (csrc/model_io.hip: the row transpose on the device, in front of one pinned copy per chunk of rows), by name; the reference's own
     methods are kept and serve a model that is not on the device.  GOF_TORCH_PLY=1 leaves the three methods alone.  `import plyfile`
     (scene/gaussian_model.py:18, scene/dataset_readers.py:22: fetchPly / storePly still go through it) resolves to the stand-in of
     shims/ where plyfile is not installed, and `import cv2` (train.py:15, nothing of it is called) to the one of shims_dtu/ for every
     script; an installed package wins.
 14. utils/camera_utils.py:19-62 builds the scene's cameras in a serial loop: Pillow decodes and resizes each image on one CPU thread,
     np.array(...) / 255.0 turns 3 bytes per pixel into 12 and the float tensor is uploaded from pageable memory: loadCam and
     cameraList_from_camInfos become scene_images' (csrc/scene_images.hip: Pillow's bicubic resampler and the conversion to float planes
     on the device, bit for bit; worker threads decode ahead, the raw bytes travel through two pinned buffers), by name, in
     utils.camera_utils and in `scene` (scene/__init__.py:19 takes cameraList_from_camInfos by name, and the two modules import each
     other, so `scene` is imported first and its name rebound too).  The reference's own functions are kept and serve an
     image whose mode is not RGB, RGBA or L.  The output is bit-identical; the loading time has not been measured on the device yet, so
     the binding is asked for with GOF_HIP_IMAGES=1 (SCENE_IMAGES_BY_DEFAULT below) and GOF_PIL_IMAGES=1 leaves both functions alone
     whatever else is set; GOF_IMAGE_DECODE_THREADS (default 8, 1..16) sizes the decoding pool.
 15. render.py:35-36 saves two PNG files per view through torchvision.utils.save_image: a blocking copy to the host and Pillow's encoder on
     one CPU thread, next to a render of a few milliseconds.  With GOF_HIP_PNG=1 `torchvision.utils.save_image` (the stand-in's of 11. or an
     installed torchvision's: render.py reaches it by attribute) becomes image_writer.save_image before the script runs
     (csrc/png_encode.hip: quantisation, PNG filters, deflate and Adler-32 on the device; one writer thread frames and writes the files
     behind a ring of pinned buffers, so the render loop does not synchronise per image).  The files are valid PNGs with identical pixels,
     not Pillow's bytes.  Anything that is not a float32 image of 1 or 3 channels going to a .png file name (train.py:235's jpg, file
     objects) goes to the function that was bound before.  image_writer.flush() runs after the script's __main__ returns or raises (and at
     exit): an error of the writer thread surfaces there.  Its speed has not been measured on the device yet, so the binding is asked for
     (PNG_WRITER_BY_DEFAULT below); GOF_PIL_PNG=1 leaves the function alone whatever else is set.
 16. metrics.py:25-36 defines readImages: for every test view it opens two PNG files with Pillow (inflate and unfilter on one CPU thread),
     divides by 255 through to_tensor and uploads from pageable memory, for all views of a method before the first metric.  With
     GOF_HIP_PNG_READ=1 the script's name becomes png_reader.read_images_for_metrics (csrc/png_decode.hip: inflate, the PNG filters and the
     conversion to float planes on the device for a batch of files; worker threads read the files and walk the chunks), rebound as 6.
     rebinds `evaluage_alpha`: the same file order, the same three lists, the tensors bit-identical.  A file the unit does not take
     (interlaced, not 8 bits, a palette, tRNS) goes through the script's own function, which run_script keeps (SCRIPT_OWN).  Its speed has
     not been measured on the device yet, so the binding is asked for (PNG_READER_BY_DEFAULT below); GOF_PIL_PNG_READ=1 leaves the script
     alone whatever else is set.  scene_images' decoding of PNG training images stays Pillow's.
 17. Opt-in only: GOF_MESH_COMPONENTS=<spec> (`largest:1`, `min_area_ratio:0.2,connectivity:vertex`; the keys are the keyword arguments of
     DeviceMesh.keep_components) removes the small disconnected pieces of the extracted mesh (mesh_components.py, csrc/mesh_components.hip,
     DESIGN.md 3.18).  The replacements of 9. and of extract_mesh_tsdf.py's `tsdf_fusion` first write the file they always wrote, byte for
     byte; then that file is read back, reduced to the selected components and written next to it as mesh_binary_search_7_clean.ply /
     tsdf_clean.ply.  A malformed spec is an error before the script starts.  Unset: nothing differs.
     Likewise GOF_MESH_SIMPLIFY=<spec> (`grid:1024`, `target_vertices:2000000`, `cell:0.01,dedupe:0`; the keyword arguments of
     DeviceMesh.simplify: mesh_simplify.py, csrc/mesh_simplify.hip) writes mesh_binary_search_7_simplified.ply /
     tsdf_simplified.ply next to the file, from the cleaned mesh where GOF_MESH_COMPONENTS is set as well, else from the file itself.
 18. eval_tnt/cull_mesh.py asks pyrender (OpenGL over EGL) for a depth image of the mesh per camera and torch for the views that see each
     vertex in front of it: for a script that defines both `Mesher` and `extract_depth_from_mesh` the two names become
     mesh_cull.TntMesher and mesh_cull.render_depth (csrc/mesh_raster.hip, DESIGN.md 3.19: a triangle rasteriser with a z-buffer and the
     per-vertex count over it, a batch of views at a time), rebound as 6. rebinds `evaluage_alpha`; the script's __main__, its get_traj
     and its intrinsics run as they are.  `import pyrender` resolves to the stand-in of shims/ where pyrender is not installed, open3d,
     trimesh and cv2 to theirs (2., 10., 13.).  The mesh that is culled is the file the script is given (its own
     extract_depth_from_mesh loads a file of its author's, :28).  GOF_TNT_CULL_TORCH=1 leaves the script alone.
 19. mesh_viewer.py PATH asks Open3D for compute_vertex_normals and an OpenGL window (:48-71); no window can open on a machine without
     a display, so the headless stand-in runs instead: mesh_render's command line (csrc/mesh_render.hip, DESIGN.md 3.20: area-weighted
     vertex normals, a face buffer beside the z-buffer, a resolve pass) with `PATH --turntable 8 --mode shaded --out PATH_views/`, which
     writes PATH_views/00000.png .. 00007.png through image_writer.  Open3D is not imported.  GOF_MESH_VIEWER_WINDOW=1 leaves the script
     alone.
"""
import importlib
import os
import runpy
import sys

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rebind_train_epilogue():
    """Swap the reference's pure-torch loss helpers and optimizer for the HIP ones, by name, before the script's
    `from ... import` statements run.  Modules that are not importable (a script that does not train) are skipped."""
    import train_epilogue as T
    from train_epilogue import deferred
    # train.py:150-189 composes its loss inline from these helpers, the image's channel slices and the camera pose: with deferred
    # evaluation on, the script's own lines collect coefficients and loss.backward() is ONE fused call (train_epilogue/deferred.py: any
    # other spelling computes eagerly with the mirrors below); GOF_EAGER_LOSS=1 keeps every line eager
    deferred.enable(os.environ.get("GOF_EAGER_LOSS") != "1")
    try:
        import utils.loss_utils as ref_loss
        ref_loss.ssim = deferred.ssim                       # (eager: T.ssim)
        ref_loss.l1_loss = deferred.l1_loss                 # (eager: T.l1_loss)
    except ImportError:
        pass
    try:
        import utils.depth_utils as ref_depth
        ref_depth.depth_to_normal = deferred.depth_to_normal      # (eager: T.depth_to_normal)
        ref_depth.depths_to_points = T.depths_to_points
    except ImportError:
        pass
    # train.py:177-179 inverts the camera pose and multiplies its 3x3 block with the normal image every iteration: the Camera's
    # world_view_transform becomes a tensor that remembers its inverse and applies the block with one streaming launch
    # (train_epilogue/pose.py); GOF_PLAIN_POSE=1 keeps the plain tensor
    if os.environ.get("GOF_PLAIN_POSE") != "1":
        try:
            import scene.cameras as ref_cameras
            _cam_init = ref_cameras.Camera.__init__

            def _camera_init(self, *a, **k):
                _cam_init(self, *a, **k)
                self.world_view_transform = T.PoseMatrix.wrap(self.world_view_transform)
            ref_cameras.Camera.__init__ = _camera_init
        except Exception:
            pass
    try:
        from scene.gaussian_model import GaussianModel
    except Exception:
        return
    _setup = GaussianModel.training_setup

    def training_setup(self, training_args):
        _setup(self, training_args)
        groups = self.optimizer.param_groups               # six named groups with their lr (gaussian_model.py:349-358)
        old = self.optimizer
        self.optimizer = T.FusedAdam([{"params": g["params"], "lr": g["lr"], "name": g["name"]} for g in groups], lr=0.0, eps=1e-15)
        for hook in getattr(old, "_optimizer_step_pre_hooks", {}).values():      # e.g. the DP gradient all-reduce (run_train_dp.py)
            self.optimizer.register_step_pre_hook(hook)
        for hook in getattr(old, "_optimizer_step_post_hooks", {}).values():
            self.optimizer.register_step_post_hook(hook)
    GaussianModel.training_setup = training_setup
    GaussianModel.compute_3D_filter = T.compute_3D_filter      # train.py:118,261,269: after every densification
    GaussianModel.add_densification_stats = T.add_densification_stats   # train.py:256: every iteration until densify_until_iter
    # train.py:260: clone / split / prune as ordered device index lists + one row gather per tensor (train_epilogue/densify.py)
    if os.environ.get("GOF_TORCH_DENSIFY") != "1":
        current = GaussianModel.densify_and_prune
        if hasattr(current, "inner"):          # the data-parallel launcher's wrapper (statistics all-reduce first): replace what it calls
            current.inner = T.densify_and_prune
        else:
            GaussianModel.densify_and_prune = T.densify_and_prune
    # the three derived tensors render() reads every iteration (gaussian_renderer/__init__.py:60,70-71)
    GaussianModel.get_scaling_with_3D_filter = property(T.activations.get_scaling_with_3D_filter)
    GaussianModel.get_opacity_with_3D_filter = property(T.activations.get_opacity_with_3D_filter)
    GaussianModel.get_rotation = property(T.activations.get_rotation)
    # get_features (gaussian_model.py:173-176) concatenates _features_dc and _features_rest -- 192 B per Gaussian copied, and the
    # gradient split back, every iteration.  render() / integrate() hand the result straight to the rasterizer
    # (gaussian_renderer/__init__.py:94,194), which reads the two stored tensors directly when given a SplitSH; any other use of
    # the object (pipe.convert_SHs_python, :84-85) sees the concatenation.  GOF_CAT_FEATURES=1 keeps the reference's property.
    if os.environ.get("GOF_CAT_FEATURES") != "1":
        from diff_gaussian_rasterization import SplitSH
        GaussianModel.get_features = property(lambda self: SplitSH(self._features_dc, self._features_rest))


def rebind_integrate_with_view_cache():
    """extract_mesh.py:23-31 calls integrate(points, view, gaussians, ...) for every view, once per bisection step, with the
    same Gaussians.  The wrapper announces a key made of the identities + version counters of everything but the points."""
    import torch
    import diff_gaussian_rasterization as DGR
    try:
        import gaussian_renderer as GR
    except Exception:
        return
    orig = GR.integrate

    def stamp(t):
        return (t.data_ptr(), t._version, tuple(t.shape)) if isinstance(t, torch.Tensor) else t

    def integrate(points3D, viewpoint_camera, pc, pipe, bg_color, kernel_size, scaling_modifier=1.0, override_color=None, subpixel_offset=None):
        if override_color is not None or subpixel_offset is not None or torch.is_grad_enabled():
            return orig(points3D, viewpoint_camera, pc, pipe, bg_color, kernel_size, scaling_modifier, override_color, subpixel_offset)
        cam = viewpoint_camera
        key = (id(cam), getattr(cam, "uid", None), stamp(cam.world_view_transform), stamp(cam.full_proj_transform),
               int(cam.image_width), int(cam.image_height), float(cam.FoVx), float(cam.FoVy), id(pc), int(pc.active_sh_degree),
               tuple(stamp(getattr(pc, n, None)) for n in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation", "filter_3D")),
               stamp(bg_color), float(kernel_size), float(scaling_modifier),
               bool(getattr(pipe, "compute_cov3D_python", False)), bool(getattr(pipe, "convert_SHs_python", False)), bool(getattr(pipe, "debug", False)))
        with DGR.integrate_view_key(key):
            return orig(points3D, viewpoint_camera, pc, pipe, bg_color, kernel_size, scaling_modifier, override_color, subpixel_offset)
    GR.integrate = integrate


class _OsWithInProcessEval:
    """`os` for evaluate_dtu_mesh.py: system("python dtu_eval/eval.py <args>") runs mesh_eval.main(<args>) in this process, every
    other attribute and command is the real os's."""

    def __getattr__(self, name):
        return getattr(os, name)

    @staticmethod
    def system(cmd):
        import shlex
        try:
            words = shlex.split(cmd)
        except ValueError:
            return os.system(cmd)
        if len(words) >= 2 and os.path.basename(words[0]).startswith("python") and words[1].replace("\\", "/").endswith("dtu_eval/eval.py"):
            import mesh_eval
            mesh_eval.main(words[2:])
            return 0
        return os.system(cmd)


def dtu_eval_rebinding(script):
    """the names to replace in `script`'s namespace for the DTU evaluation: {"os": stand-in} for evaluate_dtu_mesh.py"""
    if os.path.basename(script) != "evaluate_dtu_mesh.py" or os.environ.get("GOF_DTU_EVAL_SUBPROCESS", "0") == "1":
        return {}
    return {"os": _OsWithInProcessEval()}


_DTU_PACKAGES = ("trimesh", "skimage", "cv2")


def _is_dtu_script(script):
    return os.path.basename(script) == "evaluate_dtu_mesh.py" and os.environ.get("GOF_DTU_CULL_TORCH", "0") != "1"


def _importable(name):
    import importlib.util
    shim = os.path.join(PKG, "shims_dtu")
    try:
        spec = importlib.util.find_spec(name)
    except (ImportError, ValueError):
        return False
    return spec is not None and not (spec.origin or "").startswith(shim)


def _cull_mesh(cameras, mesh):
    import mesh_cull
    return mesh_cull.cull_mesh(cameras, mesh)


def _load_dtu_camera(DTU):
    import mesh_cull
    return mesh_cull.load_dtu_camera(DTU)


class _TrimeshNamespace:
    """`trimesh` for evaluate_dtu_mesh.py where trimesh is not installed: load() reads the mesh onto the device (mesh_cull.load), any
    other attribute is the import stand-in's (which raises when called)."""

    @staticmethod
    def load(path, *a, **k):
        import mesh_cull
        return mesh_cull.load(path)

    def __getattr__(self, name):
        return getattr(importlib.import_module("trimesh"), name)


def dtu_cull_rebinding(script):
    """the names to replace in `script`'s namespace for the DTU mesh culling: for evaluate_dtu_mesh.py `cull_mesh` always,
    `load_dtu_camera` where cv2 is missing, `trimesh` where trimesh is missing.  The replacements import mesh_cull when they are
    called, not here."""
    if not _is_dtu_script(script):
        return {}
    rebind = {"cull_mesh": _cull_mesh}
    if not _importable("cv2"):
        rebind["load_dtu_camera"] = _load_dtu_camera
    if not _importable("trimesh"):
        rebind["trimesh"] = _TrimeshNamespace()
    return rebind


def add_dtu_shims(script):
    """for evaluate_dtu_mesh.py: the import stand-ins of the packages that are not installed, appended to sys.path (an installed
    package wins; no other script's imports change)"""
    if not _is_dtu_script(script):
        return
    for name in _DTU_PACKAGES:
        shim = os.path.join(PKG, "shims_dtu", name)
        if not _importable(name) and shim not in sys.path:
            sys.path.append(shim)


def add_trimesh_stand_in():
    """for every script: scene/gaussian_model.py:23 and extract_mesh.py:12 import trimesh at module top, and with 10. nothing of it is
    called -- where it is not installed its import stand-in goes LAST on sys.path (an installed trimesh wins)"""
    shim = os.path.join(PKG, "shims_dtu", "trimesh")
    if not _importable("trimesh") and shim not in sys.path:
        sys.path.append(shim)


def add_cv2_stand_in():
    """for every script: train.py:15 imports cv2 at module top and calls nothing of it -- where it is not installed its import stand-in
    goes LAST on sys.path (an installed cv2 wins)"""
    shim = os.path.join(PKG, "shims_dtu", "cv2")
    if not _importable("cv2") and shim not in sys.path:
        sys.path.append(shim)


def add_import_stand_ins():
    """shims/ goes LAST on sys.path when one of the packages it stands in for is not importable: tetranerf and open3d (2., 6.),
    lpips and torchvision (11.), plyfile (13.) and pyrender (18.).  An installed package comes earlier on the path and wins; lpips and plyfile are
    looked up without importing them (the real lpips imports torchvision's models at import)."""
    import importlib.util
    shim = os.path.join(PKG, "shims")
    missing = False
    for mod in ("tetranerf.utils.extension", "open3d"):
        try:
            importlib.import_module(mod)
        except Exception:
            missing = True
    for mod in ("lpips", "torchvision", "plyfile", "pyrender"):
        try:
            missing = missing or importlib.util.find_spec(mod) is None
        except (ImportError, ValueError):
            missing = True
    if missing and shim not in sys.path:
        sys.path.append(shim)


def _torch_extract():
    return os.environ.get("GOF_TORCH_EXTRACT", "0") == "1"


def _get_tetra_points(self, views, near=0.02, far=1e6):
    import mesh_extraction
    return mesh_extraction.get_tetra_points(self, views, near, far)


def rebind_tetra_points():
    """GaussianModel.get_tetra_points (scene/gaussian_model.py:433-463) -> mesh_extraction.get_tetra_points, by name.  The replacement
    imports mesh_extraction when it is called, not here (a script that never extracts a mesh does not load it)."""
    if _torch_extract():
        return
    try:
        from scene.gaussian_model import GaussianModel
    except Exception:
        return
    GaussianModel.get_tetra_points = _get_tetra_points


# the reference's own save_ply / save_fused_ply / load_ply as they were when rebind_model_io replaced them: model_io calls them for a
# model that is not float32 on a ROCm device
_REFERENCE_PLY = {}


def _model_io():
    import model_io
    model_io.reference = _REFERENCE_PLY
    return model_io


def _save_ply(self, path):
    return _model_io().save_ply(self, path)


def _save_fused_ply(self, path):
    return _model_io().save_fused_ply(self, path)


def _load_ply(self, path):
    return _model_io().load_ply(self, path)


def rebind_model_io():
    """GaussianModel.save_ply / save_fused_ply / load_ply (scene/gaussian_model.py:390-430, 486-530) -> model_io's, by name.  The
    replacements import model_io when they are called, not here; GOF_TORCH_PLY=1 leaves the reference's methods in place."""
    if os.environ.get("GOF_TORCH_PLY", "0") == "1":
        return
    try:
        from scene.gaussian_model import GaussianModel
    except Exception:
        return
    for name, new in (("save_ply", _save_ply), ("save_fused_ply", _save_fused_ply), ("load_ply", _load_ply)):
        current = getattr(GaussianModel, name, None)
        if current is None or current is new:
            continue
        _REFERENCE_PLY[name] = current
        setattr(GaussianModel, name, new)


# the reference's own loadCam / cameraList_from_camInfos as they were when rebind_scene_images replaced them: scene_images calls loadCam
# for an image mode the resampler does not take
_REFERENCE_IMAGES = {}


def _scene_images():
    import scene_images
    scene_images.reference = _REFERENCE_IMAGES
    return scene_images


def _load_cam(args, id, cam_info, resolution_scale):
    return _scene_images().load_cam(args, id, cam_info, resolution_scale)


def _camera_list_from_cam_infos(cam_infos, resolution_scale, args):
    return _scene_images().camera_list_from_cam_infos(cam_infos, resolution_scale, args)


# Whether the two functions are rebound without being asked for: decided by the measured loading time (profiles/scene_images_timing.md;
# tests/devtools/dev_scene_images.py measures it).  The output is bit-identical either way; the binding becomes the default once the
# new loader has been shown faster than the reference's at both sizes of that record.  Until then GOF_HIP_IMAGES=1 asks for it.
SCENE_IMAGES_BY_DEFAULT = False


def rebind_scene_images():
    """utils.camera_utils.loadCam / cameraList_from_camInfos (utils/camera_utils.py:19-62) -> scene_images', by name.  The reference's
    utils.camera_utils imports scene.cameras and scene/__init__.py:19 takes cameraList_from_camInfos from it by name -- a cycle that only
    resolves when `scene` is imported first -- so `scene` is imported here and the name in ITS namespace (the one Scene.__init__ calls)
    is rebound together with the two in utils.camera_utils.  The replacements import scene_images when they are called, not here;
    GOF_PIL_IMAGES=1 leaves the reference's functions in place whatever else is set; while the binding is not the default,
    GOF_HIP_IMAGES=1 asks for it."""
    if os.environ.get("GOF_PIL_IMAGES", "0") == "1":
        return
    if not SCENE_IMAGES_BY_DEFAULT and os.environ.get("GOF_HIP_IMAGES", "0") != "1":
        return
    try:
        import scene as ref_scene
        import utils.camera_utils as cu
    except Exception:
        return
    for name, new in (("loadCam", _load_cam), ("cameraList_from_camInfos", _camera_list_from_cam_infos)):
        current = getattr(cu, name, None)
        if current is None or current is new:
            continue
        _REFERENCE_IMAGES[name] = current
        setattr(cu, name, new)
        if getattr(ref_scene, name, None) is current:
            setattr(ref_scene, name, new)


# what torchvision.utils.save_image was when rebind_png_writer replaced it: image_writer calls it for everything but a PNG file of a
# float32 image with 1 or 3 channels
_PREVIOUS_SAVE_IMAGE = {}

# Whether save_image is rebound without being asked for: decided by the measured time of render.py's loop (profiles/png_encode.md;
# tests/devtools/dev_png_encode.py measures it).  Until that record shows the device path faster at both sizes, GOF_HIP_PNG=1 asks for it.
PNG_WRITER_BY_DEFAULT = False


def _image_writer():
    import image_writer
    image_writer.previous = _PREVIOUS_SAVE_IMAGE.get("save_image")
    return image_writer


def _save_image(tensor, fp, format=None, **kwargs):
    return _image_writer().save_image(tensor, fp, format=format, **kwargs)


def rebind_png_writer():
    """torchvision.utils.save_image (render.py:35-36) -> image_writer.save_image, by attribute of the module the script imports (the
    stand-in of shims/ or an installed torchvision).  The replacement imports image_writer when it is called, not here; GOF_PIL_PNG=1
    leaves the function in place whatever else is set; while the binding is not the default, GOF_HIP_PNG=1 asks for it."""
    if os.environ.get("GOF_PIL_PNG", "0") == "1":
        return
    if not PNG_WRITER_BY_DEFAULT and os.environ.get("GOF_HIP_PNG", "0") != "1":
        return
    try:
        import torchvision.utils as tvu
    except Exception:
        return
    current = getattr(tvu, "save_image", None)
    if current is None or current is _save_image:
        return
    _PREVIOUS_SAVE_IMAGE["save_image"] = current
    tvu.save_image = _save_image


# Whether metrics.py's readImages is rebound without being asked for: decided by the measured time of reading one scene's files
# (profiles/png_decode.md).  Until that record shows the device path faster than the script's own loop AND than a Pillow thread pool,
# GOF_HIP_PNG_READ=1 asks for it.
PNG_READER_BY_DEFAULT = False

# the functions a script defined itself under the names run_script replaced: {name: the script's own function}
SCRIPT_OWN = {}


def _read_images_for_metrics(renders_dir, gt_dir):
    import png_reader
    png_reader.previous = SCRIPT_OWN.get("readImages")
    return png_reader.read_images_for_metrics(renders_dir, gt_dir)


def png_reader_rebinding(script):
    """the names to replace in `script`'s namespace for the PNG decoder (metrics.py:25-36): `readImages` for every script that defines
    it.  GOF_PIL_PNG_READ=1 keeps the script's own function whatever else is set; while the binding is not the default,
    GOF_HIP_PNG_READ=1 asks for it.  The replacement imports png_reader when it is called, not here."""
    if os.environ.get("GOF_PIL_PNG_READ", "0") == "1":
        return {}
    if not PNG_READER_BY_DEFAULT and os.environ.get("GOF_HIP_PNG_READ", "0") != "1":
        return {}
    return {"readImages": _read_images_for_metrics}


def flush_png_writer():
    """wait for the files image_writer still holds; re-raises the first error of its writer thread"""
    iw = sys.modules.get("image_writer")
    if iw is not None:
        iw.flush()


def _fused_evaluate_alpha(points, views, gaussians, pipeline, background, kernel_size, return_color=False):
    import mesh_extraction
    return mesh_extraction.evaluate_alpha(points, views, gaussians, pipeline, background, kernel_size, return_color)


def _marching_tetrahedra_with_binary_search(model_path, name, iteration, views, gaussians, pipeline, background, kernel_size, filter_mesh,
                                            texture_mesh, near, far):
    """extract_mesh.py:36-120 -> mesh_extraction's, with the field queried through the `evaluage_alpha` of the script's namespace as it
    is bound when this is called (the launcher's own fused loop: mesh_extraction reads the transmittance directly)"""
    import mesh_extraction
    query = getattr(sys.modules.get("__main__"), "evaluage_alpha", None)
    if query is _fused_evaluate_alpha:
        query = None
    return mesh_extraction.marching_tetrahedra_with_binary_search(model_path, name, iteration, views, gaussians, pipeline, background, kernel_size,
                                                                  filter_mesh, texture_mesh, near, far, evaluate_alpha=query)


def extract_rebinding(script):
    """the names to replace in `script`'s namespace for the mesh extraction: `marching_tetrahedra_with_binary_search` for every script
    that defines it (extract_mesh.py), whether or not trimesh is importable; GOF_TORCH_EXTRACT=1: none"""
    if _torch_extract():
        return {}
    return {"marching_tetrahedra_with_binary_search": _marching_tetrahedra_with_binary_search}


# Whether train.py's L1_loss_appearance is rebound without being asked for: decided by the measured iteration time (DESIGN.md §5,
# profiles/appearance_timing.md).  The HIP path is bit-reproducible; it is the default only where it is no slower than torch's.
APPEARANCE_BY_DEFAULT = False


def _l1_loss_appearance(image, gt_image, gaussians, view_idx, return_transformed_image=False):
    from train_epilogue import appearance
    return appearance.L1_loss_appearance(image, gt_image, gaussians, view_idx, return_transformed_image)


def appearance_rebinding(script):
    """the names to replace in `script`'s namespace for the decoupled-appearance L1 (train.py:67-88): `L1_loss_appearance` for every
    script that defines it.  GOF_TORCH_APPEARANCE=1 (or GOF_TORCH_EPILOGUE=1) keeps the script's own function; while the HIP path is not
    the default, GOF_HIP_APPEARANCE=1 asks for it.  The replacement imports train_epilogue.appearance when it is called, not here."""
    if os.environ.get("GOF_TORCH_APPEARANCE", "0") == "1" or os.environ.get("GOF_TORCH_EPILOGUE", "0") == "1":
        return {}
    if not APPEARANCE_BY_DEFAULT and os.environ.get("GOF_HIP_APPEARANCE", "0") != "1":
        return {}
    return {"L1_loss_appearance": _l1_loss_appearance}


def mesh_components_spec():
    """GOF_MESH_COMPONENTS=<spec> -> the keyword arguments of DeviceMesh.keep_components, None where it is unset or empty; a malformed
    spec raises ValueError (main() asks before the script starts)"""
    spec = os.environ.get("GOF_MESH_COMPONENTS", "")
    if not spec.strip():
        return None
    import mesh_components
    return mesh_components.parse_spec(spec)


# (the name rebound, the directory below <model_path>/<name>/ours_<iteration>, the file it writes, the file written next to it)
CLEAN_MESH_FILES = (("marching_tetrahedra_with_binary_search", "fusion", "mesh_binary_search_7.ply", "mesh_binary_search_7_clean.ply"),
                    ("tsdf_fusion", "tsdf", "tsdf.ply", "tsdf_clean.ply"))


def _with_clean_mesh(fn, subdir, written, clean, criteria):
    def run(model_path, name, iteration, *args, **kwargs):
        out = fn(model_path, name, iteration, *args, **kwargs)       # (writes its file as always, first)
        import mesh_components
        folder = os.path.join(model_path, name, "ours_{}".format(iteration), subdir)
        kept, dropped = mesh_components.clean_file(os.path.join(folder, written), os.path.join(folder, clean), **criteria)
        print("mesh components: kept %d of %d -> %s" % (kept, kept + dropped, os.path.join(folder, clean)))
        return out
    return run


def mesh_components_rebinding(rebind):
    """the entries of `rebind` that write a mesh, wrapped so that the cleaned mesh is written next to theirs -- only where
    GOF_MESH_COMPONENTS is set (17.); a name that is not rebound (GOF_TORCH_EXTRACT=1) is left alone"""
    criteria = mesh_components_spec()
    if criteria is None:
        return {}
    return {name: _with_clean_mesh(rebind[name], subdir, written, clean, criteria) for name, subdir, written, clean in CLEAN_MESH_FILES
            if name in rebind}


def mesh_simplify_spec():
    """GOF_MESH_SIMPLIFY=<spec> -> the keyword arguments of DeviceMesh.simplify, None where it is unset or empty; a malformed spec
    raises ValueError (main() asks before the script starts)"""
    spec = os.environ.get("GOF_MESH_SIMPLIFY", "")
    if not spec.strip():
        return None
    import mesh_simplify
    return mesh_simplify.parse_spec(spec)


SIMPLIFIED_MESH_FILES = {"mesh_binary_search_7.ply": "mesh_binary_search_7_simplified.ply", "tsdf.ply": "tsdf_simplified.ply"}


def _with_simplified_mesh(fn, subdir, written, clean, how):
    def run(model_path, name, iteration, *args, **kwargs):
        out = fn(model_path, name, iteration, *args, **kwargs)       # (writes its file, and with GOF_MESH_COMPONENTS the cleaned one, first)
        import mesh_simplify
        folder = os.path.join(model_path, name, "ours_{}".format(iteration), subdir)
        src = os.path.join(folder, clean if mesh_components_spec() is not None else written)
        dst = os.path.join(folder, SIMPLIFIED_MESH_FILES[written])
        st = mesh_simplify.simplify_file(src, dst, **how)
        print("mesh simplify: %d -> %d faces (cell %.9g) -> %s" % (st["faces_before"], st["faces_after"], st["cell"], dst))
        return out
    return run


def mesh_simplify_rebinding(rebind):
    """the entries of `rebind` that write a mesh (after mesh_components_rebinding has wrapped them), wrapped so that the simplified mesh
    is written next to theirs -- only where GOF_MESH_SIMPLIFY is set (17.); the cleaned mesh is the input where GOF_MESH_COMPONENTS is
    set as well"""
    how = mesh_simplify_spec()
    if how is None:
        return {}
    return {name: _with_simplified_mesh(rebind[name], subdir, written, clean, how) for name, subdir, written, clean in CLEAN_MESH_FILES
            if name in rebind}


def _tnt_mesher(*args, **kwargs):
    import mesh_cull
    return mesh_cull.TntMesher(*args, **kwargs)


def _tnt_render_depth(mesh, c2w_list, H, W, fx, fy, cx, cy, far=20.0):
    import mesh_cull
    return list(mesh_cull.render_depth(mesh, c2w_list, H, W, fx, fy, cx, cy, zfar=far))


def tnt_cull_rebinding(script):
    """the names to replace in `script`'s namespace for the Tanks-and-Temples mesh culling (18.): `Mesher` and
    `extract_depth_from_mesh`, for a script that defines both (eval_tnt/cull_mesh.py).  The replacements import mesh_cull when they are
    called, not here."""
    import ast
    if os.environ.get("GOF_TNT_CULL_TORCH", "0") == "1" or not os.path.isfile(script):
        return {}
    with open(script, "rb") as f:
        try:
            tree = ast.parse(f.read(), filename=script)
        except SyntaxError:
            return {}
    defined = {n.name for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef))}
    if not {"Mesher", "extract_depth_from_mesh"} <= defined:
        return {}
    return {"Mesher": _tnt_mesher, "extract_depth_from_mesh": _tnt_render_depth}


def _tnt_eval_main(argv):
    import tnt_eval
    return tnt_eval.main(argv)


def tnt_eval_rebinding(script):
    """what replaces `script` as a whole for the Tanks-and-Temples evaluation: {"main": tnt_eval's command line} for eval_tnt/run.py"""
    if not os.path.abspath(script).replace(os.sep, "/").endswith("eval_tnt/run.py") or os.environ.get("GOF_TNT_EVAL_SUBPROCESS", "0") == "1":
        return {}
    return {"main": _tnt_eval_main}


def _mesh_viewer_main(argv):
    import mesh_render
    if len(argv) != 1:
        print("Usage: mesh_viewer.py path_to_ply_file")
        return 2
    return mesh_render.main([argv[0], "--turntable", "8", "--mode", "shaded", "--out", argv[0] + "_views"])


def mesh_viewer_rebinding(script):
    """what replaces `script` as a whole for the mesh viewer (19.): {"main": mesh_render's command line over a turntable} for
    mesh_viewer.py, unless GOF_MESH_VIEWER_WINDOW=1 asks for the script's own window"""
    if os.path.basename(script) != "mesh_viewer.py" or os.environ.get("GOF_MESH_VIEWER_WINDOW", "0") == "1":
        return {}
    return {"main": _mesh_viewer_main}


def main():
    if len(sys.argv) < 2:
        print(__doc__)
        sys.exit(2)
    script = os.path.abspath(sys.argv[1])
    viewer = mesh_viewer_rebinding(script)
    if viewer:
        sys.path.insert(0, PKG)
        sys.exit(viewer["main"](sys.argv[2:]))
    tnt = tnt_eval_rebinding(script)
    if tnt:
        sys.path.insert(0, PKG)
        tnt["main"](sys.argv[2:])
        return
    if script.replace(os.sep, "/").endswith("dtu_eval/eval.py") and os.environ.get("GOF_DTU_EVAL_SUBPROCESS", "0") != "1":
        sys.path.insert(0, PKG)
        import mesh_eval
        mesh_eval.main(sys.argv[2:])
        return
    ref_root = os.path.dirname(script)
    sys.path.insert(0, ref_root)
    sys.path.insert(0, PKG)
    add_import_stand_ins()
    add_dtu_shims(script)
    add_trimesh_stand_in()
    add_cv2_stand_in()
    import diff_gaussian_rasterization  # noqa: F401  fail early and loudly if libgof_hip.so is missing
    if os.environ.get("GOF_STATS_JSON"):
        # the binding's counters of the whole run (frames redone for a pool / capacity learnt too small, read-backs, shapes that inherited
        # their pools across a densification: _backend._stats) written at exit -- evidence runs read them (tests/devtools/dev_r6_trajectory.py)
        import atexit
        import json

        def _dump_stats(path=os.environ["GOF_STATS_JSON"]):
            st = getattr(getattr(diff_gaussian_rasterization, "_C", None), "_stats", None)
            if st is not None:
                st = dict(st)
                d = sys.modules.get("train_epilogue.deferred")
                if d is not None:                       # how many iterations' losses were one fused call / fell back to the eager mirrors
                    st["deferred_loss"] = dict(d.stats)
                ap = sys.modules.get("train_epilogue.appearance")
                if ap is not None:                      # how many appearance L1s ran on the HIP unit (12.)
                    st["appearance"] = dict(ap.stats)
                with open(path, "w") as f:
                    json.dump(st, f)
        atexit.register(_dump_stats)
    try:
        import utils.tetmesh as ref_tetmesh
        import tetmesh as hip_tetmesh
        ref_tetmesh.marching_tetrahedra = hip_tetmesh.marching_tetrahedra
    except ImportError:
        pass
    if os.environ.get("GOF_TORCH_EPILOGUE", "0") != "1":
        rebind_train_epilogue()
    rebind_tetra_points()
    rebind_model_io()
    rebind_scene_images()
    rebind_png_writer()
    if os.environ.get("GOF_INTEGRATE_CACHE_GB", "") not in ("0", "0.0"):
        rebind_integrate_with_view_cache()
    sys.argv = [script] + sys.argv[2:]
    rebind = {}
    if os.environ.get("GOF_TORCH_VIEW_REDUCE", "0") != "1":
        # extract_mesh.py:17-34: the script's own view loop -> the one whose min / arg-min reduction is fused into the point pass
        rebind["evaluage_alpha"] = _fused_evaluate_alpha
    rebind.update(extract_rebinding(script))
    # extract_mesh_tsdf.py:16-83: the script's Open3D VoxelBlockGrid loop -> the HIP TSDF fusion (csrc/tsdf.hip)
    import tsdf_fusion
    rebind["tsdf_fusion"] = tsdf_fusion.tsdf_fusion
    rebind.update(dtu_eval_rebinding(script))
    rebind.update(dtu_cull_rebinding(script))
    rebind.update(appearance_rebinding(script))
    rebind.update(png_reader_rebinding(script))
    rebind.update(tnt_cull_rebinding(script))
    rebind.update(mesh_components_rebinding(rebind))
    rebind.update(mesh_simplify_rebinding(rebind))
    try:
        run_script(script, rebind)
    except BaseException:
        try:
            flush_png_writer()                  # (the files queued before the script failed are still written; its own error is the one reported)
        except Exception:
            pass
        raise
    flush_png_writer()


def _is_main_guard(node):
    """`if __name__ == "__main__":` at module level"""
    import ast
    if not isinstance(node, ast.If) or not isinstance(node.test, ast.Compare) or len(node.test.ops) != 1:
        return False
    t = node.test
    sides = [t.left, t.comparators[0]]
    return (isinstance(t.ops[0], ast.Eq) and any(isinstance(x, ast.Name) and x.id == "__name__" for x in sides)
            and any(isinstance(x, ast.Constant) and x.value == "__main__" for x in sides))


def run_script(script, rebind):
    """Run `script` as __main__.  Functions the script DEFINES ITSELF (extract_mesh.py's evaluage_alpha) cannot be rebound through an
    imported module: when the script defines one of the names in `rebind`, its module body is executed first WITHOUT the
    `if __name__ == "__main__":` block(s), the names are replaced in its namespace, then the guarded block(s) run -- the script's
    text is untouched and every statement runs exactly once, in order (the guard blocks are at the end of the reference's scripts)."""
    import ast
    import types
    with open(script, "rb") as f:
        src = f.read()
    tree = ast.parse(src, filename=script)
    defined = {n.name for n in tree.body if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef))}      # (a class: 18.'s Mesher)
    # (and the modules it imports under their own name at top level: evaluate_dtu_mesh.py's `import os`)
    defined |= {a.asname or a.name for n in tree.body if isinstance(n, ast.Import) for a in n.names if "." not in (a.asname or a.name)}
    names = [k for k in rebind if k in defined]
    guards = [n for n in tree.body if _is_main_guard(n)]
    # only split when every guard block comes after everything else (otherwise the order of execution would change)
    tail_ok = bool(guards) and all(_is_main_guard(n) for n in tree.body[len(tree.body) - len(guards):])
    if not names or not tail_ok:
        runpy.run_path(script, run_name="__main__")
        return
    mod = types.ModuleType("__main__")
    mod.__file__ = script
    mod.__builtins__ = __builtins__
    prev_main = sys.modules.get("__main__")
    sys.modules["__main__"] = mod
    try:
        head = ast.Module(body=[n for n in tree.body if not _is_main_guard(n)], type_ignores=[])
        exec(compile(head, script, "exec"), mod.__dict__)
        for k in names:
            SCRIPT_OWN[k] = mod.__dict__.get(k)
            mod.__dict__[k] = rebind[k]
        exec(compile(ast.Module(body=guards, type_ignores=[]), script, "exec"), mod.__dict__)
    finally:
        if prev_main is not None:
            sys.modules["__main__"] = prev_main


if __name__ == "__main__":
    main()
