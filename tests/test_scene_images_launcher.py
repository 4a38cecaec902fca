"""Needs the reference's Python scripts as __graft_entry__.build() stages them (oracle/_ref/refpy, byte-identical copies; skipped where
they were not staged) and Pillow: item 14 of launch/run_reference_script.py -- utils.camera_utils.loadCam / cameraList_from_camInfos become
scene_images', and load_cam hands Camera what the reference's own loadCam hands it.  On the CPU the kernels run through the host
emulator (tests/hipemu) and both functions are given a recording stand-in for Camera (the real one calls .cuda()); the case
"real_camera" is run by tests/test_scene_images_gpu.py on the device with the reference's Camera on both sides.

Every case runs in a child process with the launcher's own path set-up: the cases change sys.path and import the reference's packages."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "refpy")
PKG = os.path.join(ROOT, "gaussian-opacity-fields_amd")
pytestmark = pytest.mark.skipif(not os.path.isdir(REF), reason="oracle/_ref/refpy not staged (build() stages it where the reference exists)")

RESOLUTIONS = (1, 2, 4, 8, -1, 37)
SCALES = (1.0, 2.0)


def _launcher():
    import importlib.util
    spec = importlib.util.spec_from_file_location("gof_launcher", os.path.join(PKG, "launch", "run_reference_script.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _set_up_paths(L):
    sys.path.insert(0, REF)
    sys.path.insert(0, PKG)
    L.add_import_stand_ins()
    L.add_trimesh_stand_in()
    L.add_cv2_stand_in()


def _scene(tmp, R):
    rng = np.random.default_rng(11)
    files = [("rgb", "RGB", rng.integers(0, 256, (67, 101, 3), dtype=np.uint8)), ("rgba", "RGBA", rng.integers(0, 256, (31, 53, 4), dtype=np.uint8)),
             ("l", "L", rng.integers(0, 256, (30, 40), dtype=np.uint8)), ("wide", "RGB", rng.integers(0, 256, (5, 1604, 3), dtype=np.uint8))]
    # (the 1604 x 5 image serves the -1 branch alone: Pillow itself refuses the height of 0 that most other settings give it)
    return lambda tag, res: R.write_scene(os.path.join(tmp, tag), files=files if res == -1 else files[:3])


def _child(case, tmp):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))
    import scene_images_cases as K
    import scene_images_runs as R
    L = _launcher()
    _set_up_paths(L)
    out = {}
    if case in ("rebound", "pil_images", "default"):
        import scene as ref_scene
        import utils.camera_utils as cu
        orig = {n: getattr(cu, n) for n in ("loadCam", "cameraList_from_camInfos")}
        L.rebind_scene_images()
        out["rebound"] = {n: getattr(cu, n) is not orig[n] for n in orig}
        out["to_launcher"] = {"loadCam": cu.loadCam is L._load_cam, "cameraList_from_camInfos": cu.cameraList_from_camInfos is L._camera_list_from_cam_infos}
        out["scene_name"] = ref_scene.cameraList_from_camInfos is cu.cameraList_from_camInfos
        out["kept"] = {n: L._REFERENCE_IMAGES.get(n) is orig[n] for n in orig}
        if case == "rebound":
            import scene_images as SI
            import test_scene_images_host as TH
            TH.host_seams(SI)
            cu.Camera = R.RecordingCamera
            make = _scene(tmp, R)
            bad = []
            for res in RESOLUTIONS:
                for scale in SCALES:
                    ref = [orig["loadCam"](R.Args(res), i, c, scale) for i, c in enumerate(make("ref_%s_%s" % (res, scale), res))]
                    new = [cu.loadCam(R.Args(res), i, c, scale) for i, c in enumerate(make("new_%s_%s" % (res, scale), res))]
                    pool = cu.cameraList_from_camInfos(make("pool_%s_%s" % (res, scale), res), scale, R.Args(res))
                    for a, b, c in zip(ref, new, pool):
                        for x in (b, c):
                            same = (K.same_bits(a.image.contiguous().numpy(), x.image.contiguous().numpy()) and (a.gt_alpha_mask is None) == (x.gt_alpha_mask is None)
                                    and (a.gt_alpha_mask is None or K.same_bits(a.gt_alpha_mask.contiguous().numpy(), x.gt_alpha_mask.contiguous().numpy()))
                                    and {k: v for k, v in a.fields.items() if k not in ("R", "T")} == {k: v for k, v in x.fields.items() if k not in ("R", "T")}
                                    and a.fields["R"] is not None and np.array_equal(a.fields["R"], x.fields["R"]) and np.array_equal(a.fields["T"], x.fields["T"]))
                            if not same:
                                bad.append([res, scale, a.fields["image_name"]])
                    if res == -1 and scale == 1.0:
                        out["wide_size"] = list(new[3].image.shape)
            out["bad"] = bad
            out["compared"] = len(RESOLUTIONS) * len(SCALES) * 3 + len(SCALES)
            out["reference_is_the_launchers"] = SI.reference is L._REFERENCE_IMAGES
    elif case == "real_camera":
        os.environ["GOF_HIP_IMAGES"] = "1"
        import torch
        import scene as ref_scene  # noqa: F401
        import utils.camera_utils as cu
        orig = cu.loadCam
        L.rebind_scene_images()
        assert cu.loadCam is not orig
        make = _scene(tmp, R)
        for res in RESOLUTIONS:
            for scale in SCALES:
                ref = [orig(R.Args(res), i, c, scale) for i, c in enumerate(make("ref_%s_%s" % (res, scale), res))]
                new = cu.cameraList_from_camInfos(make("new_%s_%s" % (res, scale), res), scale, R.Args(res))
                for a, b in zip(ref, new):
                    assert type(a) is type(b) and a.uid == b.uid and a.image_name == b.image_name and a.colmap_id == b.colmap_id
                    assert (a.image_width, a.image_height) == (b.image_width, b.image_height)
                    assert b.original_image.is_cuda and torch.equal(a.original_image.contiguous().view(torch.int32), b.original_image.contiguous().view(torch.int32)), (res, scale, a.image_name)
                    assert (a.gt_alpha_mask is None) == (b.gt_alpha_mask is None)
                    assert a.gt_alpha_mask is None or torch.equal(a.gt_alpha_mask.contiguous().view(torch.int32), b.gt_alpha_mask.contiguous().view(torch.int32))
        torch.cuda.synchronize()
        print("RESULT ok")
        return
    else:
        raise KeyError(case)
    print("RESULT " + json.dumps(out))


def _run(case, tmp_path, env=None):
    sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))
    import host_child
    e = dict(os.environ, GOF_HIP_LIB=host_child.emulated_library())
    for k in ("GOF_PIL_IMAGES", "GOF_HIP_IMAGES"):
        e.pop(k, None)
    e.update(env or {})
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case, str(tmp_path)], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "%s failed (rc %d):\n%s\n%s" % (case, r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0][7:])


def test_both_functions_are_rebound_and_hand_camera_the_references_tensors(tmp_path):
    pytest.importorskip("PIL")
    out = _run("rebound", tmp_path, env={"GOF_HIP_IMAGES": "1"})
    both = {"loadCam": True, "cameraList_from_camInfos": True}
    assert out["rebound"] == both and out["to_launcher"] == both and out["kept"] == both and out["scene_name"]
    assert out["bad"] == [] and out["compared"] == 38 and out["reference_is_the_launchers"]
    assert out["wide_size"] == [3, 4, 1600]                 # 1604 x 5 at -r -1: scaled to a width of 1600


def test_gof_pil_images_leaves_the_reference_alone(tmp_path):
    out = _run("pil_images", tmp_path, env={"GOF_PIL_IMAGES": "1", "GOF_HIP_IMAGES": "1"})
    none = {"loadCam": False, "cameraList_from_camInfos": False}
    assert out["rebound"] == none and out["kept"] == none and out["scene_name"]


def test_the_binding_is_opt_in(tmp_path):
    """the loader has not been timed against the reference's on the device yet (profiles/scene_images_timing.md): without
    GOF_HIP_IMAGES=1 the launcher leaves the reference's functions in place"""
    out = _run("default", tmp_path)
    assert out["rebound"] == {"loadCam": False, "cameraList_from_camInfos": False}


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
