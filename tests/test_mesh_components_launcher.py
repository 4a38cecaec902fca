"""The launcher's opt-in mesh cleaning (run_reference_script.py 17.): GOF_MESH_COMPONENTS=<spec> makes the replacements
of extract_mesh.py's `marching_tetrahedra_with_binary_search` and extract_mesh_tsdf.py's `tsdf_fusion` write a second file next to the
one they always wrote.  A synthetic script defines the two names and calls them; the functions the launcher binds in their place are
stand-ins that write a known mesh where the real ones write theirs, so the test is about the launcher: unset, no extra file appears and
the original bytes are what they were; with `largest:1` the extra file holds exactly the largest component; a malformed spec is refused
before the script runs.  The cleaning itself runs through the host emulator, in a child process."""
import importlib.util
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
import host_child  # noqa: E402
from host_child import PKG  # noqa: E402
import mesh_components_cases as K  # noqa: E402
import mesh_components_restatement as R  # noqa: E402

SCRIPT = (
    "def marching_tetrahedra_with_binary_search(model_path, name, iteration, *rest):\n"
    "    raise SystemExit('the script\\'s own extraction ran')\n"
    "def tsdf_fusion(model_path, name, iteration, *rest):\n"
    "    raise SystemExit('the script\\'s own fusion ran')\n"
    "if __name__ == '__main__':\n"
    "    import sys\n"
    "    marching_tetrahedra_with_binary_search(sys.argv[1], 'test', 30000, 'views', 'gaussians', 'pipe', 'bg', 0.0, True, True, 0.02, 1e6)\n"
    "    tsdf_fusion(sys.argv[1], 'test', 30000, 'views', 'gaussians', 'pipe', 'bg', 0.0)\n")
FILES = {"fusion": ("mesh_binary_search_7.ply", "mesh_binary_search_7_clean.ply"), "tsdf": ("tsdf.ply", "tsdf_clean.ply")}


def launcher():
    spec = importlib.util.spec_from_file_location("gof_launcher_components", os.path.join(PKG, "launch", "run_reference_script.py"))
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)
    return L


def _child(case, out):
    import mesh_cull as M
    import mesh_components as MC
    import tsdf_fusion
    check = host_child.install_seams(M, MC, buffers="all")
    L = launcher()
    tmp = os.path.dirname(out)
    model = os.path.join(tmp, "model_" + case.replace(":", "_"))
    script = os.path.join(tmp, "extract_mesh.py")
    open(script, "w").write(SCRIPT)
    V, F, N, Col = K.keep_mesh()

    def folder(model_path, name, iteration, sub):
        d = os.path.join(model_path, name, "ours_{}".format(iteration), sub)
        os.makedirs(d, exist_ok=True)
        return d

    def extraction(model_path, name, iteration, *rest):       # what mesh_extraction's writes: a DeviceMesh with colours, no normals
        M.DeviceMesh(V, F, None, Col).export(os.path.join(folder(model_path, name, iteration, "fusion"), FILES["fusion"][0]))
        return "mesh"

    def fusion(model_path, name, iteration, *rest):           # what tsdf_fusion writes
        tsdf_fusion.write_ply(os.path.join(folder(model_path, name, iteration, "tsdf"), FILES["tsdf"][0]), V, F, Col / 255.0, N)
    kind, spec = case.split(":", 1)
    if spec:
        os.environ["GOF_MESH_COMPONENTS"] = spec
    else:
        os.environ.pop("GOF_MESH_COMPONENTS", None)
    rebind = {"marching_tetrahedra_with_binary_search": extraction, "tsdf_fusion": fusion}
    res = {}
    try:
        rebind.update(L.mesh_components_rebinding(rebind))
        res["refused"] = np.array("")
    except ValueError as e:
        res["refused"] = np.array(str(e))
    if not str(res["refused"]):
        argv = sys.argv
        sys.argv = [script, model]
        try:
            L.run_script(script, rebind)
        finally:
            sys.argv = argv
    res["script_ran"] = np.array(os.path.isdir(model))
    for sub, names in FILES.items():
        d = os.path.join(model, "test", "ours_30000", sub)
        res[sub + "_files"] = np.array(",".join(sorted(os.listdir(d))) if os.path.isdir(d) else "")
        for tag, name in zip(("written", "clean"), names):
            p = os.path.join(d, name)
            if os.path.exists(p):
                res["%s_%s" % (sub, tag)] = np.frombuffer(open(p, "rb").read(), np.uint8)
    res["buffers"] = np.array(check())
    np.savez(out, **res)


def _originals():
    V, F, N, Col = K.keep_mesh()
    tsdf_colours = np.round(np.clip(Col / 255.0, 0.0, 1.0) * 255.0).astype(np.uint8)
    return {"fusion": R.ply_bytes(V, F, None, Col), "tsdf": R.ply_bytes(V, F, N, tsdf_colours)}


def test_unset_nothing_differs(tmp_path):
    res = host_child.run_child(__file__, "unset:", tmp_path, timeout=600)
    assert str(res["refused"]) == "" and bool(res["script_ran"])
    for sub, (written, _) in FILES.items():
        assert str(res[sub + "_files"]) == written and sub + "_clean" not in res
        assert res[sub + "_written"].tobytes() == _originals()[sub]


@pytest.mark.parametrize("spec,criteria", [("largest:1", dict(largest=1)), ("min_area_ratio:0.05,connectivity:vertex", dict(min_area_ratio=0.05, connectivity="vertex"))])
def test_the_clean_file_holds_the_selected_components(spec, criteria, tmp_path):
    res = host_child.run_child(__file__, "set:" + spec, tmp_path, timeout=600)
    assert str(res["refused"]) == "" and int(res["buffers"]) > 0
    V, F, N, Col = K.keep_mesh()
    for sub, names in FILES.items():
        assert str(res[sub + "_files"]) == ",".join(sorted(names))
        assert res[sub + "_written"].tobytes() == _originals()[sub]                      # written first, byte for byte what it is without the variable
        n = N if sub == "tsdf" else None
        v, f, n2, c2, kept, _ = R.keep_components(V, F, n, Col, **criteria)
        assert res[sub + "_clean"].tobytes() == R.ply_bytes(v, f, n2, c2)
        if spec == "largest:1":
            assert kept == 1 and len(f) == 40 and np.array_equal(v, V[:42])              # exactly the largest component (the first of the two of 40 faces)


@pytest.mark.parametrize("spec", ["largest", "biggest:1", "largest:1;by:area", "connectivity:vertex"])
def test_a_malformed_spec_is_refused_before_the_script_starts(spec, tmp_path):
    res = host_child.run_child(__file__, "bad:" + spec, tmp_path, timeout=600)
    assert "GOF_MESH_COMPONENTS" in str(res["refused"]) and not bool(res["script_ran"])


def test_the_launcher_asks_before_the_script(monkeypatch):
    """main() builds the rebinding, and with it parses the spec, before run_script; other scripts' names are left alone"""
    L = launcher()
    src = open(os.path.join(PKG, "launch", "run_reference_script.py")).read()
    assert src.index("rebind.update(mesh_components_rebinding(rebind))") < src.index("        run_script(script, rebind)")
    monkeypatch.delenv("GOF_MESH_COMPONENTS", raising=False)
    assert L.mesh_components_rebinding({"tsdf_fusion": len}) == {}
    monkeypatch.setenv("GOF_MESH_COMPONENTS", "largest:1")
    out = L.mesh_components_rebinding({"tsdf_fusion": len, "evaluage_alpha": len})
    assert set(out) == {"tsdf_fusion"} and out["tsdf_fusion"] is not len
    monkeypatch.setenv("GOF_MESH_COMPONENTS", "largest:x")
    with pytest.raises(ValueError, match="GOF_MESH_COMPONENTS"):
        L.mesh_components_rebinding({"tsdf_fusion": len})


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
