"""The launcher's opt-in mesh simplification (run_reference_script.py 17.): GOF_MESH_SIMPLIFY=<spec> makes the
replacements of extract_mesh.py's `marching_tetrahedra_with_binary_search` and extract_mesh_tsdf.py's `tsdf_fusion` write one more file
next to the one they always wrote.  As in tests/test_mesh_components_launcher.py a synthetic script defines the two names and calls them
and the functions bound in their place are stand-ins that write a known mesh: unset, no extra file appears and the original bytes are
what they were; set, the extra file holds the restatement's simplified mesh; with GOF_MESH_COMPONENTS as well, the cleaned mesh is the
input; a malformed spec is refused before the script runs.  The simplification itself runs through the host emulator, in a child."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
import host_child  # noqa: E402
from host_child import PKG  # noqa: E402
import mesh_components_restatement as RC  # noqa: E402
import mesh_simplify_cases as K  # noqa: E402
import mesh_simplify_restatement as R  # noqa: E402
from test_mesh_components_launcher import SCRIPT, launcher  # noqa: E402

FILES = {"fusion": ("mesh_binary_search_7.ply", "mesh_binary_search_7_clean.ply", "mesh_binary_search_7_simplified.ply"),
         "tsdf": ("tsdf.ply", "tsdf_clean.ply", "tsdf_simplified.ply")}
CELL = 0.3


def mesh():
    """an icosphere and a floater of four faces far away -> (V, F, N, Col), coordinates as the file holds them"""
    V, F, N, Col, _, _ = K.icosphere(3)
    V = np.vstack([V, K.icosphere(0)[0][:6] * 0.05 + 3.0])
    F = np.vstack([F, K.strip(4, len(V) - 6)])
    N2, C2 = K._attrs(len(V), 5)
    return V.astype(np.float32).astype(np.float64), F.astype(np.int32), N2, C2


def _child(case, out):
    import mesh_cull as M
    import mesh_components as MC
    import mesh_render as MR
    import mesh_simplify as MS
    import tsdf_fusion
    check = host_child.install_seams(M, MC, MR, MS, buffers="all")
    L = launcher()
    tmp = os.path.dirname(out)
    model = os.path.join(tmp, "model")
    script = os.path.join(tmp, "extract_mesh.py")
    open(script, "w").write(SCRIPT)
    V, F, N, Col = mesh()

    def folder(model_path, name, iteration, sub):
        d = os.path.join(model_path, name, "ours_{}".format(iteration), sub)
        os.makedirs(d, exist_ok=True)
        return d

    def extraction(model_path, name, iteration, *rest):
        M.DeviceMesh(V, F, None, Col).export(os.path.join(folder(model_path, name, iteration, "fusion"), FILES["fusion"][0]))

    def fusion(model_path, name, iteration, *rest):
        tsdf_fusion.write_ply(os.path.join(folder(model_path, name, iteration, "tsdf"), FILES["tsdf"][0]), V, F, Col / 255.0, N)
    simplify, components = case.split("|")
    for var, spec in (("GOF_MESH_SIMPLIFY", simplify), ("GOF_MESH_COMPONENTS", components)):
        if spec:
            os.environ[var] = spec
        else:
            os.environ.pop(var, None)
    rebind = {"marching_tetrahedra_with_binary_search": extraction, "tsdf_fusion": fusion}
    res = {}
    try:
        rebind.update(L.mesh_components_rebinding(rebind))
        rebind.update(L.mesh_simplify_rebinding(rebind))
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
        for tag, name in zip(("written", "clean", "simplified"), names):
            p = os.path.join(d, name)
            if os.path.exists(p):
                res["%s_%s" % (sub, tag)] = np.frombuffer(open(p, "rb").read(), np.uint8)
    res["buffers"] = np.array(check())
    np.savez(out, **res)


def _originals():
    V, F, N, Col = mesh()
    tsdf_colours = np.round(np.clip(Col / 255.0, 0.0, 1.0) * 255.0).astype(np.uint8)
    return {"fusion": (V, F, None, Col), "tsdf": (V, F, N, tsdf_colours)}


def test_unset_nothing_differs(tmp_path):
    res = host_child.run_child(__file__, "|", tmp_path, timeout=600)
    assert str(res["refused"]) == "" and bool(res["script_ran"])
    for sub, names in FILES.items():
        assert str(res[sub + "_files"]) == names[0] and sub + "_simplified" not in res
        assert res[sub + "_written"].tobytes() == R.ply_bytes(*_originals()[sub])


@pytest.mark.parametrize("spec,how", [("cell:%r" % CELL, dict(h=CELL)), ("cell:%r,dedupe:0" % CELL, dict(h=CELL, dedupe=False))])
def test_the_simplified_file_is_written_next_to_the_original(spec, how, tmp_path):
    res = host_child.run_child(__file__, spec + "|", tmp_path, timeout=600)
    assert str(res["refused"]) == "" and int(res["buffers"]) > 0
    for sub, names in FILES.items():
        V, F, N, Col = _originals()[sub]
        assert str(res[sub + "_files"]) == ",".join(sorted((names[0], names[2])))
        assert res[sub + "_written"].tobytes() == R.ply_bytes(V, F, N, Col)                  # written first, byte for byte what it is without the variable
        r = R.simplify(V, F, N, Col, **how)
        assert 0 < len(r["f"]) < len(F) and res[sub + "_simplified"].tobytes() == R.ply_bytes(r["v"], r["f"], r["n"], r["c"])


def test_with_components_the_cleaned_mesh_is_the_input(tmp_path):
    res = host_child.run_child(__file__, "grid:8|largest:1", tmp_path, timeout=600)
    assert str(res["refused"]) == ""
    for sub, names in FILES.items():
        V, F, N, Col = _originals()[sub]
        assert str(res[sub + "_files"]) == ",".join(sorted(names))
        v, f, n, c, kept, dropped = RC.keep_components(V, F, N, Col, largest=1)
        assert (kept, dropped) == (1, 1) and res[sub + "_clean"].tobytes() == R.ply_bytes(v, f, n, c)
        v = v.astype(np.float32).astype(np.float64)                                          # the cleaned FILE is what is read
        r = R.simplify(v, f, n, c, np.ptp(v, axis=0).max() / 8.0)
        assert res[sub + "_simplified"].tobytes() == R.ply_bytes(r["v"], r["f"], r["n"], r["c"])
        whole = R.simplify(V, F, N, Col, np.ptp(V, axis=0).max() / 8.0)
        assert len(whole["v"]) != len(r["v"])                                                # (the floater would have changed the grid)


@pytest.mark.parametrize("spec", ["grid", "cells:3", "grid:4;dedupe:0", "dedupe:1", "grid:4,cell:0.1"])
def test_a_malformed_spec_is_refused_before_the_script_starts(spec, tmp_path):
    res = host_child.run_child(__file__, spec + "|", tmp_path, timeout=600)
    assert "GOF_MESH_SIMPLIFY" in str(res["refused"]) and not bool(res["script_ran"])


def test_the_launcher_asks_before_the_script(monkeypatch):
    L = launcher()
    src = open(os.path.join(PKG, "launch", "run_reference_script.py")).read()
    assert src.index("rebind.update(mesh_components_rebinding(rebind))") < src.index("rebind.update(mesh_simplify_rebinding(rebind))") \
        < src.index("        run_script(script, rebind)")
    monkeypatch.delenv("GOF_MESH_SIMPLIFY", raising=False)
    assert L.mesh_simplify_rebinding({"tsdf_fusion": len}) == {}
    monkeypatch.setenv("GOF_MESH_SIMPLIFY", "grid:64")
    out = L.mesh_simplify_rebinding({"tsdf_fusion": len, "evaluage_alpha": len})
    assert set(out) == {"tsdf_fusion"} and out["tsdf_fusion"] is not len
    monkeypatch.setenv("GOF_MESH_SIMPLIFY", "grid:x")
    with pytest.raises(ValueError, match="GOF_MESH_SIMPLIFY"):
        L.mesh_simplify_rebinding({"tsdf_fusion": len})


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
