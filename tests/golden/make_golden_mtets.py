"""Generates tests/golden/ref_mtets_golden.npz by IMPORTING the reference's utils/tetmesh.py from /root/reference and running its
marching_tetrahedra on the CPU on every case of tests/mtets_cases.py's golden classes (run in the build container only; the GPU box
has no /root/reference and only reads the committed .npz).

Outputs only: per case the edge ids and faces (int32: every id is below 2^31) and the bit patterns of the end points' positions, sdf
and scales (uint32, so NaN payloads count), or -- for a case whose outputs exceed mtets_cases.INLINE_BYTES -- the sha256 of each of
these arrays; the counts (E, F); and the sha256 of the case's inputs, which are regenerated from the seed, never stored.
`big_chunked` (32 Mi + 17 tets: the reference's own chunk loop, tetmesh.py:55-95) keeps digests of ids and faces only; it needs about
12 GB and a few minutes, `--skip-big` carries its entries over from the existing file.  The archive is written with fixed
timestamps, so a regeneration is byte-for-byte the committed file.  No reference code is copied: the function is called where it lies."""
import io
import os
import sys
import zipfile

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, "gaussian-opacity-fields_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from utils.tetmesh import marching_tetrahedra           # noqa: E402

import mtets_cases as MC                                # noqa: E402

OUT = os.path.join(HERE, "ref_mtets_golden.npz")


def reference(verts, tets, sdf, scales):
    t = lambda a: torch.from_numpy(a if a.flags.writeable else a.copy())      # noqa: E731  (the cached cases are read-only)
    res = marching_tetrahedra(t(verts)[None], t(tets), t(sdf)[None], t(scales)[None, :, None])
    (pos, esdf), esc, faces, ids = [r[0] for r in res]
    return ids.numpy(), pos.numpy(), esdf.numpy(), esc.numpy(), faces.numpy()


out = {}
for cls in MC.GOLDEN_CLASSES:
    for name in MC.CASES[cls]:
        inputs = MC.case(name)
        got = MC.canonical(reference(*inputs))
        MC.check_surface(inputs, (got["ids"], got["pos"].view(np.float32), got["sdf"].view(np.float32), got["scales"].view(np.float32), got["faces"]),
                         oriented=cls == "shuffled_grid")
        out[name + "__in"] = np.array(MC.digest(*inputs))
        out[name + "__EF"] = np.array([len(got["ids"]), len(got["faces"])], np.int64)
        inline = sum(a.nbytes for a in got.values()) <= MC.INLINE_BYTES
        for f in MC.FIELDS:
            if inline:
                out["%s__%s" % (name, f)] = got[f].astype(np.int32) if got[f].dtype == np.int64 else got[f]
            else:
                out["%s__%s_sha" % (name, f)] = np.array(MC.digest(got[f]))
        print(name, "E, F =", out[name + "__EF"], "arrays" if inline else "digests", flush=True)

if "--skip-big" in sys.argv:
    old = np.load(OUT)
    for k in old.files:
        if k.startswith("big_chunked__"):
            out[k] = old[k]
else:
    inputs = MC.big_chunked_case()
    assert len(inputs[1]) == 32 * 1024 * 1024 + 17
    got = MC.canonical(reference(*inputs))
    out["big_chunked__in"] = np.array(MC.digest(*inputs))
    out["big_chunked__EF"] = np.array([len(got["ids"]), len(got["faces"])], np.int64)
    out["big_chunked__ids_sha"] = np.array(MC.digest(got["ids"]))
    out["big_chunked__faces_sha"] = np.array(MC.digest(got["faces"]))
    print("big_chunked E, F =", out["big_chunked__EF"], flush=True)

with zipfile.ZipFile(OUT, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
    for k in sorted(out):
        buf = io.BytesIO()
        np.lib.format.write_array(buf, np.asanyarray(out[k]), allow_pickle=False)
        info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
        info.compress_type = zipfile.ZIP_DEFLATED
        z.writestr(info, buf.getvalue(), compresslevel=9)
print("wrote", OUT, os.path.getsize(OUT), "bytes")
