"""Import shim for ``tetranerf.utils.extension.cpp`` (reference submodules/tetra-triangulation, CPU CGAL Delaunay;
extract_mesh.py:51), used when the real module is not importable.  Device tensors go to the HIP Delaunay tetrahedralization
(``delaunay.triangulate``, DESIGN.md §3.7: CGAL's finite cells, positively oriented); host tensors keep SciPy's Qhull Delaunay."""
import torch


class cpp:  # noqa: N801  (mirrors the reference's attribute access `cpp.triangulate`)
    @staticmethod
    def triangulate(points: torch.Tensor) -> torch.Tensor:
        if points.device.type == "cuda":
            import delaunay
            return delaunay.triangulate(points.detach().float())
        from scipy.spatial import Delaunay
        tri = Delaunay(points.detach().cpu().double().numpy())
        return torch.from_numpy(tri.simplices.astype("int32")).to(points.device)
