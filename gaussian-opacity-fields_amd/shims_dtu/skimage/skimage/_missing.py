class Missing:
    """An attribute chain of the stand-in: every attribute exists, calling one raises."""

    def __init__(self, name):
        self._name = name

    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return Missing(self._name + "." + k)

    def __call__(self, *a, **k):
        raise RuntimeError("%s: skimage is not installed; this backend culls the DTU meshes with mesh_cull.py (HIP), which "
                           "launch/run_reference_script.py binds in place of evaluate_dtu_mesh.py's cull_mesh, load_dtu_camera and "
                           "trimesh.load" % self._name)
