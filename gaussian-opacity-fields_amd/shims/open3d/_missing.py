class Missing:
    """An attribute chain of the stand-in: every attribute exists, calling one raises."""

    def __init__(self, name):
        self._name = name

    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return Missing(self._name + "." + k)

    def __call__(self, *a, **k):
        raise RuntimeError("%s: open3d is not installed; this backend fuses TSDF volumes with tsdf_fusion.py (HIP), which "
                           "launch/run_reference_script.py binds in place of extract_mesh_tsdf.py's tsdf_fusion" % self._name)
