class Missing:
    """An attribute chain of the stand-in: every attribute exists, calling one raises."""

    def __init__(self, name):
        self._name = name

    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return Missing(self._name + "." + k)

    def __call__(self, *a, **k):
        raise RuntimeError("%s: pyrender is not installed (it needs an OpenGL stack); this backend renders mesh depth with "
                           "mesh_cull.render_depth (HIP), which launch/run_reference_script.py binds in place of "
                           "eval_tnt/cull_mesh.py's extract_depth_from_mesh" % self._name)
