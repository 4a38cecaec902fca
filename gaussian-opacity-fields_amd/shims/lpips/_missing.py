class Missing:
    """An attribute chain of the stand-in: every attribute exists, calling one raises."""

    def __init__(self, name):
        self._name = name

    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return Missing(self._name + "." + k)

    def __call__(self, *a, **k):
        raise RuntimeError("%s: the lpips package is not installed; this backend provides lpips.LPIPS(net='vgg') only "
                           "(image_metrics.py, HIP)" % self._name)
