class Missing:
    """An attribute chain of the stand-in: every attribute exists, calling one raises."""

    def __init__(self, name):
        self._name = name

    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return Missing(self._name + "." + k)

    def __call__(self, *a, **k):
        raise RuntimeError("%s: torchvision is not installed; this backend provides torchvision.utils.save_image and "
                           "torchvision.transforms.functional.to_tensor only (what render.py and metrics.py use)" % self._name)
