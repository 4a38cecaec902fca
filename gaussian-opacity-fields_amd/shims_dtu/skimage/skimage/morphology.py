from ._missing import Missing

binary_dilation = Missing("skimage.morphology.binary_dilation")
disk = Missing("skimage.morphology.disk")


def __getattr__(name):
    if name.startswith("__"):
        raise AttributeError(name)
    return Missing("skimage.morphology." + name)
