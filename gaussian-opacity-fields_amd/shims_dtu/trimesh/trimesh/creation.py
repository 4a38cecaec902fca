"""`trimesh.creation.box()` of the stand-in: the axis-aligned cube of edge 1 around the origin, 8 vertices and 12 triangles."""
import numpy as np

from ._missing import Missing


class Box:
    def __init__(self):
        self.vertices = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)], np.float64)
        self.faces = np.array([[1, 3, 0], [4, 1, 0], [0, 3, 2], [2, 4, 0], [1, 7, 3], [5, 1, 4],
                               [5, 7, 1], [3, 7, 2], [6, 4, 2], [2, 7, 6], [6, 5, 4], [7, 5, 6]], np.int64)


def box():
    return Box()


def __getattr__(name):
    if name.startswith("__"):
        raise AttributeError(name)
    return Missing("trimesh.creation." + name)
