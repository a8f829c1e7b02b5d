"""Generates tests/golden/unstructured_2d.npz and unstructured_3d.npz (run here, committed with its output): the
Delaunay "fan" meshes of tests/unstructured_meshes.py, coordinates `x` (float64) and `cells` (int32) only.  The files are
committed, not just this recipe, so that another qhull build cannot change the meshes under test.

    python tests/golden/make_unstructured.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in ("knp-emi-fenics-x_amd", "oracle", "examples/idealized_geometries", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import unstructured_meshes as um  # noqa: E402

if __name__ == "__main__":
    for dim in (2, 3):
        x, cells = um.build_fan_points_and_cells(dim)
        np.savez_compressed(os.path.join(HERE, f"unstructured_{dim}d.npz"), x=x.astype(np.float64),
                            cells=cells.astype(np.int32))
        print(dim, um.mesh_statistics(um.fan_mesh(dim)))
