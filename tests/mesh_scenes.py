"""The mesh and the camera of the large-scene parity tests (tests/test_gpu_large_scenes.py, tests/test_mesh_scene.py).

The builders keep a bounded number of pre-candidates per cell -- the oracle 512, the device 256 (MDH_PART_MAX_PRE) -- and
CPU_Best chooses among them, so a parity test of that builder needs a mesh whose every cell stays strictly below 256.
The example's torus does not (the cells on its axis are equally far from hundreds of triangles), nor does a flat sheet
(a cell far from it sees a whole disc of it).  A sheet that undulates through the whole depth of the 30 x 20 x 20 grid
has no cell far from it: measured on the oracle (CPU_Fast under Index_Count 600) at most 103 pre-candidates in a cell.
tests/test_mesh_scene.py asserts the bound on the CPU; the GPU tests rely on it."""
from madarch_amd import meshes

# in front of the sheet, looking down +z (the identity orientation): the example's own camera (0, 1, -5) sees the
# mesh in a few per cent of its pixels, this one in more than a tenth (asserted where it is used)
PARITY_CAMERA = (1.5, 1.0, -1.5)


def parity_mesh():
    """1000 triangles, centred on the origin (examples.obj_mesh adds the example's offset (1.5, 1, 1))"""
    return meshes.sheet(25, 20, size=(2.9, 1.9), height=0.7, waves=(3.5, 3.0))
