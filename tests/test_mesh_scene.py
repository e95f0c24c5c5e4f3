"""The procedural meshes (madarch_amd/meshes.py) and the obj_mesh example on the oracle: no GPU needed."""
import numpy as np

from helpers import SMALL_PROBES
from madarch_amd import _binding as B
from madarch_amd import examples, meshes, renderers
from mesh_scenes import PARITY_CAMERA, parity_mesh

OFFSET = np.asarray(examples.OBJ_MESH_OFFSET, dtype=np.float32)
GRID_HI = np.array([3.0, 2.0, 2.0], dtype=np.float32)  # 30 x 20 x 20 cells of 0.1, no offset (obj_mesh/main.adb:30-36)


def test_generators_are_deterministic_and_fill_the_example():
    for make in (lambda: meshes.torus(25, 20), lambda: meshes.torus(25, 20, axis=2), parity_mesh, lambda: meshes.sheet(25, 20)):
        a, b = make(), make()
        assert a.dtype == np.float32 and a.shape == (examples.OBJ_MESH_TRIANGLES, 3, 3)
        assert a.tobytes() == b.tobytes()
        assert len(meshes.degenerate(a)) == 0
        placed = a + OFFSET
        assert (placed > 0.0).all() and (placed < GRID_HI).all()  # inside the partition's grid
    assert meshes.torus(5, 4).shape == (40, 3, 3)
    assert list(meshes.degenerate(np.zeros((1, 3, 3), dtype=np.float32))) == [0]


def test_obj_mesh_builds_and_renders_on_the_oracle(orc):
    assert examples.SCENES["obj_mesh"] is examples.obj_mesh
    R = examples.obj_mesh(64, 40, Probes=SMALL_PROBES, Binding=orc)  # the example's call order, GPU_Fast included
    R.Set_Option(B.OPT_GBUFFER, 1)
    P = R.Read_Partitioning()
    assert P.shape == (30 * 20 * 20, 1 + 150) and 0 < P[:, 0].max() <= 150
    R.Render()
    assert R.Read_Framebuffer().shape == (40, 64, 3)
    R.Set_Camera_Position((1.5, 1.0, -1.5))  # (the example's camera sees the torus edge-on: a few pixels)
    R.Render()
    idx, t, steps = R.Read_Gbuffer()
    assert (idx >= 0).any() and idx.max() < examples.OBJ_MESH_TRIANGLES


def test_parity_mesh_meets_the_cap_condition(orc):
    """Every cell of the parity tests' mesh has fewer pre-candidates than the smaller of the two builders' caps (the
    device's 256; the oracle keeps 512): CPU_Fast lists a cell's pre-candidates in scene order, cut at Index_Count,
    so under Index_Count 600 the first count of a cell's record is their number unless a cap cut it."""
    R = examples.obj_mesh(16, 16, Probes=SMALL_PROBES, Binding=orc, Partitioning_Method=renderers.CPU_Fast, Mesh=parity_mesh(), Index_Count=600)
    most = int(R.Read_Partitioning()[:, 0].max())
    print("most pre-candidates in a cell: %d" % most)
    assert most < 256
    # and the camera of the parity tests sees the mesh in more than a tenth of its pixels
    R2 = examples.obj_mesh(80, 50, Probes=SMALL_PROBES, Binding=orc, Mesh=parity_mesh())
    R2.Set_Option(B.OPT_GBUFFER, 1)
    R2.Set_Camera_Position(PARITY_CAMERA)
    R2.Render()
    assert (R2.Read_Gbuffer()[0] >= 0).mean() >= 0.1
