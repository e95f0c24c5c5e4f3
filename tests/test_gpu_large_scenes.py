"""Scenes whose table does not fit a workgroup's LDS (the reference's obj_mesh example: 1000 triangles) and the
residency that carries them: geometry and material ids read from the table's image in device memory
(MDH_OPT_TABLE_RESIDENCY 1, mdh_device.h: Geo), against the oracle and against the LDS residency of scenes that fit."""
import os
import subprocess

import numpy as np
import pytest

import fuzz_scenes
from helpers import SEED, SMALL_PROBES, assert_parity, make, same_bits, seeded_points, snapshot
from madarch_amd import _binding as B
from madarch_amd import examples, materials, renderers, scenes, windows
from madarch_amd.lights import point_lights, spot_lights
from madarch_amd.primitives import boxes, planes, spheres, triangles
from mesh_scenes import PARITY_CAMERA, parity_mesh
from test_gpu_full_size import tile_mask

pytestmark = pytest.mark.gpu

RES = B.OPT_TABLE_RESIDENCY


def mesh_renderer(binding, W, H, method=None, probes=SMALL_PROBES, **kw):
    R = examples.obj_mesh(W, H, Probes=probes, Binding=binding, Partitioning_Method=method, Mesh=parity_mesh(), **kw)
    R.Set_Camera_Position(PARITY_CAMERA)
    R.Set_Option(B.OPT_GBUFFER, 1)
    return R


def hit_share(snap):
    return float((snap["gb_index"] >= 0).mean())


def test_obj_mesh_three_builders_against_the_oracle(hip, orc):
    """obj_mesh at 320x200: for each builder the partition table and the warning count of the oracle, then two frames
    at the parity bar.  The scene cannot be committed without global residency (MDH_E_INVALID on the parent commit).
    The mesh is mesh_scenes.parity_mesh: every cell stays below the builders' 256 pre-candidates
    (tests/test_mesh_scene.py asserts it on the oracle), so CPU_Best too sees the same candidates on both sides."""
    Rh, Ro = (mesh_renderer(b, 320, 200) for b in (hip, orc))
    assert Rh.Get_Option(RES) == 1
    for method in (renderers.GPU_Fast, renderers.CPU_Fast, renderers.CPU_Best):
        Rh.Update_Partitioning(Method=method)
        Ro.Update_Partitioning(Method=method)
        assert np.array_equal(Rh.Read_Partitioning(), Ro.Read_Partitioning()), method
        wh, wo = Rh.Partition_Warnings(), Ro.Partition_Warnings()
        print("method %d: %d warnings (oracle %d)" % (method, wh, wo))
        assert wh == wo, method
        sh, so = snapshot(Rh, 2), snapshot(Ro, 2)
        print("method %d: %.3f of the pixels hit the mesh" % (method, hit_share(so)))
        assert hit_share(so) >= 0.1  # a frame of misses is no parity
        assert_parity(sh, so)
    assert Rh.Get_Option(RES) == 1


def both_residencies(build):
    """`build(force)` -> the outputs of one run on the HIP library; automatic against forced global residency"""
    auto, forced = build(False), build(True)
    assert sorted(auto) == sorted(forced)
    for k in auto:
        assert same_bits(auto[k], forced[k]), k


@pytest.mark.parametrize("method", [renderers.CPU_Best, renderers.CPU_Fast, renderers.GPU_Fast])
def test_forced_residency_simple_scene(hip, method):
    def build(force):
        R = make("simple_scene", 96, 64, hip, probes=SMALL_PROBES, Partitioning_Method=None)
        R.Set_Option(RES, 1 if force else 0)
        R.Update_Partitioning(Method=method)
        out = snapshot(R, 2)
        out["partition"] = R.Read_Partitioning()
        assert R.Get_Option(RES) == (1 if force else 0)
        return out
    both_residencies(build)


def test_forced_residency_ball_game(hip):
    def build(force):
        G = examples.ball_game(96, 64, Probes=SMALL_PROBES, Binding=hip)
        G.R.Set_Option(B.OPT_GBUFFER, 1)
        G.R.Set_Option(RES, 1 if force else 0)
        for f in range(12):
            if f in (0, 4):
                G.Throw_Ball()
                G.Move_Camera((0.3, 0.1, 0.0))
            G.Frame()
        out = snapshot(G.R, 1)
        out["balls"] = np.concatenate([np.concatenate((b[1], b[2])) for b in G.Ball_Bodies])
        assert G.R.Get_Option(RES) == (1 if force else 0)
        return out
    both_residencies(build)


def _fuzz_partition_on(seed):
    """the second draw of fuzz_scenes.build (seed): is the space partition on?"""
    rng = np.random.default_rng(seed)
    rng.integers(0, 4)
    return bool(rng.integers(0, 2))


def test_forced_residency_fuzz_scene_with_triangles(hip, monkeypatch):
    """one scene of fuzz_scenes' generator that has triangles behind a partition (checked on the renderer it builds)"""
    seen = {}

    def build(force):
        create = renderers.Create

        def create_forced(*a, **kw):
            R = create(*a, **kw)
            R.Set_Option(RES, 1 if force else 0)
            seen["R"] = R
            return R
        monkeypatch.setattr(fuzz_scenes.renderers, "Create", create_forced)
        try:
            out = fuzz_scenes.build(seen["seed"], hip)
        finally:
            monkeypatch.setattr(fuzz_scenes.renderers, "Create", create)
        R = seen["R"]
        assert R.Get_Option(RES) == (1 if force else 0)
        return out

    for seed in range(1, 200):  # the first seed whose scene has a partition and at least two triangles
        if not _fuzz_partition_on(seed):
            continue
        seen["seed"] = seed
        probe = build(False)
        R = seen["R"]
        off, cnt = scenes.Get_Primitives_Location(R.Scene, triangles.Triangle)
        ntri = int(np.frombuffer(R.Read_Scene_Buffer(), dtype=np.int32)[cnt // 4])
        if ntri >= 2 and "partition" in probe:
            break
    else:
        pytest.fail("no seed with triangles behind a partition")
    print("fuzz seed %d: %d triangles" % (seed, ntri))
    both_residencies(build)


def fallback_scene(binding, force):
    """a Fallback border: rays leave the 4 x 3 x 3 grid of 1.5-cells on their way through the room"""
    part = scenes.Partitioning_Settings(Enable=True, Index_Count=12, Border_Behavior=scenes.Fallback, Grid_Dimensions=(4, 3, 3),
                                        Grid_Spacing=(1.5, 1.5, 1.5), Grid_Offset=(0.0, 0.0, 0.0))
    scene = scenes.Compile([(spheres.Sphere, 6), (planes.Plane, 8), (boxes.Box, 4), (triangles.Triangle, 5)],
                           [(point_lights.Point_Light, 2)], Partitioning=part)
    R = renderers.Create(windows.Open(96, 64), scene, Probes=SMALL_PROBES, Volumetrics=renderers.No_Volumetrics, Binding=binding)
    if force is not None:
        R.Set_Option(RES, 1 if force else 0)
    for m, a in enumerate(((0.8, 0.8, 0.8), (0.9, 0.1, 0.1), (0.1, 0.2, 0.9), (0.2, 0.8, 0.3))):
        R.Set_Material(m, materials.Create(a, 0.2 * m, 0.3 + 0.2 * m))
    for i, (n, o) in enumerate((((0, 1, 0), 1.0), ((0, -1, 0), 7.0), ((1, 0, 0), 1.0), ((-1, 0, 0), 7.0), ((0, 0, 1), 6.0), ((0, 0, -1), 7.0))):
        R.Add_Primitive(planes.Plane, planes.Create(n, o, i % 3))
    for c, r in (((1.0, 1.0, 2.0), 0.6), ((4.5, 0.5, 3.5), 0.8), ((2.5, 2.5, 5.0), 0.5)):
        R.Add_Primitive(spheres.Sphere, spheres.Create(c, r, 3))
    for c, s in (((3.0, 0.0, 4.0), (1.0, 1.0, 1.0)), ((5.5, 3.0, 2.0), (0.5, 0.8, 0.4))):
        R.Add_Primitive(boxes.Box, boxes.Create(c, s, 2))
    for a, b, c in (((0.5, 0.0, 1.0), (2.0, 0.2, 1.5), (1.0, 2.0, 2.5)), ((3.5, 2.0, 1.0), (5.0, 2.5, 1.2), (4.0, 4.0, 2.0)), ((2.0, -0.5, 5.5), (3.5, 1.0, 5.0), (2.5, 2.0, 4.0))):
        R.Add_Primitive(triangles.Triangle, triangles.Create(a, b, c, 1))
    R.Set_Light(1, point_lights.Point_Light, point_lights.Create((3.0, 4.0, 1.0), (0.9, 0.9, 0.9)))
    R.Set_Camera_Position((2.0, 2.0, -0.5))
    R.Set_Option(B.OPT_GBUFFER, 1)
    R.Update_Partitioning(Method=renderers.CPU_Fast)
    return R


def test_forced_residency_fallback_border(hip, orc):
    def build(force):
        R = fallback_scene(hip, force)
        out = snapshot(R, 2)
        out["partition"] = R.Read_Partitioning()
        out["eval_d"], out["eval_n"] = R.Eval_Distances_To(seeded_points(64, -1.0, 7.0), (spheres.Sphere, boxes.Box, triangles.Triangle))
        assert R.Get_Option(RES) == (1 if force else 0)
        return out
    both_residencies(build)
    assert_parity(build(True), snapshot(fallback_scene(orc, None), 2))


def test_no_partition_900_triangles_against_the_oracle(hip, orc):
    """the brute-force scan over 900 triangles in memory: partition disabled, 64x40, the renderer's own pixel program
    (screen mode 0: primary march with the arg-min at the hit, light and probe-visibility marches through the scan)"""
    tris = parity_mesh()[:900] + np.asarray(examples.OBJ_MESH_OFFSET, dtype=np.float32)
    snaps = []
    for b in (hip, orc):
        scene = scenes.Compile([(triangles.Triangle, 900)], [(point_lights.Point_Light, 4)], Partitioning=scenes.Partitioning_Settings(Enable=False))
        R = renderers.Create(windows.Open(64, 40), scene, Probes=SMALL_PROBES, Volumetrics=renderers.No_Volumetrics, Binding=b)
        mat = R.Add_Material(materials.Create((0.8, 0.2, 0.1), 0.0, 1.0))
        for a, bb, c in tris:
            R.Add_Primitive(triangles.Triangle, triangles.Create(a, bb, c, mat))
        R.Set_Light(1, point_lights.Point_Light, point_lights.Create((0.0, 1.0, -5.0), (0.9, 0.9, 0.9)))
        R.Set_Camera_Position(PARITY_CAMERA)
        R.Set_Option(B.OPT_GBUFFER, 1)
        if b is hip:
            assert R.Get_Option(RES) == 1
        snaps.append(snapshot(R, 1))
    assert hit_share(snaps[1]) >= 0.1
    assert_parity(snaps[0], snaps[1])


def test_edits_in_flight(hip):
    """frames kept in flight read the table their launch was given: Set_Primitive on some triangles and a partition
    rebuild every frame, six frames, overlap 2 against overlap 0"""
    outs = []
    for overlap in (2, 0):
        R = mesh_renderer(hip, 160, 100, method=renderers.GPU_Fast)
        R.Set_Option(B.OPT_FRAME_OVERLAP, overlap)
        mesh = parity_mesh() + np.asarray(examples.OBJ_MESH_OFFSET, dtype=np.float32)
        mat = 0
        for f in range(6):
            for i in range(40 * f, 40 * f + 40):  # forty triangles drift a little each frame
                a, b, c = mesh[i] + np.float32(0.02 * (f + 1))
                R.Set_Primitive(triangles.Triangle, i + 1, triangles.Create(a, b, c, mat))
            R.Update_Partitioning(Method=renderers.GPU_Fast)
            R.Render()
        out = snapshot(R, 0)
        out["partition"] = R.Read_Partitioning()
        assert R.Get_Option(RES) == 1
        outs.append(out)
    for k in outs[0]:
        assert same_bits(outs[0][k], outs[1][k]), k


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_frame_adds_up(hip, world):
    """`world` ranks emulated on one GPU as tests/test_gpu_full_size.py does it: radiance slices exchanged through the
    host, every rank folds the irradiance and draws its tiles; the framebuffers add up to the unsharded frame"""
    W, H = 160, 100
    whole = mesh_renderer(hip, W, H, method=renderers.GPU_Fast)
    for _ in range(2):
        whole.Render()
    img_w = whole.Read_Framebuffer()
    rad_w, irr_w = whole.Read_Texture(B.TEX_RADIANCE), whole.Read_Texture(B.TEX_IRRADIANCE)
    Rs = [mesh_renderer(hip, W, H, method=renderers.GPU_Fast) for _ in range(world)]
    for r, R in enumerate(Rs):
        R.Set_Option(B.OPT_WORLD, world)
        R.Set_Option(B.OPT_RANK, r)
        assert R.Get_Option(RES) == 1
    P = Rs[0].Probe_Total()
    bounds = [P * r // world for r in range(world + 1)]
    for _ in range(2):
        for R in Rs:
            R.Render_Pass(B.PASS_RADIANCE)
        parts = [R.Read_Atlas_Slice(B.TEX_RADIANCE, bounds[r], bounds[r + 1] - bounds[r]) for r, R in enumerate(Rs)]
        for r, R in enumerate(Rs):
            for q in range(world):
                if q != r:
                    R.Write_Atlas_Slice(B.TEX_RADIANCE, bounds[q], parts[q])
        for R in Rs:
            R.Render_Pass(B.PASS_IRRADIANCE)
        for R in Rs:
            R.Render_Pass(B.PASS_SCREEN)
    acc = np.zeros_like(img_w)
    for r, R in enumerate(Rs):
        img = R.Read_Framebuffer()
        assert not img[~tile_mask(W, H, world, r)].any()
        acc += img
        assert same_bits(R.Read_Texture(B.TEX_RADIANCE), rad_w) and same_bits(R.Read_Texture(B.TEX_IRRADIANCE), irr_w)
    assert same_bits(acc, img_w)


def test_eval_distances_against_the_oracle(hip, orc):
    pts = seeded_points(256, (0.0, 0.0, 0.0), (3.0, 2.0, 2.0), SEED)
    res = []
    for b in (hip, orc):
        R = mesh_renderer(b, 16, 16)
        res.append(R.Eval_Distances_To(pts, (triangles.Triangle,)))
    assert same_bits(res[0][0], res[1][0]) and same_bits(res[0][1], res[1][1])


def test_resident_part_over_the_budget_is_still_refused(hip):
    """1500 spot lights are 4500 float4 of the part that must be in LDS: no residency carries that"""
    scene = scenes.Compile([(spheres.Sphere, 4)], [(spot_lights.Spot_Light, 1500)], Partitioning=scenes.Partitioning_Settings(Enable=False))
    R = renderers.Create(windows.Open(16, 16), scene, Probes=SMALL_PROBES, Volumetrics=renderers.No_Volumetrics, Binding=hip)
    R.Add_Primitive(spheres.Sphere, spheres.Create((0.0, 0.0, 3.0), 1.0, 0))
    for i in range(1500):
        R.Set_Light(i + 1, spot_lights.Spot_Light, spot_lights.Create((0.0, 3.0, 0.0), (0.0, -1.0, 0.0), 0.7, (0.5, 0.5, 0.5)))
    with pytest.raises(B.MadarchError) as e:
        R.Render()
    assert e.value.status == B.MDH_E_INVALID and "scene tables exceed the 64 KiB LDS budget of a workgroup" in str(e.value)


def test_cpp_obj_mesh_example_runs(hip, tmp_path):
    """examples/obj_mesh.cpp on the C++ mirror: the same scene (its torus comes out of the C library's sin / cos, so the
    frame is held against the Python mirror's at the parity bar's colour tolerance, not bit for bit)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-s", "-C", os.path.join(root, "examples")])
    W, H = 72, 48
    path = str(tmp_path / "obj_mesh.f32")
    out = subprocess.run([os.path.join(root, "examples", "bin", "obj_mesh"), str(W), str(H), "2", path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got = np.fromfile(path, dtype=np.float32).reshape(H, W, 3)
    R = examples.obj_mesh(W, H, Binding=hip)
    for _ in range(2):
        R.Render()
    want = R.Read_Framebuffer()
    assert (np.isnan(got) == np.isnan(want)).mean() > 0.99
    ok = np.isclose(got, want, rtol=1e-4, atol=1e-5, equal_nan=True)
    assert ok.mean() > 0.99
