"""The free rays, the atlases and the float64 answers that the shaded-ray tests share (tests/test_shade_rays_host.py on the
CPU, tests/test_gpu_shade_rays.py on the device): 257 seeded rays in the "room" and the "open" scene of ref64_cases, the
seeded atlases of the frame tests, and ref64's pixel_color_probes along those rays as stated and twice jittered."""
import contextlib

import numpy as np

import ray_query_cases as Q
import ref64
import ref64_cases
from helpers import SEED
from madarch_amd import _binding as B
from madarch_amd import scenes, windows

N_FREE = 257
SEEDS = (None, 1, 2)
MODES = (0, 2)
AO_STEPS, SPEC_MODE = 3, 2  # ref64_cases.describe's defaults: what make_renderer sets


def free_rays(name):
    if name == "room":
        return Q.rays_inside(N_FREE, Q.ROOM_LO, Q.ROOM_HI, SEED + 31)
    return Q.open_rays(N_FREE, SEED + 37)


def free_atlases(desc):
    return ref64_cases.atlases(desc, SEED % 1000 + 3)  # irradiance, radiance


def free_runs(name, mode):
    """ref64's pixel_color_probes along the free rays of scene `name`: three runs, computed once"""
    def compute():
        desc = ref64_cases.describe(name)
        assert desc["ao_steps"] == AO_STEPS and desc["spec_mode"] == SPEC_MODE
        irr, rad = free_atlases(desc)
        sc = ref64.Scene(desc)
        org, drs = free_rays(name)
        return [ref64.Run(sc, seed, irr, rad).pixel_color_probes(org, drs, mode, True, SPEC_MODE, AO_STEPS) for seed in SEEDS]
    return ref64_cases.cached(("shade_rays", name, mode), compute)


FRAME_W, FRAME_H = 20, 12  # partial 8x8 tiles in both directions; 240 rays: a partial workgroup


@contextlib.contextmanager
def frame_size(W=FRAME_W, H=FRAME_H):
    """the scene builders of ray_query_cases and ref64_cases with a window of W x H pixels instead of their own 16 x 16 (the
    window's size is the only thing they give windows.Open that matters to a renderer)"""
    saved = windows.Open
    windows.Open = lambda w, h, *a, **k: saved(W, H, *a, **k)
    try:
        yield
    finally:
        windows.Open = saved


# name -> the renderer over a binding: every variant k_ray_shade is built for, and the census kernels of the frame beside them
FRAME_SCENES = {
    "rooms": Q.gi_room,
    "partition, Clamp": lambda b: Q.simple_partition(b, scenes.Clamp, 0),
    "partition, Fallback": lambda b: Q.simple_partition(b, scenes.Fallback, 0),
    "partition, Clamp, global residency": lambda b: Q.simple_partition(b, scenes.Clamp, 1),
    "partition, Fallback, global residency": lambda b: Q.simple_partition(b, scenes.Fallback, 1),
    "mesh, scanned": lambda b: mesh(b),
    "mesh, global residency": lambda b: mesh(b, residency=1),
    "mesh, triangle BVH": lambda b: mesh(b, residency=1, bvh=1),
    "open scene": lambda b: Q.described(b, "open")[0],
}


def mesh(binding, **kw):
    R = Q.small_mesh(binding, **kw)
    R.Set_Camera_Position((0.25, 1.0, 0.0))  # in front of the strip of triangles: a dozen pixels of it, sky around them
    return R


def seeded_atlases(R, seed=SEED % 1000 + 3):
    """uniform (0, 1) atlases of the renderer's own shapes: irradiance, radiance"""
    rng = np.random.RandomState(seed)
    return [rng.uniform(0.0, 1.0, size=R.Texture_Shape(tex)).astype(np.float32) for tex in (B.TEX_IRRADIANCE, B.TEX_RADIANCE)]


def frame_renderer(binding, name, mode):
    """scene `name` at FRAME_W x FRAME_H in screen mode `mode`, geometry buffer on, seeded atlases written"""
    with frame_size():
        R = FRAME_SCENES[name](binding)
    assert (R.Width, R.Height) == (FRAME_W, FRAME_H)
    R.Set_Option(B.OPT_GBUFFER, 1)
    R.Set_Option(B.OPT_SCREEN_MODE, mode)
    irr, rad = seeded_atlases(R)
    R.Write_Texture(B.TEX_IRRADIANCE, irr)
    R.Write_Texture(B.TEX_RADIANCE, rad)
    return R


def bits(a):
    """an array's bits, for comparisons that count a NaN as equal to itself and -0 as different from +0"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a
