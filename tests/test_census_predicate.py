"""Host-only checks of the census fuzzer (tests/fuzz_census.py): its restatement of run_pass's census predicates on
hand-made descriptions, and that every seed of the GPU suite lands in the census its family is meant to reach."""
import numpy as np
import pytest

import fuzz_census as fc
from madarch_amd import scenes
from test_gpu_census_fuzz import NEAR, PSMALL, ROOM

WALLS = [((1.0, 0.0, 0.0), 1.0), ((-1.0, 0.0, 0.0), 7.0), ((0.0, 1.0, 0.0), 1.0)]


def _desc(**kw):
    d = dict(kinds=[("sphere", 1), ("plane", 6), ("box", 1)], planes=list(WALLS), spheres=[((2.0, 2.0, 2.0), 0.5)], boxes=[((4.0, 1.0, 4.0), (0.5, 0.5, 0.5))],
             triangles=[], custom=[], part=None)
    d.update(kw)
    return d


def _part(**kw):
    p = dict(dims=(4, 4, 4), spacing=(1.0, 2.0, 0.5), offset=(-1.0, -1.0, -1.0), border=scenes.Clamp, index_count=4, builder=0)
    p.update(kw)
    return p


def test_room_predicate():
    assert fc.census(_desc()) == "room"
    assert fc.census(_desc(planes=[((-0.0, 1.0, -0.0), 1.0)])) == "room"  # -0.0 components fold
    assert fc.census(_desc(planes=WALLS + [((1.0, 0.0, 0.0), float(np.nextafter(np.float32(1.0), np.float32(2))))])) == "room"
    assert fc.census(_desc(planes=[])) is None  # n_axis > 0
    assert fc.census(_desc(planes=WALLS + [((0.0, 1.0, 0.0), float("nan"))])) is None  # a NaN offset is a general plane
    assert fc.census(_desc(planes=WALLS + [((0.6, 0.8, 0.0), 1.0)])) is None
    assert fc.census(_desc(planes=WALLS + [((0.0, 2.0, 0.0), 1.0)])) is None  # not a unit axis
    assert fc.census(_desc(spheres=[])) is None and fc.census(_desc(boxes=[])) is None
    assert fc.census(_desc(spheres=[((0, 0, 0), 1.0)] * 2)) is None
    assert fc.census(_desc(triangles=[((0, 0, 0), (1, 0, 0), (0, 1, 0))])) is None
    assert fc.census(_desc(kinds=[("sphere", 1), ("plane", 6), ("box", 1), ("triangle", 1)])) == "room"  # declared, none added
    assert fc.census(_desc(kinds=[("sphere", 1), ("plane", 6), ("box", 1), ("custom", 1)])) is None
    assert fc.expected_pfk(_desc()) == 16 and fc.expected_pfk(_desc(kinds=[("sphere", 1), ("custom", 1)])) == 2


def test_psmall_predicate():
    assert fc.census(_desc(part=_part())) == "psmall" and fc.expected_pfk(_desc(part=_part())) == 33
    assert fc.census(_desc(part=_part(spacing=(1.0, 1.5, 1.0)))) is None
    assert fc.census(_desc(part=_part(border=scenes.Fallback))) is None and fc.expected_pfk(_desc(part=_part(border=scenes.Fallback))) == 9
    assert fc.census(_desc(part=_part(), kinds=[("sphere", 33), ("plane", 6)])) is None
    assert fc.census(_desc(part=_part(), kinds=[("sphere", 32), ("plane", 32)])) == "psmall"
    assert fc.census(_desc(part=_part(), kinds=[("sphere", 32), ("plane", 32), ("box", 1)])) is None  # 65 declared
    assert fc.census(_desc(part=_part(), kinds=[("sphere", 1), ("plane", 6), ("triangle", 1)])) is None  # a triangle kind declared
    assert fc.census(_desc(part=_part(), kinds=[("sphere", 1), ("sphere", 1)])) is None  # two kinds of one type
    assert fc.census(_desc(part=_part(), kinds=[("sphere", 1), ("custom", 1)])) is None and fc.expected_pfk(_desc(part=_part(), kinds=[("custom", 1)])) == 3
    assert fc.census(_desc(part=_part(dims=(256, 256, 256)))) is None  # 2^24 cells


@pytest.mark.parametrize("seeds,want", [(ROOM, "room"), (PSMALL, "psmall"), (NEAR, None)])
def test_suite_seeds_reach_their_census(seeds, want):
    assert len(seeds) >= {"room": 24, "psmall": 12, None: 10}[want]
    changes = set()
    for s in seeds:
        desc, change = fc.describe(s)
        assert fc.census(desc) == want, (s, change)
        changes.add(change)
    if want is None:
        assert changes == set(fc.NEAR)
