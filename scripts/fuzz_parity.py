"""Differential fuzzing: random scenes (tests/fuzz_scenes.py) rendered by the HIP library and by the CPU oracle
must agree like the parity tests demand.  Usage: python scripts/fuzz_parity.py [--census room|psmall|near] [first seed] [seeds]
--census draws the scenes from tests/fuzz_census.py instead: the rooms' census, the partition's small form, or scenes one
change away from either (seed numbers count from the start of that family's range)."""
import argparse, os, sys, traceback
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle_engine import oracle_binding
from madarch_amd import _binding as B
from fuzz_scenes import build, compare

ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("--census", choices=("room", "psmall", "near"))
ap.add_argument("first", type=int, nargs="?", default=0)
ap.add_argument("count", type=int, nargs="?", default=50)
args = ap.parse_args()
if args.census:
    import fuzz_census
    build, seeds = fuzz_census.build, fuzz_census.seeds(args.census, args.first, args.count)
else:
    seeds = range(args.first, args.first + args.count)
orc = oracle_binding()
hip = orc if os.environ.get("FUZZ_ORACLE_ONLY") else B.hip_binding()  # (oracle only: a dry run of the generator on a CPU)
bad = []
for seed in seeds:
    try:
        compare(build(seed, hip), build(seed, orc))
        print("seed %d ok" % seed, flush=True)
    except Exception as e:  # noqa: BLE001
        bad.append(seed)
        print("seed %d FAILED: %s: %s" % (seed, type(e).__name__, str(e).splitlines()[0] if str(e) else ""), flush=True)
        if os.environ.get("FUZZ_TRACE"):
            traceback.print_exc()
print("failed seeds:", bad)
sys.exit(1 if bad else 0)
