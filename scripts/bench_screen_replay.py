#!/usr/bin/env python3
"""Times BASELINE config 3 (global_illumination, 32 x 16 probes, 1920 x 1080) with MDH_OPT_SCREEN_REPLAY on (a) and off (b),
alternating them in one process so that they share the session's clocks and neighbours, for --rounds rounds: frames kept in
flight, one device-synchronised frame at a time, and the screen pass's kernel time from the strictly serial schedule.  Then
the same with the light set anew before every frame, and once for light_shafts.  Prints one JSON line and writes it to --out:
every run, and per variant the median and the spread (max - min) over the rounds.

    python scripts/bench_screen_replay.py [--width 1920 --height 1080] [--rounds 3] [--steps 200] [--out profiles/r09_screen_replay.json]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(args, scene, replay):
    from madarch_amd import _binding as B
    from madarch_amd import examples
    R = examples.SCENES[scene](args.width, args.height, Probes=examples.GI_8X8X8_PROBES)
    R.Set_Option(B.OPT_SCREEN_REPLAY, replay)
    return R


def edit_light(R, scene, f):
    from madarch_amd.lights import point_lights, spot_lights
    s = 0.2 * math.sin(0.1 * f)
    if scene == "light_shafts":
        R.Set_Light(1, point_lights.Point_Light, point_lights.Create((5.0 + s, 3.0, 6.0), (0.9, 0.9, 0.9)))
    else:
        R.Set_Light(1, spot_lights.Spot_Light, spot_lights.Create((3.5 + s, 5.0, 2.0), (1.0, 0.0, 0.0), 3.1415 / 4.0, (0.9, 0.9, 0.8)))


def timed(R, scene, steps, sync, animate):
    t0 = time.perf_counter()
    for f in range(steps):
        if animate:
            edit_light(R, scene, f)
        R.Render()
        if sync:
            R.Finish()
    R.Finish()
    return (time.perf_counter() - t0) / steps


def run(args, scene, replay, animate):
    from madarch_amd import _binding as B
    R = build(args, scene, replay)
    mpix = args.width * args.height / 1e6
    for f in range(4):  # the marching pass, the recording pass, replaying passes
        R.Render()
    R.Finish()
    out = {"in_flight_mpix_s": mpix / timed(R, scene, args.steps, False, animate),
           "serial_mpix_s": mpix / timed(R, scene, args.steps, True, animate)}
    R.Set_Option(B.OPT_FRAME_OVERLAP, 0)
    R.Set_Option(B.OPT_TIMING, 1)
    for f in range(4):
        R.Render()
    R.Finish()
    R.Reset_Pass_Times()
    timed(R, scene, max(8, args.steps // 4), True, animate)
    ms, n = R.Pass_Time(B.PASS_SCREEN)
    out["screen_ms"] = ms / max(n, 1)
    out["screen_passes"] = list(R.Screen_Replay_Stats())
    R.Destroy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_screen_replay.json"))
    args = ap.parse_args()
    cases = [("global_illumination", False, args.rounds), ("global_illumination", True, args.rounds), ("light_shafts", True, 1)]
    result = {"width": args.width, "height": args.height, "steps": args.steps, "cases": []}
    for scene, animate, rounds in cases:
        runs = {"a": [], "b": []}
        for _ in range(rounds):
            for v, replay in (("a", 1), ("b", 0)):
                runs[v].append(run(args, scene, replay, animate))
        case = {"scene": scene, "light_edit_every_frame": animate, "runs": runs, "summary": {}}
        for v in runs:
            case["summary"][v] = {k: {"median": statistics.median(r[k] for r in runs[v]), "spread": max(r[k] for r in runs[v]) - min(r[k] for r in runs[v])}
                                  for k in ("in_flight_mpix_s", "serial_mpix_s", "screen_ms")}
        result["cases"].append(case)
    line = json.dumps(result)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
