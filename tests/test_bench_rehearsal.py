"""bench.py's N-rank control flow, launched exactly as the driver launches it (python -m torch.distributed.run ...
bench.py --gpus N --steps K --warmup W), on the CPU: gloo, the oracle as the engine (--rehearse-cpu).  The frame the
ranks assemble must be the single-process frame, whatever N."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(n, port, *extra):
    cmd = [sys.executable]
    if n > 1:
        cmd += ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1", "--master-port", str(port)]
    cmd += [os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "2", "--warmup", "1", "--rehearse-cpu", *extra]
    env = dict(os.environ, OMP_NUM_THREADS="2")
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 0 and len(lines) == 1, out.stdout[-2000:] + out.stderr[-3000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("n", [2, 3])
def test_bench_control_flow_with_n_ranks(n):
    one = _run(1, 0, "--full")
    many = _run(n, 29540 + n + (os.getpid() % 500), "--full")
    assert many["rehearsal"] and many["n_gpus"] == n and many["steps"] == 2
    assert many["frame_sha1"] == one["frame_sha1"]  # tiles and probe slices of n ranks = the whole frame
    # the oracle has no communicator: every rank agrees on the exchange through host memory, in the same process,
    # and the line says so; the pre-warm blocks and the serial segment ran with the same frame count on every rank
    # (or the ranks' collectives would have paired wrongly and the frames differed)
    assert "HOST EXCHANGE FALL-BACK" in many["parallelism"] and "no communicator" in many["parallelism"]
    assert many["serial_segment"] and one["serial_segment"]


def test_plain_run_skips_the_serial_segment_and_dumps_the_last_timed_frame(tmp_path):
    import hashlib

    import numpy as np
    d = _run(1, 0, "--dump-outputs", str(tmp_path))
    assert not d["serial_segment"] and d["steps"] == 2 and d["ms_per_step"] > 0
    img, code = np.load(tmp_path / "framebuffer.npy"), np.load(tmp_path / "framebuffer_nonfinite.npy")
    assert img.dtype == code.dtype == np.float32 and img.shape == code.shape == (64, 96, 3)
    assert np.isfinite(img).all() and np.isin(code, (0, 1, 2, 3)).all() and not img[code > 0].any()
    img[code == 1], img[code == 2], img[code == 3] = np.nan, np.inf, -np.inf
    assert hashlib.sha1(img.tobytes()).hexdigest() == d["frame_sha1"]  # nothing ran after the timed steps


def test_dump_is_finite_and_marks_what_was_not(tmp_path):
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    img = np.arange(4 * 5 * 3, dtype=np.float32).reshape(4, 5, 3)
    img[0, 0, 0], img[1, 2, 1], img[3, 4, 2] = np.nan, np.inf, -np.inf
    bench.dump_outputs(str(tmp_path), img, 0)
    got, code = np.load(tmp_path / "framebuffer.npy"), np.load(tmp_path / "framebuffer_nonfinite.npy")
    assert np.isfinite(got).all() and got[0, 0, 0] == got[1, 2, 1] == got[3, 4, 2] == 0
    assert (code[0, 0, 0], code[1, 2, 1], code[3, 4, 2]) == (1, 2, 3) and (code > 0).sum() == 3
    finite = code == 0
    assert np.array_equal(got[finite], img[finite])


def test_dump_of_a_large_frame_is_a_fixed_sample_of_its_pixels(tmp_path, monkeypatch):
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 2 * 12 * 40)  # room for 40 pixels in the two arrays
    H, W = 16, 24
    img = np.repeat(np.arange(H * W, dtype=np.float32), 3).reshape(H, W, 3)  # each pixel holds its flat index
    img[..., 1] += 0.25
    img[..., 2] += 0.5
    img[5, 7, 1] = np.nan
    samples = []
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), img, 0)
        got, code = np.load(tmp_path / run / "framebuffer.npy"), np.load(tmp_path / run / "framebuffer_nonfinite.npy")
        assert got.shape == code.shape == (40, 3) and np.isfinite(got).all()
        samples.append((got, code))
    assert np.array_equal(samples[0][0], samples[1][0]) and np.array_equal(samples[0][1], samples[1][1])
    got, code = samples[0]
    px = got[:, 0].astype(np.int64)
    assert (np.diff(px) > 0).all() and px[-1] < H * W  # distinct pixels, ascending flat indices
    want = img.reshape(H * W, 3)[px]
    assert np.array_equal(np.where(code == 1, np.nan, got), want, equal_nan=True)
    assert np.array_equal(code == 1, np.isnan(want))
