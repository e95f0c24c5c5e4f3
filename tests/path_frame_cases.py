"""What the tests of the path-traced frame share (tests/test_path_frame_host.py on the CPU, tests/test_gpu_path_frame.py and
tests/path_frame_device_checks.py on the device): the numpy float32 restatement of a pixel's screen position (csrc/mdh_path.h:
path_pixel_uv) over path_trace_cases.u01, of camera_ray behind it, and a camera that is no identity."""
import numpy as np

import path_trace_cases as PT

W, H = 20, 12  # two and a half by one and a half 8 x 8 tiles: both kinds of cut tile
SEED = PT.SEED_PATHS
F = np.float32

# a camera that looks somewhere: a rotation about y by 0.3 and about x by -0.2 (rows), inside the gi room
CAM_POS = (3.25, 2.5, 0.75)


def cam_rows():
    cy, sy, cx, sx = np.cos(0.3), np.sin(0.3), np.cos(-0.2), np.sin(-0.2)
    ry = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])
    return (ry @ rx).astype(np.float32)


def pixel_ids(width, height):
    """(i, j, id) of every pixel, rows top first"""
    j, i = np.divmod(np.arange(width * height, dtype=np.int64), width)
    return i, j, (j * width + i).astype(np.uint32)


def axis(k, n, jitter, jk):
    """path_pixel_axis: every step one binary32 operation"""
    k = np.asarray(k, dtype=np.int64)
    if jitter:
        num = (2 * k).astype(np.float32) + F(2.0) * np.asarray(jk, dtype=np.float32)
    else:
        num = (2 * k + 1).astype(np.float32)
    return (num.astype(np.float32) / F(n)).astype(np.float32) - F(1.0)


def pixel_uv(width, height, seed, sample, jitter, i=None, j=None):
    """(u, v) float32 of pixels (i, j) (default: all, rows top first) for sample `sample`"""
    if i is None:
        i, j, _ = pixel_ids(width, height)
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    ids = (j * width + i).astype(np.uint32)
    jx = PT.u01(seed, ids, sample, 0, 3) if jitter else None
    jy = PT.u01(seed, ids, sample, 0, 4) if jitter else None
    u = axis(i, width, jitter, jx)
    v = -axis(j, height, jitter, jy)
    return u.astype(np.float32), v.astype(np.float32)


def camera_ray(u, v, pos, rows):
    """camera_ray (mdh_device.h; draw_screen.glsl:20-24) in float32: normalize = component / correctly rounded length,
    mat_mul in the order (m0 x + m3 y) + m6 z.  rows[r][c] is the orientation as Set_Camera_Orientation takes it."""
    u, v = np.asarray(u, dtype=np.float32), np.asarray(v, dtype=np.float32)
    m = np.asarray(rows, dtype=np.float32)
    z = np.full_like(u, F(0.0) - F(-1.5))
    length = np.sqrt(((u * u + v * v).astype(np.float32) + z * z).astype(np.float32)).astype(np.float32)
    d = [(c / length).astype(np.float32) for c in (u, v, z)]
    frag = [u, v, np.zeros_like(u)]

    def mul(x):
        return np.stack([((m[r, 0] * x[0] + m[r, 1] * x[1]).astype(np.float32) + m[r, 2] * x[2]).astype(np.float32) for r in range(3)], axis=1)
    org = (mul(frag) + np.asarray(pos, dtype=np.float32)[None, :]).astype(np.float32)
    return org, mul(d)


def frame_rays(width, height, seed, sample, jitter, pos, rows):
    u, v = pixel_uv(width, height, seed, sample, jitter)
    return camera_ray(u, v, pos, rows)


def same_or_nan(a, b):
    """bit for bit, NaN matching NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
