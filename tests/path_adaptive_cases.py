"""What the tests of the adaptive path-traced frame share (tests/test_path_adaptive_host.py on the CPU, tests/test_gpu_path_adaptive.py
and tests/path_adaptive_device_checks.py on the device): the numpy float32 restatement of a pixel's update and of the stopping
rule (csrc/mdh_path.h: path_pixel_update, path_pixel_active), the chain of public queries an adaptive frame is held against, and the
rule's parameters per scene."""
import numpy as np

import path_frame_cases as PF
import path_trace_cases as PT

F = np.float32
SEED = PF.SEED
BAD = np.array([PT.BAD_BITS], np.uint32).view(np.float32)[0]  # the quiet NaN of a pixel that was not traced

# the chain's rounds and bounds (the issue's): rounds of (2, 2, 3, 1) samples, 2 .. 8 samples a pixel
ROUNDS, MIN_SAMPLES, MAX_SAMPLES = (2, 2, 3, 1), 2, 8
FLOOR = 0.01
# the tolerance per scene, fixed on the device so that on the 20 x 12 frame some pixels retire before MAX_SAMPLES and some
# reach it, with and without jitter (test_gpu_path_adaptive.py asserts both on the chain's own result and names this table).
# Seen at 0.1, pixels that reached 8 samples with / without jitter: rooms 6 / 5 (its camera sees mostly unlit wall, whose
# variance is exactly 0), partition 99 / 21, mesh 15 / 11, open scene 102 / 88 of 240; at 0.8 the partition and the rooms have none.
TOLERANCE = {"rooms": 0.1, "partition, Clamp": 0.1, "mesh, triangle BVH": 0.1, "open scene": 0.1, "partition, Clamp, global residency": 0.1}
# the one large frame: 67 584 slots, 264 workgroup totals -- the scan crosses its chunk of 256.  At 0.05 the room keeps 1 647
# pixels running behind the first round, 12 of them in the slots of workgroups 256 .. 263
LARGE_W, LARGE_H, LARGE_ROUNDS, LARGE_MAX, LARGE_TOLERANCE = 264, 256, (2, 2, 2), 6, 0.05


def update(rgb, n, m1, m2):
    """path_pixel_update for the pixels of `rgb` (k, 3): every step one binary32 operation -> n, m1, m2"""
    rgb = np.asarray(rgb, dtype=np.float32)
    y = ((rgb[:, 0] + rgb[:, 1]).astype(np.float32) + rgb[:, 2]).astype(np.float32)
    yy = (y * y).astype(np.float32)
    return n + 1, (m1 + y).astype(np.float32), (m2 + yy).astype(np.float32)


def active(n, m1, m2, min_samples, max_samples, tolerance, floor):
    """path_pixel_active: -> bool array"""
    n = np.asarray(n, dtype=np.int64)
    m1, m2 = np.asarray(m1, dtype=np.float32), np.asarray(m2, dtype=np.float32)
    with np.errstate(all="ignore"):
        c = n.astype(np.float32)
        mean = (m1 / c).astype(np.float32)
        q = (m2 / c).astype(np.float32)
        mm = (mean * mean).astype(np.float32)
        var = (q - mm).astype(np.float32)
        e = (var / c).astype(np.float32)
        lim = (F(tolerance) * (mean + F(floor)).astype(np.float32)).astype(np.float32)
        ll = (lim * lim).astype(np.float32)
        judged = e > ll  # (any NaN: False)
    return np.where(n >= max_samples, False, np.where(np.isnan(m1) | np.isnan(m2), False, np.where(n < min_samples, True, judged)))


def radiances(R, width, height, seed, bounces, jitter, samples):
    """radiance[s] (W H, 3): what sample s adds to each pixel, from public queries only -- Path_Trace over Path_Frame_Rays (s) with
    sample_first = s, sample_count = 1 into zeroed sums.  (0 + rgb against rgb differs only for a -0 radiance, which the estimator
    cannot produce from a +0 start: nothing is masked.)  Opens, and leaves open, a plain frame of R."""
    R.Path_Frame_Begin(width, height, Seed=seed, Bounces=bounces, Jitter=jitter)
    out = []
    for s in range(samples):
        org, drs = R.Path_Frame_Rays(s)
        out.append(R.Path_Trace(org, drs, Seed=seed, Id_First=0, Sample_First=s, Sample_Count=1, Bounces=bounces)["rgb"])
    return out


class Chain:
    """the state of an adaptive frame restated in numpy float32 over `radiance`: a pixel's k-th sample is radiance[k] of that
    pixel, the rule is evaluated where a round starts"""

    def __init__(self, radiance, min_samples, max_samples, tolerance, floor):
        self.radiance = np.stack(radiance)  # (sample, pixel, channel)
        self.rule = (min_samples, max_samples, tolerance, floor)
        pixels = len(radiance[0])
        self.sums = np.zeros((pixels, 3), np.float32)
        self.n = np.zeros(pixels, np.int64)
        self.m1 = np.zeros(pixels, np.float32)
        self.m2 = np.zeros(pixels, np.float32)

    def active(self):
        return active(self.n, self.m1, self.m2, *self.rule)

    def round(self, sample_count):
        running = self.active()
        target = np.minimum(self.n + sample_count, self.rule[1])
        for _ in range(sample_count):
            take = np.nonzero(running & (self.n < target))[0]
            if len(take) == 0:
                break
            rgb = self.radiance[self.n[take], take]
            untraced = np.isnan(rgb).any(axis=1)  # (Path_Trace's answer to a ray outside its bound: the pixel is not marched)
            good, bad = take[~untraced], take[untraced]
            self.sums[good] = (self.sums[good] + rgb[~untraced]).astype(np.float32)
            self.n[good], self.m1[good], self.m2[good] = update(rgb[~untraced], self.n[good], self.m1[good], self.m2[good])
            self.sums[bad] = BAD
            self.m1[bad] = BAD
            self.m2[bad] = BAD
            running[bad] = False  # (the lane leaves its loop)

    def state(self):
        return {"sums": self.sums.copy(), "count": self.n.astype(np.int32), "m1": self.m1.copy(), "m2": self.m2.copy(), "active": int(self.active().sum()),
                "total_samples": int(self.n.sum())}


def device_state(R):
    """the same of renderer R's adaptive frame"""
    st = R.Path_Frame_Stats()
    sums = R.Path_Frame_Read(Rgb=False, Sums=True)["sums"].reshape(-1, 3)
    mom = st["moments"].reshape(-1, 2)
    return {"sums": sums, "count": st["count"].reshape(-1), "m1": np.ascontiguousarray(mom[:, 0]), "m2": np.ascontiguousarray(mom[:, 1]), "active": st["active"],
            "total_samples": st["total_samples"]}


def differences(got, want):
    """the names of what differs between two states, bit for bit (NaN matching NaN)"""
    out = []
    for k in ("sums", "m1", "m2"):
        if not PF.same_or_nan(got[k], want[k]):
            bad = np.nonzero(~((np.asarray(got[k]).view(np.uint32) == np.asarray(want[k]).view(np.uint32)) | (np.isnan(got[k]) & np.isnan(want[k]))).reshape(len(got[k]), -1).all(axis=1))[0]
            out.append("%s at %d pixels, first %d: %s against %s" % (k, len(bad), bad[0], got[k][bad[0]], want[k][bad[0]]))
    if not np.array_equal(got["count"], want["count"]):
        bad = np.nonzero(got["count"] != want["count"])[0]
        out.append("count at %d pixels, first %d: %d against %d" % (len(bad), bad[0], got["count"][bad[0]], want["count"][bad[0]]))
    for k in ("active", "total_samples"):
        if int(got[k]) != int(want[k]):
            out.append("%s: %d against %d" % (k, got[k], want[k]))
    return out
