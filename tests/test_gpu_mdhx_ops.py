"""Every MDH_X operation at the IEEE edges on the device: the kernels' interpreter through the Eval window (raw bits), the
hiprtc build through the Frame window (the geometry buffer), both against the exact reference of tests/mdhx_cases.py and,
bit for bit, against the oracle; the register file's two banks, the encodings, and the culled min forms of jit_min_form."""
import numpy as np
import pytest

import mdhx_cases as M
from madarch_amd import _binding as B
from madarch_amd import exprs as X

pytestmark = pytest.mark.gpu


def held(specs, got, want_oracle, label):
    """Complaints of `got` against the reference, and against the oracle's bits (NaN-ness where either is a NaN)."""
    bad = M.mismatches(specs, got, label)
    if not M.same_non_nan_bits(got, want_oracle):
        g, o = (np.asarray(v).view(np.uint32).ravel() for v in (got, want_oracle))
        bad += ["%s #%d: 0x%08X, the oracle has 0x%08X" % (label, i, g[i], o[i]) for i in np.nonzero(g != o)[0]
                if not (M.is_nan(int(g[i])) and M.is_nan(int(o[i])))][:20]
    return bad


# ------------------------------------------------------------------------------------------ 1. the interpreter, raw bits
@pytest.mark.parametrize("ada", [0, 1])
def test_interpreter_binary_operations(hip, orc, ada):
    pair_list = M.pairs(M.EDGES) + M.POW_CASES
    got, want = M.binary_window(hip, pair_list, ada), M.binary_window(orc, pair_list, ada)
    bad = []
    for op in M.BINARY:
        specs = [M.pow_spec(a, b) if op == X.X_POW else M.ref_op(op, a, b, ada=ada) for a, b in pair_list]
        bad += held(specs, got[op], want[op], M.OP_NAME[op])
    assert not bad, "%d complaints:\n%s" % (len(bad), "\n".join(bad[:40]))


def test_interpreter_unary_operations_and_sel(hip, orc):
    bad = []
    for op in M.UNARY:
        bad += held([M.ref_op(op, a) for a in M.unary_operands(op)], M.unary_window(hip, op), M.unary_window(orc, op), M.OP_NAME[op])
    pts = M.sel_points()
    p = M.three_ops([X.X_SEL])
    bad += held([M.ref_op(X.X_SEL, int(a), int(b), int(c)) for a, b, c in pts], M.eval_window(hip, p, pts)[:, 0], M.eval_window(orc, p, pts)[:, 0], "SEL")
    assert not bad, "%d complaints:\n%s" % (len(bad), "\n".join(bad[:40]))


@pytest.mark.parametrize("count", [1, 63, 64, 65])
def test_interpreter_sqrt_over_the_wave_layouts(hip, count):
    """`count` points, one radicand per point and lane, 64 lanes to a wavefront: ordinary radicands only, tiny ones only, and
    exactly one radicand below 2^-96 (positive, or a negative subnormal) in the first lane, the last lane of the first wave
    and the last point -- the wave-level branch of sqrt_ takes either side with every kind of operand on it."""
    bad = [m for v in M.sqrt_count_layouts(count) for m in M.lanes_complaints(hip, X.X_SQRT, v)]
    assert not bad, "\n".join(bad[:40])


def test_interpreter_sqrt_over_whole_waves(hip, orc):
    """Seven whole waves and a tail: none / all / one (lane 0, 63, 29) below 2^-96, one negative subnormal, only such."""
    v = M.sqrt_wave_points()
    assert not M.lanes_complaints(hip, X.X_SQRT, v)
    assert M.same_non_nan_bits(M.lanes_window(hip, X.X_SQRT, v), M.lanes_window(orc, X.X_SQRT, v))


@pytest.mark.xfail(strict=True, reason="pow (FLT_MAX = 0x7F7FFFFF, 1 = 0x3F800000): float64 gives FLT_MAX; the oracle, the kernels' interpreter and the "
                   "hiprtc build all give +inf (0x7F800000): log2 (FLT_MAX) rounds to 128 in binary32 and 2^128 overflows")
def test_interpreter_pow_unsettled(hip):
    got = M.binary_window(hip, M.POW_UNSETTLED, ops=[X.X_POW])[X.X_POW]
    assert not M.mismatches([M._pow(a, b) for a, b in M.POW_UNSETTLED], got, "POW")


# ------------------------------------------------------------------------------------------ 2. registers and encodings
def test_registers_and_encodings(hip, orc):
    M.registers_and_encodings([hip, orc], [hip])


# ------------------------------------------------------------------------------------------ 3. the hiprtc build, every operation
GROUPS = {"arith": [X.X_ADD, X.X_SUB, X.X_MUL, X.X_DIV, X.X_DIVF, X.X_POW], "order": [X.X_MIN, X.X_MAX, X.X_LT, X.X_GT, X.X_LE, X.X_GE, X.X_SEL],
          "unary": M.UNARY}


@pytest.fixture(scope="module")
def oracle_bits(orc):
    return M.oracle_case_bits(orc, M.frame_cases())


@pytest.fixture(scope="module")
def frame_windows(hip):
    fws = {}

    def get(jit):
        if jit not in fws:
            fws[jit] = M.Frame_Window(hip, M.frame_distance_ops(), jit)
        return fws[jit]
    yield get
    for fw in fws.values():
        fw.destroy()


@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("jit", [1, 0])
def test_frame_window_every_operation(frame_windows, oracle_bits, jit, group):
    """One Distance program (one hiprtc build) computes every operation; value mode on every case whose expectation is a
    nonzero finite number, class mode on every case."""
    fw = frame_windows(jit)
    cases = [c for c in M.frame_cases() if M.FRAME_OPS[c[0]] in GROUPS[group]]
    bad = []
    for case in cases:
        bad += M.check_frame_case(fw, case, M.frame_spec(case), oracle_bits[case])
    assert fw.R.Get_Option(B.OPT_JIT) == jit  # (a failed hiprtc build would have switched it off)
    assert not bad, "%d complaints over %d cases:\n%s" % (len(bad), len(cases), "\n".join(bad[:40]))


# ------------------------------------------------------------------------------------------ 4. the hiprtc build, literal operands
def test_frame_window_literal_operands(hip, orc):
    """(operation, LIT a, LIT b) at edge values, which the compiler may fold: against the reference and the oracle, and the
    compiled frames equal to the interpreted ones."""
    want = M.literal_window(orc)
    assert not held([M.literal_spec(t) for t in M.LITERAL_TRIPLES], np.array(M.literal_window(hip), dtype=np.uint32), np.array(want, dtype=np.uint32), "literal, interpreted")
    logs = []
    for jit in (1, 0):
        fw = M.Frame_Window(hip, M.frame_distance_literals(M.LITERAL_TRIPLES), jit)
        try:
            bad = []
            for i in range(len(M.LITERAL_TRIPLES)):
                bad += M.check_literal_case(fw, i, want[i])
            assert fw.R.Get_Option(B.OPT_JIT) == jit
            assert not bad, "jit %d:\n%s" % (jit, "\n".join(bad))
            logs.append(fw.log)
        finally:
            fw.destroy()
    assert logs[0] == logs[1]


# ------------------------------------------------------------------------------------------ 5. the min forms
def test_min_forms_against_the_running_minimum(hip, tmp_path, monkeypatch):
    dump = tmp_path / "mdh_jit_kinds.h"
    monkeypatch.setenv("MADARCH_HIP_JIT_DUMP", str(dump))
    for jit in (1, 0):
        bad, opt = M.check_min_forms(hip, jit)
        assert opt == jit
        assert not bad, "jit %d:\n%s" % (jit, "\n".join(bad[:40]))
    text = dump.read_text()
    assert all("float jit_p%d_min(" % k in text for k in (1, 2, 3, 4)) and "float jit_p0_min(" not in text  # the four Roots; the Gate has no root
    for k, fin in ((1, "sqrt_(d2_) - r"), (2, "sqrt_(d2_) + r"), (3, " + sqrt_(d2_)"), (4, "sqrt_(d2_))")):
        body = text.split("float jit_p%d_min(" % k)[1].split("\n}\n")[0]
        assert fin in body, (k, body)
