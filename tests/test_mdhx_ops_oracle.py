"""Every MDH_X operation (include/madarch_hip.h) at the IEEE edges, on the CPU: the exact reference of tests/mdhx_cases.py
against itself and against hand-computed bit patterns, then the oracle's interpreter held to that reference -- never to
another evaluator -- through the Eval window (raw bits out of Eval_Distances_To) and the Frame window (the geometry buffer)."""
import numpy as np
import pytest

import mdhx_cases as M
from madarch_amd import _binding as B
from madarch_amd import exprs as X

H = lambda s: int(s, 16)


# ------------------------------------------------------------------------------------------ the reference against itself
def test_reference_hand_computed_bit_patterns():
    r = M.ref_op
    for op, a, b, want in [
            (X.X_ADD, 0x3F800000, 0x33800000, 0x3F800000),  # 1 + 2^-24: a tie, to even
            (X.X_ADD, 0x3F800001, 0x33800000, 0x3F800002),  # (1 + ulp) + 2^-24: a tie, to even: up
            (X.X_ADD, 0x7F7FFFFF, 0x73000000, 0x7F800000),  # FLT_MAX + half an ulp: overflow
            (X.X_ADD, 0x7F7FFFFF, 0x72FFFFFF, 0x7F7FFFFF),  # ... just less: stays
            (X.X_ADD, 0x80000000, 0x80000000, 0x80000000), (X.X_ADD, 0x00000000, 0x80000000, 0x00000000),
            (X.X_ADD, 0x3F800000, 0xBF800000, 0x00000000), (X.X_ADD, 0x00000001, 0x00000001, 0x00000002),
            (X.X_SUB, 0x00000000, 0x00000000, 0x00000000), (X.X_SUB, 0x80000000, 0x00000000, 0x80000000),
            (X.X_SUB, 0x40A00000, 0x40400000, 0x40000000),
            (X.X_MUL, 0x00800000, 0x3F000000, 0x00400000),  # FLT_MIN / 2: subnormal, exact
            (X.X_MUL, 0x00000001, 0x3F000000, 0x00000000),  # 2^-150: a tie, to even: 0
            (X.X_MUL, 0x00000003, 0x3F000000, 0x00000002),  # 1.5 * 2^-149: a tie, to even: 2
            (X.X_MUL, 0x80000001, 0x3F400000, 0x80000001),  # -0.75 * 2^-149 rounds to -2^-149
            (X.X_MUL, 0x7F7FFFFF, 0x40000000, 0x7F800000), (X.X_MUL, 0x80000000, 0x3F800000, 0x80000000),
            (X.X_MUL, 0x3EAAAAAB, 0x40400000, 0x3F800000),  # fl (1/3) * 3 = 1 + 2^-25: rounds to 1
            (X.X_DIV, 0x3F800000, 0x40400000, 0x3EAAAAAB), (X.X_DIV, 0x40A00000, 0x40400000, 0x3FD55555),
            (X.X_DIV, 0x3F800000, 0x80000000, 0xFF800000), (X.X_DIV, 0x00000001, 0x40000000, 0x00000000),
            (X.X_DIV, 0x00000000, 0xBF800000, 0x80000000), (X.X_DIV, 0x3F800000, 0x7F800000, 0x00000000),
            (X.X_DIVF, 0x40A00000, 0x40400000, 0x3FD55555),
            (X.X_MIN, 0x00000000, 0x80000000, 0x80000000), (X.X_MIN, 0x80000000, 0x00000000, 0x80000000),
            (X.X_MAX, 0x00000000, 0x80000000, 0x00000000), (X.X_MAX, 0x80000000, 0x00000000, 0x00000000),
            (X.X_MIN, 0x7FC00000, 0x3F800000, 0x3F800000), (X.X_MAX, 0x3F800000, 0x7FC00000, 0x3F800000),
            (X.X_MIN, 0xFF800000, 0x3F800000, 0xFF800000), (X.X_MAX, 0x7F800000, 0x7F7FFFFF, 0x7F800000),
            (X.X_LT, 0x80000000, 0x00000000, 0x00000000), (X.X_LE, 0x80000000, 0x00000000, 0x3F800000),
            (X.X_GE, 0x7FC00000, 0x7FC00000, 0x00000000), (X.X_GT, 0x7F800000, 0x7F7FFFFF, 0x3F800000),
            (X.X_POW, 0x7F800000, 0xBF800000, 0x00000000), (X.X_POW, 0x7F800000, 0x00000000, 0x3F800000),
            (X.X_POW, 0x7F800000, 0x40000000, 0x7F800000), (X.X_POW, 0x00000000, 0x00000000, 0x00000000),
            (X.X_POW, 0x00000000, 0xBF800000, 0x00000000)]:
        assert r(op, a, b) == want, (M.OP_NAME[op], hex(a), hex(b), r(op, a, b))
    assert r(X.X_DIVF, H("40A00000"), H("40400000"), ada=1) == H("41000000")  # Madarch.Values."/": 5 "/" 3 = 8
    for op, a, want in [
            (X.X_SQRT, 0x40800000, 0x40000000), (X.X_SQRT, 0x40000000, 0x3FB504F3), (X.X_SQRT, 0x80000000, 0x80000000),
            (X.X_SQRT, 0x00000001, 0x1A3504F3),  # sqrt (2^-149) = sqrt 2 * 2^-75
            (X.X_SQRT, 0x0F800000, 0x27800000),  # sqrt (2^-96) = 2^-48
            (X.X_SQRT, 0x7F7FFFFF, 0x5F7FFFFF), (X.X_SQRT, 0x7F800000, 0x7F800000), (X.X_SQRT, 0x3F7FFFFF, 0x3F7FFFFF),
            (X.X_FLOOR, 0xBF000000, 0xBF800000), (X.X_FLOOR, 0x3F000000, 0x00000000), (X.X_FLOOR, 0x80000000, 0x80000000),
            (X.X_FLOOR, 0xC0200000, 0xC0400000), (X.X_FLOOR, 0x4AFFFFFF, 0x4AFFFFFE), (X.X_FLOOR, 0xCAFFFFFF, 0xCB000000),
            (X.X_FLOOR, 0x80000001, 0xBF800000), (X.X_FLOOR, 0xFF800000, 0xFF800000),
            (X.X_SIGN, 0x80000001, 0xBF800000), (X.X_SIGN, 0x80000000, 0x00000000), (X.X_SIGN, 0x7FC00000, 0x00000000), (X.X_SIGN, 0x7F800000, 0x3F800000),
            (X.X_NEG, 0x00000000, 0x80000000), (X.X_NEG, 0x7F800000, 0xFF800000), (X.X_ABS, 0x80000000, 0x00000000), (X.X_ABS, 0xFF7FFFFF, 0x7F7FFFFF),
            (X.X_ITOF, 0x00000007, 0x40E00000), (X.X_ITOF, 0xFFFFFFFF, 0xBF800000), (X.X_ITOF, 0x80000000, 0xCF000000),
            (X.X_ITOF, 0x7FFFFFFF, 0x4F000000), (X.X_ITOF, 0x01000001, 0x4B800000), (X.X_ITOF, 0x01000003, 0x4B800002),
            (X.X_ITOF, 0x7FFFFFBF, 0x4EFFFFFF), (X.X_ITOF, 0x7FFFFFC0, 0x4F000000), (X.X_ITOF, 0x80000001, 0xCF000000),
            (X.X_MOV, 0x7F800000, 0x7F800000)]:
        assert r(op, a) == want, (M.OP_NAME[op], hex(a), hex(r(op, a)) if isinstance(r(op, a), int) else r(op, a))
    for op, a, b in [(X.X_ADD, M.INF, 0xFF800000), (X.X_SUB, M.INF, M.INF), (X.X_MUL, 0, M.INF), (X.X_DIV, 0, M.SIGN), (X.X_DIV, M.INF, 0xFF800000),
                     (X.X_SQRT, 0xBF800000, 0), (X.X_SQRT, 0x80000001, 0), (X.X_ADD, M.QNAN, M.ONE), (X.X_MIN, M.QNAN, 0x7FFFFFFF), (X.X_FLOOR, M.QNAN, 0),
                     (X.X_POW, 0xBF800000, M.ONE), (X.X_POW, M.QNAN, 0), (X.X_ACOS, 0x3F800001, 0), (X.X_ASIN, 0xC0200000, 0), (X.X_SIN, M.INF, 0),
                     (X.X_TAN, 0xFF800000, 0), (X.X_COS, M.QNAN, 0), (X.X_ATAN, M.QNAN, 0)]:
        assert r(op, a, b) is M.NAN, (M.OP_NAME[op], hex(a), hex(b))
    # SEL takes b when a != 0: a NaN condition takes b, -0 takes c
    assert [r(X.X_SEL, c, 7, 9) for c in (0, M.SIGN, 1, M.QNAN, M.ONE, 0xFF800000)] == [9, 9, 7, 7, 7, 7]
    assert M.check(r(X.X_ATAN, M.INF), M.PI_2) and M.check(r(X.X_ATAN, 0xFF800000), M.PI_2 | M.SIGN)


def test_reference_is_consistent_with_itself():
    r = M.ref_op
    finite = [v for v in M.EDGES if not (M.is_nan(v) or M.is_inf(v))]
    for a, b in M.pairs(M.EDGES):
        for op in (X.X_ADD, X.X_MUL, X.X_MIN, X.X_MAX):
            assert r(op, a, b) == r(op, b, a), (M.OP_NAME[op], hex(a), hex(b))  # commutative, the sign of zero included
        assert r(X.X_LT, a, b) == r(X.X_GT, b, a) and r(X.X_LE, a, b) == r(X.X_GE, b, a)
        s, n = r(X.X_SUB, a, b), r(X.X_SUB, b, a)
        assert (s is M.NAN and n is M.NAN) or M.is_zero(s) or s == n ^ M.SIGN  # a - b = -(b - a) (an exact zero is +0 both ways)
    # DIV against MUL where the product is exact: (a * 2^k) / 2^k = a, and the quotient of a product by a factor
    for a in finite:
        for p in (0x40000000, 0x3F000000, 0x41800000, 0xC0000000):
            prod = r(X.X_MUL, a, p)
            if M.is_inf(prod) or M.frac(prod) != M.frac(a) * M.frac(p):
                continue  # overflowed, or rounded in the subnormal range
            assert r(X.X_DIV, prod, p) == a, (hex(a), hex(p))
    for a, b in ((3, 5), (7, 9), (1 << 20, 3), (12345, 6789)):
        fa, fb = M.bits(float(a)), M.bits(float(b))
        assert r(X.X_DIV, r(X.X_MUL, fa, fb), fb) == fa
    # sqrt of a square, and x * x against the rounded root's square bracket
    for a in (M.bits(3.0), M.bits(1.5), 0x3F800001, M.bits(4097.0), 0x1A3504F3):
        sq = M.frac(a) ** 2
        assert M._sqrt(M.round_f32(sq)) == a or M.frac(M.round_f32(sq)) != sq
    for a in finite:
        if a & M.SIGN or M.is_zero(a):
            continue
        s = M.frac(M._sqrt(a))
        ulp = M.frac(M._sqrt(a) + 1) - s
        assert (s - ulp / 2) ** 2 <= M.frac(a) <= (s + ulp / 2) ** 2, hex(a)  # within half an ulp of the true root
    # numpy's own binary32 arithmetic (IEEE on the CPU) as a second opinion over every pair
    A, Bv = (np.array(v, dtype=np.uint32).view(np.float32) for v in zip(*M.pairs(M.EDGES)))
    with np.errstate(all="ignore"):
        for op, got in ((X.X_ADD, A + Bv), (X.X_SUB, A - Bv), (X.X_MUL, A * Bv), (X.X_DIV, A / Bv)):
            assert not M.mismatches([r(op, a, b) for a, b in M.pairs(M.EDGES)], got, M.OP_NAME[op])
        e = np.array(M.EDGES, dtype=np.uint32).view(np.float32)
        assert not M.mismatches([r(X.X_SQRT, a) for a in M.EDGES], np.sqrt(e), "SQRT")
        assert not M.mismatches([r(X.X_FLOOR, a) for a in M.EDGES], np.floor(e), "FLOOR")
        ints = np.array(M.EDGES + M.ITOF_EXTRA, dtype=np.uint32).view(np.int32)
        assert not M.mismatches([r(X.X_ITOF, a) for a in M.EDGES + M.ITOF_EXTRA], ints.astype(np.float32), "ITOF")


def test_run_program_walks_the_registers():
    R = M.run_program(M.register_walk(), comps=[0, 0, 0, M.bits(2.0), 3])
    total = float(sum(range(3, 64)) + 1)  # R63 = 1 + 3 + ... + 63
    r37 = float(sum(range(3, 38)) + 1) ** 2
    assert M.val(R[0]) == total - r37 and M.val(R[2]) == total + M.val(R[62]) and M.val(R[62]) == 1.0 + 3 + 4
    assert len(M.add_chain(X.X_MAX_WORDS)) == X.X_MAX_WORDS and M.val(M.run_program(M.add_chain(X.X_MAX_WORDS))[0]) == X.X_MAX_WORDS - 4 + 0.5


# ------------------------------------------------------------------------------------------ the oracle, Eval window
@pytest.mark.parametrize("ada", [0, 1])
def test_oracle_binary_operations_over_the_edges(orc, ada):
    """Every binary operation over EDGES x EDGES (and POW's own cases), both MDH_OPT_ADA_EVAL_DIV settings."""
    pair_list = M.pairs(M.EDGES)
    got = M.binary_window(orc, pair_list, ada)
    bad, n = [], 0
    for op in M.BINARY:
        bad += M.mismatches([M.ref_op(op, a, b, ada=ada) for a, b in pair_list], got[op], M.OP_NAME[op])
        n += len(pair_list)
    pw = M.binary_window(orc, M.POW_CASES, ada, ops=[X.X_POW])[X.X_POW]
    bad += M.mismatches([M.pow_spec(a, b) for a, b in M.POW_CASES], pw, "POW case")
    assert not bad, "%d of %d cases:\n%s" % (len(bad), n + len(M.POW_CASES), "\n".join(bad[:40]))


def test_oracle_pow_bound_is_not_tuned(orc):
    """The worst ratio of the oracle's POW error to the bound over the held cases, printed (and below 1)."""
    pair_list = M.pairs(M.EDGES) + M.POW_CASES
    got = M.binary_window(orc, pair_list, ops=[X.X_POW])[X.X_POW]
    worst = (0.0, ())
    for (a, b), g in zip(pair_list, got):
        spec = M._pow(a, b)
        if isinstance(spec, tuple) and not (M.is_nan(int(g)) or M.is_inf(int(g))):
            ratio = abs(M.val(int(g)) - spec[1]) / (spec[2] * abs(spec[1]))
            worst = max(worst, (ratio, (hex(a), hex(b))))
    print("POW: worst error / bound = %.3f at %s" % worst)
    assert worst[0] < 1.0


def test_oracle_unary_operations_over_the_edges(orc):
    bad, n = [], 0
    for op in M.UNARY:
        ops_ = M.unary_operands(op)
        bad += M.mismatches([M.ref_op(op, a) for a in ops_], M.unary_window(orc, op), M.OP_NAME[op])
        n += len(ops_)
    pts = M.sel_points()
    got = M.eval_window(orc, M.three_ops([X.X_SEL]), pts)[:, 0]
    bad += M.mismatches([M.ref_op(X.X_SEL, int(a), int(b), int(c)) for a, b, c in pts], got, "SEL")
    assert not bad, "%d of %d cases:\n%s" % (len(bad), n + len(pts), "\n".join(bad[:40]))


@pytest.mark.parametrize("count", [1, 63, 64, 65])
def test_oracle_sqrt_over_the_wave_layouts(orc, count):
    """`count` points, one radicand per point (the lane it has on the device): see sqrt_count_layouts."""
    bad = [m for v in M.sqrt_count_layouts(count) for m in M.lanes_complaints(orc, X.X_SQRT, v)]
    assert not bad, "\n".join(bad[:40])


def test_oracle_sqrt_over_whole_waves(orc):
    assert not M.lanes_complaints(orc, X.X_SQRT, M.sqrt_wave_points())


def test_oracle_registers_and_encodings(orc):
    M.registers_and_encodings([orc], [orc])


@pytest.mark.xfail(strict=True, reason="pow (FLT_MAX = 0x7F7FFFFF, 1 = 0x3F800000): float64 gives FLT_MAX; the oracle, the kernels' interpreter and the "
                   "hiprtc build all give +inf (0x7F800000): log2 (FLT_MAX) rounds to 128 in binary32 and 2^128 overflows")
def test_oracle_pow_unsettled(orc):
    got = M.binary_window(orc, M.POW_UNSETTLED, ops=[X.X_POW])[X.X_POW]
    assert not M.mismatches([M._pow(a, b) for a, b in M.POW_UNSETTLED], got, "POW")


# ------------------------------------------------------------------------------------------ the oracle, Frame window
@pytest.fixture(scope="module")
def frame_oracle(orc):
    fw = M.Frame_Window(orc, M.frame_distance_ops())
    yield fw
    fw.destroy()


def test_oracle_frame_window_carries_a_quotient(frame_oracle):
    """a / b with 5 and 3: gb_t is fl (5/3) scaled by 2 in all 64 pixels, steps 2."""
    i = M.FRAME_OPS.index(X.X_DIV)
    assert frame_oracle.result_bits(M.bits(5.0), M.bits(3.0), 0, i, 5.0 / 3.0) == 0x3FD55555
    assert frame_oracle.class_code(M.bits(5.0), M.bits(3.0), 0, i) == M.CLASS_OTHER
    assert frame_oracle.class_code(0, M.SIGN, 0, i) == M.CLASS_NAN


def test_oracle_frame_window_every_operation(frame_oracle):
    """Every frame-window case on the oracle against the exact reference, both modes; each expectation is reachable (a class
    code, or a value scaled into [2, 4): never the guard's 7.5)."""
    cases = M.frame_cases()
    bad = []
    for case in cases:
        bad += M.check_frame_case(frame_oracle, case, M.frame_spec(case))
    assert not bad, "%d complaints over %d cases:\n%s" % (len(bad), len(cases), "\n".join(bad[:40]))


def test_oracle_frame_window_literal_operands(orc):
    fw = M.Frame_Window(orc, M.frame_distance_literals(M.LITERAL_TRIPLES))
    try:
        bad = []
        for i in range(len(M.LITERAL_TRIPLES)):
            bad += M.check_literal_case(fw, i)
        assert not bad, "\n".join(bad)
    finally:
        fw.destroy()


# ------------------------------------------------------------------------------------------ the oracle, the min forms
def test_oracle_min_forms(orc):
    bad, _ = M.check_min_forms(orc)
    assert not bad, "\n".join(bad[:40])


def test_oracle_literal_operands_eval_window(orc):
    got = M.literal_window(orc)
    assert not M.mismatches([M.literal_spec(t) for t in M.LITERAL_TRIPLES], np.array(got, dtype=np.uint32), "literal")
