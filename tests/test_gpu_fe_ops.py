"""GPU: every device field primitive on directed operands, placed lane by lane.

The library's test hook `stark_test_fe_op` (csrc/ntt.hip) runs one primitive of fp_dev.h, fe_mul_asm.inc, fe_db.h
or one lazy-range helper of ntt.hip per launch, record i in lane i % 64 of wave i / 64.  tests/fe_cases.py holds
the tables (carry and borrow chains at their edges, values at 2p and at 2p's top word, Shoup products whose
truncated quotient is one short laid out wave by wave, digit-basis products next to the quotient margin) and
the exact expected words; tests/test_fe_cases_cpu.py checks the tables themselves.  Mode 1 enters the primitive
on the odd lanes only (a partial exec); the even lanes copy their first operand.  Every record of every table is
compared bit for bit."""
import ctypes

import numpy as np
import pytest

import fe_cases as F
import stark_amd as S

pytestmark = pytest.mark.gpu

BAD_ARG = 3  # STARK_ERR_BAD_ARG (include/stark_hip.h)


def _hook():
    fn = S.load_library().stark_test_fe_op
    fn.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                   ctypes.c_uint32, ctypes.c_void_p]
    fn.restype = ctypes.c_int
    return fn


def _run(c, op, ins, mode):
    """ins: (n, 8 * elements read) u32 -> (n, 8 * elements written) u32."""
    num, n_in, n_out = F.OPS[op]
    n = len(ins)
    assert ins.dtype == np.uint32 and ins.shape == (n, 8 * n_in)
    out = np.full((n, 8 * n_out), 0xA5A5A5A5, dtype=np.uint32)
    d_in, d_out = c.alloc(ins.nbytes), c.alloc(out.nbytes)
    try:
        c.h2d(d_in, ins)
        c.h2d(d_out, out)
        rc = _hook()(c.h, num, d_in, d_out, n, mode, None)
        assert rc == 0, (op, rc)
        c.d2h(out, d_out)
    finally:
        c.free(d_in)
        c.free(d_out)
    return out


def _hex(words):
    return [hex(sum(int(x) << (32 * k) for k, x in enumerate(words[8 * e: 8 * e + 8]))) for e in range(len(words) // 8)]


def _compare(op, mode, recs, got, want):
    if np.array_equal(got, want):
        return
    bad = np.flatnonzero((got != want).any(axis=1))
    i = int(bad[0])
    raise AssertionError(f"{op} mode {mode}: {len(bad)} of {len(recs)} records wrong, first record {i} (lane {i % 64}, "
                         f"wave {i // 64}): operands {[hex(v) for v in recs[i]]}, got {_hex(got[i])}, "
                         f"want {_hex(want[i])}")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("op", sorted(F.OPS, key=lambda k: F.OPS[k][0]))
def test_fe_op(ctx, op, mode):
    recs = F.table(op)
    got = _run(ctx, op, F.encode(op, recs), mode)
    _compare(op, mode, recs, got, F.expected_array(op, mode))


@pytest.mark.parametrize("op", sorted(F.OPS, key=lambda k: F.OPS[k][0]))
def test_one_record(ctx, op):
    """n_records = 1: one lane of one wave, in both modes (mode 1 copies: lane 0 is even)."""
    recs = F.table(op)[:1]
    for mode in (0, 1):
        got = _run(ctx, op, F.encode(op, recs), mode)
        _compare(op, mode, recs, got, F.expected_array(op, mode)[:1])


def test_error_returns(ctx):
    fn = _hook()
    d = ctx.alloc(320 * 64)
    try:
        assert fn(None, 0, d, d, 1, 0, None) == BAD_ARG
        assert fn(ctx.h, 0, None, d, 1, 0, None) == BAD_ARG
        assert fn(ctx.h, 0, d, None, 1, 0, None) == BAD_ARG
        assert fn(ctx.h, F.N_OPS, d, d, 1, 0, None) == BAD_ARG
        assert fn(ctx.h, 0xFFFFFFFF, d, d, 1, 0, None) == BAD_ARG
        assert fn(ctx.h, 0, d, d, (1 << 20) + 1, 0, None) == BAD_ARG
        assert fn(ctx.h, 0, d, d, 1, 2, None) == BAD_ARG
    finally:
        ctx.free(d)
