"""GPU parity of the first passes stark_test_ntt_plan cannot reach (its source is the output buffer itself):

  * the sparse first passes of ntt_pass_kernel (csrc/ntt.hip): all eight kColSparse instances at every copy-stage
    count, and the dense instances on a compact zero-padded source, through stark_test_ntt_plan_from -- every case
    of tests/ntt_pass_cases.py, forward and inverse, one transform and a batch of three, on three inputs;
  * the T-major first pass of the cold verifier (ntt_first_pass_tmajor) through stark_test_ntt_first_pass_tmajor,
    against its definition (ntt_pass_cases.tmajor_want, held to the oracle's transform on the CPU tier).

Everything is compared bit for bit.  Source and output sit between guard runs of 64 elements of 0xFF: a row read
from memory where the kernel should take an implicit zero changes the output, and a stray store shows in a guard.
"""
import ctypes

import numpy as np
import pytest

import ntt_pass_cases as N
import oracle as O
import stark_amd as S

pytestmark = pytest.mark.gpu

OFF = 3        # fusion policy: none
BAD_ROOT, BAD_ARG = 2, 3    # stark_status


def _from_hook():
    fn = S.load_library().stark_test_ntt_plan_from
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                   ctypes.POINTER(ctypes.c_uint64), ctypes.c_int, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32,
                   ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
    fn.restype = ctypes.c_int
    return fn


def _tmajor_hook():
    fn = S.load_library().stark_test_ntt_first_pass_tmajor
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                   ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
    fn.restype = ctypes.c_int
    return fn


def _rows(got, want):
    return np.flatnonzero((got != want).any(axis=1))[:8]


def _plan_from(c, src, zero_log, dst, log_n, batch, inverse, plan, policy=OFF):
    radices = (ctypes.c_uint32 * len(plan))(*plan)
    used = ctypes.c_uint32(0xFFFFFFFF)
    rc = _from_hook()(c.h, src, zero_log, dst, log_n, batch, N.limbs_arg(O.root_of_unity(log_n)), int(inverse), radices,
                      len(plan), policy, None, ctypes.byref(used))
    return rc, used.value


@pytest.mark.parametrize("case", N.sparse_cases(), ids=N.case_id)
def test_sparse_first_pass(ctx, oracle, case):
    plan, z = case
    log_n = sum(plan)
    n, m = 1 << log_n, 1 << (log_n - z)
    for kind in N.INPUTS:
        x = N.sparse_input(log_n, z, kind)
        for inverse in (False, True):
            want = N.sparse_want(oracle, log_n, z, kind, inverse)
            for batch in (1, N.BATCH):
                what = (plan, z, kind, "inverse" if inverse else "forward", batch)
                xs = np.array(x[:batch * m])
                with N.Guarded(ctx, batch * m, xs) as src, N.Guarded(ctx, batch * n) as dst:
                    rc, used = _plan_from(ctx, src.ptr, z, dst.ptr, log_n, batch, inverse, plan)
                    assert rc == 0, (what, rc)
                    assert used == 0, (what, used)
                    got = dst.get(f"{what} output")
                    assert np.array_equal(src.get(f"{what} source"), xs), (what, "the source changed")
                bad = _rows(got, want[:batch * n])
                assert bad.size == 0, (what, "first differing elements", bad)


@pytest.mark.parametrize("log_n,zero_log", N.tmajor_cases())
def test_tmajor_first_pass(ctx, oracle, log_n, zero_log):
    n, m = 1 << log_n, 1 << (log_n - zero_log)
    first = S.ntt_plan(log_n)[0]
    assert first == N.TMAJOR_FIRST[log_n]
    x = N.tmajor_input(log_n, zero_log)
    want = np.concatenate([N.tmajor_want(oracle, np.array(x[b * m:(b + 1) * m]), log_n, first)
                           for b in range(N.TMAJOR_BATCH)])
    for batch in (1, N.TMAJOR_BATCH):
        xs = np.array(x[:batch * m])
        log_t = ctypes.c_uint32(0xFFFFFFFF)
        with N.Guarded(ctx, batch * m, xs) as src, N.Guarded(ctx, batch * n) as dst:
            rc = _tmajor_hook()(ctx.h, src.ptr, zero_log, dst.ptr, log_n, batch, N.limbs_arg(O.root_of_unity(log_n)),
                                None, ctypes.byref(log_t))
            assert rc == 0, (batch, rc)
            got = dst.get(f"batch {batch} output")
            assert np.array_equal(src.get(f"batch {batch} source"), xs), "the source changed"
        assert log_t.value == first
        bad = _rows(got, want[:batch * n])
        assert bad.size == 0, (batch, "first differing elements (t A + j)", bad)


def test_refused_arguments(ctx):
    """What the hooks validate returns its status before any launch: source and output keep their 0xFF."""
    log_n, z, plan = 8, 2, (4, 4)
    n, m = 1 << log_n, 1 << (log_n - z)
    w = N.limbs_arg(O.root_of_unity(log_n))
    ff = np.uint64(0xFFFFFFFFFFFFFFFF)
    with N.Guarded(ctx, m) as src, N.Guarded(ctx, n) as dst:
        def refused_from(src_p, zz, dst_p, ln, batch, pl, policy=OFF):
            rc, _ = _plan_from(ctx, src_p, zz, dst_p, ln, batch, False, pl, policy)
            assert rc == BAD_ARG, (zz, ln, batch, pl, policy, rc)
        refused_from(src.ptr, 0, dst.ptr, log_n, 1, plan)            # zero_log 0
        refused_from(src.ptr, log_n + 1, dst.ptr, log_n, 1, plan)    # zero_log above log_n
        refused_from(dst.ptr, z, dst.ptr, log_n, 1, plan)            # in place
        refused_from(None, z, dst.ptr, log_n, 1, plan)
        refused_from(src.ptr, z, None, log_n, 1, plan)
        refused_from(src.ptr, z, dst.ptr, log_n, 0, plan)            # no transform
        refused_from(src.ptr, z, dst.ptr, log_n, 1, (4, 3))          # radices do not sum to log_n
        refused_from(src.ptr, z, dst.ptr, log_n, 1, (7, 1))          # radix 2^1
        refused_from(src.ptr, z, dst.ptr, 10, 1, (10,))              # radix 2^10
        refused_from(src.ptr, z, dst.ptr, log_n, 1, plan, policy=4)
        refused_from(src.ptr, z, dst.ptr, log_n, (1 << 26) + 1, plan)  # batch << log_n above 2^34
        refused_from(src.ptr, 6, dst.ptr, log_n, (1 << 26) + 1, plan)  # the same on the pad path
        log_t = ctypes.c_uint32(0)

        def refused_tmajor(src_p, zz, dst_p, ln, batch, root=w, status=BAD_ARG):
            rc = _tmajor_hook()(ctx.h, src_p, zz, dst_p, ln, batch, root, None, ctypes.byref(log_t))
            assert rc == status, (zz, ln, batch, rc)
        refused_tmajor(src.ptr, 0, dst.ptr, log_n, 1)                # zero_log 0
        refused_tmajor(src.ptr, 9, dst.ptr, log_n, 1)                # zero_log above the first radix (2^8)
        refused_tmajor(dst.ptr, z, dst.ptr, log_n, 1)
        refused_tmajor(None, z, dst.ptr, log_n, 1)
        refused_tmajor(src.ptr, z, dst.ptr, log_n, 0)
        refused_tmajor(src.ptr, z, dst.ptr, 1, 1)
        refused_tmajor(src.ptr, z, dst.ptr, log_n, (1 << 26) + 1)
        refused_tmajor(src.ptr, z, dst.ptr, log_n, 1, root=N.limbs_arg(O.root_of_unity(log_n - 1)),
                       status=BAD_ROOT)                                  # a root of order 2^7
        assert (src.get("source") == ff).all() and (dst.get("output") == ff).all()
