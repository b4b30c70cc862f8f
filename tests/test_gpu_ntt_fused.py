"""GPU parity of the fused column twiddles (csrc/ntt.hip, ntt_pass_kernel FUSE): a radix-2^8 pass that
also applies the next pass's column twiddle (staged: merged Shoup pairs gathered from t16; streamed: a
per-element table in place of the last pass's full table), plus the wave-uniform residual product.

The default plans fuse only where it measured faster (2^24, covered in full by tests/test_gpu_large.py);
the small shapes here reach the fused kernels through the library's test hook `stark_test_ntt_plan`,
which runs a caller-given pass plan under a fusion policy and reports the mode each pass ran in:
  * (2, 8, 8) at 2^18 and (4, 8, 8) at 2^20: streamed, producer with its own t16 column twiddle,
    c != 0, r' != 0, Ns = 4 = B at 2^18, the scaled table in the inverse;
  * (8, 8, 2) at 2^18 and (8, 4, 8) at 2^20: staged, consumer radix 2^8 and 2^4.
2^16 = (8, 8) cannot fuse: it has one column per r', so a 4-column tile spans four r' and the residual
constant is not wave-uniform.  Its cases below run the unfused passes (the hook reports mode 0) and pin
that the policies leave such a size alone.
"""
import ctypes
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import oracle as O
import stark_amd as S

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BIG = json.load(open(os.path.join(HERE, "golden", "large_digests.json")))

AUTO, ALL, STREAMED, OFF = 0, 1, 2, 3  # the hook's fusion policies
STAGED_P0 = 1       # `used`: pass 0 staged
STREAMED_P1 = 2 << 2  # `used`: pass 1 streamed


def _hook():
    fn = S.load_library().stark_test_ntt_plan
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                   ctypes.POINTER(ctypes.c_uint64), ctypes.c_int, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32,
                   ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
    fn.restype = ctypes.c_int
    return fn


def _limbs(x):
    return (ctypes.c_uint64 * 4)(*[(x >> (64 * k)) & (2**64 - 1) for k in range(4)])


def _plan_ntt(c, x, log_n, w, inverse, plan, policy, batch=1):
    """(output, used) of the hook on `batch` transforms of x."""
    used = ctypes.c_uint32(0xFFFFFFFF)
    d = c.alloc(x.nbytes)
    try:
        c.h2d(d, x)
        radices = (ctypes.c_uint32 * len(plan))(*plan)
        rc = _hook()(c.h, d, log_n, batch, _limbs(w), int(inverse), radices, len(plan), policy, None,
                     ctypes.byref(used))
        assert rc == 0, rc
        out = np.empty_like(x)
        c.d2h(out, d)
    finally:
        c.free(d)
    return out, used.value


def _dev_ntt(c, x, log_n, w, inverse, batch=1):
    d = c.alloc(x.nbytes)
    try:
        c.h2d(d, x)
        c.ntt_dev(d, log_n, batch, w, inverse=inverse)
        out = np.empty_like(x)
        c.d2h(out, d)
    finally:
        c.free(d)
    return out


@functools.lru_cache(maxsize=None)
def _input(log_n, kind):
    n = 1 << log_n
    if kind == "random":
        x = O.random_elements(n, 0x5EED0000 + log_n)
    elif kind == "random3":
        x = O.random_elements(3 * n, 0xF05ED000 + log_n)
    else:
        x = np.zeros((n, 4), dtype=np.uint64)
        if kind == "max":
            x[:] = O.to_limbs([O.P - 1])[0]
        elif kind == "alt":
            x[0::2] = O.to_limbs([O.P - 1])[0]
            x[1::2] = O.to_limbs([1])[0]
        else:
            assert kind == "zero"
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _want(log_n, kind, inverse, root_pow=1):
    """The oracle's transform of _input(log_n, kind), computed once (per transform for a batch)."""
    o = O.Oracle()
    w = pow(O.root_of_unity(log_n), root_pow, O.P)
    x = _input(log_n, kind)
    n = 1 << log_n
    f = o.inv_best_fft if inverse else o.best_fft
    out = np.concatenate([f(np.array(x[i:i + n]), w, log_n, cpus=8) for i in range(0, len(x), n)])
    out.setflags(write=False)
    return out


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.uint64).tobytes()).hexdigest()


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("batch", [1, 3])
def test_default_plan_2_16(ctx, inverse, batch):
    kind = "random" if batch == 1 else "random3"
    got = _dev_ntt(ctx, np.array(_input(16, kind)), 16, O.root_of_unity(16), inverse, batch)
    assert np.array_equal(got, _want(16, kind, inverse))


@pytest.mark.parametrize("inverse", [False, True])
def test_streamed_2_18(ctx, inverse):
    got, used = _plan_ntt(ctx, np.array(_input(18, "random")), 18, O.root_of_unity(18), inverse, (2, 8, 8), STREAMED)
    assert used == STREAMED_P1
    assert np.array_equal(got, _want(18, "random", inverse))


def test_streamed_2_18_batch(ctx):
    """batch > 1: the tile's r' and table offset come from the tile index within its transform."""
    got, used = _plan_ntt(ctx, np.array(_input(18, "random3")), 18, O.root_of_unity(18), False, (2, 8, 8), ALL, batch=3)
    assert used == STREAMED_P1
    assert np.array_equal(got, _want(18, "random3", False))


@pytest.mark.parametrize("plan,policy,want_used", [((4, 8, 8), STREAMED, STREAMED_P1), ((8, 4, 8), ALL, STAGED_P0)])
def test_fused_2_20_digests(ctx, plan, policy, want_used):
    rec = BIG["ntt_2^20"]
    x = np.array(_input(20, "random"))
    assert _sha(x) == rec["input_sha256"]
    w = O.root_of_unity(20)
    fwd, used = _plan_ntt(ctx, x, 20, w, False, plan, policy)
    assert used == want_used
    assert _sha(fwd) == rec["forward_sha256"]
    inv, used = _plan_ntt(ctx, x, 20, w, True, plan, policy)
    assert used == want_used
    assert _sha(inv) == rec["inverse_sha256"]


@pytest.mark.parametrize("inverse", [False, True])
def test_staged_2_18(ctx, inverse):
    """(8, 8, 2): a staged boundary with a radix-2^8 consumer (N' = 2^16, the 4096-entry residual table)."""
    got, used = _plan_ntt(ctx, np.array(_input(18, "random")), 18, O.root_of_unity(18), inverse, (8, 8, 2), ALL)
    assert used == STAGED_P0
    assert np.array_equal(got, _want(18, "random", inverse))


@pytest.mark.parametrize("policy", [ALL, STREAMED])
def test_forced_2_16_stays_unfused(ctx, policy):
    got, used = _plan_ntt(ctx, np.array(_input(16, "random")), 16, O.root_of_unity(16), False, (8, 8), policy)
    assert used == 0
    assert np.array_equal(got, _want(16, "random", False))


def test_unfused_fallback_under_cache_cap(ctx):
    """A context whose cache cap is below the streamed table runs the whole transform unfused, same output."""
    x = np.array(_input(18, "random"))
    w = O.root_of_unity(18)
    c = S.Context(0)
    try:
        c.set_cache_limit((32 << 18) - 1)
        for inverse in (False, True):
            got, used = _plan_ntt(c, x, 18, w, inverse, (2, 8, 8), STREAMED)
            assert used == 0
            assert c.memory()["cached"] == 0
            fused, used = _plan_ntt(ctx, x, 18, w, inverse, (2, 8, 8), STREAMED)
            assert used == STREAMED_P1
            assert np.array_equal(got, fused)
            assert np.array_equal(got, _want(18, "random", inverse))
    finally:
        c.close()


def test_table_kinds_share_one_slot():
    """The streamed table takes the full table's slot: alternating plans on one context rebuild it,
    never hold both, and every output stays right."""
    x = np.array(_input(20, "random"))
    w = O.root_of_unity(20)
    rec = BIG["ntt_2^20"]
    c = S.Context(0)
    try:
        for plan, policy in [((4, 8, 8), STREAMED), ((8, 4, 8), OFF), ((4, 8, 8), STREAMED)]:
            fwd, _ = _plan_ntt(c, x, 20, w, False, plan, policy)
            assert _sha(fwd) == rec["forward_sha256"], (plan, policy)
            assert c.memory()["cached"] == 32 << 20
    finally:
        c.close()


@pytest.mark.parametrize("kind", ["max", "zero", "alt"])
def test_range_edges(ctx, kind):
    for inverse in (False, True):
        got = _dev_ntt(ctx, np.array(_input(16, kind)), 16, O.root_of_unity(16), inverse)
        assert np.array_equal(got, _want(16, kind, inverse)), inverse
        for plan, policy, want_used in [((2, 8, 8), STREAMED, STREAMED_P1), ((8, 8, 2), ALL, STAGED_P0)]:
            got, used = _plan_ntt(ctx, np.array(_input(18, kind)), 18, O.root_of_unity(18), inverse, plan, policy)
            assert used == want_used
            assert np.array_equal(got, _want(18, kind, inverse)), (plan, inverse)


def test_other_root(ctx):
    w16 = pow(O.root_of_unity(16), 3, O.P)
    assert np.array_equal(_dev_ntt(ctx, np.array(_input(16, "random")), 16, w16, False), _want(16, "random", False, 3))
    w18 = pow(O.root_of_unity(18), 3, O.P)
    for plan, policy, want_used in [((2, 8, 8), STREAMED, STREAMED_P1), ((8, 8, 2), ALL, STAGED_P0)]:
        got, used = _plan_ntt(ctx, np.array(_input(18, "random")), 18, w18, False, plan, policy)
        assert used == want_used
        assert np.array_equal(got, _want(18, "random", False, 3)), plan
