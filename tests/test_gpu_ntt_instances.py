"""GPU parity of every unfused ntt_pass_kernel instance (csrc/ntt.hip): radices 2^2..2^9, each with no
column twiddle, Shoup pairs from t16, the last pass's full table, and the two-level lo * hi form.

The default plans launch only some of these; the rest are reached through the library's test hook
`stark_test_ntt_plan` with policy 3 (no fusion).  For each radix r:
  * (4, r) and (r, 4) at 2^(4 + r): r as a last pass on t16 and as a first pass, with partial tiles
    (the radix-2^9 first pass also takes the store's Ns < B path);
  * prefix + (r,) at 2^17, once on the shared context, where the last pass takes the cached full
    table, and once on a context whose cache cap is 0, where it takes the two-level form.
Forward and inverse are compared bit for bit with the oracle; the 2^17 plans share one expected output
per direction.

The same plans also transform structured inputs whose outputs are known in closed form (Python integers, no
oracle): the constant p - 1, a delta of p - 1 at 1 and at n - 1, and the pure tones (p - 1) w^(-m i) for
m = 1, n / 2 + 1, n - 1.  Every buffer sits between two guard runs of 0xFF that must come back untouched, and the
small pairs, two 2^17 plans per last-pass form and the two-point transform also run as batches (the kernel maps
a tile to its transform by tile >> log_tiles).  A tone's butterflies meet X' = T (mod p) at every stage, so the
passes' lazy values are exactly p, 2p and 3p and the last reduction takes exactly p: values random data never
produces.
"""
import ctypes
import functools

import numpy as np
import pytest

import oracle as O
import stark_amd as S
from ntt_pass_cases import Guarded

pytestmark = pytest.mark.gpu

OFF = 3  # the hook's fusion policy: none
RADICES = range(2, 10)
BATCH = 3
# 2^17 plans run as a batch of three, per column source: (8, 9)'s last pass takes the full table or, without the
# cache, the two-level form; the middle pass of (5, 5, 7) takes Shoup pairs from t16 (Ns R = 2^10 <= 2^16).
BATCH_PLANS_2_17 = [(8, 9), (5, 5, 7)]
PREFIX_2_17 = {2: (8, 7), 3: (7, 7), 4: (7, 6), 5: (6, 6), 6: (6, 5), 7: (5, 5), 8: (9,), 9: (8,)}


def _hook():
    fn = S.load_library().stark_test_ntt_plan
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                   ctypes.POINTER(ctypes.c_uint64), ctypes.c_int, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32,
                   ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
    fn.restype = ctypes.c_int
    return fn


def _limbs(x):
    return (ctypes.c_uint64 * 4)(*[(x >> (64 * k)) & (2**64 - 1) for k in range(4)])


def _plan_ntt(c, log_n, inverse, plan, x=None, batch=1):
    """`batch` transforms (x: batch * 2^log_n elements, default _input_batch) in place in a buffer between two
    guard runs of 0xFF, which must come back untouched."""
    assert sum(plan) == log_n
    if x is None:
        x = _input_batch(log_n, batch)
    assert len(x) == batch << log_n
    used = ctypes.c_uint32(0xFFFFFFFF)
    with Guarded(c, len(x), np.array(x)) as d:
        radices = (ctypes.c_uint32 * len(plan))(*plan)
        rc = _hook()(c.h, d.ptr, log_n, batch, _limbs(O.root_of_unity(log_n)), int(inverse), radices, len(plan), OFF,
                     None, ctypes.byref(used))
        assert rc == 0, rc
        out = d.get((plan, inverse, batch)).copy()
    assert used.value == 0
    return out


@functools.lru_cache(maxsize=None)
def _input(log_n, column=0):
    x = O.random_elements(1 << log_n, 0x1A57A9CE + log_n + 0x10000 * column)
    x.setflags(write=False)
    return x


def _input_batch(log_n, batch):
    """Column 0 is _input(log_n); the others are distinct."""
    return _input(log_n) if batch == 1 else np.concatenate([_input(log_n, b) for b in range(batch)])


@functools.lru_cache(maxsize=None)
def _want(log_n, inverse, column=0):
    """The oracle's transform of _input(log_n, column), computed once."""
    o = O.Oracle()
    f = o.inv_best_fft if inverse else o.best_fft
    out = f(np.array(_input(log_n, column)), O.root_of_unity(log_n), log_n, cpus=8)
    out.setflags(write=False)
    return out


def _want_batch(log_n, inverse, batch):
    return _want(log_n, inverse) if batch == 1 else np.concatenate([_want(log_n, inverse, b) for b in range(batch)])


STRUCTURED = ("const", "delta_1", "delta_last", "tone_1", "tone_half_1", "tone_last")


def _to_limbs(vals):
    a = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()
    a.setflags(write=False)
    return a


def _powers(c, g, n):
    """c g^k, k < n."""
    out = [c] * n
    for k in range(1, n):
        out[k] = out[k - 1] * g % O.P
    return out


@functools.lru_cache(maxsize=None)
def _structured(log_n, kind):
    """(input, forward transform, inverse transform) in closed form: out[k] = sum_j x[j] w^(j k) forward,
    n^-1 sum_j x[j] w^(-j k) inverse."""
    n, w, v = 1 << log_n, O.root_of_unity(log_n), O.P - 1
    n_inv = pow(n, -1, O.P)
    fwd, inv = [0] * n, [0] * n
    if kind == "const":
        x = [v] * n
        fwd[0], inv[0] = n * v % O.P, v
    elif kind.startswith("delta"):
        j = 1 if kind == "delta_1" else n - 1
        x = [0] * n
        x[j] = v
        fwd, inv = _powers(v, pow(w, j, O.P), n), _powers(v * n_inv % O.P, pow(w, -j, O.P), n)
    else:
        m = {"tone_1": 1, "tone_half_1": n // 2 + 1, "tone_last": n - 1}[kind]
        x = _powers(v, pow(w, -m, O.P), n)
        fwd[m], inv[n - m] = n * v % O.P, v
    return _to_limbs(x), _to_limbs(fwd), _to_limbs(inv)


def _check_structured(c, log_n, plan):
    for kind in STRUCTURED:
        x, fwd, inv = _structured(log_n, kind)
        for inverse, want in ((False, fwd), (True, inv)):
            got = _plan_ntt(c, log_n, inverse, plan, x)
            assert np.array_equal(got, want), (plan, kind, inverse, np.flatnonzero((got != want).any(axis=1))[:8])


@pytest.fixture(scope="module")
def ctx_nocache():
    c = S.Context(0)
    c.set_cache_limit(0)
    yield c
    c.close()


@pytest.mark.parametrize("first", [False, True], ids=["last", "first"])
@pytest.mark.parametrize("r", RADICES)
def test_small_pair(ctx, r, first):
    log_n = 4 + r
    plan = (r, 4) if first else (4, r)
    for inverse in (False, True):
        got = _plan_ntt(ctx, log_n, inverse, plan)
        assert np.array_equal(got, _want(log_n, inverse)), (plan, inverse)
        got = _plan_ntt(ctx, log_n, inverse, plan, batch=BATCH)  # (tile >> log_tiles selects the transform)
        assert np.array_equal(got, _want_batch(log_n, inverse, BATCH)), (plan, inverse, BATCH)


@pytest.mark.parametrize("first", [False, True], ids=["last", "first"])
@pytest.mark.parametrize("r", RADICES)
def test_small_pair_structured(ctx, r, first):
    _check_structured(ctx, 4 + r, (r, 4) if first else (4, r))


@pytest.mark.parametrize("r", RADICES)
def test_2_17_full_table_structured(ctx, r):
    _check_structured(ctx, 17, PREFIX_2_17[r] + (r,))


@pytest.mark.parametrize("r", RADICES)
def test_2_17_two_level_structured(ctx_nocache, r):
    _check_structured(ctx_nocache, 17, PREFIX_2_17[r] + (r,))
    assert ctx_nocache.memory()["cached"] == 0


@pytest.mark.parametrize("r", RADICES)
def test_2_17_full_table(ctx, r):
    plan = PREFIX_2_17[r] + (r,)
    for inverse in (False, True):
        got = _plan_ntt(ctx, 17, inverse, plan)
        assert np.array_equal(got, _want(17, inverse)), (plan, inverse)
    assert ctx.memory()["cached"] >= 2 * (32 << 17)  # (both directions' last passes read a cached table)


@pytest.mark.parametrize("r", RADICES)
def test_2_17_two_level(ctx_nocache, r):
    plan = PREFIX_2_17[r] + (r,)
    for inverse in (False, True):
        got = _plan_ntt(ctx_nocache, 17, inverse, plan)
        assert np.array_equal(got, _want(17, inverse)), (plan, inverse)
    assert ctx_nocache.memory()["cached"] == 0


@pytest.mark.parametrize("plan", BATCH_PLANS_2_17, ids=lambda p: "x".join(map(str, p)))
def test_2_17_batch_full_table(ctx, plan):
    for inverse in (False, True):
        got = _plan_ntt(ctx, 17, inverse, plan, batch=BATCH)
        assert np.array_equal(got, _want_batch(17, inverse, BATCH)), (plan, inverse)
    assert ctx.memory()["cached"] >= 2 * (32 << 17)


@pytest.mark.parametrize("plan", BATCH_PLANS_2_17, ids=lambda p: "x".join(map(str, p)))
def test_2_17_batch_two_level(ctx_nocache, plan):
    for inverse in (False, True):
        got = _plan_ntt(ctx_nocache, 17, inverse, plan, batch=BATCH)
        assert np.array_equal(got, _want_batch(17, inverse, BATCH)), (plan, inverse)
    assert ctx_nocache.memory()["cached"] == 0


def test_ntt_dev_two_points_batch(ctx, oracle):
    """stark_ntt_dev at log_n = 1 (ntt2_kernel, one workgroup per transform): a batch of five, both directions."""
    batch, w = 5, O.root_of_unity(1)
    x = np.array(_input(4)[:2 * batch])
    x[2], x[3] = O.to_limbs([O.P - 1, O.P - 1])   # (a + b wraps; a - b is zero)
    x[5] = x[4]
    for inverse in (False, True):
        f = oracle.inv_best_fft if inverse else oracle.best_fft
        want = np.concatenate([f(x[2 * b:2 * b + 2], w, 1) for b in range(batch)])
        with Guarded(ctx, 2 * batch, x) as d:
            ctx.ntt_dev(d.ptr, 1, batch, w, inverse=inverse)
            got = d.get(("ntt2", inverse)).copy()
        assert np.array_equal(got, want), (inverse, np.flatnonzero((got != want).any(axis=1)))
