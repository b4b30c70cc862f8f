"""Interpolation plans (stark_interp_plan_*, Context.interp_plan) and lagrange_interp_batch: lagrange_interp
(poly_utils.rs:409-439) of many value vectors over one point set, against an exact-integer Lagrange
interpolation and against the single call.  The field arithmetic is exact: every comparison is for equality."""
import ctypes
import random

import numpy as np
import pytest

import oracle as O
from stark_amd import StarkError

pytestmark = pytest.mark.gpu

P = O.P


def py_interp(xs, ys):
    """The coefficients, low degree first, of sum_i ys[i] / den_i * Z / (X - xs[i]) with 1 / 0 = 0
    (poly_utils.rs:409-439), in O(n^2) on Python integers."""
    n = len(xs)
    z = [1]
    for x in xs:
        z = [((z[j - 1] if j else 0) - (z[j] * x if j < len(z) else 0)) % P for j in range(len(z) + 1)]
    out = [0] * n
    for x, y in zip(xs, ys):
        q, carry = [0] * n, z[n]
        for d in range(n, 0, -1):  # Z / (X - x) by synthetic division
            q[d - 1] = carry
            carry = (z[d - 1] + carry * x) % P
        den = 0
        for c in reversed(q):
            den = (den * x + c) % P
        if den == 0 or y == 0:
            continue
        s = y * pow(den, -1, P) % P
        for j in range(n):
            out[j] = (out[j] + q[j] * s) % P
    return out


def points(n, seed):
    rng = random.Random(seed)
    xs = []
    while len(xs) < n:
        x = rng.randrange(P)
        if x not in xs:
            xs.append(x)
    if n >= 3:
        xs[n // 2] = 0
    return xs


def values(batch, n, seed):
    rng = random.Random(seed)
    ys = [[rng.randrange(P) for _ in range(n)] for _ in range(batch)]
    if n >= 2:
        ys[0][1] = 0
        ys[-1][n - 1] = P - 1
    return ys


def limbs3(ys):
    return np.stack([O.to_limbs(y) for y in ys]) if len(ys[0]) else np.zeros((len(ys), 0, 4), dtype=np.uint64)


def ints(arr):
    return [O.from_limbs(a) for a in arr]


# 32 | 33: the leaf launch alone against one NTT level; 64 | 65: the next pad; 200: three levels
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 65, 200])
def test_plan_matches_exact_interpolation(ctx, n, batch):
    xs, ys = points(n, 7 * n), values(batch, n, 11 * n + batch)
    want = [py_interp(xs, y) for y in ys]
    plan = ctx.interp_plan(O.to_limbs(xs))
    try:
        got = plan.apply(limbs3(ys))
        assert got.shape == (batch, n, 4)
        assert ints(got) == want
    finally:
        plan.close()
    assert ints(ctx.lagrange_interp_batch(O.to_limbs(xs), limbs3(ys))) == want


def test_bits_size_matches_single_calls(ctx):
    """1,062 points (the `bits` circuit's count): six NTT levels, two vectors, against lagrange_interp per vector."""
    n = 1062
    xs, ys = O.to_limbs(points(n, 5)), limbs3(values(2, n, 6))
    want = np.stack([ctx.lagrange_interp(xs, y) for y in ys])
    assert np.array_equal(ctx.lagrange_interp_batch(xs, ys), want)


@pytest.mark.parametrize("log_order", [11, 7])
def test_domain_plan_equals_arbitrary_points(ctx, log_order):
    """xs[i] = root^exps[i].  With 200 points and log_order 7 the exponents repeat and Z' does not fit the domain:
    the hint is dropped, as in the single call, and the repeated points drop out."""
    n = 200
    root = O.root_of_unity(log_order)
    rng = random.Random(log_order)
    exps = rng.sample(range(1 << log_order), n) if n <= 1 << log_order else \
        [rng.randrange(1 << log_order) for _ in range(n)]
    xs = [pow(root, e, P) for e in exps]
    ys = limbs3(values(3, n, 21))
    a = ctx.interp_plan(exps, root, log_order)
    b = ctx.interp_plan(O.to_limbs(xs))
    try:
        got = a.apply(ys)
        assert np.array_equal(got, b.apply(ys))
        assert np.array_equal(got[1], ctx.lagrange_interp(exps, ys[1], root, log_order))
    finally:
        a.close()
        b.close()
    assert np.array_equal(ctx.lagrange_interp_batch(exps, ys, root, log_order), got)


def test_repeated_point_drops_out(ctx):
    n = 40
    xs = points(n, 3)
    xs[23] = xs[7]
    ys = limbs3(values(2, n, 4))
    got = ctx.lagrange_interp_batch(O.to_limbs(xs), ys)
    for b in range(2):
        assert np.array_equal(got[b], ctx.lagrange_interp(O.to_limbs(xs), ys[b]))
    assert ints(got) == [py_interp(xs, y) for y in ints(ys)]


def test_plan_survives_other_calls(ctx):
    """The plan owns its memory: zpoly and eval_poly_multipoint overwrite the context's tree arena between two
    applications."""
    n = 200
    xs = points(n, 31)
    y0, y1 = values(2, n, 32), values(3, n, 33)
    plan = ctx.interp_plan(O.to_limbs(xs))
    try:
        first = plan.apply(limbs3(y0))
        assert ints(first) == [py_interp(xs, y) for y in y0]
        other = O.to_limbs(points(700, 34))
        ctx.zpoly(other)
        ctx.eval_poly_multipoint(other, other[:300])
        assert ints(plan.apply(limbs3(y1))) == [py_interp(xs, y) for y in y1]
        assert plan.apply(limbs3(y0)).tobytes() == first.tobytes()
    finally:
        plan.close()


def test_apply_dev_on_a_torch_stream(ctx):
    import torch
    from stark_amd import torch_stream
    n, batch = 65, 3
    xs, ys = points(n, 41), limbs3(values(batch, n, 42))
    plan = ctx.interp_plan(O.to_limbs(xs))
    try:
        want = plan.apply(ys)
        d_ys = torch.from_numpy(ys.view(np.uint8).reshape(-1).copy()).cuda()
        d_out = torch.zeros_like(d_ys)
        host = torch.empty(d_ys.numel(), dtype=torch.uint8).pin_memory()
        torch.cuda.synchronize()
        with torch.cuda.stream(torch.cuda.Stream()):  # the copy back behind it, no host synchronisation between
            plan.apply_dev(d_ys.data_ptr(), batch, d_out.data_ptr(), torch_stream())
            host.copy_(d_out, non_blocking=True)
        torch.cuda.synchronize()
        assert np.array_equal(host.numpy().view(np.uint64).reshape(batch, n, 4), want)
    finally:
        plan.close()


def test_chunks_of_one_give_the_same_output(ctx):
    n, batch = 65, 3
    xs, ys = points(n, 51), limbs3(values(batch, n, 52))
    plan = ctx.interp_plan(O.to_limbs(xs))
    try:
        want = plan.apply(ys)
        try:
            ctx.set_prove_batch_limit(1)
            got = plan.apply(ys)
        finally:
            ctx.set_prove_batch_limit(0)
        assert np.array_equal(got, want)
        assert ints(want) == [py_interp(xs, y) for y in ints(ys)]
    finally:
        plan.close()


def test_empty_batch_and_empty_plan_touch_nothing(ctx):
    lib = ctx.lib
    u64p = ctypes.POINTER(ctypes.c_uint64)
    out = np.full((2, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    keep = out.copy()
    xs, ys = O.to_limbs(points(2, 61)), limbs3(values(1, 2, 62))
    p64 = lambda a: a.ctypes.data_as(u64p)
    assert lib.stark_lagrange_interp_batch(ctx.h, p64(xs), p64(ys), 2, 0, p64(out)) == 0
    assert lib.stark_lagrange_interp_batch(ctx.h, p64(xs), p64(ys), 0, 1, p64(out)) == 0
    plan = ctx.interp_plan(xs)
    empty = ctx.interp_plan(np.zeros((0, 4), dtype=np.uint64))
    try:
        assert lib.stark_interp_plan_apply(plan.h, p64(ys), 0, p64(out)) == 0
        assert lib.stark_interp_plan_apply(empty.h, p64(ys), 1, p64(out)) == 0
        assert empty.apply(np.zeros((3, 0, 4), dtype=np.uint64)).shape == (3, 0, 4)
    finally:
        plan.close()
        empty.close()
    assert np.array_equal(out, keep)


def test_bad_exponent_is_bad_arg(ctx):
    root = O.root_of_unity(5)
    with pytest.raises(StarkError) as e:
        ctx.interp_plan([0, 3, 32], root, 5)
    assert e.value.code == 3


def test_plan_freed_after_its_context():
    """Closing the context releases a live plan's device memory; the plan's close() then frees the handle alone."""
    import stark_amd as S
    c = S.Context(0)
    xs = O.to_limbs(points(65, 81))
    plan = c.interp_plan(xs)
    want = plan.apply(xs.reshape(1, 65, 4))
    c.close()
    plan.close()
    assert plan.h is None
    c = S.Context(0)
    try:
        assert np.array_equal(c.lagrange_interp_batch(xs, xs.reshape(1, 65, 4)), want)
    finally:
        c.close()


def test_close_gives_the_memory_back():
    import stark_amd as S
    c = S.Context(0)
    try:
        xs = O.to_limbs(points(200, 71))
        c.lagrange_interp(xs, xs)  # the context's own buffers at their size for these points
        warm = c.interp_plan(xs)
        warm.apply(xs.reshape(1, 200, 4))
        warm.close()
        before = c.memory()["resident"]
        plan = c.interp_plan(xs)
        held = c.memory()["resident"] - before
        assert held == 32 * (200 + 200 + 2 * 256 * 3)  # the points, 1 / Z', three levels of 2 N transform points
        plan.apply(xs.reshape(1, 200, 4))
        plan.close()
        assert c.memory()["resident"] == before
    finally:
        c.close()
