"""Evaluation plans (stark_eval_plan_*, Context.eval_plan) and eval_poly_multipoint_batch: eval_poly_at
(poly_utils.rs:93-102) of many polynomials at one point set, against the oracle's C Horner per polynomial and the
library's untouched one-thread-per-point kernel (eval_poly_at_multi), which must agree with each other and with the
plan bit for bit.  The field arithmetic is exact: every comparison is for equality."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import oracle as O
from stark_amd import Context, StarkError, torch_stream
from test_gpu_poly import limbs, points, values

pytestmark = pytest.mark.gpu

P = O.P
SENTINEL = 0xA5A5A5A5A5A5A5A5
U64P = ctypes.POINTER(ctypes.c_uint64)
# n: 1, 2, 31, 32 the leaf launch alone; 33 the first NTT level; 65 and 129 the first and second wrapped levels
# (Adj changes); 257, 600 several levels with padding
PLAN_N = [1, 2, 31, 32, 33, 64, 65, 128, 129, 257, 600]


def padded(n):
    N = 32
    while N < n:
        N *= 2
    return N


def plan_elems(n, max_deg_plus_1):
    """Elements of device memory a plan holds (include/stark_hip.h): the points, the leaf level, 2 N per NTT level,
    alpha and its transform (3 K)."""
    N, K = padded(n), padded(max_deg_plus_1)
    return n + N + 2 * N * (N.bit_length() - 6) + 3 * K


def scratch_elems(n, deg_plus_1):
    """Scratch elements of one polynomial of an application (include/stark_hip.h): 3 K' + 3 N."""
    return 3 * padded(deg_plus_1) + 3 * padded(n)


def degs_for(n):
    N = padded(n)
    return sorted({d for d in (1, n - 1, n, n + 1, N, N + 1, 3 * N + 7) if d > 0})


@functools.lru_cache(maxsize=None)
def xs_for(n):
    """x = 0 in the middle and xs[1] repeated at the end (n >= 3)."""
    return limbs(points(n, 5000 + n, True))


@functools.lru_cache(maxsize=None)
def polys_for(batch, d):
    p = O.random_elements(batch * d, 6000 + 131 * batch + d) if d else np.empty((0, 4), dtype=np.uint64)
    return np.ascontiguousarray(p).reshape(batch, d, 4)


def expected(ctx, oracle, polys, xs):
    """Per polynomial: the oracle's Horner and the library's one-thread-per-point kernel, which must agree."""
    rows = []
    for p in polys:
        want = oracle.eval_poly_multi(p, xs)
        assert np.array_equal(want, ctx.eval_poly_at_multi(p, xs))
        rows.append(want)
    return np.stack(rows)


def dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def host(t: torch.Tensor, *shape) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64).reshape(*shape, 4)


def p64(a):
    return a.ctypes.data_as(U64P)


@pytest.fixture
def batch_limit(ctx):
    yield ctx.set_prove_batch_limit
    ctx.set_prove_batch_limit(0)


@pytest.fixture
def tree_min(ctx):
    yield ctx.set_multipoint_tree_min
    ctx.set_multipoint_tree_min(0)


@pytest.mark.parametrize("n", PLAN_N)
def test_one_plan_every_degree(ctx, oracle, n):
    """One plan with the bound 3 N + 7 for every degree class: all but the last use a prefix of alpha."""
    xs, N = xs_for(n), padded(n)
    with ctx.eval_plan(xs, 3 * N + 7) as plan:
        for d in degs_for(n):
            polys = polys_for(3, d)
            got = plan.apply(polys)
            assert got.shape == (3, n, 4), d
            assert np.array_equal(got, expected(ctx, oracle, polys, xs)), d
            if n >= 3:
                assert np.array_equal(got[:, n - 1], got[:, 1]), d  # the repeated x
                assert np.array_equal(got[:, n // 2], polys[:, 0]), d  # x = 0: the constant term
        with pytest.raises(StarkError) as e:
            plan.apply(polys_for(1, 3 * N + 8))
        assert e.value.code == 1


@pytest.mark.parametrize("n", PLAN_N)
def test_degree_equal_to_the_bound(ctx, oracle, n):
    """max_deg_plus_1 == deg_plus_1: the plan's own transform of alpha is taken as it is."""
    xs, d = xs_for(n), n + 1
    polys = polys_for(3, d)
    with ctx.eval_plan(xs, d) as plan:
        assert np.array_equal(plan.apply(polys), expected(ctx, oracle, polys, xs))


def test_long_polynomials_few_points(ctx, oracle):
    """K >> N: 80 points against 2^16 + 3 coefficients."""
    xs, polys = xs_for(80), polys_for(3, (1 << 16) + 3)
    with ctx.eval_plan(xs, (1 << 16) + 3) as plan:
        assert np.array_equal(plan.apply(polys), expected(ctx, oracle, polys, xs))


def test_many_points_short_polynomials(ctx, oracle):
    """N >> K: 70,000 random points (eleven NTT levels, padding) against 40 coefficients."""
    xs, polys = O.random_elements(70000, 5070), polys_for(2, 40)
    with ctx.eval_plan(xs, 40) as plan:
        assert np.array_equal(plan.apply(polys), expected(ctx, oracle, polys, xs))


def test_rows_are_independent(ctx, oracle):
    """An all-zero polynomial, one with zero leading coefficients, the constant 1 and a random one: each row is
    its polynomial's alone, whatever its neighbours."""
    n, d = 65, 70
    xs = xs_for(n)
    polys = polys_for(4, d).copy()
    polys[0] = 0
    polys[1, d - 9:] = 0
    polys[2] = 0
    polys[2, 0, 0] = 1
    order = [3, 1, 0, 2]
    with ctx.eval_plan(xs, 3 * 128 + 7) as plan:
        got = plan.apply(polys)
        assert np.array_equal(got, expected(ctx, oracle, polys, xs))
        assert not got[0].any()
        assert O.from_limbs(got[2]) == [1] * n
        assert np.array_equal(plan.apply(polys[order]), got[order])


def test_degenerate_sizes(ctx):
    n = 33
    xs = xs_for(n)
    out = np.full((2, n, 4), SENTINEL, dtype=np.uint64)
    keep = out.copy()
    polys = polys_for(2, 5)
    with ctx.eval_plan(xs, 40) as plan, ctx.eval_plan(np.empty((0, 4), dtype=np.uint64), 40) as empty:
        zeros = plan.apply(np.empty((2, 0, 4), dtype=np.uint64))  # deg_plus_1 = 0
        assert zeros.shape == (2, n, 4) and not zeros.any()
        assert ctx.lib.stark_eval_plan_apply(plan.h, p64(polys), 5, 0, p64(out)) == 0  # batch 0
        assert ctx.lib.stark_eval_plan_apply(empty.h, p64(polys), 5, 2, p64(out)) == 0  # n = 0
        assert empty.apply(polys).shape == (2, 0, 4)
        assert ctx.lib.stark_eval_poly_multipoint_batch(ctx.h, p64(polys), 5, 0, p64(xs), n, p64(out)) == 0
        assert ctx.lib.stark_eval_poly_multipoint_batch(ctx.h, p64(polys), 5, 2, p64(xs), 0, p64(out)) == 0
        assert np.array_equal(out, keep)
        d_out = torch.full((2 * n * 32,), 0xA5, dtype=torch.uint8, device="cuda")
        d_polys = dev(polys)
        plan.apply_dev(d_polys.data_ptr(), 5, 5, 0, d_out.data_ptr(), n)
        empty.apply_dev(d_polys.data_ptr(), 5, 5, 2, d_out.data_ptr(), 0)
        ctx.synchronize()
        assert np.array_equal(host(d_out, 2, n), keep)
        # refused: a polynomial beyond the bound, strides below the row lengths
        with pytest.raises(StarkError) as e:
            plan.apply(polys_for(2, 41))
        assert e.value.code == 1
        for args in ((5, 4, 2, d_out.data_ptr(), n), (5, 5, 2, d_out.data_ptr(), n - 1)):
            with pytest.raises(StarkError) as e:
                plan.apply_dev(d_polys.data_ptr(), *args)
            assert e.value.code == 3
        ctx.synchronize()
        assert np.array_equal(host(d_out, 2, n), keep)
    with pytest.raises(StarkError) as e:  # max_deg_plus_1 = 0
        ctx.eval_plan(xs, 0)
    assert e.value.code == 3


def test_bound_beyond_the_tree_limit_is_refused_unallocated(ctx):
    """max_deg_plus_1 + N > 2^27 (N = 64 here): STARK_ERR_BAD_LENGTH before anything is allocated."""
    xs = xs_for(33)
    before = ctx.memory()["resident"]
    for bound in ((1 << 27) - 63, 1 << 40):
        with pytest.raises(StarkError) as e:
            ctx.eval_plan(xs, bound)
        assert e.value.code == 1
    with pytest.raises(StarkError) as e:
        ctx.eval_plan([0, 1, 2], (1 << 27) - 31, O.root_of_unity(5), 5)
    assert e.value.code == 1
    assert ctx.memory()["resident"] == before


def test_strided_device_form(ctx, oracle):
    """poly_stride = deg_plus_1 + 5, out_stride = n + 3: the gaps of the output keep their sentinel."""
    n, d, batch = 65, 70, 5
    xs, polys = xs_for(n), polys_for(batch, d)
    wide = np.full((batch, d + 5, 4), SENTINEL, dtype=np.uint64)
    wide[:, :d] = polys
    d_polys = dev(wide)
    d_out = torch.full((batch * (n + 3) * 32,), 0xA5, dtype=torch.uint8, device="cuda")
    with ctx.eval_plan(xs, 100) as plan:
        plan.apply_dev(d_polys.data_ptr(), d, d + 5, batch, d_out.data_ptr(), n + 3)
        ctx.synchronize()
    got = host(d_out, batch, n + 3)
    assert np.array_equal(got[:, :n], expected(ctx, oracle, polys, xs))
    assert (got[:, n:] == SENTINEL).all()
    assert np.array_equal(host(d_polys, batch, d + 5), wide)


@pytest.mark.parametrize("bound", [70, 3 * 128 + 7])
def test_chunks_give_the_same_output(ctx, oracle, batch_limit, bound):
    """Chunks of one, and chunks of two from the documented scratch per polynomial (batch 5: 2, 2, 1), with alpha's
    own transform and with a prefix's; the host form and the device form."""
    n, d, batch = 65, 70, 5
    xs, polys = xs_for(n), polys_for(batch, d)
    d_polys = dev(polys)
    with ctx.eval_plan(xs, bound) as plan:
        want = plan.apply(polys)
        assert np.array_equal(want, expected(ctx, oracle, polys, xs))
        for limit in (1, 2 * 32 * scratch_elems(n, d)):
            batch_limit(limit)
            assert np.array_equal(plan.apply(polys), want), limit
            d_out = torch.zeros(batch * n * 32, dtype=torch.uint8, device="cuda")
            plan.apply_dev(d_polys.data_ptr(), d, d, batch, d_out.data_ptr(), n)
            ctx.synchronize()
            assert np.array_equal(host(d_out, batch, n), want), limit


def test_side_stream_between_neighbours(ctx, oracle, tree_min):
    """apply_dev on a side stream between a single tree evaluation and an interpolation plan's application on the
    context stream, which share the context's tree arena: all three results are unchanged."""
    n, d, batch = 129, 200, 3
    xs, polys = xs_for(n), polys_for(batch, d)
    other_xs, other_poly = xs_for(257), polys_for(1, 300)[0]
    ipts = limbs(points(65, 5900, False))
    ivals = np.stack([limbs(values(65, 5901 + b)) for b in range(2)])
    tree_min(1)
    single_want = ctx.eval_poly_multipoint(other_poly, other_xs)
    assert np.array_equal(single_want, oracle.eval_poly_multi(other_poly, other_xs))
    iplan = ctx.interp_plan(ipts)
    try:
        interp_want = iplan.apply(ivals)
        with ctx.eval_plan(xs, d) as plan:
            want = plan.apply(polys)
            assert np.array_equal(want, expected(ctx, oracle, polys, xs))
            d_polys = dev(polys)
            d_out = torch.zeros(batch * n * 32, dtype=torch.uint8, device="cuda")
            back = torch.empty(batch * n * 32, dtype=torch.uint8).pin_memory()
            tp, tx = dev(other_poly), dev(other_xs)
            t_single = torch.zeros(257 * 32, dtype=torch.uint8, device="cuda")
            ti = dev(ivals)
            t_interp = torch.zeros_like(ti)
            torch.cuda.synchronize()
            ctx.eval_poly_multipoint_dev(tp.data_ptr(), 300, tx.data_ptr(), 257, t_single.data_ptr())
            with torch.cuda.stream(torch.cuda.Stream()):
                plan.apply_dev(d_polys.data_ptr(), d, d, batch, d_out.data_ptr(), n, torch_stream())
                back.copy_(d_out, non_blocking=True)
            iplan.apply_dev(ti.data_ptr(), 2, t_interp.data_ptr())
            ctx.synchronize()
            torch.cuda.synchronize()
            assert np.array_equal(back.numpy().view(np.uint64).reshape(batch, n, 4), want)
            assert np.array_equal(host(t_single, 257), single_want)
            assert np.array_equal(host(t_interp, 2, 65), interp_want)
    finally:
        iplan.close()


def test_two_plans_alternately(ctx, oracle):
    a_xs, b_xs = xs_for(65), xs_for(257)
    pa, pb = polys_for(2, 100), polys_for(3, 300)
    with ctx.eval_plan(a_xs, 100) as a, ctx.eval_plan(b_xs, 400) as b:
        ra, rb = a.apply(pa), b.apply(pb)
        assert np.array_equal(ra, expected(ctx, oracle, pa, a_xs))
        assert np.array_equal(rb, expected(ctx, oracle, pb, b_xs))
        for _ in range(2):
            assert a.apply(pa).tobytes() == ra.tobytes()
            assert b.apply(pb).tobytes() == rb.tobytes()
        assert np.array_equal(b.apply(pa), expected(ctx, oracle, pa, b_xs))


@pytest.mark.parametrize("log_order", [11, 7])
def test_domain_plan_equals_expanded_points(ctx, oracle, log_order):
    """xs[i] = root^exps[i]; with log_order 7 the 200 exponents repeat."""
    n, d = 200, 150
    root = O.root_of_unity(log_order)
    rng = np.random.default_rng(log_order)
    exps = [int(e) for e in rng.integers(0, 1 << log_order, n)]
    xs = limbs([pow(root, e, P) for e in exps])
    polys = polys_for(3, d)
    with ctx.eval_plan(exps, d, root, log_order) as a, ctx.eval_plan(xs, d) as b:
        got = a.apply(polys)
        assert np.array_equal(got, b.apply(polys))
        assert np.array_equal(got, expected(ctx, oracle, polys, xs))


def test_domain_plan_errors(ctx):
    g = O.root_of_unity(10)
    with pytest.raises(StarkError) as e:  # an exponent outside the domain
        ctx.eval_plan([0, 3, 1 << 10], 8, g, 10)
    assert e.value.code == 3
    with pytest.raises(StarkError) as e:  # not a primitive 2^9-th root
        ctx.eval_plan([1], 8, g, 9)
    assert e.value.code == 2


@pytest.mark.parametrize("n", [33, 129, 600])
def test_round_trip_on_one_stream(ctx, n):
    """Values -> coefficients (InterpPlan.apply_dev) -> values (EvalPlan.apply_dev, deg_plus_1 = n) on one stream
    with no host synchronisation between them: the original values, with no oracle involved."""
    batch = 4
    xs = limbs(points(n, 7000 + n, False))
    ys = np.stack([limbs(values(n, 7100 + n + b)) for b in range(batch)])
    iplan = ctx.interp_plan(xs)
    try:
        with ctx.eval_plan(xs, n) as plan:
            d_ys = dev(ys)
            d_coeffs, d_back = torch.zeros_like(d_ys), torch.zeros_like(d_ys)
            back = torch.empty(d_ys.numel(), dtype=torch.uint8).pin_memory()
            torch.cuda.synchronize()
            with torch.cuda.stream(torch.cuda.Stream()):
                iplan.apply_dev(d_ys.data_ptr(), batch, d_coeffs.data_ptr(), torch_stream())
                plan.apply_dev(d_coeffs.data_ptr(), n, n, batch, d_back.data_ptr(), n, torch_stream())
                back.copy_(d_back, non_blocking=True)
            torch.cuda.synchronize()
            assert np.array_equal(back.numpy().view(np.uint64).reshape(batch, n, 4), ys)
    finally:
        iplan.close()


def test_convenience_call_equals_the_plan(ctx, oracle):
    n, d = 257, 300
    xs, polys = xs_for(n), polys_for(3, d)
    with ctx.eval_plan(xs, d) as plan:
        want = plan.apply(polys)
    got = ctx.eval_poly_multipoint_batch(polys, xs)
    assert got.shape == (3, n, 4)
    assert np.array_equal(got, want)
    assert np.array_equal(got, expected(ctx, oracle, polys, xs))
    zeros = ctx.eval_poly_multipoint_batch(np.empty((2, 0, 4), dtype=np.uint64), xs)
    assert zeros.shape == (2, n, 4) and not zeros.any()


def test_close_gives_the_memory_back():
    c = Context(0)
    try:
        n, bound = 200, 300
        xs, polys = xs_for(n), polys_for(2, bound)
        warm = c.eval_plan(xs, bound)  # the context's own buffers and tables at their size for this plan
        warm.apply(polys)
        warm.close()
        before = c.memory()["resident"]
        plan = c.eval_plan(xs, bound)
        held = c.memory()["resident"] - before
        assert held == 32 * plan_elems(n, bound) == 32 * (200 + 256 + 2 * 256 * 3 + 3 * 512)
        plan.apply(polys)
        plan.close()
        assert c.memory()["resident"] == before
        plan.close()  # twice: harmless
        assert plan.h is None
    finally:
        c.close()


def test_plan_freed_after_its_context(oracle):
    """Closing the context releases a live plan's device memory; the plan's close() then frees the handle alone."""
    c = Context(0)
    xs, polys = xs_for(65), polys_for(2, 70)
    plan = c.eval_plan(xs, 70)
    want = plan.apply(polys)
    c.close()
    plan.close()
    assert plan.h is None
    c = Context(0)
    try:
        assert np.array_equal(c.eval_poly_multipoint_batch(polys, xs), want)
        assert np.array_equal(want[0], oracle.eval_poly_multi(polys[0], xs))
    finally:
        c.close()
