"""zpoly / lagrange_interp (poly_utils.rs:362-439) and the DFT mul_polys / div_polys (fft.rs:381-432) on the
GPU against a plain-int restatement of the reference's routines (quadratic, written for these sizes)."""
import functools
import random

import numpy as np
import pytest

import oracle as O
from stark_amd import StarkError

pytestmark = pytest.mark.gpu

P = O.P
# 32 | 33: the last size the LDS leaf kernel multiplies out alone, the first with an NTT level above it
SIZES = [0, 1, 2, 3, 5, 31, 32, 33, 257, 600]


def py_zpoly(xs):
    """zpoly (poly_utils.rs:362-373), low degree first."""
    z = [1]
    for x in xs:
        z = [((z[j - 1] if j else 0) - (z[j] * x if j < len(z) else 0)) % P for j in range(len(z) + 1)]
    return z


def py_eval(poly, x):
    y = 0
    for c in reversed(poly):
        y = (y * x + c) % P
    return y


def py_lagrange_interp(xs, ys):
    """lagrange_interp (poly_utils.rs:409-439): nums by dividing zpoly back by each X - x, denominators by
    evaluating them, multi_inv (0 -> 0), the sum of the rescaled nums."""
    n = len(xs)
    root = py_zpoly(xs)
    b = [0] * n
    for x, y in zip(xs, ys):
        num = [0] * n
        carry = root[n]
        for d in range(n, 0, -1):  # synthetic division of root by X - x
            num[d - 1] = carry
            carry = (root[d - 1] + carry * x) % P
        den = py_eval(num, x)
        s = y * pow(den, P - 2, P) % P if den else 0
        if s:
            for j in range(n):
                b[j] = (b[j] + num[j] * s) % P
    return b


def py_cyclic(a, b, n):
    """mul_polys (fft.rs:381-395): the product of a and b mod X^n - 1."""
    out = [0] * n
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[(i + j) % n] = (out[(i + j) % n] + x * y) % P
    return out


def points(n, seed, repeat):
    """n field elements: 0 among them (n >= 3), all distinct, or with xs[1] repeated at the end (n >= 3)."""
    rng = random.Random(seed)
    xs = []
    while len(xs) < n:
        x = rng.randrange(P)
        if x not in xs:
            xs.append(x)
    if n >= 3:
        xs[n // 2] = 0
        if repeat:
            xs[n - 1] = xs[1]
    return xs


def values(n, seed):
    rng = random.Random(seed)
    ys = [rng.randrange(P) for _ in range(n)]
    for i in range(0, n, 7):
        ys[i] = 0
    return ys


@functools.lru_cache(maxsize=None)
def case(n, repeat):
    xs, ys = points(n, 1000 + n, repeat), values(n, 2000 + n)
    return xs, ys, py_zpoly(xs), py_lagrange_interp(xs, ys)


def limbs(v):
    return O.to_limbs(v) if len(v) else np.empty((0, 4), dtype=np.uint64)


@pytest.mark.parametrize("repeat", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_zpoly(ctx, n, repeat):
    xs, _, want, _ = case(n, repeat)
    got = ctx.zpoly(limbs(xs))
    assert O.from_limbs(got) == want
    assert O.from_limbs(got[n:]) == [1]
    if n:
        assert not ctx.eval_poly_at_multi(got, limbs(xs)).any()


@pytest.mark.parametrize("n", SIZES)
def test_lagrange_interp(ctx, n):
    xs, ys, _, want = case(n, False)
    got = ctx.lagrange_interp(limbs(xs), limbs(ys))
    assert O.from_limbs(got) == want
    if n:
        assert O.from_limbs(ctx.eval_poly_at_multi(got, limbs(xs))) == ys


@pytest.mark.parametrize("n", [n for n in SIZES if n >= 3])
def test_lagrange_interp_repeated_x(ctx, n):
    """Both points of a repeated x have a zero denominator, which multi_inv maps to zero: they drop out."""
    xs, ys, _, want = case(n, True)
    assert O.from_limbs(ctx.lagrange_interp(limbs(xs), limbs(ys))) == want


@pytest.mark.parametrize("count", [1, 7, 700])
def test_lagrange_interp_domain(ctx, count):
    """xs = g^w over a random subset of a 2^10 domain: the hinted path (one transform of Z', a gather) and the
    unhinted one (Horner at every point) agree."""
    g = O.root_of_unity(10)
    w = random.Random(30 + count).sample(range(1 << 10), count)
    xs = [pow(g, e, P) for e in w]
    ys = values(count, 40 + count)
    plain = ctx.lagrange_interp(limbs(xs), limbs(ys))
    hinted = ctx.lagrange_interp(w, limbs(ys), root_of_unity=g, log_order_of_root=10)
    assert np.array_equal(plain, hinted)
    assert O.from_limbs(ctx.eval_poly_at_multi(hinted, limbs(xs))) == ys
    if count <= 7:
        assert O.from_limbs(hinted) == py_lagrange_interp(xs, ys)


def test_lagrange_interp_domain_errors(ctx):
    g = O.root_of_unity(10)
    with pytest.raises(StarkError) as e:  # an exponent outside the domain
        ctx.lagrange_interp([1 << 10], limbs([5]), root_of_unity=g, log_order_of_root=10)
    assert e.value.code == 3
    with pytest.raises(StarkError) as e:  # not a primitive 2^9-th root
        ctx.lagrange_interp([1], limbs([5]), root_of_unity=g, log_order_of_root=9)
    assert e.value.code == 2


# (log_n, la, lb): full lengths (la = n; la + lb - 1 > n wraps), a product that fits, and at 2^13 a full a
# against a short b (the restatement is la x lb products)
@pytest.mark.parametrize("log_n,la,lb", [(2, 4, 4), (2, 2, 2), (8, 256, 256), (8, 100, 57), (13, 8192, 5),
                                         (13, 3000, 9)])
def test_mul_polys(ctx, log_n, la, lb):
    n = 1 << log_n
    a = O.random_elements(la, 50 + la)
    b = O.random_elements(lb, 51 + lb)
    got = ctx.mul_polys(a, b, O.root_of_unity(log_n), log_n)
    assert O.from_limbs(got) == py_cyclic(O.from_limbs(a), O.from_limbs(b), n)


@pytest.mark.parametrize("log_n", [2, 8, 13])
def test_div_polys(ctx, log_n):
    n = 1 << log_n
    w = O.root_of_unity(log_n)
    # b = X - 3 (against a = (X - 3)(X + 5) the restatement is exact division), then a random full-length b
    a = [(-15) % P, 2, 1]
    assert O.from_limbs(ctx.div_polys(limbs(a), limbs([P - 3, 1]), w, log_n)) == [5, 1] + [0] * (n - 2)
    a = O.random_elements(n, 60 + log_n)
    b = O.random_elements(n, 61 + log_n)
    assert ctx.best_fft(b, w, log_n).any(axis=1).all()  # b's transform has no zero
    prod = ctx.mul_polys(a, b, w, log_n)
    assert np.array_equal(ctx.div_polys(prod, b, w, log_n), a)


def test_div_polys_zero_of_the_transform(ctx):
    """multi_inv maps a zero of b's transform to zero (fft.rs:423): b = X - 1 vanishes at the first point."""
    log_n, n = 4, 16
    w = O.root_of_unity(log_n)
    a = O.from_limbs(O.random_elements(n, 70))
    ta = [py_eval(a, pow(w, i, P)) for i in range(n)]
    tb = [(pow(w, i, P) - 1) % P for i in range(n)]
    q = [x * (pow(y, P - 2, P) if y else 0) % P for x, y in zip(ta, tb)]
    winv, ninv = pow(w, P - 2, P), pow(n, P - 2, P)
    want = [py_eval(q, pow(winv, i, P)) * ninv % P for i in range(n)]
    assert O.from_limbs(ctx.div_polys(limbs(a), limbs([P - 1, 1]), w, log_n)) == want


def test_mul_polys_errors(ctx):
    a = O.random_elements(9, 80)
    with pytest.raises(StarkError) as e:  # a root of order 2^4 for a 2^3 transform
        ctx.mul_polys(a[:4], a[:4], O.root_of_unity(4), 3)
    assert e.value.code == 2
    with pytest.raises(StarkError) as e:  # a root of order 2^2
        ctx.div_polys(a[:4], a[:4], O.root_of_unity(2), 3)
    assert e.value.code == 2
    with pytest.raises(StarkError) as e:  # la > n
        ctx.mul_polys(a, a[:4], O.root_of_unity(3), 3)
    assert e.value.code == 1
    with pytest.raises(StarkError) as e:  # lb > n
        ctx.div_polys(a[:4], a, O.root_of_unity(3), 3)
    assert e.value.code == 1
