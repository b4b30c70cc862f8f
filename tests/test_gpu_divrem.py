"""Division with remainder (poly_utils::div_polys and mod_polys, poly_utils.rs:235-295, in one call) on the GPU
against a plain-int restatement of the reference's long division."""
import random

import numpy as np
import pytest

import oracle as O
from stark_amd import StarkError

pytestmark = pytest.mark.gpu

P = O.P


def py_div_polys(a, b):
    """div_polys (poly_utils.rs:235-262): b's trailing zeros dropped, then long division from the top."""
    b = list(b)
    while b and b[-1] == 0:
        b.pop()
    assert len(a) >= len(b) > 0
    c, o = list(a), []
    apos, bpos = len(a) - 1, len(b) - 1
    inv = pow(b[bpos], P - 2, P)
    for d in range(apos - bpos, -1, -1):
        quot = c[apos] * inv % P
        o.append(quot)
        for i in range(bpos, -1, -1):
            c[d + i] = (c[d + i] - b[i] * quot) % P
        apos -= 1
    o.reverse()
    return o


def py_mul(a, b):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] = (out[i + j] + x * y) % P
    return out


def py_mod_polys(a, b, quot):
    """mod_polys (poly_utils.rs:291-295): the first len(b) - 1 coefficients of a - b quot, quot = div_polys(a, b)."""
    prod = py_mul(b, quot)
    diff = [(x - (prod[i] if i < len(prod) else 0)) % P for i, x in enumerate(a)]
    return (diff + [0] * len(b))[:len(b) - 1]


def limbs(v):
    return O.to_limbs(v) if len(v) else np.empty((0, 4), dtype=np.uint64)


def check(ctx, a, b):
    q, r = ctx.divrem_polys(limbs(a), limbs(b))
    q, r = O.from_limbs(q), O.from_limbs(r)
    want = py_div_polys(a, b)
    assert q == want
    assert r == py_mod_polys(a, b, want)
    assert len(r) == len(b) - 1
    # b q + r = a in plain integers, from the GPU's own q and r
    back = py_mul(b, q)
    back = [(x + (r[i] if i < len(r) else 0)) % P for i, x in enumerate(back)]
    assert back[:len(a)] == list(a) and not any(back[len(a):])
    return q, r


def rand_poly(n, seed):
    rng = random.Random(seed)
    v = [rng.randrange(P) for _ in range(n)]
    v[-1] = v[-1] or 1
    return v


# The reference's own cases (poly_utils.rs:264-327) are over F7: p2 = 6 + x + 2x^2, quotient 4 + 2x + x^3 and the
# remainders 2 + 2x, 2 and 0.  Over this field the same small integers divide exactly when the dividend is made
# from them: a = p2 q + r.
REF_B, REF_Q = [6, 1, 2], [4, 2, 0, 1]


@pytest.mark.parametrize("rem", [[0, 0], [2, 2], [2, 0]])
def test_reference_cases(ctx, rem):
    a = py_mul(REF_B, REF_Q)
    a = [(x + (rem[i] if i < 2 else 0)) % P for i, x in enumerate(a)]
    assert len(a) == 6
    q, r = check(ctx, a, REF_B)
    assert q == REF_Q and r == rem


@pytest.mark.parametrize("la,lb", [(1, 1), (6, 3), (32, 32), (33, 32), (64, 33), (65, 2), (257, 129), (3000, 700)])
def test_random(ctx, la, lb):
    check(ctx, rand_poly(la, 100 + la), rand_poly(lb, 200 + lb))


def test_trailing_zeros_of_b(ctx):
    a, b = rand_poly(100, 1), rand_poly(20, 2)
    q, r = check(ctx, a, b + [0, 0, 0])
    q0, r0 = check(ctx, a, b)
    assert q == q0 and r == r0 + [0, 0, 0] and len(r) == 22


def test_exact_product(ctx):
    b, c = rand_poly(40, 3), rand_poly(75, 4)
    q, r = check(ctx, py_mul(b, c), b)
    assert q == c and not any(r)


def test_leading_zeros_of_a(ctx):
    """a's leading zeros are not trimmed: the quotient keeps its length, its top coefficients zero."""
    a, b = rand_poly(50, 5) + [0, 0, 0, 0], rand_poly(9, 6)
    q, _ = check(ctx, a, b)
    assert len(q) == 54 - 9 + 1 and q[-4:] == [0, 0, 0, 0]


def test_constant_divisor(ctx):
    q, r = check(ctx, rand_poly(70, 7), [5])
    assert len(q) == 70 and r == []


def test_errors(ctx):
    a = limbs(rand_poly(6, 8))
    with pytest.raises(StarkError) as e:  # b = 0: the reference underflows
        ctx.divrem_polys(a, limbs([0, 0, 0]))
    assert e.value.code == 3
    with pytest.raises(StarkError) as e:  # assert!(a.len() >= b.len()) (poly_utils.rs:244, :278-288)
        ctx.divrem_polys(a[:3], a)
    assert e.value.code == 1
