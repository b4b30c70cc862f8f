"""Multi-point evaluation (eval_poly_at over every x, poly_utils.rs:93-102) by the split Horner and by the
descent of the subproduct tree, against the oracle's C Horner and the library's untouched one-thread-per-point
kernel (eval_poly_at_multi); and lagrange_interp (poly_utils.rs:409-439) with its denominators taken down the
tree.  All arithmetic is exact: every route gives the same bits."""
import functools

import numpy as np
import pytest
import torch

import oracle as O
from stark_amd import Context, torch_stream
from test_gpu_poly import limbs, points, py_lagrange_interp, values

pytestmark = pytest.mark.gpu

NEVER = Context.MULTIPOINT_TREE_NEVER


def padded(n):
    N = 32
    while N < n:
        N *= 2
    return N


# n: 32 | 33 the leaf launch alone against the first NTT level; 65 and 129 the first and second wrapped
# levels (Adj changes); 257, 600 several levels with padding
TREE_N = [1, 2, 31, 32, 33, 64, 65, 128, 129, 257, 600]


def tree_degs(n):
    N = padded(n)
    return sorted({d for d in (0, 1, n - 1, n, n + 1, N, N + 1, 3 * N + 7) if d >= 0})


TREE_CASES = [(n, d) for n in TREE_N for d in tree_degs(n)]
SPLIT_CASES = [(n, d) for n in (1, 3, 80) for d in (1, 255, 256, 257, 4097, (1 << 16) + 3)]


@pytest.fixture
def tree_min(ctx):
    yield ctx.set_multipoint_tree_min
    ctx.set_multipoint_tree_min(0)


@functools.lru_cache(maxsize=None)
def xs_for(n):
    return limbs(points(n, 3000 + n, True))


@functools.lru_cache(maxsize=None)
def poly_for(d):
    return O.random_elements(d, 4000 + d) if d else np.empty((0, 4), dtype=np.uint64)


def check(ctx, oracle, n, d):
    poly, xs = poly_for(d), xs_for(n)
    got = ctx.eval_poly_multipoint(poly, xs)
    assert got.shape == (n, 4)
    want = oracle.eval_poly_multi(poly, xs) if d else np.zeros((n, 4), dtype=np.uint64)
    assert np.array_equal(got, want)
    assert np.array_equal(got, ctx.eval_poly_at_multi(poly, xs))
    if n >= 3:
        assert np.array_equal(got[n - 1], got[1])  # the repeated x
        assert np.array_equal(got[n // 2], poly[0] if d else np.zeros(4, dtype=np.uint64))  # x = 0


@pytest.mark.parametrize("n,d", TREE_CASES)
def test_tree_forced(ctx, oracle, tree_min, n, d):
    tree_min(1)
    check(ctx, oracle, n, d)


@pytest.mark.parametrize("n,d", SPLIT_CASES)
def test_split_forced(ctx, oracle, tree_min, n, d):
    tree_min(NEVER)
    check(ctx, oracle, n, d)


@pytest.mark.parametrize("n,d", [(3000, 300), (70000, 40), (600000, 3)])
def test_split_many_points(ctx, oracle, tree_min, n, d):
    """With many points a point's sum is split over fewer lanes (8, 2 and 1 here), several points per workgroup,
    the last workgroup part empty."""
    tree_min(NEVER)
    poly, xs = poly_for(d), O.random_elements(n, 3000 + n)
    got = ctx.eval_poly_multipoint(poly, xs)
    assert np.array_equal(got, oracle.eval_poly_multi(poly, xs))
    assert np.array_equal(got, ctx.eval_poly_at_multi(poly, xs))


@pytest.mark.parametrize("n,d", [(80, 1 << 16), (600, 600), (4096, 5)])
def test_default_dispatch(ctx, oracle, n, d):
    ctx.set_multipoint_tree_min(0)
    poly, xs = poly_for(d), xs_for(n) if n <= 600 else O.random_elements(n, 3000 + n)
    assert np.array_equal(ctx.eval_poly_multipoint(poly, xs), oracle.eval_poly_multi(poly, xs))


def test_no_points(ctx):
    assert ctx.eval_poly_multipoint(poly_for(5), np.empty((0, 4), dtype=np.uint64)).shape == (0, 4)


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


@pytest.mark.parametrize("m", [1, NEVER])
def test_device_form_on_a_torch_stream(ctx, oracle, tree_min, m):
    """The _dev entry on a torch stream, the copy back enqueued behind it with no host synchronisation between."""
    tree_min(m)
    n, d = 600, 1000
    poly, xs = poly_for(d), xs_for(n)
    tp, tx = _dev(poly), _dev(xs)
    out = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    host = torch.empty(n * 32, dtype=torch.uint8).pin_memory()
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        ctx.eval_poly_multipoint_dev(tp.data_ptr(), d, tx.data_ptr(), n, out.data_ptr(), stream=torch_stream())
        host.copy_(out, non_blocking=True)
    torch.cuda.synchronize()
    assert np.array_equal(host.numpy().view(np.uint64).reshape(-1, 4), oracle.eval_poly_multi(poly, xs))


@pytest.mark.parametrize("n", [33, 257, 600])
def test_lagrange_interp_by_the_descent(ctx, tree_min, n):
    """Z'(x_i) down the tree against Z'(x_i) by the untouched Horner kernel: identical interpolants."""
    xs, ys = limbs(points(n, 1000 + n, False)), limbs(values(n, 2000 + n))
    tree_min(1)
    a = ctx.lagrange_interp(xs, ys)
    tree_min(NEVER)
    b = ctx.lagrange_interp(xs, ys)
    assert np.array_equal(a, b)
    if n == 33:
        assert O.from_limbs(a) == py_lagrange_interp(O.from_limbs(xs), O.from_limbs(ys))
