"""Every single-GPU entry point on poisoned and on reused context scratch (tests/ctx_tour.py).

The other GPU tests compare each entry point with the oracle on whatever memory the context happens to hold: fresh
from hipMalloc (usually zero) or left by the same test's previous call.  Here the library's poison flag fills every
new allocation, and stark_test_poison_ctx refills every scratch buffer of the context between calls, with 0xA5 or
0xFF: as limbs both are >= p, as counters and flags both are non-zero, so a kernel that reads an element nobody
wrote, or that relies on a pad being zero, gives wrong bytes here instead of passing by the luck of test order.
The expected bytes never come from a GPU run."""
import hashlib
import json
import os
import random

import pytest
import torch  # noqa: F401  (before the library is loaded, as in the other modules that hand torch buffers to it)

import ctx_tour as T
import stark_amd as S

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "r1cs_proofs.json")))


@pytest.fixture
def poisoned(request):
    """A new context with the poison flag on (0xA5); the flag always ends off."""
    request.addfinalizer(lambda: S.set_poison(False, 0))
    S.set_poison(True, 0xA5)
    ctx = S.Context(0)

    def done():
        T.release(ctx)
        ctx.close()
    request.addfinalizer(done)
    return ctx


def _same(op, which, got: bytes, what: str):
    want = op.want(which)
    if got != want:
        k = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
        pytest.fail(f"{op.name} shape {which} = {op.shapes[which]!r} {what}: {len(got)} bytes for {len(want)}, "
                    f"first difference at byte {k}: {got[k:k + 32].hex()} for {want[k:k + 32].hex()}", pytrace=False)


@pytest.mark.parametrize("op", T.OPS, ids=lambda op: op.name)
def test_poisoned(poisoned, op):
    """A on fresh poisoned allocations; B inside A's larger buffers refilled with 0xFF; A again on 0xA5."""
    ctx = poisoned
    _same(op, "A", op.call(ctx, "A"), "on new poisoned allocations")
    S.poison_ctx(ctx, 0xFF)
    _same(op, "B", op.call(ctx, "B"), "in A's buffers filled with 0xFF")
    S.poison_ctx(ctx, 0xA5)
    _same(op, "A", op.call(ctx, "A"), "after B, buffers filled with 0xA5")


def _compute_golden(ctx):
    from stark_amd.r1cs import prove_with_witness
    r1, wt = T._r1cs_in("compute")
    js = prove_with_witness(ctx, r1, wt).to_json()
    assert hashlib.sha256(js.encode()).hexdigest() == GOLDEN["compute"]["json_sha256"]


def _tour(ctx, seed):
    """Every (op, shape) pair in a seeded order on one context, the scratch refilled before every call with the
    byte alternating; each device entry alternates between the context's stream and a second torch stream."""
    calls = [(op, which) for op in T.OPS for which in ("A", "B")]
    random.Random(seed).shuffle(calls)
    second = {}
    for k, (op, which) in enumerate(calls):
        S.poison_ctx(ctx, 0xFF if k % 2 else 0xA5)
        second[op.name] = not second.get(op.name, bool(seed % 2))
        where = "second torch stream" if op.dev and second[op.name] else "context stream"
        _same(op, which, op.call(ctx, which, second[op.name]), f"as call {k} of order {seed} ({where})")


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_mixed_order(poisoned, seed):
    ctx = poisoned
    _tour(ctx, seed)
    S.poison_ctx(ctx, 0xA5)
    _compute_golden(ctx)


def test_tour_reaches_every_buffer(poisoned):
    """After the whole tour on one context every scratch buffer holds memory, so each was run on poison; the
    kept tables the tour builds are there too."""
    ctx = poisoned
    for op in T.OPS:
        for which in ("A", "B"):
            _same(op, which, op.call(ctx, which), "in table order")
    report = S.poison_ctx(ctx, 0xA5)
    assert {n: c for n, _, c in report} == T.BUFFERS
    empty = [n for n, held, c in report if c == T.SCRATCH and held == 0]
    print("\n".join("%-18s %12d %s" % r for r in report))
    assert sorted(empty) == sorted(T.UNREACHED), empty
    held = {n: b for n, b, _ in report}
    for name in ("tree_counters", "tw", "ext_idx", "eval_plans", "long_lists"):
        assert held[name] > 0, name
    _compute_golden(ctx)
