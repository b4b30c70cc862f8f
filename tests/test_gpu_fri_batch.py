"""GPU parity: prove_low_degree for a batch of vectors through one launch chain, each proof byte for byte
against the oracle's proof of its vector (the oracle called once per member)."""
import json

import numpy as np
import pytest

import oracle as O
import stark_amd as S

pytestmark = pytest.mark.gpu


def _vectors(oracle, log_n, deg_div, batch, repeat=None):
    """batch vectors of 2^log_n values of degree < n / deg_div, different by seed; repeat = (a, b): vector b is
    vector a again."""
    n = 1 << log_n
    w = O.root_of_unity(log_n)
    vs = [oracle.best_fft(O.random_elements(n // deg_div, 7000 + 100 * log_n + b), w, log_n, cpus=8)
          for b in range(batch)]
    if repeat:
        vs[repeat[1]] = vs[repeat[0]].copy()
    return w, vs


def _first_difference(got: str, want: str) -> str:
    """Where two proofs' JSON texts differ, by field (never the megabytes of text themselves)."""
    g, w = json.loads(got), json.loads(want)
    if len(g) != len(w):
        return "%d entries, expected %d" % (len(g), len(w))
    for l, (a, b) in enumerate(zip(g, w)):
        if list(a) != list(b):
            return "entry %d is %s, expected %s" % (l, list(a), list(b))
        kind = list(a)[0]
        for key in b[kind]:
            x, y = a[kind].get(key), b[kind][key]
            if x == y:
                continue
            if key in ("column_branches", "poly_branches"):
                if len(x) != len(y):
                    return "entry %d %s: %d branches, expected %d" % (l, key, len(x), len(y))
                for i, (p, q) in enumerate(zip(x, y)):
                    for part in ("leaf", "nodes"):
                        if p[part] != q[part]:
                            return "entry %d %s[%d].%s" % (l, key, i, part)
            return "entry %d %s" % (l, key)
    return "texts differ, parsed values equal"


def _assert_proofs(got: list, want: list):
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        if g != w:
            pytest.fail("proof %d of %d: %s" % (b, len(want), _first_difference(g, w)))


# (log_n, exclude, deg_div, batch): 11 x 65 has more than one gather launch's requests; 13 / 4096 has zero
# layers; 18 takes the forest's wide leaf kernel.
CASES = [(7, 8, 4, 3), (10, 2, 4, 5), (11, 3, 4, 65), (12, 8, 4, 64), (13, 8, 4096, 2), (14, 0, 4, 7), (16, 8, 8, 4),
         (18, 8, 4, 2)]


@pytest.mark.parametrize("log_n,excl,deg_div,batch", CASES)
def test_fri_batch_vs_oracle(ctx, oracle, log_n, excl, deg_div, batch):
    n = 1 << log_n
    w, vs = _vectors(oracle, log_n, deg_div, batch)
    want = [oracle.prove_low_degree_json(v, w, n // deg_div, excl, chunks=8) for v in vs]
    got = [p.to_json() for p in ctx.prove_low_degree_batch(np.stack(vs), w, n // deg_div, excl)]
    _assert_proofs(got, want)


def test_fri_batch_repeated_vector(ctx, oracle):
    log_n, batch = 10, 4
    n = 1 << log_n
    w, vs = _vectors(oracle, log_n, 4, batch, repeat=(1, 3))
    got = [p.to_json() for p in ctx.prove_low_degree_batch(vs, w, n // 4, 8)]  # (a list of vectors)
    assert got[1] == got[3]
    assert got[0] != got[1]
    _assert_proofs(got, [oracle.prove_low_degree_json(v, w, n // 4, 8, chunks=8) for v in vs])


def test_fri_batch_dev_equals_host_form(ctx, oracle):
    log_n, batch = 12, 6
    n = 1 << log_n
    w, vs = _vectors(oracle, log_n, 4, batch)
    vals = np.ascontiguousarray(np.stack(vs))
    host = [p.to_json() for p in ctx.prove_low_degree_batch(vals, w, n // 4, 8)]
    d = ctx.alloc(vals.nbytes)
    try:
        ctx.h2d(d, vals)
        dev = [p.to_json() for p in ctx.prove_low_degree_batch_dev(d, n, batch, w, n // 4, 8)]
        after = np.empty_like(vals)
        ctx.d2h(after, d)
    finally:
        ctx.free(d)
    _assert_proofs(dev, host)
    assert np.array_equal(after, vals), "the device values were modified"


def test_fri_single_batch_single(ctx, oracle):
    """A single proof before and after a batch on one context: the same bytes (the batch shares the column
    buffer and the gather's staging with the single path)."""
    log_n = 12
    n = 1 << log_n
    w, vs = _vectors(oracle, log_n, 4, 5)
    first = ctx.prove_low_degree(vs[2], w, n // 4, 8).to_json()
    batch = [p.to_json() for p in ctx.prove_low_degree_batch(vs, w, n // 4, 8)]
    second = ctx.prove_low_degree(vs[2], w, n // 4, 8).to_json()
    assert first == second
    assert batch[2] == first
    assert first == oracle.prove_low_degree_json(vs[2], w, n // 4, 8, chunks=8)


def test_fri_batch_proofs_verify(ctx, oracle):
    from stark_amd.verify import verify_low_degree_proof
    log_n, batch = 10, 3
    n = 1 << log_n
    w, vs = _vectors(oracle, log_n, 4, batch)
    proofs = ctx.prove_low_degree_batch(vs, w, n // 4, 8)
    for b, p in enumerate(proofs):
        leaves = b"".join(O.to_bytes_le(x) for x in O.from_limbs(vs[b]))
        root, _ = oracle.merkle(leaves, n, 32, [], chunks=4)
        assert verify_low_degree_proof(root, w, p.layers(), n // 4, 8), b
    other, _ = oracle.merkle(b"".join(O.to_bytes_le(x) for x in O.from_limbs(vs[1])), n, 32, [], chunks=4)
    with pytest.raises(AssertionError):
        assert verify_low_degree_proof(other, w, proofs[0].layers(), n // 4, 8)


def test_fri_batch_errors(ctx):
    w = O.root_of_unity(8)
    vals = O.random_elements(512, 1).reshape(2, 256, 4)
    with pytest.raises(S.StarkError) as e:
        ctx.prove_low_degree_batch(vals[:, :128], w, 64, 8)  # len != order of root
    with pytest.raises(S.StarkError) as e1:
        ctx.prove_low_degree(vals[0, :128], w, 64, 8)
    assert e.value.code == e1.value.code
    with pytest.raises(S.StarkError) as e:
        ctx.prove_low_degree_batch(vals, w, 64, 1)  # exclude_multiples_of = 1
    with pytest.raises(S.StarkError) as e1:
        ctx.prove_low_degree(vals[0], w, 64, 1)
    assert e.value.code == e1.value.code
    assert ctx.prove_low_degree_batch([], w, 64, 8) == []
    assert ctx.prove_low_degree_batch_dev(0, 256, 0, w, 64, 8) == []


def test_fri_batch_second_call_allocates_nothing(ctx, oracle):
    log_n, batch = 11, 9
    n = 1 << log_n
    w, vs = _vectors(oracle, log_n, 4, batch)
    ctx.prove_low_degree_batch(vs, w, n // 4, 8)
    first = ctx.memory()["resident"]
    ctx.prove_low_degree_batch(vs, w, n // 4, 8)
    assert ctx.memory()["resident"] == first
