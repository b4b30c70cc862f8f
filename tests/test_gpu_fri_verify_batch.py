"""Batched FRI verification from proof handles (stark_verify_low_degree_batch): every status against the single
call and against the oracle's verifier, every reason mask against a classifier built from the oracle's item
functions alone, with the Last elements checked by the host workers and by the device.

The classifier is never told where a proof was tampered with: it evaluates the three classes of checks -- Merkle
paths, rows, the Last element -- independently of one another from the proof as given, as the entry documents."""
import copy
import ctypes

import numpy as np
import pytest

import oracle as O
import stark_amd as S
import stark_verify as V
from stark_amd.verify import (FAIL_FRI_LAST, FAIL_FRI_PATHS, FAIL_FRI_ROWS, FAIL_SINGLE, verify_low_degree_batch,
                              verify_low_degree_proof)

pytestmark = pytest.mark.gpu
P = O.P


# ---- the classifier: oracle/stark_verify.py's item functions, class by class -------------------------------------
def _order(w):
    n, t = 1, w
    while t != 1:
        n, t = 2 * n, t * t % P
    return n


def classify(root, w, proof, bound, excl):
    """(mask, last_root_holds, last_degree_holds) of a Middle* + Last proof."""
    deg = _order(w)
    quartic = V.quartic_roots(w, deg)
    mask, cur = 0, bytes(root)
    for prf in proof[:-1]:
        m = prf["Middle"]
        root2 = bytes(m["root2"])
        ys = V.get_pseudorandom_indices(root2, deg // 4, 40, excl)
        pos = [j * (deg // 4) + y for y in ys for j in range(4)]
        for idx, br in zip(ys, m["column_branches"]):
            if V.path_root(idx, br["leaf"], br["nodes"]) != root2:
                mask |= FAIL_FRI_PATHS
        for idx, br in zip(pos, m["poly_branches"]):
            if V.path_root(idx, br["leaf"], br["nodes"]) != cur:
                mask |= FAIL_FRI_PATHS
        sx = V.fe(cur)
        for i, y in enumerate(ys):
            row = [m["poly_branches"][4 * i + j]["leaf"] for j in range(4)]
            if not V.fri_row_holds(w, quartic, y, row, m["column_branches"][i]["leaf"], sx):
                mask |= FAIL_FRI_ROWS
        cur, w, bound, deg = root2, pow(w, 4, P), bound // 4, deg // 4
    last = [bytes(v) for v in proof[-1]["Last"]["last"]]
    root_ok = V.last_layer_root_holds(last, cur)
    admissible = [p for p in range(len(last)) if excl == 0 or p % excl != 0]
    # the two Last asserts (fri.rs:348-351, :359), and split_off's panic on too few admissible points
    sized = bound >= V.MIN_DEG_DIRECT_CHECKING // 2 and len(last) > bound and len(admissible) >= bound
    degree_ok = sized and V.last_layer_degree_holds(last, w, deg, bound, excl)
    if not (sized and root_ok and degree_ok):
        mask |= FAIL_FRI_LAST
    return mask, root_ok, degree_ok


def oracle_accepts(root, w, proof, bound, excl):
    try:
        return V.verify_low_degree_proof(bytes(root), w, proof, bound, excl)
    except AssertionError:
        return False


def single_status(root, w, proof, bound, excl):
    try:
        verify_low_degree_proof(bytes(root), w, proof, bound, excl)
        return 0
    except AssertionError:
        return 8
    except S.StarkError as e:
        return e.code


# ---- proofs: made once per parameter set, shared and never changed -----------------------------------------------
_SETS = {}


def _root_of(oracle, v):
    n = len(v)
    return oracle.merkle(np.ascontiguousarray(v, dtype=np.uint64).tobytes(), n, 32, [], chunks=4)[0]


def proof_set(ctx, oracle, log_n, bound, excl, batch, degree=None):
    """(w, roots, parsed proofs) of `batch` vectors of 2^log_n values of degree < `degree` (default: the bound)."""
    key = (log_n, bound, excl, batch, degree)
    if key not in _SETS:
        w = O.root_of_unity(log_n)
        vs = [oracle.best_fft(O.random_elements(degree or bound, 9000 + 64 * log_n + b), w, log_n, cpus=8)
              for b in range(batch)]
        try:
            proofs = [p.layers() for p in ctx.prove_low_degree_batch(np.stack(vs), w, bound, excl)]
        except S.StarkError:  # (a parameter set the prover refuses: the oracle's proofs)
            import json
            proofs = [json.loads(oracle.prove_low_degree_json(v, w, bound, excl, chunks=4)) for v in vs]
        _SETS[key] = (w, [_root_of(oracle, v) for v in vs], proofs)
    w, roots, proofs = _SETS[key]
    return w, list(roots), copy.deepcopy(proofs)


def run_both(ctx, roots, w, proofs, bound, excl):
    """The batch under both Last modes; the results must be identical.  (Parsed proofs become handles through
    FriProofList.from_parts inside verify_low_degree_batch.)"""
    out = {}
    try:
        for mode in (1, 2):
            ctx.set_verify_batch_last(mode)
            out[mode] = verify_low_degree_batch(ctx, roots, w, proofs, bound, excl)
    finally:
        ctx.set_verify_batch_last(0)
    assert out[1] == out[2]
    return out[2]


def check_all(ctx, roots, w, proofs, bound, excl):
    """Every assertion of a case for every proof; returns [(status, mask)]."""
    got = run_both(ctx, roots, w, proofs, bound, excl)
    for b, (proof, root) in enumerate(zip(proofs, roots)):
        status, why = got[b]
        mask, _, _ = classify(root, w, proof, bound, excl)
        accepts = oracle_accepts(root, w, proof, bound, excl)
        assert status == single_status(root, w, proof, bound, excl), b
        assert status == (0 if accepts else 8), b
        assert why == mask, (b, why, mask)
        assert (mask == 0) == accepts, b
    return got


def flip(value, bit=0):
    v = bytearray(bytes(value))
    v[bit // 8] ^= 1 << (bit % 8)
    return list(v)


def plus_p(value):
    x = int.from_bytes(bytes(value), "little") + P
    assert x < 1 << 256
    return list(x.to_bytes(32, "little"))


def admissible(n, excl):
    return [p for p in range(n) if excl == 0 or p % excl != 0]


# ---- the parameter sets of the entry's code paths ------------------------------------------------------------------
# (log n, bound, exclusion, layers, Last, m)
TABLE = [(6, 16, 8, 0, 64, 16),      # the caller's root is the Last's root
         (7, 32, 8, 1, 32, 8),
         (8, 64, 0, 1, 64, 16),      # no exclusion
         (9, 48, 3, 1, 128, 12),     # m not a power of two, exclusion 3
         (9, 100, 8, 2, 32, 6),      # every proof refused: the degree of direct checking is too low
         (8, 256, 8, 2, 16, 16),     # n_last <= m
         (12, 16, 8, 0, 4096, 16),   # the wide-Last route
         (14, 1 << 12, 8, 4, 64, 16)]  # four Middle layers
SMALL = TABLE[:3]


def _table_case(ctx, oracle, log_n, bound, excl, layers, n_last, m, batch):
    w, roots, proofs = proof_set(ctx, oracle, log_n, bound, excl, batch)
    for p in proofs:
        assert len(p) == layers + 1 and len(p[-1]["Last"]["last"]) == n_last
    assert bound // 4 ** layers == m
    refused = m < 8 or n_last <= m
    if batch >= 3:  # one proof's Last value at a rest point is changed: its neighbours must not notice
        at = admissible(n_last, excl)[-1]
        proofs[1][-1]["Last"]["last"][at] = flip(proofs[1][-1]["Last"]["last"][at], 9)
    got = check_all(ctx, roots, w, proofs, bound, excl)
    for b, (status, why) in enumerate(got):
        if refused or (batch >= 3 and b == 1):
            assert (status, why) == (8, FAIL_FRI_LAST), b
        else:
            assert (status, why) == (0, 0), b


@pytest.mark.parametrize("log_n,bound,excl,layers,n_last,m", TABLE)
def test_table(ctx, oracle, log_n, bound, excl, layers, n_last, m):
    _table_case(ctx, oracle, log_n, bound, excl, layers, n_last, m, 3)


@pytest.mark.parametrize("batch", [1, 65])
@pytest.mark.parametrize("log_n,bound,excl,layers,n_last,m", SMALL)
def test_batches(ctx, oracle, log_n, bound, excl, layers, n_last, m, batch):
    _table_case(ctx, oracle, log_n, bound, excl, layers, n_last, m, batch)


def test_chunks(ctx, oracle):
    """A staging cap of 64 KiB holds one proof of (2^7, 32) (some 44 KB staged): seven chunks."""
    w, roots, proofs = proof_set(ctx, oracle, 7, 32, 8, 7)
    proofs[2][0]["Middle"]["root2"] = flip(proofs[2][0]["Middle"]["root2"])
    proofs[5][-1]["Last"]["last"][3] = flip(proofs[5][-1]["Last"]["last"][3])
    whole = check_all(ctx, roots, w, proofs, 32, 8)
    try:
        ctx.set_verify_batch_limit(64 << 10)
        chunked = run_both(ctx, roots, w, proofs, 32, 8)
    finally:
        ctx.set_verify_batch_limit(0)
    assert chunked == whole
    assert [s for s, _ in whole] == [0, 0, 8, 0, 0, 8, 0]


# ---- directed tampers: one proof each inside an otherwise valid batch -----------------------------------------------
T_LOG, T_BOUND, T_EXCL = 10, 256, 8  # two Middle layers, a Last of 64 values, m = 16


def _node(which, layer):
    def f(proofs, roots, b):
        br = proofs[b][layer]["Middle"][which][7]
        br["nodes"][1] = flip(br["nodes"][1], 77)
    return f


def _leaf(which):
    def f(proofs, roots, b):
        br = proofs[b][0]["Middle"][which][5]
        br["leaf"] = flip(br["leaf"], 3)
    return f


def _column_leaf_plus_p(proofs, roots, b):
    br = proofs[b][1]["Middle"]["column_branches"][11]
    br["leaf"] = plus_p(br["leaf"])


def _root2(proofs, roots, b):
    proofs[b][0]["Middle"]["root2"] = flip(proofs[b][0]["Middle"]["root2"], 200)


def _wrong_root(proofs, roots, b):
    roots[b] = bytes(flip(roots[b], 5))


def _last_at(which, change=flip):
    def f(proofs, roots, b):
        last = proofs[b][-1]["Last"]["last"]
        adm = admissible(len(last), T_EXCL)
        at = {"excluded": T_EXCL, "interp": adm[3], "rest": adm[T_BOUND // 16 + 5]}[which]
        last[at] = change(last[at])
    return f


PATHS, ROWS, LAST = FAIL_FRI_PATHS, FAIL_FRI_ROWS, FAIL_FRI_LAST
# (name, tamper, the classes the entry documents for it; None: whatever the classifier finds, not zero)
TAMPERS = [("column node, first layer", _node("column_branches", 0), PATHS),
           ("polynomial node, first layer", _node("poly_branches", 0), PATHS),
           ("column node, last layer", _node("column_branches", 1), PATHS),
           ("polynomial node, last layer", _node("poly_branches", 1), PATHS),
           ("polynomial leaf", _leaf("poly_branches"), PATHS | ROWS),
           ("column leaf", _leaf("column_branches"), PATHS | ROWS),
           ("column leaf + p", _column_leaf_plus_p, PATHS),
           ("root2", _root2, None),
           ("wrong merkle root", _wrong_root, None),
           ("Last value at an excluded position", _last_at("excluded"), LAST),
           ("Last value at an interpolation point", _last_at("interp"), LAST),
           ("Last value at a rest point", _last_at("rest"), LAST),
           ("Last value + p", _last_at("rest", plus_p), LAST)]


def test_directed_tampers(ctx, oracle):
    n_t = len(TAMPERS)
    w, roots, proofs = proof_set(ctx, oracle, T_LOG, T_BOUND, T_EXCL, 2 * n_t + 1)
    for k, (_, tamper, _) in enumerate(TAMPERS):  # the odd entries; every even entry is a valid neighbour
        tamper(proofs, roots, 2 * k + 1)
    got = check_all(ctx, roots, w, proofs, T_BOUND, T_EXCL)
    for b, (status, why) in enumerate(got):
        if b % 2 == 0:
            assert (status, why) == (0, 0), b
            continue
        name, _, want = TAMPERS[b // 2]
        assert not oracle_accepts(roots[b], w, proofs[b], T_BOUND, T_EXCL), name
        assert status == 8 and why != 0, name
        if want is not None:
            assert why == want, (name, why)
    # which of the Last element's two checks refuses, by the oracle's item functions
    at = {name: 2 * k + 1 for k, (name, _, _) in enumerate(TAMPERS)}
    for name, want in (("Last value at an excluded position", (False, True)), ("Last value + p", (False, True)),
                       ("Last value at an interpolation point", (False, False)),
                       ("Last value at a rest point", (False, False))):
        b = at[name]
        assert classify(roots[b], w, proofs[b], T_BOUND, T_EXCL)[1:] == want, name
    b = at["column leaf + p"]  # the row still holds on the value mod p
    assert classify(roots[b], w, proofs[b], T_BOUND, T_EXCL)[0] & ROWS == 0


def test_wrong_root_without_layers(ctx, oracle):
    w, roots, proofs = proof_set(ctx, oracle, 6, 16, 8, 3)
    roots[1] = bytes(flip(roots[1], 100))
    got = check_all(ctx, roots, w, proofs, 16, 8)
    assert got == [(0, 0), (8, LAST), (0, 0)]
    assert not oracle_accepts(roots[1], w, proofs[1], 16, 8)


def test_degree_alone_fails(ctx, oracle):
    """An honest proof of a vector of degree < n / 2 under the bound n / 4: every path and row holds, the Last
    values' tree is the last root2's, and their degree alone is too high."""
    w, roots, proofs = proof_set(ctx, oracle, T_LOG, T_BOUND, T_EXCL, 3)
    _, high_root, high = proof_set(ctx, oracle, T_LOG, T_BOUND, T_EXCL, 1, degree=1 << (T_LOG - 1))
    roots[1], proofs[1] = high_root[0], high[0]
    got = check_all(ctx, roots, w, proofs, T_BOUND, T_EXCL)
    assert got == [(0, 0), (8, LAST), (0, 0)]
    assert classify(roots[1], w, proofs[1], T_BOUND, T_EXCL) == (LAST, True, False)
    assert not oracle_accepts(roots[1], w, proofs[1], T_BOUND, T_EXCL)


def test_swapped_proofs(ctx, oracle):
    w, roots, proofs = proof_set(ctx, oracle, 7, 32, 8, 4)
    proofs[1], proofs[2] = proofs[2], proofs[1]
    got = check_all(ctx, roots, w, proofs, 32, 8)
    assert got[0] == (0, 0) and got[3] == (0, 0)
    for b in (1, 2):
        assert got[b][0] == 8 and got[b][1] & PATHS
        assert not oracle_accepts(roots[b], w, proofs[b], 32, 8)


# ---- structure: everything but the exact shape goes through the single-proof verifier --------------------------------
def _no_last(p):
    return p[:-1]


def _last_in_the_middle(p):
    return [p[-1]] + p


def _39_columns(p):
    p[0]["Middle"]["column_branches"].pop()
    return p


def _31_byte_leaves(p):
    for br in p[0]["Middle"]["column_branches"]:
        br["leaf"] = br["leaf"][:31]
    return p


def _one_node_too_few(p):
    for br in p[0]["Middle"]["poly_branches"]:
        br["nodes"].pop()
    return p


def _last_of_48(p):
    p[-1]["Last"]["last"] = (p[-1]["Last"]["last"] * 2)[:48]
    return p


STRUCTURAL = [_no_last, _last_in_the_middle, _39_columns, _31_byte_leaves, _one_node_too_few, _last_of_48]


def test_structural_cases(ctx, oracle):
    w, roots, proofs = proof_set(ctx, oracle, 7, 32, 8, 2 * len(STRUCTURAL) + 5)
    _, other_roots, other = proof_set(ctx, oracle, 9, 48, 3, 3)
    for k, change in enumerate(STRUCTURAL):
        proofs[2 * k + 1] = change(proofs[2 * k + 1])
    b_other, b_null = 2 * len(STRUCTURAL) + 1, 2 * len(STRUCTURAL) + 3
    proofs[b_other], roots[b_other] = other[0], other_roots[0]  # a proof of another size
    proofs[b_null] = None
    got = run_both(ctx, roots, w, proofs, 32, 8)
    for b, (status, why) in enumerate(got):
        if b % 2 == 0:
            assert (status, why) == (0, 0), b
            continue
        want = 3 if b == b_null else single_status(roots[b], w, proofs[b], 32, 8)
        assert want != 0, b
        assert (status, why) == (want, FAIL_SINGLE), b
    assert [got[2 * k + 1][0] for k in range(2)] == [3, 3]  # no Last, a Last in the middle: malformed
    assert got[b_other][0] == 8


def test_root_of_unity_of_no_two_power_order(ctx, oracle):
    _, roots, proofs = proof_set(ctx, oracle, 7, 32, 8, 3)
    got = run_both(ctx, roots, 5, proofs, 32, 8)
    for b in range(3):
        assert single_status(roots[b], 5, proofs[b], 32, 8) == 3
    assert got == [(3, FAIL_SINGLE)] * 3


# ---- the contract ------------------------------------------------------------------------------------------------------
def _raw_call(ctx, roots, w, handles, bound, excl, statuses=True, ctx_h=True, n=None):
    n = len(handles) if n is None else n
    hs = (ctypes.c_void_p * max(len(handles), 1))(*[None if h is None else h.h for h in handles])
    sts = (ctypes.c_int * max(n, 1))(*([-1] * max(n, 1)))
    why = (ctypes.c_uint32 * max(n, 1))(*([0xFFFF] * max(n, 1)))
    rou = None if w is None else S._limbs(w).ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    rc = ctx.lib.stark_verify_low_degree_batch(ctx.h if ctx_h else None, roots, rou, hs if handles is not None else None,
                                               n, bound, excl, sts if statuses else None, why)
    return rc, list(sts), list(why)


def test_whole_call_errors_and_empty_batch(ctx, oracle):
    w, roots, proofs = proof_set(ctx, oracle, 7, 32, 8, 3)
    handles = [S.FriProofList.from_parts(p) for p in proofs]
    blob = b"".join(roots)
    untouched = ([-1] * 3, [0xFFFF] * 3)
    assert _raw_call(ctx, blob, w, handles, 32, 8, ctx_h=False) == (3, *untouched)
    assert _raw_call(ctx, None, w, handles, 32, 8) == (3, *untouched)
    assert _raw_call(ctx, blob, None, handles, 32, 8) == (3, *untouched)
    rou = S._limbs(w).ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    sts = (ctypes.c_int * 3)(-1, -1, -1)
    assert ctx.lib.stark_verify_low_degree_batch(ctx.h, blob, rou, None, 3, 32, 8, sts, None) == 3  # null proofs
    assert list(sts) == [-1] * 3
    rc, s, y = _raw_call(ctx, blob, w, handles, 32, 8, n=65536)
    assert rc == 3 and s[:3] == [-1] * 3
    rc, s, y = _raw_call(ctx, blob, w, handles, 32, 8, n=0)
    assert rc == 0 and s[0] == -1 and y[0] == 0xFFFF
    assert verify_low_degree_batch(ctx, [], w, [], 32, 8) == []
    for mode in (3, 7):
        with pytest.raises(S.StarkError) as e:
            ctx.set_verify_batch_last(mode)
        assert e.value.code == 3
    rc, s, y = _raw_call(ctx, blob, w, handles, 32, 8)
    assert (rc, s, y) == (0, [0] * 3, [0] * 3)


def test_statuses_null(ctx, oracle):
    w, roots, proofs = proof_set(ctx, oracle, 7, 32, 8, 4)
    good = [S.FriProofList.from_parts(p) for p in proofs]
    blob = b"".join(roots)
    assert _raw_call(ctx, blob, w, good, 32, 8, statuses=False)[0] == 0
    proofs[2][-1]["Last"]["last"][5] = flip(proofs[2][-1]["Last"]["last"][5])
    bad = good[:2] + [S.FriProofList.from_parts(proofs[2])] + good[3:]
    rc, _, why = _raw_call(ctx, blob, w, bad, 32, 8, statuses=False)
    assert rc == 8 and why == [0, 0, LAST, 0]
    rc, _, why = _raw_call(ctx, blob, w, [good[0], None, bad[2], good[3]], 32, 8, statuses=False)
    assert rc == 3 and why == [0, FAIL_SINGLE, LAST, 0]  # the first status in batch order that is not STARK_OK


@pytest.mark.parametrize("log_n,bound,excl", [(10, 256, 8), (12, 16, 8)])
def test_second_call_allocates_nothing(ctx, oracle, log_n, bound, excl):
    w, roots, proofs = proof_set(ctx, oracle, log_n, bound, excl, 3)
    handles = [S.FriProofList.from_parts(p) for p in proofs]
    first_result = verify_low_degree_batch(ctx, roots, w, handles, bound, excl)
    first = ctx.memory()["resident"]
    assert verify_low_degree_batch(ctx, roots, w, handles, bound, excl) == first_result == [(0, 0)] * 3
    assert ctx.memory()["resident"] == first


def test_single_batch_single(ctx, oracle):
    """A single prove / verify pair before and after a batch on one context gives the same results."""
    log_n, bound = 10, 256
    w = O.root_of_unity(log_n)
    v = oracle.best_fft(O.random_elements(bound, 4242), w, log_n, cpus=8)
    root = _root_of(oracle, v)
    first = ctx.prove_low_degree(v, w, bound, 8).to_json()
    assert single_status(root, w, first, bound, 8) == 0
    _, roots, proofs = proof_set(ctx, oracle, log_n, bound, 8, 3)
    assert run_both(ctx, roots, w, proofs, bound, 8) == [(0, 0)] * 3
    second = ctx.prove_low_degree(v, w, bound, 8).to_json()
    assert second == first
    assert single_status(root, w, second, bound, 8) == 0
    assert verify_low_degree_batch(ctx, [root], w, [second], bound, 8) == [(0, 0)]


def test_prover_handles_go_in_as_they_are(ctx, oracle):
    """The prover's own handles (no from_parts on the way), one of them against another proof's root."""
    log_n, bound = 8, 64
    w = O.root_of_unity(log_n)
    vs = [oracle.best_fft(O.random_elements(bound, 777 + b), w, log_n, cpus=8) for b in range(4)]
    roots = [_root_of(oracle, v) for v in vs]
    handles = ctx.prove_low_degree_batch(np.stack(vs), w, bound, 8)
    roots[3] = roots[0]
    got = run_both(ctx, roots, w, handles, bound, 8)
    assert got[:3] == [(0, 0)] * 3 and got[3][0] == 8 and got[3][1] & PATHS
    assert got[3] == (8, classify(roots[3], w, handles[3].layers(), bound, 8)[0])
