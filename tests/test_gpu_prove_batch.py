"""stark_prove_r1cs_circuit_batch / R1csCircuit.prove_batch: B witnesses of one prepared circuit through one
chain of launches.

Bar: out[b] is the proof stark_prove_r1cs_circuit returns for wtns[b], byte for byte.  Three shapes are held
against the CPU oracle (oracle/r1cs.c, the restatement of prove.rs:14-378), three against the single call
(itself pinned to the oracle by tests/test_gpu_r1cs.py) and the golden digests.  A mismatch is reported by field
of the StarkProof, never as a diff of the texts.
"""
import ctypes
import hashlib
import json
import os
import sys

import pytest

import r1cs as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "r1cs")
GOLDEN = json.load(open(os.path.join(HERE, "golden", "r1cs_proofs.json")))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

pytestmark = pytest.mark.gpu


def _read(name, ext):
    with open(os.path.join(FIX, f"{name}.{ext}"), "rb") as f:
        return f.read()


def _sha(s: str) -> str:
    return hashlib.sha256(s.encode()).hexdigest()


def _first_difference(a, b, path="proof"):
    """Where two parsed StarkProof values first differ, as a path and the two scalars (or lengths)."""
    if type(a) is not type(b):
        return f"{path}: {type(a).__name__} against {type(b).__name__}"
    if isinstance(a, dict):
        if a.keys() != b.keys():
            return f"{path}: keys {sorted(a)} against {sorted(b)}"
        for k in a:
            d = _first_difference(a[k], b[k], f"{path}.{k}")
            if d:
                return d
        return None
    if isinstance(a, list):
        if len(a) != len(b):
            return f"{path}: {len(a)} entries against {len(b)}"
        for i, (x, y) in enumerate(zip(a, b)):
            d = _first_difference(x, y, f"{path}[{i}]")
            if d:
                return d
        return None
    return None if a == b else f"{path}: {a!r} against {b!r}"


def assert_same_proof(got: str, want: str, what: str):
    if got != want:
        diff = _first_difference(json.loads(got), json.loads(want)) or "the texts differ, the values do not"
        pytest.fail(f"{what}: {diff}")


def _synth(log_steps, inputs=None, n_public=2):
    import synth_r1cs
    return synth_r1cs.for_steps(log_steps, inputs=inputs, n_public=n_public)


def _witnesses(log_steps, count, n_public=2):
    """One synthetic circuit with `count` witnesses (the .r1cs is the same for every `inputs`)."""
    r1, _ = _synth(log_steps, n_public=n_public)
    wts = []
    for k in range(count):
        r1k, wt = _synth(log_steps, inputs=(1000 + 17 * k, R.P - 5 - k), n_public=n_public)
        assert r1k == r1
        wts.append(wt)
    return r1, wts


def _oracle_json(oracle, r1, wt):
    return R.mk_r1cs_proof_json(oracle, R.build_trace(R.read_r1cs(r1), R.read_witness(wt)))


@pytest.fixture(scope="module")
def small(ctx):
    """The 2^6-step circuit (precision 2^9) most checks here use: the circuit prepared once, five witnesses and
    their single-call proofs."""
    from stark_amd.r1cs import R1csCircuit
    r1, wts = _witnesses(6, 5)
    c = R1csCircuit(ctx, r1)
    return {"r1": r1, "wts": wts, "circuit": c, "single": [c.prove(w).to_json() for w in wts]}


# ---- parity with the oracle ---------------------------------------------------------------------------


def test_compute_repeated_matches_oracle_and_golden(ctx, oracle):
    """Precision 128: every tree has at most 256 nodes, so several share one workgroup in the forest's tail."""
    from stark_amd.r1cs import R1csCircuit
    r1, wt = _read("compute", "r1cs"), _read("compute", "wtns")
    want = _oracle_json(oracle, r1, wt)
    proofs = R1csCircuit(ctx, r1).prove_batch([wt] * 5)
    assert len(proofs) == 5
    for b, p in enumerate(proofs):
        s = p.to_json()
        assert_same_proof(s, want, f"compute, proof {b} of 5")
        assert _sha(s) == GOLDEN["compute"]["json_sha256"]


def test_2_6_steps_matches_oracle(ctx, oracle, small):
    """Precision 2^9: the forests' 512-node level crosses the tail kernel's boundary."""
    proofs = small["circuit"].prove_batch(small["wts"][:3])
    for b, p in enumerate(proofs):
        want = _oracle_json(oracle, small["r1"], small["wts"][b])
        assert_same_proof(p.to_json(), want, f"2^6 steps, proof {b} of 3")


def test_2_10_steps_41_public_points_matches_oracle(ctx, oracle):
    """A 41-coefficient I2 by Horner, different for every proof of the batch."""
    from stark_amd.r1cs import R1csCircuit
    r1, wts = _witnesses(10, 4, n_public=40)
    proofs = R1csCircuit(ctx, r1).prove_batch(wts)
    for b, p in enumerate(proofs):
        assert_same_proof(p.to_json(), _oracle_json(oracle, r1, wts[b]), f"2^10 steps, 41 points, proof {b} of 4")


# ---- parity with the single call ----------------------------------------------------------------------


def test_2_13_steps_matches_single(ctx):
    """Precision 2^16 takes the forests' wide leaf kernel."""
    from stark_amd.r1cs import R1csCircuit
    r1, wts = _witnesses(13, 2)
    c = R1csCircuit(ctx, r1)
    proofs = c.prove_batch(wts)
    for b, p in enumerate(proofs):
        assert_same_proof(p.to_json(), c.prove(wts[b]).to_json(), f"2^13 steps, proof {b} of 2")


@pytest.mark.parametrize("name", ["poseidon3_test", "pedersen_test"])
def test_fixture_repeated_matches_golden(ctx, name):
    from stark_amd.r1cs import R1csCircuit
    c = R1csCircuit(ctx, _read(name, "r1cs"))
    wt = _read(name, "wtns")
    proofs = c.prove_batch([wt, wt])
    want = c.prove(wt).to_json()
    for b, p in enumerate(proofs):
        s = p.to_json()
        assert_same_proof(s, want, f"{name}, proof {b} of 2")
        assert _sha(s) == GOLDEN[name]["json_sha256"]


@pytest.mark.parametrize("log_steps,n_public", [(10, 160), (11, 200)])
def test_column_route_matches_single(ctx, log_steps, n_public):
    """128 public points or more: I2 is a column, interpolated per witness ahead of the chain and extended in one
    batch.  (The generator's 2^10-step circuit has 57 constraints and takes at most 170 public wires, so the
    200 wires asked for need 2^11 steps; 2^10 steps run with 160 wires, 161 points, the same route.)"""
    from stark_amd.r1cs import R1csCircuit
    r1, wts = _witnesses(log_steps, 3, n_public=n_public)
    c = R1csCircuit(ctx, r1)
    proofs = c.prove_batch(wts)
    for b, p in enumerate(proofs):
        assert_same_proof(p.to_json(), c.prove(wts[b]).to_json(), f"column route, proof {b} of 3")


# ---- other checks -------------------------------------------------------------------------------------


def test_batch_of_one_equals_single(small):
    (p,) = small["circuit"].prove_batch(small["wts"][:1])
    assert_same_proof(p.to_json(), small["single"][0], "batch of one")


def test_same_witness_twice(small):
    a, b = small["circuit"].prove_batch([small["wts"][1]] * 2)
    assert_same_proof(a.to_json(), small["single"][1], "first of two equal witnesses")
    assert a.to_json() == b.to_json()


def test_every_proof_of_a_batch_verifies(ctx, small):
    from stark_amd.verify import verify_with_wtns
    proofs = small["circuit"].prove_batch(small["wts"][:3])
    for b, p in enumerate(proofs):
        assert verify_with_wtns(ctx, small["r1"], small["wts"][b], p.to_json()), b


def _call(ctx, circuit_h, wts, with_statuses=True, batch=None):
    """The C entry point itself: (return code, statuses or None, handles)."""
    n = len(wts)
    ptrs = (ctypes.c_char_p * max(n, 1))(*wts)
    lens = (ctypes.c_size_t * max(n, 1))(*[0 if w is None else len(w) for w in wts])
    out = (ctypes.c_void_p * max(n, 1))()
    sts = (ctypes.c_int * max(n, 1))(*([-1] * max(n, 1)))
    rc = ctx.lib.stark_prove_r1cs_circuit_batch(ctx.h, circuit_h, ptrs, lens, n if batch is None else batch, out,
                                                sts if with_statuses else None)
    return rc, (list(sts)[:n] if with_statuses else None), list(out)[:n]


def _json_and_free(ctx, h) -> str:
    from stark_amd.r1cs import StarkProof
    return StarkProof(ctx.lib, ctypes.c_void_p(h)).to_json()


def _bad_witnesses(wt: bytes):
    """An unsatisfying witness (the last chain value changed), one whose first value is not 1, a truncated one."""
    unsat = bytearray(wt)
    unsat[-32] ^= 1
    first = bytearray(wt)
    n_wit = (len(wt) - (4 + 5 * 4 + 4 + 32 + 4 + 3 * 4)) // 32  # wtns v2: two section headers, a 32-B prime
    first[len(wt) - 32 * n_wit] ^= 2
    return [(bytes(unsat), 8), (bytes(first), 3), (wt[:len(wt) - 40], 3)]


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_one_bad_witness_among_good_ones(ctx, small, kind):
    bad, code = _bad_witnesses(small["wts"][1])[kind]
    c = small["circuit"]
    rc, sts, hs = _call(ctx, c.h, [small["wts"][0], bad, small["wts"][2]])
    assert rc == 0
    assert sts == [0, code, 0]
    assert hs[1] is None and hs[0] and hs[2]
    assert_same_proof(_json_and_free(ctx, hs[0]), small["single"][0], "proof 0 beside a bad witness")
    assert_same_proof(_json_and_free(ctx, hs[2]), small["single"][2], "proof 2 beside a bad witness")
    # the same input without statuses: all or nothing, the first failing witness's status
    rc, _, hs = _call(ctx, c.h, [small["wts"][0], bad, small["wts"][2]], with_statuses=False)
    assert rc == code
    assert hs == [None, None, None]
    # a good batch on the same context afterwards
    for b, p in enumerate(c.prove_batch(small["wts"][:2])):
        assert_same_proof(p.to_json(), small["single"][b], f"proof {b} after a failed batch")


def test_python_strictness(small):
    from stark_amd import StarkError
    from stark_amd.r1cs import StarkProof
    bad = _bad_witnesses(small["wts"][1])[0][0]
    with pytest.raises(StarkError) as e:
        small["circuit"].prove_batch([small["wts"][0], bad])
    assert e.value.code == 8 and e.value.index == 1
    got = small["circuit"].prove_batch([small["wts"][0], bad], strict=False)
    assert isinstance(got[0], StarkProof) and isinstance(got[1], StarkError)
    assert got[1].code == 8 and got[1].index == 1


def test_argument_errors(ctx, small):
    import stark_amd as S
    wts = small["wts"][:2]
    other = S.Context(0)
    try:  # a circuit of another context
        rc, _, hs = _call(other, small["circuit"].h, wts)
        assert rc == 3 and hs == [None, None]
    finally:
        other.close()
    h = ctypes.c_void_p()  # a circuit prepared for world 2
    ctx.check(ctx.lib.stark_dprove_circuit_new(ctx.h, 2, 0, small["r1"], len(small["r1"]), ctypes.byref(h)), "world 2")
    try:
        rc, _, hs = _call(ctx, h, wts)
        assert rc == 3 and hs == [None, None]
    finally:
        ctx.lib.stark_r1cs_circuit_free(h)
    rc, sts, hs = _call(ctx, small["circuit"].h, wts[:1], batch=65536)  # refused before anything is read
    assert rc == 3 and hs == [None] and sts == [-1]
    rc, sts, hs = _call(ctx, small["circuit"].h, [], batch=0)
    assert rc == 0


def test_chunking_and_buffer_reuse(small):
    """A limit under which two proofs fit and three do not, then a limit of one byte (chunks of one): the proofs
    do not change.  The working set of one proof is what a batch of one adds to the context's resident bytes.
    A second identical call allocates nothing; a lower limit frees the batch's buffers."""
    import stark_amd as S
    from stark_amd.r1cs import R1csCircuit
    c0 = S.Context(0)
    try:
        circuit = R1csCircuit(c0, small["r1"])
        assert_same_proof(circuit.prove(small["wts"][0]).to_json(), small["single"][0], "single, own context")
        before = c0.memory()["resident"]
        circuit.prove_batch(small["wts"][:1])
        one = c0.memory()["resident"] - before
        assert one > 0
        c0.set_prove_batch_limit(2 * one + one // 2)
        for b, p in enumerate(circuit.prove_batch(small["wts"])):
            assert_same_proof(p.to_json(), small["single"][b], f"chunks of two, proof {b} of 5")
        assert c0.memory()["resident"] - before < 3 * one  # no chunk of three was allocated
        c0.set_prove_batch_limit(1)
        for b, p in enumerate(circuit.prove_batch(small["wts"])):
            assert_same_proof(p.to_json(), small["single"][b], f"chunks of one, proof {b} of 5")
        c0.set_prove_batch_limit(0)
        circuit.prove_batch(small["wts"])
        held = c0.memory()["resident"]
        circuit.prove_batch(small["wts"])
        assert c0.memory()["resident"] == held
        c0.set_prove_batch_limit(one)
        assert c0.memory()["resident"] < held
    finally:
        c0.close()


def test_single_call_after_a_batch_is_golden(ctx, small):
    """No state of a batch leaks into the context's trees and pinned slots."""
    from stark_amd.r1cs import R1csCircuit
    small["circuit"].prove_batch(small["wts"][:3])
    c = R1csCircuit(ctx, _read("pedersen_test", "r1cs"))
    assert _sha(c.prove(_read("pedersen_test", "wtns")).to_json()) == GOLDEN["pedersen_test"]["json_sha256"]
