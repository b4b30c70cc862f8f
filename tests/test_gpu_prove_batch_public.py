"""R1csCircuit.prove_batch on the column route (public-input-heavy circuits): I2's coefficients of every proof of
a chunk by one application of the circuit's interpolation plan (csrc/poly.hip interp_plan_apply) instead of one
interpolation per witness.  The arithmetic is exact: every proof is the oracle's, byte for byte."""
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


@pytest.fixture
def settings(ctx):
    """The context's thresholds and limits for one test; the defaults come back after it."""
    yield ctx
    ctx.set_public_column_min(0)
    ctx.set_prove_batch_limit(0)


@pytest.fixture(scope="module")
def synthetic(oracle):
    """2^11 steps, 200 declared public wires (201 boundary points), two witnesses of the one circuit, and the
    oracle's proof of each."""
    import synth_r1cs
    r1, wt = synth_r1cs.for_steps(11, n_public=200)
    r1b, wt2 = synth_r1cs.for_steps(11, n_public=200, inputs=(9, 4))
    assert r1b == r1
    out = {"r1cs": r1, "wtns": [wt, wt2], "json": []}
    for w in (wt, wt2):
        tr = R.build_trace(R.read_r1cs(r1), R.read_witness(w))
        assert len(tr.public_first_indices) == 201 and len(tr.witness_trace) <= 1 << 11
        out["json"].append(R.mk_r1cs_proof_json(oracle, tr))
    return out


@pytest.fixture(scope="module")
def circuit(ctx, synthetic):
    from stark_amd.r1cs import R1csCircuit
    ctx.set_public_column_min(1)
    try:
        return R1csCircuit(ctx, synthetic["r1cs"])
    finally:
        ctx.set_public_column_min(0)


def _texts(proofs):
    return [p.to_json() for p in proofs]


def test_batch_equals_the_oracle(settings, synthetic, circuit):
    w, js = synthetic["wtns"], synthetic["json"]
    settings.set_public_column_min(1)
    assert _texts(circuit.prove_batch([w[0], w[1], w[0]])) == [js[0], js[1], js[0]]


def test_chunks_of_one_equal_the_oracle(settings, synthetic, circuit):
    w, js = synthetic["wtns"], synthetic["json"]
    settings.set_public_column_min(1)
    settings.set_prove_batch_limit(1)
    assert _texts(circuit.prove_batch([w[0], w[1], w[0]])) == [js[0], js[1], js[0]]


def test_chunks_of_two_equal_the_oracle(synthetic):
    """A limit with room for two proofs' working sets and not three (a fresh context, so that what one proof's
    chunk holds can be read off its resident bytes, as tests/test_gpu_prove_batch.py does)."""
    import stark_amd as S
    from stark_amd.r1cs import R1csCircuit
    w, js = synthetic["wtns"], synthetic["json"]
    c = S.Context(0)
    try:
        c.set_public_column_min(1)
        k = R1csCircuit(c, synthetic["r1cs"])
        assert k.prove(w[0]).to_json() == js[0]
        before = c.memory()["resident"]
        assert _texts(k.prove_batch([w[1]])) == [js[1]]
        one = c.memory()["resident"] - before
        assert one > 0
        c.set_prove_batch_limit(2 * one + one // 2)
        assert _texts(k.prove_batch([w[0], w[1], w[0]])) == [js[0], js[1], js[0]]
        assert c.memory()["resident"] - before < 3 * one  # no chunk of three was allocated
    finally:
        c.close()  # (before the circuit: the context releases the circuit's plan, test_circuit_freed_after_its_context)


def test_circuit_freed_after_its_context(synthetic):
    """A circuit that took the plan route may be freed after its context: the context's destruction releases the
    plan (its bytes leave with it), and the circuit's own free then finds nothing of the context's to touch."""
    import gc
    import stark_amd as S
    from stark_amd.r1cs import R1csCircuit
    w, js = synthetic["wtns"], synthetic["json"]
    c = S.Context(0)
    c.set_public_column_min(1)
    k = R1csCircuit(c, synthetic["r1cs"])
    before = c.memory()["resident"]
    assert _texts(k.prove_batch([w[0], w[1]])) == [js[0], js[1]]
    assert c.memory()["resident"] >= before + 32 * (201 + 201 + 2 * 256 * 3)  # the plan is among what came
    c.close()
    assert k.h
    del k
    gc.collect()
    again = S.Context(0)  # the heap and the device are sound: a fresh context proves the same
    try:
        again.set_public_column_min(1)
        k2 = R1csCircuit(again, synthetic["r1cs"])
        assert _texts(k2.prove_batch([w[1]])) == [js[1]]
    finally:
        again.close()


def test_bits_twice_under_the_default_threshold(ctx):
    """1,062 boundary points: the column route by default, six NTT levels in the plan."""
    from stark_amd.r1cs import R1csCircuit
    c = R1csCircuit(ctx, _read("bits", "r1cs"))
    wt = _read("bits", "wtns")
    for _ in range(2):
        got = c.prove_batch([wt, wt])
        assert [hashlib.sha256(p.to_json().encode()).hexdigest() for p in got] == [GOLDEN["bits"]["json_sha256"]] * 2


def _public_wire_off_by_one(wt: bytes, wire: int) -> bytes:
    n_wit = (len(wt) - (4 + 5 * 4 + 4 + 32 + 4 + 3 * 4)) // 32  # wtns v2: two section headers, a 32-B prime
    at = len(wt) - 32 * n_wit + 32 * wire
    v = (int.from_bytes(wt[at:at + 32], "little") + 1) % R.P
    return wt[:at] + v.to_bytes(32, "little") + wt[at + 32:]


def test_a_bad_public_wire_fails_its_proof_alone(settings, synthetic, circuit):
    from stark_amd import StarkError
    from stark_amd.r1cs import StarkProof
    w, js = synthetic["wtns"], synthetic["json"]
    settings.set_public_column_min(1)
    bad = _public_wire_off_by_one(w[1], 100)
    assert R.read_witness(bad)[100] != R.read_witness(w[1])[100]
    got = circuit.prove_batch([w[0], bad, w[1]], strict=False)
    assert isinstance(got[1], StarkError) and got[1].code == 8 and got[1].index == 1
    assert isinstance(got[0], StarkProof) and isinstance(got[2], StarkProof)
    assert [got[0].to_json(), got[2].to_json()] == [js[0], js[1]]


def test_alternating_calls_change_no_output(settings, synthetic, circuit):
    """prove_batch, a single prove and a second circuit's prove_batch on one context: the plan, the tree arena and
    the batch's buffers carry nothing from one call into the next."""
    from stark_amd.r1cs import R1csCircuit
    w, js = synthetic["wtns"], synthetic["json"]
    bits = R1csCircuit(settings, _read("bits", "r1cs"))
    bw = _read("bits", "wtns")
    for i in range(2):
        settings.set_public_column_min(1)
        assert _texts(circuit.prove_batch([w[i], w[1 - i]])) == [js[i], js[1 - i]]
        assert circuit.prove(w[i]).to_json() == js[i]
        settings.set_public_column_min(0)
        got = bits.prove_batch([bw, bw])
        assert [hashlib.sha256(p.to_json().encode()).hexdigest() for p in got] == [GOLDEN["bits"]["json_sha256"]] * 2
