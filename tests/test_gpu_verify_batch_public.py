"""R1csCircuit.verify_batch for public-input-heavy circuits: at or above the verification threshold every chain
proof's I2 comes from one application of the circuit's interpolation plan (csrc/poly.hip interp_plan_apply),
which reads the public wires' bytes out of the staged blocks.  Statuses and reason masks equal the single call's
and the basis-matrix route's, from texts and from handles, under the host's and the device's transcript."""
import os
import sys

import pytest

import r1cs as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "r1cs")
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

pytestmark = pytest.mark.gpu

SPOT = 0x20
HOST, DEVICE = 1, 2
MATRIX = 2000  # a threshold above both circuits' point counts: the basis-matrix launch forms I2


def _read(name, ext):
    with open(os.path.join(FIX, f"{name}.{ext}"), "rb") as f:
        return f.read()


def _public(r1, wt):
    h = R.read_r1cs(r1).header
    return [int.from_bytes(w, "little") for w in R.read_witness(wt)[:1 + h.n_public_inputs + h.n_public_outputs]]


@pytest.fixture(scope="module")
def bits(ctx):
    """1,062 boundary points: the plan route under the default threshold (1,024)."""
    from stark_amd.r1cs import R1csCircuit
    r1, wt = _read("bits", "r1cs"), _read("bits", "wtns")
    c = R1csCircuit(ctx, r1)
    pub = _public(r1, wt)
    return {"circuit": c, "pubs": [pub] * 2, "proofs": [c.prove(wt)] * 2, "min": 0}


@pytest.fixture(scope="module")
def synthetic(ctx):
    """2^11 steps, 201 boundary points, four proofs of two witnesses: the plan route with the threshold at 2."""
    import synth_r1cs
    from stark_amd.r1cs import R1csCircuit
    r1, wt = synth_r1cs.for_steps(11, n_public=200)
    _, wt2 = synth_r1cs.for_steps(11, n_public=200, inputs=(9, 4))
    c = R1csCircuit(ctx, r1)
    ws = [wt, wt2, wt2, wt]
    return {"circuit": c, "pubs": [_public(r1, w) for w in ws], "proofs": c.prove_batch(ws), "min": 2}


@pytest.fixture
def column_min(ctx):
    yield ctx.set_public_column_min
    ctx.set_public_column_min(0)
    ctx.set_verify_batch_transcript(0)


def _single(ctx, circuit, pub, proof):
    from stark_amd.verify import _wire_bytes
    js, pb = proof.to_json().encode(), _wire_bytes(pub)
    return ctx.lib.stark_verify_r1cs_circuit(ctx.h, circuit.h, pb, len(pb) // 32, js, len(js))


def _both_entries(ctx, f, pubs, m):
    """(status, reasons) per proof with the threshold at m, equal from handles and from texts and under both
    transcript settings."""
    from stark_amd.verify import verify_circuit_batch, verify_circuit_batch_proofs
    ctx.set_public_column_min(m)
    got = []
    for mode in (HOST, DEVICE):
        ctx.set_verify_batch_transcript(mode)
        got.append(verify_circuit_batch_proofs(ctx, f["circuit"], pubs, f["proofs"]))
        got.append(verify_circuit_batch(ctx, f["circuit"], pubs, [p.to_json() for p in f["proofs"]]))
    print(f"threshold {m}: {got}")
    assert got[0] == got[1] == got[2] == got[3]
    return got[0]


def _off_by_one(pub, wire):
    off = list(pub)
    off[wire] = (off[wire] + 1) % R.P
    return off


@pytest.mark.parametrize("which", ["bits", "synthetic"])
def test_accepts_on_every_route(ctx, column_min, request, which):
    f = request.getfixturevalue(which)
    n = len(f["proofs"])
    plan = _both_entries(ctx, f, f["pubs"], f["min"])
    matrix = _both_entries(ctx, f, f["pubs"], MATRIX)
    ctx.set_public_column_min(f["min"])
    singles = [_single(ctx, f["circuit"], p, h) for p, h in zip(f["pubs"], f["proofs"])]
    assert plan == matrix == [(0, 0)] * n
    assert singles == [0] * n


@pytest.mark.parametrize("which", ["bits", "synthetic"])
def test_a_bad_public_wire_fails_alike_on_every_route(ctx, column_min, request, which):
    """Only I2 can tell a public wire that is off by one: the proof fails its spot checks, its neighbours pass."""
    f = request.getfixturevalue(which)
    n = len(f["proofs"])
    wire = min(100, len(f["pubs"][0]) - 1)
    pubs = list(f["pubs"])
    pubs[1] = _off_by_one(pubs[1], wire)
    want = [(0, 0)] * n
    want[1] = (8, SPOT)
    plan = _both_entries(ctx, f, pubs, f["min"])
    matrix = _both_entries(ctx, f, pubs, MATRIX)
    ctx.set_public_column_min(f["min"])
    singles = [_single(ctx, f["circuit"], p, h) for p, h in zip(pubs, f["proofs"])]
    assert plan == matrix == want
    assert singles == [st for st, _ in want]


@pytest.mark.parametrize("which", ["bits", "synthetic"])
def test_an_unreduced_public_wire_gets_the_single_calls_verdict(ctx, column_min, request, which):
    """A public wire given as v + p (below 2^256): the plan's first product reduces the bytes as they are."""
    f = request.getfixturevalue(which)
    pubs = list(f["pubs"])
    wire = min(100, len(pubs[0]) - 1)
    unreduced = list(pubs[0])
    unreduced[wire] += R.P
    assert unreduced[wire] < 1 << 256
    pubs[0] = unreduced
    plan = _both_entries(ctx, f, pubs, f["min"])
    matrix = _both_entries(ctx, f, pubs, MATRIX)
    ctx.set_public_column_min(f["min"])
    singles = [_single(ctx, f["circuit"], p, h) for p, h in zip(pubs, f["proofs"])]
    print(f"single {singles}")
    assert [st for st, _ in plan] == singles
    assert plan == matrix


def test_the_second_call_reuses_the_plan(synthetic):
    """A fresh context: the first call on the plan route builds the circuit's plan, the second allocates nothing."""
    import stark_amd as S
    from stark_amd.r1cs import R1csCircuit
    import synth_r1cs
    r1, _ = synth_r1cs.for_steps(11, n_public=200)
    c = S.Context(0)
    try:
        k = R1csCircuit(c, r1)
        texts = [p.to_json() for p in synthetic["proofs"]]
        c.set_public_column_min(MATRIX)
        assert k.verify_batch(synthetic["pubs"], texts) == [(0, 0)] * 4
        before = c.memory()["resident"]
        c.set_public_column_min(2)
        assert k.verify_batch(synthetic["pubs"], texts) == [(0, 0)] * 4
        first = c.memory()["resident"]
        assert first >= before + 32 * (201 + 201 + 2 * 256 * 3)  # the plan's points, 1 / Z', three levels
        assert k.verify_batch(synthetic["pubs"], texts) == [(0, 0)] * 4
        assert c.memory()["resident"] == first
    finally:
        c.close()
