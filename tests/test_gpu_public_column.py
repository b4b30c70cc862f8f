"""The column route for public-input-heavy circuits (stark_ctx_set_public_column_min): Zb2 and I2 extended
from their coefficients (the subproduct tree of csrc/poly.hip) instead of a product / Horner loop over the
public points at every point of the domain, and the verifier's interpolant from the same tree.  The
arithmetic is exact, so every proof is the Horner route's byte for byte, and every verdict the same."""
import hashlib
import json
import os
import struct
import sys

import pytest

import r1cs as R
from oracle import to_limbs

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "r1cs")
GOLDEN = json.load(open(os.path.join(HERE, "golden", "r1cs_proofs.json")))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

pytestmark = pytest.mark.gpu

COLUMN, HORNER = 1, (1 << 64) - 1  # every circuit with a public point | SIZE_MAX: never
ROUTES = [pytest.param(COLUMN, id="column"), pytest.param(HORNER, id="horner")]


def _read(name, ext):
    with open(os.path.join(FIX, f"{name}.{ext}"), "rb") as f:
        return f.read()


def _sha(proof):
    return hashlib.sha256(proof.to_json().encode()).hexdigest()


@pytest.fixture
def route(ctx):
    """Sets the context's threshold for one test; the default comes back after it."""
    yield ctx.set_public_column_min
    ctx.set_public_column_min(0)


@pytest.fixture(scope="module")
def synthetic(oracle):
    """2^11 steps, 200 declared public wires (201 boundary points), two witnesses of the one circuit, and
    the oracle's proof of each."""
    import synth_r1cs
    r1, wt = synth_r1cs.for_steps(11, n_public=200)
    r1b, wt2 = synth_r1cs.for_steps(11, n_public=200, inputs=(9, 4))
    assert r1b == r1
    out = {"r1cs": r1, "wtns": [wt, wt2], "trace": [], "json": []}
    for w in (wt, wt2):
        tr = R.build_trace(R.read_r1cs(r1), R.read_witness(w))
        assert len(tr.public_first_indices) == 201 and len(tr.witness_trace) <= 1 << 11
        out["trace"].append(tr)
        out["json"].append(R.mk_r1cs_proof_json(oracle, tr))
    return out


def test_generator_default_is_unchanged():
    """n_public is a keyword: without it the generator's bytes are what large_digests.json was made from."""
    import synth_r1cs
    r1, wt = synth_r1cs.for_steps(8)
    assert hashlib.sha256(r1).hexdigest() == "aa7be869a71b4e184e460944f8b51b0d74342c1ad9668729161950668159ac96"
    assert hashlib.sha256(wt).hexdigest() == "706e80429fd77d6fe8893df1b1c56841d21583d27a552d4473d27aad95f00cac"
    assert synth_r1cs.for_steps(8, n_public=2) == (r1, wt)


@pytest.mark.parametrize("m", ROUTES)
@pytest.mark.parametrize("name", list(GOLDEN))
def test_golden_digests_on_both_routes(ctx, route, name, m):
    """The device trace entry, the host trace entry and a prepared circuit (built under the same setting:
    its 1 / Zb2 takes the same route), twice."""
    from stark_amd.r1cs import R1csCircuit, prove_with_witness, prove_with_witness_host_trace
    r1, wt = _read(name, "r1cs"), _read(name, "wtns")
    want = GOLDEN[name]["json_sha256"]
    route(m)
    assert _sha(prove_with_witness(ctx, r1, wt)) == want
    assert _sha(prove_with_witness_host_trace(ctx, r1, wt)) == want
    c = R1csCircuit(ctx, r1)
    for _ in range(2):
        assert _sha(c.prove(wt)) == want


@pytest.fixture(scope="module")
def golden_proofs(ctx):
    from stark_amd.r1cs import prove_with_witness
    out = {}
    for name in GOLDEN:
        js = prove_with_witness(ctx, _read(name, "r1cs"), _read(name, "wtns")).to_json()
        assert hashlib.sha256(js.encode()).hexdigest() == GOLDEN[name]["json_sha256"]
        out[name] = js
    return out


@pytest.mark.parametrize("m", ROUTES)
@pytest.mark.parametrize("name", list(GOLDEN))
def test_verifier_on_both_routes(ctx, route, golden_proofs, name, m):
    """verify_with_wtns accepts the golden proof, and rejects it against a witness whose public wire 1
    differs (its boundary value: B2's check, verify.rs:227-233)."""
    from stark_amd.verify import verify_with_wtns
    r1, wt = _read(name, "r1cs"), _read(name, "wtns")
    route(m)
    assert verify_with_wtns(ctx, r1, wt, golden_proofs[name])
    bad = bytearray(wt)
    n_wit = struct.unpack_from("<I", bad, 4 + 5 * 4 + 4 + 32)[0]  # wtns v2: header section, 32-B prime
    bad[len(bad) - 32 * n_wit + 32] ^= 1                          # witness value 1
    with pytest.raises(AssertionError):
        verify_with_wtns(ctx, r1, bytes(bad), golden_proofs[name])
    assert verify_with_wtns(ctx, r1, wt, golden_proofs[name])


@pytest.mark.parametrize("m", ROUTES)
def test_synthetic_200_public_wires_matches_oracle(ctx, route, synthetic, m):
    from stark_amd.r1cs import prove_with_witness, prove_with_witness_host_trace
    from stark_amd.verify import verify_with_wtns
    route(m)
    js = prove_with_witness(ctx, synthetic["r1cs"], synthetic["wtns"][0]).to_json()
    assert js == synthetic["json"][0]
    assert prove_with_witness_host_trace(ctx, synthetic["r1cs"], synthetic["wtns"][0]).to_json() == js
    assert verify_with_wtns(ctx, synthetic["r1cs"], synthetic["wtns"][0], js)
    with pytest.raises(AssertionError):  # the other witness has other public wires
        verify_with_wtns(ctx, synthetic["r1cs"], synthetic["wtns"][1], js)


@pytest.mark.parametrize("m", ROUTES)
def test_synthetic_prepared_circuit_two_witnesses(ctx, route, synthetic, m):
    """One prepared circuit (its 1 / Zb2 built once), each witness' I2 of its own."""
    from stark_amd.r1cs import R1csCircuit
    route(m)
    c = R1csCircuit(ctx, synthetic["r1cs"])
    for k in (0, 1, 0):
        assert c.prove(synthetic["wtns"][k]).to_json() == synthetic["json"][k]


def test_prepared_circuit_and_proof_on_different_routes(ctx, route, synthetic):
    """A circuit keeps the 1 / Zb2 it was built with; I2 follows the setting at the proof: any mix agrees."""
    from stark_amd.r1cs import R1csCircuit
    route(COLUMN)
    c = R1csCircuit(ctx, synthetic["r1cs"])
    route(HORNER)
    h = R1csCircuit(ctx, synthetic["r1cs"])
    assert c.prove(synthetic["wtns"][1]).to_json() == synthetic["json"][1]
    route(COLUMN)
    assert h.prove(synthetic["wtns"][1]).to_json() == synthetic["json"][1]


def _mk(ctx, tr, **over):
    from stark_amd.r1cs import mk_r1cs_proof
    a = dict(witness_trace=tr.witness_trace, computational_trace=tr.computational_trace,
             public_wires=tr.public_wires)
    a.update(over)
    return mk_r1cs_proof(ctx, to_limbs(a["witness_trace"]), to_limbs(a["computational_trace"]),
                         to_limbs(a["public_wires"]), tr.public_first_indices, tr.permuted_indices,
                         to_limbs(tr.coefficients), to_limbs(tr.flag0), to_limbs(tr.flag1), to_limbs(tr.flag2),
                         tr.n_constraints, tr.n_wires)


def test_column_route_error_bits(ctx, route, synthetic):
    """Under the column route a public wire off by one breaks B2 (utils.rs:477-499) and a trace that does not
    satisfy the constraints breaks D (utils.rs:379-418): STARK_ERR_CHECK (8), as on the Horner route."""
    from stark_amd import StarkError
    tr = synthetic["trace"][0]
    route(COLUMN)
    assert _mk(ctx, tr).to_json() == synthetic["json"][0]
    for wire in (1, 100, 200):
        pw = list(tr.public_wires)
        pw[wire] = (pw[wire] + 1) % R.P
        with pytest.raises(StarkError) as e:
            _mk(ctx, tr, public_wires=pw)
        assert e.value.code == 8
    ct = list(tr.computational_trace)
    ct[3] = (ct[3] + 1) % R.P
    with pytest.raises(StarkError) as e:
        _mk(ctx, tr, computational_trace=ct)
    assert e.value.code == 8
    assert _mk(ctx, tr).to_json() == synthetic["json"][0]  # the context is still good


def test_threshold_selects_the_route(synthetic):
    """The tree's arena is the column route's alone: a context holds it only once a proof at or above its
    threshold ran (201 boundary points here), and 0 gives the default back."""
    import stark_amd as S
    from stark_amd.r1cs import prove_with_witness
    c = S.Context(0)
    try:
        resident = []
        for m in (HORNER, 202, 201):
            c.set_public_column_min(m)
            assert prove_with_witness(c, synthetic["r1cs"], synthetic["wtns"][0]).to_json() == synthetic["json"][0]
            resident.append(c.memory()["resident"])
        assert resident[0] == resident[1] < resident[2]
        tree = resident[2] - resident[1]
        assert tree >= 256 * 32 * 7  # 201 points pad to 256: the top and three levels of transforms
    finally:
        c.close()


def test_alternating_routes_leave_no_state(ctx, route, synthetic):
    """Proofs alternating the two routes, and two circuits, on one context: nothing leaks through the
    tree's arena or the columns' slots."""
    from stark_amd.r1cs import prove_with_witness
    bits = _read("bits", "r1cs"), _read("bits", "wtns")
    for i in range(4):
        route(COLUMN if i % 2 == 0 else HORNER)
        assert prove_with_witness(ctx, synthetic["r1cs"], synthetic["wtns"][i % 2]).to_json() == synthetic["json"][i % 2]
        assert _sha(prove_with_witness(ctx, *bits)) == GOLDEN["bits"]["json_sha256"]
