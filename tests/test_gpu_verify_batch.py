"""stark_verify_r1cs_circuit_batch / R1csCircuit.verify_batch: B proofs of one prepared circuit checked on the
GPU through one chain of launches (csrc/verify_batch.hip).

Bar: statuses[b] is what stark_verify_r1cs_circuit returns for the same public wires and text, on the same
context -- every status here is compared with that call as well as with the expected value -- and reasons[b]
names the classes of checks that failed, each evaluated on its own.  An accepted proof is the strong check of
the kernels' arithmetic: any wrong hash, cubic or equality rejects it.
"""
import copy
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

PUBLIC_ONE, FRI_PATHS, FRI_ROWS, FRI_LAST, OPENING_PATHS, SPOT, SINGLE = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40


def _read(name, ext):
    with open(os.path.join(FIX, f"{name}.{ext}"), "rb") as f:
        return f.read()


def _public(r1, wt):
    h = R.read_r1cs(r1).header
    return [int.from_bytes(w, "little") for w in R.read_witness(wt)[:1 + h.n_public_inputs + h.n_public_outputs]]


class _Circuits:
    """Prepared circuits with one proof each, made on first use and kept for the module."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.made = {}

    def __call__(self, name):
        if name not in self.made:
            from stark_amd.r1cs import R1csCircuit
            r1, wt = _read(name, "r1cs"), _read(name, "wtns")
            c = R1csCircuit(self.ctx, r1)
            self.made[name] = {"circuit": c, "pub": _public(r1, wt), "js": c.prove(wt).to_json(), "wt": wt}
        return self.made[name]


@pytest.fixture(scope="module")
def fixtures(ctx):
    return _Circuits(ctx)


@pytest.fixture(scope="module")
def synth10(ctx):
    """A synthetic 2^10-step circuit (precision 2^13, four Middle layers) with 7 distinct witnesses, proved as one
    batch: distinct positions, indices and public wires per proof."""
    import synth_r1cs
    from stark_amd.r1cs import R1csCircuit
    r1, _ = synth_r1cs.for_steps(10)
    wts = [synth_r1cs.for_steps(10, inputs=(1000 + 17 * k, R.P - 5 - k))[1] for k in range(7)]
    c = R1csCircuit(ctx, r1)
    return {"circuit": c, "pubs": [_public(r1, w) for w in wts], "js": [p.to_json() for p in c.prove_batch(wts)]}


def _single(ctx, circuit, pub, proof):
    """stark_verify_r1cs_circuit's status for one pair (None entries are the batch's null pointers)."""
    from stark_amd.verify import _json_bytes, _wire_bytes
    if pub is None or proof is None:
        return 3
    js, pb = _json_bytes(proof), _wire_bytes(pub)
    return ctx.lib.stark_verify_r1cs_circuit(ctx.h, circuit.h, pb, len(pb) // 32, js, len(js))


def _batch(ctx, circuit, pubs, proofs):
    """verify_batch's result, each status held against the single call's on the same context."""
    got = circuit.verify_batch(pubs, proofs)
    assert len(got) == len(proofs)
    for b, (st, why) in enumerate(got):
        assert st == _single(ctx, circuit, pubs[b], proofs[b]), f"proof {b}: batch status {st} (reasons {why:#x})"
        assert (why == 0) == (st == 0) or st == 3, f"proof {b}: status {st}, reasons {why:#x}"
    return got


# ---- accepts ------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,batch", [("compute", 1), ("compute", 2), ("compute", 5), ("poseidon3_test", 3),
                                        ("pedersen_test", 2), ("bits", 2)])
def test_accepts_fixture_proofs(ctx, fixtures, name, batch):
    """compute: precision 128, one Middle layer, depth-7 and depth-5 trees (the smallest shape); pedersen: six
    layers; bits: 1,062 public points (I2 interpolated on the GPU, the long Zb2 and I2 loops of the spot kernel)."""
    f = fixtures(name)
    got = _batch(ctx, f["circuit"], [f["pub"]] * batch, [f["js"]] * batch)
    assert got == [(0, 0)] * batch


def test_accepts_distinct_witnesses(ctx, synth10):
    got = _batch(ctx, synth10["circuit"], synth10["pubs"], synth10["js"])
    assert got == [(0, 0)] * 7


# ---- rejects, by class --------------------------------------------------------------------------------


def _tampered(js):
    """(what, proof dict, expected reasons, exactly) -- tests/test_gpu_verify.py's tamperings and a FRI
    polynomial leaf."""
    p = json.loads(js)
    out = []

    def t(what, f, why, exactly=True):
        q = copy.deepcopy(p)
        f(q)
        out.append((what, q, why, exactly))

    def flip(a, i, bit=1):
        a[i] ^= bit
    t("main leaf", lambda q: flip(q["main_branches"][0]["leaf"], 40), OPENING_PATHS | SPOT)
    t("main node", lambda q: flip(q["main_branches"][7]["nodes"][2], 0), OPENING_PATHS)
    t("lcomb leaf", lambda q: flip(q["linear_comb_branches"][3]["leaf"], 0, 4), OPENING_PATHS | SPOT)
    t("m_root", lambda q: flip(q["m_root"], 5), OPENING_PATHS | SPOT, False)
    t("a_root", lambda q: flip(q["a_root"], 0), SPOT)
    t("l_root", lambda q: flip(q["l_root"], 31), OPENING_PATHS | FRI_PATHS, False)
    t("fri column", lambda q: flip(q["fri_proof"][0]["Middle"]["column_branches"][1]["leaf"], 3), FRI_PATHS | FRI_ROWS)
    t("fri poly", lambda q: flip(q["fri_proof"][0]["Middle"]["poly_branches"][9]["leaf"], 2), FRI_PATHS | FRI_ROWS)
    t("fri last", lambda q: flip(q["fri_proof"][-1]["Last"]["last"][2], 0), FRI_LAST)
    return out


def _reject_batch(ctx, circuit, pub, js):
    cases = _tampered(js)
    pubs = [pub] + [pub] * len(cases)
    proofs = [js] + [q for _, q, _, _ in cases]
    want = [("good first", 0, True)] + [(w, why, ex) for w, _, why, ex in cases]
    off = list(pub)
    off[1] = (off[1] + 1) % R.P
    pubs += [off, [2] + list(pub[1:]), pub]
    proofs += [js, js, js]
    want += [("public wire 1 off by one", SPOT, True), ("public wire 0 = 2", PUBLIC_ONE, True), ("good last", 0, True)]
    got = _batch(ctx, circuit, pubs, proofs)
    for (what, why, exactly), (st, reasons) in zip(want, got):
        assert st == (8 if why else 0), f"{what}: status {st}"
        if exactly:
            assert reasons == why, f"{what}: reasons {reasons:#x}, expected exactly {why:#x}"
        else:
            assert reasons & why == why, f"{what}: reasons {reasons:#x}, expected at least {why:#x}"
            assert reasons & (PUBLIC_ONE | SINGLE) == 0, f"{what}: reasons {reasons:#x}"


def test_rejects_by_class_compute(ctx, fixtures):
    f = fixtures("compute")
    _reject_batch(ctx, f["circuit"], f["pub"], f["js"])


def test_rejects_by_class_synthetic(ctx, synth10):
    _reject_batch(ctx, synth10["circuit"], synth10["pubs"][3], synth10["js"][3])


# ---- fallback and isolation ---------------------------------------------------------------------------


def test_fallback_and_isolation(ctx, fixtures):
    """Proofs of another shape go through the single-proof verifier, unparsable ones are refused, and neither
    changes a neighbour's status."""
    f = fixtures("compute")
    js, pub, c = f["js"], f["pub"], f["circuit"]
    other = fixtures("poseidon3_test")["js"]
    short = json.loads(js)
    short["main_branches"][3]["nodes"][2] = [1]  # a short digest
    short = json.dumps(short, separators=(",", ":"))
    spaced = js.replace(",", ", ").replace(":", " : ").replace("[", "[ ")
    proofs = [js, other, js[:len(js) // 2], "{}", short, spaced, None]
    pubs = [pub] * len(proofs)
    got = _batch(ctx, c, pubs, proofs)
    assert got[0] == (0, 0)
    assert got[1] == (8, SINGLE)
    assert got[2][0] == 3 and got[3][0] == 3 and got[4][0] == 3 and got[6][0] == 3
    assert got[5] == (0, 0)
    # statuses = NULL: the first status in batch order that is not STARK_OK
    from stark_amd.verify import _json_bytes, _wire_bytes
    n = len(proofs)
    texts = [None if p is None else _json_bytes(p) for p in proofs]
    pb = _wire_bytes(pub)
    fn = ctx.lib.stark_verify_r1cs_circuit_batch

    def call(order):
        t = [texts[i] for i in order]
        return fn(ctx.h, c.h, (ctypes.c_char_p * len(t))(*[pb] * len(t)), len(pb) // 32, (ctypes.c_char_p * len(t))(*t),
                  (ctypes.c_size_t * len(t))(*[0 if x is None else len(x) for x in t]), len(t), None, None)
    assert call(range(n)) == 8
    assert call([0, 5, 3, 1]) == 3
    assert call([0, 5, 0]) == 0
    # a wrong count of public wires is each proof's STARK_ERR_BAD_ARG, as the single call's
    assert _batch(ctx, c, [list(pub) + [5]] * 2, [js, js]) == [(3, 0), (3, 0)]


# ---- chunking -----------------------------------------------------------------------------------------


def test_chunks_and_resident_bytes(ctx, fixtures, synth10):
    c, pubs, proofs = synth10["circuit"], list(synth10["pubs"][:5]), list(synth10["js"][:5])
    bad = json.loads(proofs[2])
    bad["linear_comb_branches"][0]["leaf"][1] ^= 1
    proofs[2] = bad
    whole = _batch(ctx, c, pubs, proofs)
    assert [st for st, _ in whole] == [0, 0, 8, 0, 0] and whole[2][1] == OPENING_PATHS | SPOT
    try:
        ctx.set_verify_batch_limit(1)  # below one proof: chunks of one
        assert c.verify_batch(pubs, proofs) == whole
        small = ctx.memory()["resident"]
        ctx.set_verify_batch_limit(0)  # the default again: one chunk
        assert c.verify_batch(pubs, proofs) == whole
        held = ctx.memory()["resident"]
        assert held > small  # (the batch's buffers are counted, and five proofs take more than one)
        for _ in range(10):
            assert c.verify_batch(pubs, proofs) == whole
        assert ctx.memory()["resident"] == held
        ctx.set_verify_batch_limit(1)  # lowering the cap below what they hold frees them
        assert ctx.memory()["resident"] < small
    finally:
        ctx.set_verify_batch_limit(0)


# ---- after the batch ----------------------------------------------------------------------------------


def test_context_intact_after_batches(ctx, fixtures):
    """The context's buffers and stream order after batches: a single verification and a proof still succeed,
    the proof with the golden digest."""
    from stark_amd.verify import verify_circuit
    f = fixtures("compute")
    assert _batch(ctx, f["circuit"], [f["pub"]] * 3, [f["js"]] * 3) == [(0, 0)] * 3
    assert verify_circuit(ctx, f["circuit"], f["pub"], f["js"])
    js = f["circuit"].prove(f["wt"]).to_json()
    assert hashlib.sha256(js.encode()).hexdigest() == GOLDEN["compute"]["json_sha256"]
