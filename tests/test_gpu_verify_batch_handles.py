"""stark_verify_r1cs_circuit_batch_proofs / R1csCircuit.verify_batch on StarkProof handles, with the batch's
transcript derived on the host and on the device (csrc/verify_batch.hip).

Bar, held by one helper for every case and under both transcript modes: the handle entry's (status, reasons)
equal stark_verify_r1cs_circuit_batch's for the handles' own text; each status equals
stark_verify_r1cs_circuit's; and the JSON entry with the device's transcript equals itself with the host's.  An
accepted proof is the strong check of the derived indices, challenges and records: any wrong one rejects it.
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
HOST, DEVICE = 1, 2


def _read(name, ext):
    with open(os.path.join(FIX, f"{name}.{ext}"), "rb") as f:
        return f.read()


def _public(r1, wt):
    h = R.read_r1cs(r1).header
    return [int.from_bytes(w, "little") for w in R.read_witness(wt)[:1 + h.n_public_inputs + h.n_public_outputs]]


class _Circuits:
    """Prepared circuits with one proof handle each, made on first use and kept for the module."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.made = {}

    def __call__(self, name):
        if name not in self.made:
            from stark_amd.r1cs import R1csCircuit
            r1, wt = _read(name, "r1cs"), _read(name, "wtns")
            c = R1csCircuit(self.ctx, r1)
            self.made[name] = {"circuit": c, "pub": _public(r1, wt), "proof": c.prove(wt), "wt": wt}
        return self.made[name]


@pytest.fixture(scope="module")
def fixtures(ctx):
    return _Circuits(ctx)


@pytest.fixture(scope="module")
def synth10(ctx):
    """tests/test_gpu_verify_batch.py's synthetic 2^10-step circuit (precision 2^13, four Middle layers) with 7
    distinct witnesses proved as one batch: every proof has its own roots, so every derived index and constant
    differs from one workgroup of the transcript kernel to the next."""
    import synth_r1cs
    from stark_amd.r1cs import R1csCircuit
    r1, _ = synth_r1cs.for_steps(10)
    wts = [synth_r1cs.for_steps(10, inputs=(1000 + 17 * k, R.P - 5 - k))[1] for k in range(7)]
    c = R1csCircuit(ctx, r1)
    return {"circuit": c, "pubs": [_public(r1, w) for w in wts], "proofs": c.prove_batch(wts)}


def _single(ctx, circuit, pub, text):
    from stark_amd.verify import _wire_bytes
    if pub is None or text is None:
        return 3
    js, pb = text.encode(), _wire_bytes(pub)
    return ctx.lib.stark_verify_r1cs_circuit(ctx.h, circuit.h, pb, len(pb) // 32, js, len(js))


def _check(ctx, circuit, pubs, handles):
    """The handle entry's result under the host's transcript, after holding the bar of the module's docstring
    under both modes."""
    from stark_amd.verify import verify_circuit_batch, verify_circuit_batch_proofs
    texts = [None if h is None else h.to_json() for h in handles]
    singles = [_single(ctx, circuit, p, t) for p, t in zip(pubs, texts)]
    got = {}
    try:
        for mode in (HOST, DEVICE):
            ctx.set_verify_batch_transcript(mode)
            by_handle = verify_circuit_batch_proofs(ctx, circuit, pubs, handles)
            by_text = verify_circuit_batch(ctx, circuit, pubs, texts)
            print(f"transcript {mode}: handles {by_handle} texts {by_text} single {singles}")
            assert by_handle == by_text, f"transcript {mode}"
            assert [st for st, _ in by_handle] == singles, f"transcript {mode}"
            for st, why in by_handle:
                assert (why == 0) == (st == 0) or st == 3
            got[mode] = (by_handle, by_text)
        assert got[DEVICE][1] == got[HOST][1]
        assert got[DEVICE][0] == got[HOST][0]
    finally:
        ctx.set_verify_batch_transcript(0)
    return got[HOST][0]


# ---- accepts ------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,batch", [("compute", 1), ("compute", 2), ("compute", 5), ("poseidon3_test", 3),
                                        ("pedersen_test", 2), ("bits", 2)])
def test_accepts_fixture_handles(ctx, fixtures, name, batch):
    """Handles straight from prove.  compute: the smallest shape (precision 128, one Middle layer, 40 rows: less
    than a wave); pedersen: six layers; bits: 1,062 public points, I2 by the per-proof route."""
    f = fixtures(name)
    assert _check(ctx, f["circuit"], [f["pub"]] * batch, [f["proof"]] * batch) == [(0, 0)] * batch


def test_accepts_distinct_witnesses(ctx, synth10):
    """Handles straight from prove_batch, each with its own roots; through R1csCircuit.verify_batch as well."""
    c = synth10["circuit"]
    assert _check(ctx, c, synth10["pubs"], synth10["proofs"]) == [(0, 0)] * 7
    assert c.verify_batch(synth10["pubs"], synth10["proofs"]) == [(0, 0)] * 7
    from stark_amd import StarkError
    with pytest.raises(StarkError):
        c.verify_batch(synth10["pubs"][:2], [synth10["proofs"][0], synth10["proofs"][1].to_json()])


# ---- both I2 routes -----------------------------------------------------------------------------------


def _off_by_one(pub):
    off = list(pub)
    off[1] = (off[1] + 1) % R.P
    return off


def test_interp2_routes_agree(ctx, fixtures, synth10):
    """I2 by the basis-matrix launch (the default below the threshold) against the per-proof route
    (set_public_column_min(2): verify_interp2 for every proof), on the same inputs: accepted proofs, and one whose
    public wire 1 is off by one, which only I2 can tell."""
    f = fixtures("compute")
    cases = [(f["circuit"], [f["pub"], _off_by_one(f["pub"]), f["pub"]], [f["proof"]] * 3, [(0, 0), (8, SPOT), (0, 0)]),
             (synth10["circuit"], synth10["pubs"][:3] + [_off_by_one(synth10["pubs"][3])], synth10["proofs"][:4],
              [(0, 0)] * 3 + [(8, SPOT)])]
    for c, pubs, proofs, want in cases:
        matrix = _check(ctx, c, pubs, proofs)
        try:
            ctx.set_public_column_min(2)
            per_proof = _check(ctx, c, pubs, proofs)
        finally:
            ctx.set_public_column_min(0)
        assert matrix == per_proof == want


def test_interp2_matrix_with_many_points(ctx, fixtures):
    """bits with the threshold above its 1,062 points: the matrix kernel runs 1,062 terms per lane and 1,062 lanes
    per proof (its 36 MB matrix is under a quarter of the default cap), against the per-proof route."""
    f = fixtures("bits")
    pubs, proofs = [f["pub"], _off_by_one(f["pub"])], [f["proof"]] * 2
    per_proof = _check(ctx, f["circuit"], pubs, proofs)
    try:
        ctx.set_public_column_min(2000)
        matrix = _check(ctx, f["circuit"], pubs, proofs)
    finally:
        ctx.set_public_column_min(0)
    assert matrix == per_proof == [(0, 0), (8, SPOT)]


# ---- rejects, by class, through from_parts ------------------------------------------------------------


def _flip(b: bytes, i: int, bit: int = 1) -> bytes:
    a = bytearray(b)
    a[i] ^= bit
    return bytes(a)


def _tampered_parts(parts):
    """(what, parts, expected reasons, exactly): tests/test_gpu_verify_batch.py::_tampered's table applied to the
    parts, then a leaf of opening 0 and of the last opening of every class (main, L, each layer's column and
    polynomial openings: the first and the last record of each class)."""
    out = []

    def t(what, f, why, exactly=True):
        q = copy.deepcopy(parts)
        f(q)
        out.append((what, q, why, exactly))

    def leaf(q, path, opening, byte, bit=1):
        b = q
        for k in path:
            b = b[k]
        b["leaves"] = _flip(b["leaves"], opening * b["leaf_len"] + byte, bit)

    def node(q, path, opening, level, byte):
        b = q
        for k in path:
            b = b[k]
        b["nodes"] = _flip(b["nodes"], (opening * b["depth"] + level) * 32 + byte)

    def root(q, key, byte):
        q[key] = _flip(q[key], byte)

    def last(q, value, byte):
        q["last"] = _flip(q["last"], 32 * value + byte)
    t("main leaf", lambda q: leaf(q, ["main"], 0, 40), OPENING_PATHS | SPOT)
    t("main node", lambda q: node(q, ["main"], 7, 2, 0), OPENING_PATHS)
    t("lcomb leaf", lambda q: leaf(q, ["lcomb"], 3, 0, 4), OPENING_PATHS | SPOT)
    t("m_root", lambda q: root(q, "m_root", 5), OPENING_PATHS | SPOT, False)
    t("a_root", lambda q: root(q, "a_root", 0), SPOT)
    t("l_root", lambda q: root(q, "l_root", 31), OPENING_PATHS | FRI_PATHS, False)
    t("fri column", lambda q: leaf(q, ["layers", 0, "column"], 1, 3), FRI_PATHS | FRI_ROWS)
    t("fri poly", lambda q: leaf(q, ["layers", 0, "poly"], 9, 2), FRI_PATHS | FRI_ROWS)
    t("fri last", lambda q: last(q, 2, 0), FRI_LAST)
    classes = [(["main"], OPENING_PATHS), (["lcomb"], OPENING_PATHS)]
    for l in range(len(parts["layers"])):
        classes += [(["layers", l, "column"], FRI_PATHS), (["layers", l, "poly"], FRI_PATHS)]
    for path, why in classes:
        b = parts
        for k in path:
            b = b[k]
        for opening in (0, b["k"] - 1):
            t(f"{path} opening {opening}", lambda q, path=path, opening=opening: leaf(q, path, opening, 1), why, False)
    return out


def _reject_batch(ctx, circuit, pub, proof):
    from stark_amd.r1cs import StarkProof
    parts = proof.parts()
    cases = _tampered_parts(parts)
    bad = [StarkProof.from_parts(q) for _, q, _, _ in cases]
    want = [(w, why, ex) for w, _, why, ex in cases]
    # Chunks of two: a proof stages its openings' bytes, 32 B per record and a few hundred bytes more, between
    # 1.0 and 1.25 times the openings' bytes, so 2.5 times those bytes hold two proofs and not three.  In the first
    # order a tampered proof at an even place of `bad` is a chunk's last slot and one at an odd place its first;
    # one more good proof in front swaps them.
    opened = sum(len(b[k]) for b in [parts["main"], parts["lcomb"]] +
                 [x[p] for x in parts["layers"] for p in ("column", "poly")] for k in ("leaves", "nodes"))
    try:
        ctx.set_verify_batch_limit(int(2.5 * opened))
        for lead in (1, 2):
            proofs = [proof] * lead + bad + [proof] * 3
            pubs = [pub] * (lead + len(bad)) + [_off_by_one(pub), [2] + list(pub[1:]), pub]
            rows = [("good first", 0, True)] * lead + want + [("public wire 1 off by one", SPOT, True),
                                                             ("public wire 0 = 2", PUBLIC_ONE, True),
                                                             ("good last", 0, True)]
            got = _check(ctx, circuit, pubs, proofs)
            for (what, why, exactly), (st, reasons) in zip(rows, got):
                assert st == (8 if why else 0), f"{what}: status {st}"
                if exactly:
                    assert reasons == why, f"{what}: reasons {reasons:#x}, expected exactly {why:#x}"
                else:
                    assert reasons & why == why, f"{what}: reasons {reasons:#x}, expected at least {why:#x}"
                    assert reasons & (PUBLIC_ONE | SINGLE) == 0, f"{what}: reasons {reasons:#x}"
    finally:
        ctx.set_verify_batch_limit(0)


def test_rejects_by_class_compute(ctx, fixtures):
    f = fixtures("compute")
    _reject_batch(ctx, f["circuit"], f["pub"], f["proof"])


def test_rejects_by_class_synthetic(ctx, synth10):
    _reject_batch(ctx, synth10["circuit"], synth10["pubs"][3], synth10["proofs"][3])


# ---- untrusted handles --------------------------------------------------------------------------------


def test_untrusted_handles(ctx, fixtures):
    """A handle is input like any other: one of another circuit or of another structure leaves the chain for the
    single-proof verifier, a missing one is refused, and none changes a neighbour's status.  A handle made by
    from_parts holds none of the prover's index vectors and verifies all the same: the verifier reads none."""
    from stark_amd.r1cs import StarkProof
    f = fixtures("compute")
    good, pub, c = f["proof"], f["pub"], f["circuit"]
    other = fixtures("poseidon3_test")["proof"]
    parts = good.parts()
    rebuilt = StarkProof.from_parts(parts)
    short = copy.deepcopy(parts)  # every main path one node short
    d = short["main"]["depth"]
    short["main"]["nodes"] = b"".join(short["main"]["nodes"][32 * d * i:32 * (d * i + d - 1)]
                                       for i in range(short["main"]["k"]))
    short["main"]["depth"] = d - 1
    fewer = copy.deepcopy(parts)  # 79 L openings
    fewer["lcomb"]["k"] = 79
    fewer["lcomb"]["leaves"] = fewer["lcomb"]["leaves"][:79 * 32]
    fewer["lcomb"]["nodes"] = fewer["lcomb"]["nodes"][:79 * 32 * fewer["lcomb"]["depth"]]
    no_last = dict(parts, last=b"")
    handles = [good, other, StarkProof.from_parts(short), rebuilt, StarkProof.from_parts(fewer),
               StarkProof.from_parts(no_last), None, good]
    got = _check(ctx, c, [pub] * len(handles), handles)
    assert got[0] == (0, 0) and got[3] == (0, 0) and got[7] == (0, 0)
    assert got[1] == (8, SINGLE)
    for b in (2, 4, 5):
        assert got[b][0] != 0 and got[b][1] in (0, SINGLE), got[b]  # (the single call's status: _check compared it)
    assert got[6] == (3, 0)
    # statuses = NULL: the first status in batch order that is not STARK_OK
    from stark_amd.verify import _wire_bytes
    pb = _wire_bytes(pub)
    fn = ctx.lib.stark_verify_r1cs_circuit_batch_proofs

    def call(order):
        hs = [None if handles[i] is None else handles[i].h for i in order]
        return fn(ctx.h, c.h, (ctypes.c_char_p * len(hs))(*[pb] * len(hs)), len(pb) // 32,
                  (ctypes.c_void_p * len(hs))(*hs), len(hs), None, None)
    for mode in (HOST, DEVICE):
        try:
            ctx.set_verify_batch_transcript(mode)
            assert call(range(len(handles))) == 8
            assert call([0, 3, 6, 1]) == 3
            assert call([0, 3, 7]) == 0
        finally:
            ctx.set_verify_batch_transcript(0)
    # a wrong count of public wires is each proof's STARK_ERR_BAD_ARG, as the single call's
    assert _check(ctx, c, [list(pub) + [5]] * 2, [good, rebuilt]) == [(3, 0), (3, 0)]
    from stark_amd import StarkError
    with pytest.raises(StarkError):
        ctx.set_verify_batch_transcript(3)


# ---- chunking -----------------------------------------------------------------------------------------


def test_chunks_and_resident_bytes(ctx, synth10):
    from stark_amd.r1cs import StarkProof
    from stark_amd.verify import verify_circuit_batch_proofs
    c, pubs, proofs = synth10["circuit"], list(synth10["pubs"][:5]), list(synth10["proofs"][:5])
    bad = proofs[2].parts()
    bad["lcomb"]["leaves"] = _flip(bad["lcomb"]["leaves"], 1)
    proofs[2] = StarkProof.from_parts(bad)
    whole = _check(ctx, c, pubs, proofs)
    assert [st for st, _ in whole] == [0, 0, 8, 0, 0] and whole[2][1] == OPENING_PATHS | SPOT
    for mode in (HOST, DEVICE):
        try:
            ctx.set_verify_batch_transcript(mode)
            ctx.set_verify_batch_limit(1)  # below one proof: chunks of one
            assert verify_circuit_batch_proofs(ctx, c, pubs, proofs) == whole
            small = ctx.memory()["resident"]
            ctx.set_verify_batch_limit(0)  # the default again: one chunk
            assert verify_circuit_batch_proofs(ctx, c, pubs, proofs) == whole
            held = ctx.memory()["resident"]
            assert held > small
            for _ in range(10):
                assert verify_circuit_batch_proofs(ctx, c, pubs, proofs) == whole
            assert ctx.memory()["resident"] == held
            ctx.set_verify_batch_limit(1)  # lowering the cap below what they hold frees them
            assert ctx.memory()["resident"] < small
        finally:
            ctx.set_verify_batch_limit(0)
            ctx.set_verify_batch_transcript(0)


# ---- after the batches --------------------------------------------------------------------------------


def test_context_intact_after_batches(ctx, fixtures):
    from stark_amd.verify import verify_circuit
    f = fixtures("compute")
    assert _check(ctx, f["circuit"], [f["pub"]] * 3, [f["proof"]] * 3) == [(0, 0)] * 3
    assert verify_circuit(ctx, f["circuit"], f["pub"], f["proof"].to_json())
    js = f["circuit"].prove(f["wt"]).to_json()
    assert hashlib.sha256(js.encode()).hexdigest() == GOLDEN["compute"]["json_sha256"]
