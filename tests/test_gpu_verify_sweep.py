"""Every check of the batched verifier (csrc/verify_batch.hip) shown live, class by class: the tamper tables of
oracle/verify_tamper.py (S1-S6: every opening, every level, every field of the main leaf, one equality at a time,
encodings that change bytes and not values, roots and Last values) applied to proofs made on the GPU, each case
through the handle entry under the host's and the device's transcript, and (status, reasons) held to
(8 if mask else 0, mask) of the classifying reference (oracle/verify_classes.py), exactly.  No mask is written here.

Fixtures: `compute` (precision 128, one Middle layer, path depths 7 and 5, 40-row layers: under one wave) and proof
3 of tests/test_gpu_verify_batch.py's synthetic 2^10-step batch (precision 2^13, four Middle layers, path depths 13
down to 5): the smallest shapes that have each kind of record.
"""
import os
import random
import sys

import pytest

import r1cs as R
import verify_classes as C
import verify_tamper as T

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "r1cs")
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

pytestmark = pytest.mark.gpu

HOST, DEVICE = 1, 2
CALL = 256  # proofs per call, at most


def _public(r1, wt):
    h = R.read_r1cs(r1).header
    return [int.from_bytes(w, "little") for w in R.read_witness(wt)[:1 + h.n_public_inputs + h.n_public_outputs]]


class _Fixture:
    def __init__(self, oracle, circuit, r1, pub, proof):
        self.circuit, self.pub, self.proof = circuit, pub, proof
        self.parts = proof.parts()
        self.inputs = R.verifier_inputs(R.read_r1cs(r1), pub)
        self.cls = C.classifier(oracle, self.inputs)
        self.tabs = T.tables(self.parts, pub, self.cls.steps)

    def expected(self, pub, parts):
        mask, detail = self.cls.classify(pub, parts)
        return (8 if mask else 0, mask), detail


class _Fixtures:
    """Proved on first use and kept for the module."""

    def __init__(self, ctx, oracle):
        self.ctx, self.oracle, self.made = ctx, oracle, {}

    def __call__(self, name):
        if name not in self.made:
            from stark_amd.r1cs import R1csCircuit
            if name == "compute":
                with open(os.path.join(FIX, "compute.r1cs"), "rb") as f:
                    r1 = f.read()
                with open(os.path.join(FIX, "compute.wtns"), "rb") as f:
                    wt = f.read()
                c = R1csCircuit(self.ctx, r1)
                proof = c.prove(wt)
            else:
                import synth_r1cs
                r1, _ = synth_r1cs.for_steps(10)
                wts = [synth_r1cs.for_steps(10, inputs=(1000 + 17 * k, R.P - 5 - k))[1] for k in range(7)]
                c = R1csCircuit(self.ctx, r1)
                proof, wt = c.prove_batch(wts)[3], wts[3]
            self.made[name] = _Fixture(self.oracle, c, r1, _public(r1, wt), proof)
        return self.made[name]


@pytest.fixture(scope="module")
def fixtures(ctx, oracle):
    return _Fixtures(ctx, oracle)


def _slots(f, cases, seed):
    """The cases in a fixed-seed order, the untampered proof in every 7th slot."""
    order = list(cases)
    random.Random(seed).shuffle(order)
    out = []
    for c in order:
        if len(out) % 7 == 6:
            out.append(("untampered", f.parts, f.pub))
        out.append(c)
    out.append(("untampered", f.parts, f.pub))
    return out


def _report(wrong):
    for name, mode, got, want, detail in wrong[:40]:
        print(f"{name} [{mode}]: got {got}, the classifier gives {want}: {detail}")
    assert not wrong, f"{len(wrong)} results differ from the classifier's, the first: {wrong[0][:4]}"


def _sweep(ctx, f, cases, seed, limit=0):
    """Every slot through the handle entry, in calls of at most CALL proofs, under both transcript modes."""
    from stark_amd.r1cs import StarkProof
    from stark_amd.verify import verify_circuit_batch_proofs
    slots = _slots(f, cases, seed)
    wrong, clear = [], 0
    try:
        ctx.set_verify_batch_limit(limit)
        for at in range(0, len(slots), CALL):
            call = slots[at:at + CALL]
            want = [f.expected(pub, parts) for _, parts, pub in call]
            handles = [StarkProof.from_parts(parts) for _, parts, _ in call]
            for mode in (HOST, DEVICE):
                ctx.set_verify_batch_transcript(mode)
                got = verify_circuit_batch_proofs(ctx, f.circuit, [pub for _, _, pub in call], handles)
                for (name, _, _), g, (w, detail) in zip(call, got, want):
                    if name == "untampered":
                        assert w == (0, 0)
                        clear += g == (0, 0)
                    if g != w:
                        wrong.append((name, f"transcript {mode}", g, w, detail))
            del handles
    finally:
        ctx.set_verify_batch_transcript(0)
        ctx.set_verify_batch_limit(0)
    print(f"{len(slots)} slots x 2 transcripts, {len(wrong)} wrong")
    _report(wrong)
    assert clear == 2 * sum(name == "untampered" for name, _, _ in slots)
    return len(slots)


@pytest.mark.parametrize("sweep", ["S1", "S2", "S3", "S4", "S5", "S6"])
@pytest.mark.parametrize("name", ["compute", "synth10"])
def test_sweep(ctx, fixtures, name, sweep):
    f = fixtures(name)
    cases = f.tabs[sweep]
    if sweep == "S4":  # (what makes S4 one equality at a time; tests/test_verify_classes_cpu.py on the oracle's proofs)
        for case, parts, pub in cases:
            _, detail = f.expected(pub, parts)
            assert [eqs for _, eqs in detail.get("spot", [])] == [(T.s4_equality(case),)], (case, detail)
    _sweep(ctx, f, cases, seed=sum(map(ord, name + sweep)))


def _staged(f):
    """What one proof of the fixture's circuit stages (verify_batch.hip Shape::staged): its block -- the roots,
    a_root, the public wires, 14 constants, I2, the openings -- and 32 B per record."""
    p, layers = f.parts, len(f.parts["layers"])
    sets = [p["main"], p["lcomb"]] + [x[k] for x in p["layers"] for k in ("column", "poly")]
    opened = sum(len(b["leaves"]) + len(b["nodes"]) for b in sets)
    block = 32 * (2 + layers) + 32 + 32 * len(f.pub) + 32 * 14 + 32 * len(f.inputs["public_first_indices"]) + opened
    return block + 32 * (sum(b["k"] for b in sets) + 40 * layers + 80)


@pytest.mark.parametrize("per_chunk", [1, 3])
def test_s1_compute_in_small_chunks(ctx, fixtures, per_chunk):
    """S1 of compute again with a staging cap that holds one proof, then three, per chunk: a chunk's classes then
    end inside a wave (80 and 240 L paths and spot checks, 40 and 120 rows and column paths), and a tampered
    proof's lanes are the last of one launch and the first of the next."""
    f = fixtures("compute")
    staged = _staged(f)
    _sweep(ctx, f, f.tabs["S1"], seed=per_chunk, limit=per_chunk * staged + staged // 2)


def _other_entries_sample(f):
    kinds = {f"S4:{kind}:position{(7 * k + 3) % 80}" for k, kind in enumerate(T.S4_KINDS)}
    return T.sample(f.tabs, 80, 11, keep=lambda n: n in kinds or n.startswith("S5") or
                    (n.startswith("S6") and not n.startswith("S6:last")))


@pytest.mark.parametrize("name", ["compute", "synth10"])
def test_sample_through_the_other_entries(ctx, fixtures, name):
    """A sample (every S4 kind once, all of S5, S6's roots, more at random up to 80) through the text entry under
    both transcripts, and through the single-proof call (status only)."""
    from stark_amd.r1cs import StarkProof
    from stark_amd.verify import _wire_bytes, verify_circuit_batch
    f = fixtures(name)
    slots = _slots(f, _other_entries_sample(f), 5)
    assert len(slots) <= 80 + 80 // 6 + 1
    want = [f.expected(pub, parts) for _, parts, pub in slots]
    texts = [StarkProof.from_parts(parts).to_json() for _, parts, _ in slots]
    pubs = [pub for _, _, pub in slots]
    wrong = []
    try:
        for mode in (HOST, DEVICE):
            ctx.set_verify_batch_transcript(mode)
            got = verify_circuit_batch(ctx, f.circuit, pubs, texts)
            wrong += [(n, f"text, transcript {mode}", g, w, d) for (n, _, _), g, (w, d) in zip(slots, got, want) if g != w]
    finally:
        ctx.set_verify_batch_transcript(0)
    for (n, _, _), pub, text, (w, d) in zip(slots, pubs, texts, want):
        js, pb = text.encode(), _wire_bytes(pub)
        st = ctx.lib.stark_verify_r1cs_circuit(ctx.h, f.circuit.h, pb, len(pb) // 32, js, len(js))
        if st != w[0]:
            wrong.append((n, "single", st, w[0], d))
    _report(wrong)


@pytest.mark.parametrize("name", ["compute", "synth10"])
def test_s5_through_both_interp2_routes(ctx, fixtures, name):
    """S5 (the public wires as w + p and w + 4p among them) with I2 formed by the default route and by the route
    set_public_column_min(2) selects, through the handle and the text entry, under both transcripts."""
    from stark_amd.r1cs import StarkProof
    from stark_amd.verify import verify_circuit_batch, verify_circuit_batch_proofs
    f = fixtures(name)
    off = list(f.pub)
    off[1] = (off[1] + 1) % R.P  # a wire that is wrong by one, re-encoded: only I2 can tell
    slots = _slots(f, f.tabs["S5"] + [("wire 1 off by one, + 4p", f.parts, [w + 4 * R.P for w in off])], 3)
    want = [f.expected(pub, parts) for _, parts, pub in slots]
    assert ((8, C.SPOT), ) == tuple({w for (n, _, _), (w, _) in zip(slots, want) if n.startswith("wire 1")})
    handles = [StarkProof.from_parts(parts) for _, parts, _ in slots]
    texts = [h.to_json() for h in handles]
    pubs = [pub for _, _, pub in slots]
    wrong = []
    try:
        for column_min in (0, 2):
            ctx.set_public_column_min(column_min)
            for mode in (HOST, DEVICE):
                ctx.set_verify_batch_transcript(mode)
                for entry, got in (("handles", verify_circuit_batch_proofs(ctx, f.circuit, pubs, handles)),
                                   ("text", verify_circuit_batch(ctx, f.circuit, pubs, texts))):
                    wrong += [(n, f"{entry}, column_min {column_min}, transcript {mode}", g, w, d)
                              for (n, _, _), g, (w, d) in zip(slots, got, want) if g != w]
    finally:
        ctx.set_public_column_min(0)
        ctx.set_verify_batch_transcript(0)
    _report(wrong)
