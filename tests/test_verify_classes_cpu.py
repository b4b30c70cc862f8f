"""The classifying reference (oracle/verify_classes.py) and the tamper tables (oracle/verify_tamper.py) on the
oracle's own proofs, which stand in for the GPU's: the bar tests/test_gpu_verify_sweep.py holds the batched
verifier against must itself be right.

  * the untampered proof classifies as 0;
  * on a fixed-seed sample of 200 cases per circuit across S1-S6, mask != 0 exactly when the restated verifier
    (oracle/stark_verify.py, the reference's assertions in the reference's order) raises;
  * every S4 case fails exactly the equality it is built to fail, and no other, at all 80 positions -- what makes
    S4 a test of one equality at a time (it needs F0 F1, F2, p_x and nmr nonzero at the sampled positions);
  * S5's re-encoded leaves fail paths (or the Last root) and no arithmetic class; its re-encoded wires fail nothing;
  * S3's fields that no equality reads fail OPENING_PATHS alone.
"""
import json
import os
import sys

import pytest

import r1cs as R
import verify_classes as C
import verify_tamper as T
from stark_verify import verify_r1cs_proof

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "r1cs")
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))


class _Case:
    def __init__(self, oracle, r1cs, witness):
        self.tr = R.build_trace(r1cs, witness)
        self.pub = list(self.tr.public_wires)
        self.proof = json.loads(R.mk_r1cs_proof_json(oracle, self.tr))
        self.parts = C.parts_of_dict(self.proof)
        self.cls = C.classifier(oracle, self.tr)
        self.tabs = T.tables(self.parts, self.pub, self.cls.steps)


@pytest.fixture(scope="module", params=["compute", "synth10"])
def case(request, oracle):
    if request.param == "compute":
        return _Case(oracle, *R.load_fixture(FIX, "compute"))
    import synth_r1cs
    r1, wt = synth_r1cs.for_steps(10, inputs=(1051, R.P - 8))
    return _Case(oracle, R.read_r1cs(r1), R.read_witness(wt))


def _restated_accepts(oracle, tr, pub, parts) -> bool:
    try:
        return verify_r1cs_proof(oracle, C.dict_of_parts(parts), pub, tr.public_first_indices, tr.permuted_indices,
                                 tr.coefficients, tr.flag0, tr.flag1, tr.flag2, tr.n_constraints, tr.n_wires)
    except AssertionError:
        return False


def test_parts_round_trip(case):
    assert C.dict_of_parts(case.parts) == case.proof


def test_untampered_is_clear(case, oracle):
    assert case.cls.classify(case.pub, case.parts) == (0, {})
    assert _restated_accepts(oracle, case.tr, case.pub, case.parts)
    assert case.cls.classify([2] + case.pub[1:], case.parts)[0] == C.PUBLIC_ONE
    assert case.cls.classify([1 + R.P] + case.pub[1:], case.parts)[0] == 0


def test_table_sizes(case):
    """What the tables' definitions give: every opening once in S1, every (class, level) in S2, 384 + 800 cases."""
    parts, tabs = case.parts, case.tabs
    sets = [T._at(parts, path) for _, path in T.classes(parts)]
    assert len(tabs["S1"]) == sum(b["k"] for b in sets) == 400 + 200 * len(parts["layers"])
    levels = {tuple(n.split(":")[1::2]) for n, _, _ in tabs["S2"]}
    assert levels == {(label, f"level{l}") for (label, _), b in zip(T.classes(parts), sets) for l in range(b["depth"])}
    assert len(tabs["S3"]) == 6 * 4 * 8 * 2 and len(tabs["S4"]) == 80 * 10
    assert len(tabs["S5"]) == 5 + 2 * len(parts["layers"])
    assert len(tabs["S6"]) == 2 * (3 + len(parts["layers"])) + len(parts["last"]) // 32
    names = [n for t in tabs.values() for n, _, _ in t]
    assert len(names) == len(set(names))
    for t in tabs.values():  # every case changes something, and never the shape
        for _, q, pub in t:
            assert (q != parts) != (pub != case.pub)
            assert case.cls._in_shape(q)


def test_mask_nonzero_iff_restated_verifier_raises(case, oracle):
    sample = T.sample(case.tabs, 200, 20260)
    assert len(sample) == 200 and {n[:2] for n, _, _ in sample} == set(case.tabs)
    for name, parts, pub in sample:
        mask, detail = case.cls.classify(pub, parts)
        assert (mask != 0) == (not _restated_accepts(oracle, case.tr, pub, parts)), (name, hex(mask), detail)


def test_s4_fails_one_equality(case):
    seen = set()
    for name, parts, pub in case.tabs["S4"]:
        mask, detail = case.cls.classify(pub, parts)
        i = int(name.split(":")[2][8:])
        assert mask == C.OPENING_PATHS | C.SPOT, (name, hex(mask), detail)
        assert detail["spot"] == [(i, (T.s4_equality(name),))], (name, detail)
        assert {q // 4 if which == "main" else q for which, q in detail["opening_paths"]} == {i}, (name, detail)
        seen.add((name.split(":")[1], i))
    assert seen == {(kind, i) for kind in T.S4_KINDS for i in range(80)}


def test_s5_changes_no_value(case):
    for name, parts, pub in case.tabs["S5"]:
        mask, detail = case.cls.classify(pub, parts)
        if name.startswith("S5:wires"):
            assert (mask, detail) == (0, {}), name
            continue
        want = {"S5:main": C.OPENING_PATHS, "S5:lcom": C.OPENING_PATHS, "S5:last": C.FRI_LAST}.get(name[:7], C.FRI_PATHS)
        assert mask == want, (name, hex(mask), detail)
        if want == C.FRI_LAST:
            assert detail["fri_last"] == ["root"]
        else:  # every opening of the set fails, and nothing else
            items = detail["opening_paths" if want == C.OPENING_PATHS else "fri_paths"]
            assert len(items) == {"main": 320, "lcom": 80, "colu": 40, "poly": 160}[name[3:7]], name


def test_s3_unread_fields_fail_paths_alone(case):
    unread = 0
    for name, parts, pub in case.tabs["S3"]:
        mask, detail = case.cls.classify(pub, parts)
        i, role = int(name.split(":")[1][8:]), int(name.split(":")[2][4:])
        assert detail["opening_paths"] == [("main", 4 * i + role)], (name, detail)
        if T.s3_read(name):
            assert mask == C.OPENING_PATHS | C.SPOT and [p for p, _ in detail["spot"]] == [i], (name, hex(mask), detail)
        else:
            unread += 1
            assert mask == C.OPENING_PATHS, (name, hex(mask), detail)
    assert unread == 6 * 2 * (6 + 7 + 7)


def test_s1_s2_s6_name_their_item(case):
    """The detail of a one-item tampering is that item: the classifier finds the site it was never told."""
    for name, parts, pub in case.tabs["S1"] + case.tabs["S2"]:
        mask, detail = case.cls.classify(pub, parts)
        label, q = name.split(":")[1], int(name.split(":")[2][7:])
        if label in ("main", "lcomb"):
            assert detail["opening_paths"] == [(label, q)], (name, detail)
            assert mask & ~C.SPOT == C.OPENING_PATHS and (mask & C.SPOT == 0 or name.startswith("S1")), (name, hex(mask))
        else:
            which, layer = label[:-1], int(label[-1])
            assert detail["fri_paths"] == [(layer, which, q)], (name, detail)
            if name.startswith("S1"):
                assert mask == C.FRI_PATHS | C.FRI_ROWS and detail["fri_rows"] == [(layer, q if which == "column" else q // 4)]
            else:
                assert mask == C.FRI_PATHS
    for name, parts, pub in case.tabs["S6"]:
        mask, detail = case.cls.classify(pub, parts)
        if name.startswith("S6:last"):
            assert mask == C.FRI_LAST and "root" in detail["fri_last"], (name, detail)
        elif name.startswith("S6:a_root"):
            assert mask == C.SPOT and len(detail["spot"]) == 80, (name, detail)
        else:
            assert mask & (C.OPENING_PATHS | C.FRI_PATHS), (name, hex(mask))
