"""stark_check_r1cs_circuit_batch / R1csCircuit.check_batch: which constraints of a prepared circuit a batch of
witnesses fails, with A.w, B.w and C.w of each, against R1CS satisfaction in Python integers (failing() below).

The raw ABI is called on sentinel-filled arrays and whole byte images are compared: the listed records, their
order, reserved = 0, and every byte behind them left as it was.
"""
import ctypes
import functools
import hashlib
import json
import os
import struct

import pytest

import r1cs as R
import r1cs_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "r1cs")
GOLDEN = json.load(open(os.path.join(HERE, "golden", "r1cs_proofs.json")))
P = C.P
SENTINEL = 0xA5

pytestmark = pytest.mark.gpu


def failing(cons, raw):
    """[(index, A.w, B.w, C.w)] of the constraints with A.w B.w != C.w (mod p); cons as Circuit.cons."""
    out = []
    for i, fac in enumerate(cons):
        a, b, c = (sum(v * raw[w] for w, v in fc) % P for fc in fac)
        if (a * b - c) % P:
            out.append((i, a, b, c))
    return out


def _record(f):
    i, a, b, c = f
    return struct.pack("<II", i, 0) + b"".join(v.to_bytes(32, "little") for v in (a, b, c))


def _image(reports, cap):
    """The `failures` array a call on a sentinel-filled one must leave: reports[b] = Python's list of witness b,
    or None for a refused witness."""
    out = b""
    for rep in reports:
        body = b"".join(_record(f) for f in (rep or [])[:cap])
        out += body + bytes([SENTINEL]) * (104 * cap - len(body))
    return out


def _status(rep):
    return C.BAD_ARG if rep is None else (C.CHECK if rep else C.OK)


def raw_check(ctx, circ, ws, cap, with_statuses=True):
    """(return value, statuses, n_failed, the bytes of `failures`) of the batched call on sentinel-filled arrays."""
    from stark_amd.r1cs import R1csFailure
    n = len(ws)
    ptrs = (ctypes.c_char_p * n)(*ws)
    lens = (ctypes.c_size_t * n)(*[0 if w is None else len(w) for w in ws])
    sts = (ctypes.c_int * n)(*[77] * n)
    nf = (ctypes.c_uint32 * n)(*[77] * n)
    recs = None
    if cap:
        recs = (R1csFailure * (n * cap))()
        ctypes.memset(recs, SENTINEL, 104 * n * cap)
    rc = ctx.lib.stark_check_r1cs_circuit_batch(ctx.h, circ.h, ptrs, lens, n, sts if with_statuses else None, nf, recs,
                                                cap)
    return rc, list(sts), list(nf), bytes(recs) if cap else b""


def expect(ctx, circ, ws, reports, cap, what=""):
    rc, sts, nf, img = raw_check(ctx, circ, ws, cap)
    assert rc == 0, what
    assert sts == [_status(r) for r in reports], what
    assert nf == [len(r or []) for r in reports], what
    want = _image(reports, cap)
    if img != want:   # told by the first differing record (two multi-megabyte images do not diff)
        k = next(i for i in range(0, len(want), 104) if img[i:i + 104] != want[i:i + 104])
        pytest.fail(f"{what}: record {k // 104 % cap} of witness {k // 104 // cap}: {img[k:k + 104].hex()} for "
                    f"{want[k:k + 104].hex()}", pytrace=False)


@pytest.fixture(scope="module")
def prepared(ctx):
    """case or fixture name -> its R1csCircuit, prepared once and reused by every test."""
    from stark_amd.r1cs import R1csCircuit
    memo = {}

    def get(name, r1cs=None):
        if name not in memo:
            memo[name] = R1csCircuit(ctx, r1cs if r1cs is not None else C.CASES[name].circuit.r1cs)
        return memo[name]
    return get


def _solved(name, seed=1):
    case = C.CASES[name]
    return C.solve(case.circuit, seed, case.values, case.wire0)


def _raised(raw, wires):
    out = list(raw)
    for w in wires:
        out[w] = (out[w] + 1) % P
    return out


@functools.lru_cache(maxsize=None)
def pokes(name):
    """For every wire w >= 1 of the case: (the seed-1 witness with wire w raised by 1, Python's report)."""
    c = C.CASES[name].circuit
    raw = _solved(name)
    out = []
    for w in range(1, c.n_wires):
        r = _raised(raw, [w])
        out.append((C.wtns_bytes(r), failing(c.cons, r)))
    return out


# ---- 1. every accepted shape ----

@pytest.mark.parametrize("name", C.ACCEPTED)
def test_seed1_witness_is_satisfied_and_nothing_is_written(ctx, prepared, name):
    case = C.CASES[name]
    expect(ctx, prepared(name), [case.wtns(1)], [[]], 4, name)
    rep = prepared(name).check(case.wtns(1))
    assert rep.satisfied and rep.status == 0 and rep.n_failed == 0 and rep.failures == []


@pytest.mark.parametrize("name", C.SMALL)
def test_every_wire_raised_by_one(ctx, prepared, name):
    """One batch: wire w raised, for every w >= 1, max_failures = n_c.  Status, n_failed, indices and the three
    values of every entry are Python's; a wire that does not matter comes back satisfied."""
    c = C.CASES[name].circuit
    ws, reports = zip(*pokes(name))
    empty = sum(1 for r in reports if not r)
    print(name, "wires poked", len(ws), "reports empty", empty, "most failures", max(len(r) for r in reports))
    if name == "one_wire":
        assert empty == len(ws) == 39
    if name == "stride400":
        assert max(len(r) for r in reports) == 80
    expect(ctx, prepared(name), list(ws), list(reports), len(c.cons), name)


def test_poke_census():
    """What the batches above hold, from Python alone: the wires whose raising fails nothing (they must come back
    satisfied, and do through expect()).  tests/r1cs_cases.py gives 103 of them over C.SMALL: os6 1, os9 1,
    ragged 1, empty_mid 1, empty_last 2, long_b 6, long_mixed 5, wires64 24, wires65 20, one_wire 39,
    pub_unused2 2, noncanon_coef 1."""
    empty = {name: sum(1 for _, r in pokes(name) if not r) for name in C.SMALL}
    print({k: v for k, v in empty.items() if v})
    assert empty["one_wire"] == 39 == len(pokes("one_wire"))
    assert sum(empty.values()) == 103


def test_long_unsat_reports_the_one_constraint(ctx, prepared):
    case = C.CASES["long_unsat"]
    c = case.circuit
    want = failing(c.cons, _raised(_solved("long_unsat"), list(case.poke(c))))
    assert [f[0] for f in want] == [1]
    expect(ctx, prepared("long_mixed"), [case.wtns(1)], [want], len(c.cons))
    rep = prepared("long_mixed").check(case.wtns(1))
    assert (rep.status, rep.n_failed, rep.failures) == (C.CHECK, 1, want) and not rep.satisfied


# ---- 2. bit and wave boundaries ----

@pytest.mark.parametrize("n", [2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1025])
def test_bit_and_wave_boundaries(ctx, n):
    from stark_amd.r1cs import R1csCircuit
    c = C.circuit([(1, 1, 1)] * n, wires=C.free_only, n_in=8, pub=(1, 2), seed=n)
    raw = C.solve(c, 1)
    sets = [[0], [n - 1], [k for k in (31, 32, 63, 64, 255, 256) if k < n], list(range(n))]
    ws, reports = [], []
    for ks in sets:
        r = _raised(raw, [c.fresh[k] for k in ks])
        rep = failing(c.cons, r)
        assert [f[0] for f in rep] == ks   # raising fresh wire k alone fails exactly constraint k
        ws.append(C.wtns_bytes(r))
        reports.append(rep)
    expect(ctx, R1csCircuit(ctx, c.r1cs), ws, reports, n, f"n = {n}")


# ---- 3. lengths inside one wave ----

def test_lengths_inside_one_wave(ctx):
    from stark_amd.r1cs import R1csCircuit
    shape = [(i % 33, 1, 1) if i % 33 else (0, 0, 0) for i in range(1, 100)] + [(40, 1, 1), (1, 70, 1), (2, 2, 200)]
    c = C.circuit(shape, wires=C.free_only, n_in=16, seed=7)
    r = _raised(C.solve(c, 1), [w for w in c.fresh if w is not None])
    rep = failing(c.cons, r)
    assert [f[0] for f in rep] == [k for k, w in enumerate(c.fresh) if w is not None] and len(rep) == 99
    expect(ctx, R1csCircuit(ctx, c.r1cs), [C.wtns_bytes(r)], [rep], len(c.cons))


# ---- 4. many failures across workgroups ----

def test_many_failures_across_workgroups(ctx, prepared):
    c = C.CASES["big_pub_first"].circuit
    raw = _solved("big_pub_first")
    many = _raised(raw, range(1, 64))
    last = _raised(raw, [c.n_wires - 1])
    rep_many, rep_last = failing(c.cons, many), failing(c.cons, last)
    print("big_pub_first: wires 1..63 raised fail", len(rep_many), "of", len(c.cons))
    # (thousands of failures spread over the whole bitmap: every tile of the compaction carries a running count)
    assert 1024 < len(rep_many) <= 4096 and rep_many[-1][0] > 29000 and [f[0] for f in rep_last] == [29199]
    expect(ctx, prepared("big_pub_first"), [C.wtns_bytes(many), C.wtns_bytes(last)], [rep_many, rep_last], 4096)


# ---- 5. cap ----

def test_cap(ctx, prepared):
    ws, reports = zip(*pokes("stride400"))
    k = max(range(len(ws)), key=lambda i: len(reports[i]))
    assert len(reports[k]) == 80
    for cap in (0, 1, 16, 80, 500):
        expect(ctx, prepared("stride400"), [ws[k]], [reports[k]], cap, f"cap {cap}")
    rep = prepared("stride400").check(ws[k], max_failures=16)
    assert (rep.status, rep.n_failed, rep.failures) == (C.CHECK, 80, reports[k][:16])
    assert prepared("stride400").check(ws[k], max_failures=0).n_failed == 80


# ---- 6. widths and refusals ----

def test_witness_widths_give_one_report(ctx, prepared):
    case = C.CASES["narrow"]
    c = case.circuit
    good = _solved("narrow")
    bad = list(good)
    bad[1] += 1   # (small values: still below 2^64)
    rep = failing(c.cons, bad)
    assert rep and failing(c.cons, good) == []
    ws, reports = [], []
    for fs, surplus in ((8, 0), (16, 0), (32, 0), (8, 5), (32, 5)):
        ws += [C.wtns_bytes(good, fs, surplus), C.wtns_bytes(bad, fs, surplus)]
        reports += [[], rep]
    assert len(set(ws)) == 10
    expect(ctx, prepared("narrow"), ws, reports, len(c.cons))


@pytest.mark.parametrize("name", ["noncanon_wit", "noncanon_coef"])
def test_values_at_and_above_p(ctx, prepared, name):
    """The witness bytes stay at and above p where the case puts them there: a raised value is written as it is."""
    c = C.CASES[name].circuit
    raw = _solved(name)
    ws, reports = [C.wtns_bytes(raw)], [[]]
    for w in range(1, c.n_wires):
        if raw[w] + 1 < 1 << 256:
            r = list(raw)
            r[w] += 1
            ws.append(C.wtns_bytes(r))
            reports.append(failing(c.cons, r))
    assert any(reports)
    if name == "noncanon_wit":
        assert any(rep and raw[w] >= P for w, rep in zip(range(1, c.n_wires), reports[1:]) if raw[w] + 1 < 1 << 256)
    expect(ctx, prepared(name), ws, reports, len(c.cons), name)


def test_refused_witnesses_beside_a_good_and_a_bad_one(ctx, prepared):
    c = C.CASES["ragged"].circuit
    good = C.CASES["ragged"].wtns(1)
    k = next(i for i, (_, r) in enumerate(pokes("ragged")) if r)
    bad, rep = pokes("ragged")[k]
    ws = [None, good[:-7], C.witness(c, 1, wire0=2), good, bad]
    reports = [None, None, None, [], rep]
    expect(ctx, prepared("ragged"), ws, reports, len(c.cons))
    rc, sts, nf, img = raw_check(ctx, prepared("ragged"), ws, len(c.cons), with_statuses=False)
    assert rc == C.BAD_ARG and sts == [77] * 5   # the first status that is not STARK_OK; the arrays all the same
    assert nf == [0, 0, 0, 0, len(rep)] and img == _image(reports, len(c.cons))
    rc, _, nf, _ = raw_check(ctx, prepared("ragged"), [good, bad, None], 2, with_statuses=False)
    assert rc == C.CHECK and nf == [0, len(rep), 0]
    got = prepared("ragged").check_batch(ws, max_failures=len(c.cons))
    assert [(g.status, g.n_failed, g.failures) for g in got] == [(_status(r), len(r or []), r or []) for r in reports]


def test_whole_call_errors_and_an_empty_batch(ctx, prepared):
    from stark_amd import StarkError
    from stark_amd.r1cs import R1csFailure
    circ = prepared("ragged")
    good = C.CASES["ragged"].wtns(1)
    one = (ctypes.c_char_p * 1)(good)
    lens = (ctypes.c_size_t * 1)(len(good))
    nf = (ctypes.c_uint32 * 1)(77)
    rec = (R1csFailure * 1)()
    f = ctx.lib.stark_check_r1cs_circuit_batch
    assert f(ctx.h, circ.h, one, lens, 1, None, nf, None, 1) == C.BAD_ARG      # cap > 0 without failures
    assert f(ctx.h, circ.h, one, lens, 65536, None, nf, rec, 1) == C.BAD_ARG
    assert f(ctx.h, circ.h, None, lens, 1, None, nf, rec, 1) == C.BAD_ARG
    assert f(ctx.h, circ.h, one, None, 1, None, nf, rec, 1) == C.BAD_ARG
    assert nf[0] == 77
    assert f(ctx.h, circ.h, one, lens, 0, None, nf, rec, 1) == C.OK and nf[0] == 77
    assert f(ctx.h, circ.h, one, lens, 1, None, None, None, 0) == C.OK         # every output optional
    assert circ.check_batch([]) == []
    with pytest.raises(StarkError) as e:
        circ.check_batch([good], max_failures=-1)
    assert e.value.code == C.BAD_ARG
    assert ctx.lib.stark_check_r1cs_circuit(ctx.h, circ.h, good, len(good), nf, rec, 1) == C.OK and nf[0] == 0
    assert ctx.lib.stark_check_r1cs_circuit(ctx.h, circ.h, None, 0, nf, rec, 1) == C.BAD_ARG and nf[0] == 0


# ---- 7. chunks ----

def test_chunks_of_one_give_the_same_reports(ctx, prepared):
    c = C.CASES["long_mixed"].circuit
    ws, reports = zip(*pokes("long_mixed"))
    try:
        ctx.set_prove_batch_limit(1)
        expect(ctx, prepared("long_mixed"), list(ws), list(reports), len(c.cons), "chunks of one")
        one = raw_check(ctx, prepared("long_mixed"), list(ws), len(c.cons))
    finally:
        ctx.set_prove_batch_limit(0)
    assert raw_check(ctx, prepared("long_mixed"), list(ws), len(c.cons)) == one
    before = ctx.memory()["resident"]
    assert before > 0 and raw_check(ctx, prepared("long_mixed"), list(ws), len(c.cons)) == one
    assert ctx.memory()["resident"] == before   # the buffers are reused, and counted


# ---- 8. agreement with the prover ----

@pytest.mark.parametrize("name", C.SMALL)
def test_statuses_agree_with_the_prover(ctx, prepared, name):
    """seed 1, a raised fresh wire, a raised wire that Python says does not matter (where the case has one) and a
    raised wire 0: check_batch's statuses are prove_batch(strict=False)'s, and Python's."""
    c = C.CASES[name].circuit
    raw = _solved(name)
    ws, want = [C.wtns_bytes(raw)], [C.OK]
    fresh = next((w for w in c.fresh if w is not None), None)
    if fresh is not None:
        ws.append(pokes(name)[fresh - 1][0])
        want.append(_status(pokes(name)[fresh - 1][1]))
    idle = next((i for i, (_, r) in enumerate(pokes(name)) if not r), None)
    if idle is not None:
        ws.append(pokes(name)[idle][0])
        want.append(C.OK)
    w0 = list(raw)
    w0[0] += 1
    ws.append(C.wtns_bytes(w0))
    want.append(C.BAD_ARG)
    checked = [r.status for r in prepared(name).check_batch(ws)]
    proved = [0 if not hasattr(p, "code") else p.code for p in prepared(name).prove_batch(ws, strict=False)]
    print(name, "python", want, "check", checked, "prove", proved)
    assert checked == want
    assert checked == proved


# ---- 9. fixtures and determinism ----

def _fixture(name):
    with open(os.path.join(FIX, name + ".r1cs"), "rb") as f:
        r1 = f.read()
    with open(os.path.join(FIX, name + ".wtns"), "rb") as f:
        wt = f.read()
    cons = [[[(w, int.from_bytes(v, "little")) for w, v in fc] for fc in fac] for fac in R.read_r1cs(r1).constraints]
    raw = [int.from_bytes(v, "little") for v in R.read_witness(wt)]
    return r1, wt, cons, raw


@pytest.mark.parametrize("name", ["compute", "poseidon3_test", "pedersen_test", "bits"])
def test_golden_fixtures_and_determinism(ctx, prepared, name):
    r1, wt, cons, raw = _fixture(name)
    circ = prepared("fixture:" + name, r1)
    assert failing(cons, raw) == []
    bad = raw[:-1] + [raw[-1] + 1]
    rep = failing(cons, bad)
    print(name, "constraints", len(cons), "wires", len(raw), "last value raised fails", len(rep))
    ws, reports = [wt, C.wtns_bytes(bad)], [[], rep]
    expect(ctx, circ, ws, reports, 16, name)
    assert raw_check(ctx, circ, ws, 16) == raw_check(ctx, circ, ws, 16)
    if name == "compute":
        from stark_amd.r1cs import check_with_witness, prove_with_witness
        got = check_with_witness(ctx, r1, ws[1])
        assert (got.status, got.n_failed, got.failures) == (_status(rep), len(rep), rep[:16])
        js = prove_with_witness(ctx, r1, wt).to_json()
        assert hashlib.sha256(js.encode()).hexdigest() == GOLDEN["compute"]["json_sha256"]
