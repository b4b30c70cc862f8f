"""CPU: the case tables of tests/fe_cases.py, which tests/test_gpu_fe_ops.py runs on the GPU.
  * every record of every table lies inside the precondition its primitive's comment states;
  * where an integer formula and an emulator both exist they agree (Montgomery single and dual against
    tools/gen_fe_mul_asm.py's streams, the Shoup product and its flag against the stream's emulation), and the
    constant products keep their contract r < 2p, r = a w (mod p);
  * every class of directed case is present, so a change to a generator cannot quietly empty one."""
import pytest

import fe_cases as F
import gen_fe_mul_asm as G

P, TOP2P = F.P, F.TOP2P


@pytest.mark.parametrize("op", sorted(F.OPS))
def test_records_meet_precondition(op):
    recs = F.table(op)
    assert len(recs) % 64 == 37 and len(recs) > 64          # a partial last wave after at least one full one
    pre = F.PRE[op]
    for i, rec in enumerate(recs):
        assert all(0 <= v < F.R256 for v in rec) and pre(*rec), (op, i, [hex(v) for v in rec])
    want = F.expected(op)
    assert all(0 <= v < F.R256 for w in want for v in w)
    assert F.encode(op, recs).shape == (len(recs), 8 * F.OPS[op][1])
    assert F.expected_array(op, 0).shape == F.expected_array(op, 1).shape == (len(recs), 8 * F.OPS[op][2])
    assert sorted(n for n, _, _ in F.OPS.values()) == list(range(F.N_OPS))


def test_montgomery_formula_is_the_stream():
    """fe_mul_lazy's integer formula against the emulated single stream, on fe_mul_lazy's whole table."""
    r = [f"%{i}" for i in range(8)]
    ops = G.stream(r, [f"%{9 + i}" for i in range(8)], [f"%{17 + i}" for i in range(8)],
                   [f"%{25 + i}" for i in range(8)], "%33", "%8", [(0, 1), (2, 3)])
    recs = F.table("fe_mul_lazy")
    assert len(recs) <= 3000
    rinv = pow(F.R256, -1, P)
    for (a, b), (want,) in zip(recs, F.expected("fe_mul_lazy")):
        assert F._out(F._emulate(ops, F._mont_regs(a, b, 9, 17, 25, "%33")), 0) == want, (hex(a), hex(b))
        assert want < 2 * P and want % P == a * b * rinv % P
    assert F.table("fe_mul")[:1225] == recs[:1225]
    assert sum(a >= F.LAZY_R for a, _ in recs) >= 600 and sum(a < F.LAZY_R for a, _ in recs) >= 600


def test_dual_formula_is_the_stream():
    """fe_mul_lazy2's two formulas against the emulated interleaved streams (emit_dual's operand map)."""
    r, s = [f"%{i}" for i in range(8)], [f"%{8 + i}" for i in range(8)]
    p = [f"%{50 + i}" for i in range(8)]
    sa = G.stream(r, [f"%{18 + i}" for i in range(8)], [f"%{26 + i}" for i in range(8)], p, "%58", "%16",
                  [(0, 1), (2, 3)])
    sb = G.stream(s, [f"%{34 + i}" for i in range(8)], [f"%{42 + i}" for i in range(8)], p, "%58", "%17",
                  [(4, 5), (6, 7)])
    ops = [x for pr in zip(sa, sb) for x in pr]
    recs = F.table("fe_mul_lazy2")
    assert 2 * len(recs) <= 3000
    for (a, b, c, d), want in zip(recs, F.expected("fe_mul_lazy2")):
        regs = F._mont_regs(a, b, 18, 26, 50, "%58")
        regs.update(F._mont_regs(c, d, 34, 42))
        R = F._emulate(ops, regs)
        assert (F._out(R, 0), F._out(R, 8)) == want, [hex(v) for v in (a, b, c, d)]
    wide = [(a >= F.LAZY_R, c >= F.LAZY_R) for a, _, c, _ in recs[:1200]]
    assert all(wide.count(k) >= 290 for k in [(False, False), (True, True), (True, False), (False, True)])


def test_shoup_table():
    """Emulator, integer formula and contract agree; the flag the emulator ends with is shoup_flag; the lane
    layout holds: a wave without a flagged lane, one all short, single short lanes at 0, 31, 32 and 63,
    alternating waves, flagged lanes whose quotient is exact, and short lanes in the partial last wave.

    Flagged lanes with an exact quotient do not occur among the random or the 2^100 cases; they are built as
    a wq = -1 (mod 2^256), which every candidate with an odd wq satisfies (none had to be searched for)."""
    recs = F.table("fe_mul_shoup")
    assert len(recs) <= 3000
    flag_reg = f"%{F._SHOUP_OPS[2] + 1}"
    short, flagged = [], []
    for (a, w), (want,) in zip(recs, F.expected("fe_mul_shoup")):
        c = {}
        assert F._shoup(F._SHOUP_OPS, a, w, c) == want == F.shoup_int(a, w), (hex(a), hex(w))
        assert want < 2 * P and want % P == a * w % P
        flagged.append(F.shoup_flag(a, w))
        assert c[flag_reg] == flagged[-1]
        short.append(F._short_quotient(a, w))
        assert flagged[-1] or not short[-1]               # a short quotient is always flagged
    assert sum(short) >= 200
    for wv, lanes in F.SHOUP_WAVES.items():
        assert [lane for lane in range(64) if short[64 * wv + lane]] == lanes, wv
        assert [lane for lane in range(64) if flagged[64 * wv + lane]] == lanes, wv
    assert sum(short[64:128]) == 64                       # (at least 64 in one wave)
    e = 64 * F.SHOUP_EXACT_WAVE
    assert [lane for lane in range(64) if flagged[e + lane]] == F.SHOUP_EXACT_LANES and not any(short[e:e + 64])
    assert sum(f and not s for f, s in zip(flagged, short)) >= 40
    tail = len(recs) - 37
    assert [lane for lane in range(37) if short[tail + lane]] == F.SHOUP_TAIL_SHORT
    assert any(lane % 2 for lane in F.SHOUP_TAIL_SHORT)   # (one of them runs in mode 1 too)


@pytest.mark.parametrize("op", ["fe_mul_db", "fe_mul_db_uniform"])
def test_db_tables(op):
    recs, want = F.table(op), F.expected(op)
    assert len(recs) <= 3000
    for (a, w), (r,) in zip(recs, want):
        assert r < 2 * P and (r - a * w) % P == 0, (hex(a), hex(w))
    assert sum(r == P for (r,) in want) >= 1               # a quotient one short on a w = k p exactly
    assert {w for _, w in recs} >= set(F.DB_EDGES_W) and {a for a, _ in recs} >= set(F.DB_EDGES_A)
    assert sum(4 * P <= a < F.LAZY_R for a, _ in recs) >= (500 if op == "fe_mul_db" else 100)
    if op == "fe_mul_db":
        assert sum(a in (P, 2 * P, 3 * P) and w > 2 for a, w in recs) >= 900
        assert sum(0 < -a % P < (1 << 20) for a, _ in recs) >= 300
    else:
        for wv in range(len(recs) // 64 + 1):
            assert len({w for _, w in recs[64 * wv: 64 * wv + 64]}) == 1, wv     # one constant per wave
        mp = [wv for wv in range(len(recs) // 64) if all(a in (P, 2 * P, 3 * P) for a, _ in recs[64 * wv:64 * wv + 64])]
        assert len(mp) == F.DB_UNIFORM_MP_WAVES


def _has_alternating_wave(tops):
    """Two waves whose lanes alternate above / not above 2p's top word, one starting each way."""
    starts = set()
    for wv in range(len(tops) // 64):
        t = tops[64 * wv: 64 * wv + 64]
        if all(t[k] != t[k + 1] for k in range(63)):
            starts.add(t[0])
    return starts == {False, True}


@pytest.mark.parametrize("op", ["csub2p_top", "csub2p_t_fast", "reduce_full_fast", "bfly_fast", "sub2p"])
def test_top_word_classes(op):
    xs = [rec[0] for rec in F.table(op)]
    top = TOP2P << 224
    for v in (2 * P, top, top + (1 << 224) - 1, top + (1 << 224), 3 * P, 4 * P, F.LAZY_R - 1):
        assert v in xs or (op == "sub2p" and v < 2 * P), hex(v)      # (sub2p takes operands from 2p up only)
    assert sum((x >> 224) == TOP2P for x in xs) >= 4       # top word equal: below, at and above 2p
    assert any((x >> 224) == TOP2P and x > 2 * P for x in xs)
    assert op == "sub2p" or any((x >> 224) == TOP2P and x < 2 * P for x in xs)
    assert sum(4 * P <= x < F.LAZY_R for x in xs) >= 32
    if op != "sub2p":
        assert 0 in xs and _has_alternating_wave([(x >> 224) > TOP2P for x in xs])


@pytest.mark.parametrize("op", ["bfly_fast", "bfly", "fe_bfly_lazy", "fe_bfly_lazy_reduced"])
def test_butterfly_classes(op):
    ys = [y for _, y in F.expected(op)]
    assert {P, 2 * P, 3 * P} <= set(ys) if op != "fe_bfly_lazy_reduced" else {P, 2 * P} <= set(ys)
    assert any(t == 0 for _, t in F.table(op)) and any(t == 2 * P - 1 for _, t in F.table(op))


@pytest.mark.parametrize("op", ["fe_csub2p", "fe_reduce_lazy", "csub2p_t", "reduce_full"])
def test_lazy_classes(op):
    xs = [rec[0] for rec in F.table(op)]
    assert {0, 2 * P - 1, 2 * P, 2 * P + 1, 3 * P, 4 * P - 1} <= set(xs)
    eq = [x for x in xs if (x >> 224) == TOP2P]
    assert any(x < 2 * P for x in eq) and 2 * P in eq and any(x > 2 * P for x in eq) and len(eq) >= 15


def test_canonical_classes():
    for op in ("fe_add", "fe_add_raw", "fe_sub"):
        recs = F.table(op)
        assert {P - 1, P, P + 1, 2 * P - 2} <= {a + b for a, b in recs}
        assert sum(a == b for a, b in recs) >= 20 and sum(a == b - 1 for a, b in recs) >= 20
        assert (0, P - 1) in recs and ((1 << 224) - 1, 1) in recs and (0, 1) in recs
        assert any(F.M32 in F._limbs(a + b) for a, b in recs)
    once = [t for (t,) in F.table("fe_reduce_once")]
    assert {0, P - 1, P, P + 1, 2 * P - 1, P - (1 << 32), P + (1 << 224)} <= set(once)
    assert any(a + b == F.R256 - 1 for a, b in F.table("fe_add_raw"))
    zero = F.table("fe_is_zero")
    assert (0,) in zero and all(((1 << (32 * k)),) in zero for k in range(8))


def test_mode_1_copies_even_lanes():
    for op in ("fe_sub", "bfly_fast", "fe_mul_shoup"):
        m0, m1 = F.expected_array(op, 0), F.expected_array(op, 1)
        ins = F.encode(op, F.table(op))
        assert (m1[1::2] == m0[1::2]).all()
        for k in range(F.OPS[op][2]):
            assert (m1[0::2, 8 * k: 8 * k + 8] == ins[0::2, :8]).all()
