"""CPU: the generated modular products (tools/gen_fe_mul_asm.py, the inline asm in
stark-pure-rust_amd/csrc/fe_mul_asm.inc) emulated instruction by instruction with exact
integers for one lane: v_mad_u64_u32 / v_addc_co_u32 / v_sub(b)_co_u32 carry semantics, the
alternating accumulator pairs, the column shifts and the Shoup product's rare-correction branch.
  * Montgomery (single and the interleaved dual form): a*b*2^-256 mod p in [0, 2p) for any a < 2^256, b < p
    (a < 4p + 2^224 is the NTT passes' lazy range; the rest is the verifier's, which multiplies 32 bytes as
    they come by R^2 mod p);
  * Shoup: a*w mod p in [0, 2p) for any a < 2^256, including inputs built to make the truncated
    quotient one short (the flagged correction path)."""
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gen_fe_mul_asm as G  # noqa: E402

from fe_cases import (P, PINV, R256, _emulate, _mont_cases, _mont_regs, _mont_wide_cases, _out,  # noqa: E402
                      _shoup, _shoup_ops, _short_quotient)  # (the one-lane interpreter and the case lists)


def test_generated_montgomery_product():
    assert PINV == 0xEFFFFFFF  # STARK_PINV32 in fp_dev.h
    r = [f"%{i}" for i in range(8)]
    ops = G.stream(r, [f"%{9 + i}" for i in range(8)], [f"%{17 + i}" for i in range(8)],
                   [f"%{25 + i}" for i in range(8)], "%33", "%8", [(0, 1), (2, 3)])
    rinv = pow(R256, -1, P)
    for a, b in _mont_cases() + _mont_wide_cases():
        out = _out(_emulate(ops, _mont_regs(a, b, 9, 17, 25, "%33")), 0)
        assert out < 2 * P
        assert out % P == a * b * rinv % P


def test_generated_dual_product():
    """fe_mul_lazy2: two Montgomery products interleaved one for one (emit_dual's operand map)."""
    r, s = [f"%{i}" for i in range(8)], [f"%{8 + i}" for i in range(8)]
    p = [f"%{50 + i}" for i in range(8)]
    sa = G.stream(r, [f"%{18 + i}" for i in range(8)], [f"%{26 + i}" for i in range(8)], p, "%58", "%16",
                  [(0, 1), (2, 3)])
    sb = G.stream(s, [f"%{34 + i}" for i in range(8)], [f"%{42 + i}" for i in range(8)], p, "%58", "%17",
                  [(4, 5), (6, 7)])
    ops = [x for pr in zip(sa, sb) for x in pr]
    rinv = pow(R256, -1, P)
    cases, wide = _mont_cases(), _mont_wide_cases()
    half = len(wide) // 2
    pairs = list(zip(cases[:700], cases[700:1400])) + list(zip(wide[:half], wide[half:2 * half]))
    pairs += list(zip(wide[:300], cases[:300])) + list(zip(cases[300:600], wide[300:600]))  # wide beside narrow
    for (a, b), (c, d) in pairs:
        regs = _mont_regs(a, b, 18, 26, 50, "%58")
        regs.update(_mont_regs(c, d, 34, 42))
        R = _emulate(ops, regs)
        x, y = _out(R, 0), _out(R, 8)
        assert x < 2 * P and y < 2 * P
        assert x % P == a * b * rinv % P and y % P == c * d * rinv % P


@pytest.mark.parametrize("qbase,rbase", [(None, None), (4, None), (4, 20), (4, 36)])
def test_generated_shoup_product(qbase, rbase):
    assert sum(x << (32 * i) for i, x in enumerate(G.NP)) == R256 - P
    assert sum(x << (32 * i) for i, x in enumerate(G.P2)) == 2 * P
    ops = _shoup_ops(qbase, rbase)
    rnd = random.Random(11)
    cases = [(0, 0), (R256 - 1, P - 1), (4 * P - 1, P - 1), (1, 1), (R256 - 1, 1)]
    cases += [(rnd.randrange(4 * P), rnd.randrange(P)) for _ in range(800)]
    cases += [(rnd.randrange(R256), rnd.randrange(P)) for _ in range(400)]
    short = 0
    for _ in range(400):                      # a*wq = 2^100 mod 2^256: the dropped columns carry
        w = rnd.randrange(P)
        wq = w * R256 // P
        if wq % 2:
            a = (1 << 100) * pow(wq, -1, R256) % R256
            cases.append((a, w))
    for a, w in cases:
        r = _shoup(ops, a, w)
        short += _short_quotient(a, w)
        assert r < 2 * P, (a, w)
        assert r % P == a * w % P
    assert short > 50                         # the correction path was exercised


def test_committed_asm_is_generated():
    """fe_mul_asm.inc is exactly the generator's output."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_fe_mul_asm.py")], capture_output=True,
                         text=True, check=True).stdout
    inc = open(os.path.join(ROOT, "stark-pure-rust_amd", "csrc", "fe_mul_asm.inc")).read()
    assert out == inc
