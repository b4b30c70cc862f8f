"""Directed operands and exact expected values for the device field primitives (csrc/fp_dev.h, fe_mul_asm.inc,
fe_db.h and the lazy-range helpers of csrc/ntt.hip), shared by tests/test_fe_cases_cpu.py (the tables keep their
preconditions and their classes) and tests/test_gpu_fe_ops.py (the library's hook stark_test_fe_op runs them,
record i in lane i % 64 of wave i / 64).  Also the one-lane interpreter of the generated instruction lists that
tests/test_fe_mul_asm.py checks the generator with.

Every table: directed cases, random fill to a multiple of 64, then 37 more records (a partial last wave).
Expected values are plain-integer formulas, except the Shoup and digit-basis products, whose value within
[0, 2p) depends on a truncated quotient: theirs is the emulator's (_shoup, tools/db_check.py:db_emulate)."""
import functools
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import db_check as D  # noqa: E402
import gen_fe_mul_asm as G  # noqa: E402

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
M32 = (1 << 32) - 1
PINV = (-pow(P, -1, 1 << 32)) % (1 << 32)
R256 = 1 << 256
PINV256 = (-pow(P, -1, R256)) % R256
TOP2P = 0x60C89CE5                    # 2p's top word (STARK_2P7)
LAZY_R = 4 * P + (1 << 224)           # the radix-2^6 passes' lazy range is [0, LAZY_R)
assert (2 * P) >> 224 == TOP2P and D.P == P


def _limbs(x):
    return [(x >> (32 * i)) & M32 for i in range(8)]


def _emulate(ops, regs: dict, carries=None) -> dict:
    """Runs one lane of `ops` (exec = this lane) over `regs` (operand name -> u32).  `carries` (optional)
    receives the final carry / mask SGPR pairs by operand name."""
    R = dict(regs)
    C = {"scc": 0}          # carry / mask SGPR pairs (one lane: 0 or 1)

    def val(x):
        if x == "0":
            return 0
        if x.startswith("0x"):
            return int(x, 16)
        if x.lstrip("-").isdigit():
            return int(x) & M32
        if x.startswith("v["):
            lo, hi = map(int, x[2:-1].split(":"))
            assert lo % 2 == 0 and hi == lo + 1, "64-bit operands are even-aligned pairs"
            return R[f"v{lo}"] | (R[f"v{hi}"] << 32)
        return R[x]

    def setv(x, v):
        if x.startswith("v["):
            lo, hi = map(int, x[2:-1].split(":"))
            R[f"v{lo}"], R[f"v{hi}"] = v & M32, (v >> 32) & M32
        else:
            R[x] = v & M32

    labels = {op[:-1]: i for i, op in enumerate(ops) if op.endswith(":")}
    pc = 0
    while pc < len(ops):
        op = ops[pc]
        pc += 1
        if op.endswith(":"):
            continue
        name, rest = op.split(" ", 1)
        args = [t.strip() for t in rest.split(",")]
        if name == "v_mad_u64_u32":
            d, c, x, y, s2 = args
            res = val(x) * val(y) + val(s2)
            C[c] = res >> 64
            setv(d, res)
        elif name in ("v_addc_co_u32", "v_addc_co_u32_e32"):
            d, c, x, y, ci = args
            s = val(x) + val(y) + C[ci]
            C[c] = s >> 32
            setv(d, s)
        elif name == "v_sub_co_u32":
            d, c, x, y = args
            s = val(x) - val(y)
            C[c] = 1 if s < 0 else 0
            setv(d, s)
        elif name == "v_subb_co_u32":
            d, c, x, y, ci = args
            s = val(x) - val(y) - C[ci]
            C[c] = 1 if s < 0 else 0
            setv(d, s)
        elif name == "v_cndmask_b32":
            d, x, y, m = args
            setv(d, val(y) if C[m] else val(x))
        elif name == "v_mul_lo_u32":
            d, x, y = args
            setv(d, val(x) * val(y))
        elif name == "v_mov_b32":
            d, x = args
            setv(d, val(x))
        elif name == "v_cmp_lt_u32":
            d, x, y = args
            C[d] = 1 if val(x) < val(y) else 0
        elif name == "s_and_b64":
            d, x, y = args
            C[d] = C[x] & (1 if y == "exec" else C[y])
        elif name == "s_cmp_eq_u64":
            x, y = args
            C["scc"] = 1 if C[x] == int(y) else 0
        elif name == "s_cbranch_scc1":
            if C["scc"]:
                pc = labels[args[0]]
        else:
            raise AssertionError(f"unexpected instruction {op}")
    if carries is not None:
        carries.update(C)
    return R


def _mont_regs(a, b, base_a, base_b, base_p=None, pinv=None):
    regs = {}
    for i, (x, y) in enumerate(zip(_limbs(a), _limbs(b))):
        regs[f"%{base_a + i}"] = x
        regs[f"%{base_b + i}"] = y
    if base_p is not None:
        for i, x in enumerate(_limbs(P)):
            regs[f"%{base_p + i}"] = x
        regs[pinv] = PINV
    return regs


def _out(R, base):
    return sum(R[f"%{base + i}"] << (32 * i) for i in range(8))


def _mont_cases():
    rnd = random.Random(7)
    # [0, 4p + 2^224): the lazy range of the radix-2^6 NTT passes, whose butterflies reduce by 2p only
    # when the top word exceeds 2p's (csrc/ntt.hip)
    top = 4 * P + (1 << 224) - 1
    cases = [(0, 0), (1, 1), (P - 1, P - 1), (4 * P - 1, P - 1), (4 * P - 1, 1), (2 ** 255, P - 1),
             (top, P - 1), (top, 1), (top, top % P)]
    return cases + [(rnd.randrange(4 * P), rnd.randrange(P)) for _ in range(1500)] + \
        [(rnd.randrange(4 * P, top + 1), rnd.randrange(P)) for _ in range(200)]


def _mont_wide_cases():
    """a in [4p + 2^224, 2^256): what csrc/verify_batch.hip's arena_mont and its I2 matrix kernel hand the product,
    a leaf's or a public wire's 32 bytes as they are, against b = R^2 mod p (arena_mont's) and any b < p."""
    rnd = random.Random(13)
    lo, r2 = 4 * P + (1 << 224), R256 * R256 % P
    assert 4 * P < lo < 5 * P - 1 < R256
    edges = [R256 - 1, 5 * P - 1, 5 * P, lo]
    cases = [(a, b) for a in edges for b in (r2, P - 1, 1, 0)]
    cases += [(rnd.randrange(lo, R256), r2) for _ in range(700)]
    return cases + [(rnd.randrange(lo, R256), rnd.randrange(P)) for _ in range(700)]


def _shoup_ops(qbase=None, rbase=None):
    """emit_shoup's operand map: r = %0..%7 (or pinned v[rbase + 2c]), q = %8.. unless in place,
    then cy, flag, a, w, wq, 2^256 - p."""
    r = [f"%{i}" for i in range(8)] if rbase is None else [f"v{rbase + 2 * i}" for i in range(8)]
    nq = 0 if qbase is not None else 8
    q = [f"%{8 + i}" for i in range(nq)]
    b = 8 + nq
    ops = G.shoup_stream(r, q, [f"%{b + 2 + i}" for i in range(8)], [f"%{b + 10 + i}" for i in range(8)],
                         [f"%{b + 18 + i}" for i in range(8)], [f"%{b + 26 + i}" for i in range(8)], f"%{b}",
                         [(0, 1), (2, 3)], f"%{b + 1}", qbase, rbase)
    tmp = q if qbase is None else [f"v{qbase + 2 * i}" for i in range(8)]
    return ops + G.csub2p_block(r, tmp, "a", f"%{b + 1}", G.P2), r, b


def _shoup(opsr, a, w, carries=None):
    ops, r, b = opsr
    wq = w * R256 // P
    regs = {}
    for i in range(8):
        regs[f"%{b + 2 + i}"] = _limbs(a)[i]
        regs[f"%{b + 10 + i}"] = _limbs(w)[i]
        regs[f"%{b + 18 + i}"] = _limbs(wq)[i]
        regs[f"%{b + 26 + i}"] = G.NP[i]
    R = _emulate([o.replace("%=", "") for o in ops], regs, carries)
    return sum(R[r[i]] << (32 * i) for i in range(8))


def _short_quotient(a, w):
    wq = w * R256 // P
    lo = sum(((a >> (32 * k)) & M32) * ((wq >> (32 * (c - k))) & M32) << (32 * c)
             for c in range(6) for k in range(c + 1))
    return (a * wq - lo) // R256 != a * wq // R256


# ---- integer formulas --------------------------------------------------------------------------------------

def mont_lazy(a, b):
    """fe_mul_lazy: Montgomery reduction of a b by 2^256, not reduced below p."""
    t = a * b
    return (t + (t * PINV256 % R256) * P) >> 256


def csub2p(t):
    return t - 2 * P if t >= 2 * P else t


def csub2p_top(t):
    return t - 2 * P if (t >> 224) > TOP2P else t


def shoup_flag(a, w):
    """The correction flag of fe_mul_shoup: the column-7 word of the truncated a * wq is >= 2^32 - 8."""
    al, ql = _limbs(a), _limbs(w * R256 // P)
    c6 = sum(al[i] * ql[6 - i] for i in range(7))
    c7 = sum(al[i] * ql[7 - i] for i in range(8))
    return ((c6 >> 32) + c7) & M32 >= (1 << 32) - 8


def shoup_int(a, w):
    """fe_mul_shoup in integers: the truncated quotient, r = a w - q p, and 2p off a flagged lane's r >= 2p."""
    wq = w * R256 // P
    lo = sum(((a >> (32 * k)) & M32) * ((wq >> (32 * (c - k))) & M32) << (32 * c)
             for c in range(6) for k in range(c + 1))
    r = (a * w - ((a * wq - lo) >> 256) * P) % R256
    return r - 2 * P if shoup_flag(a, w) and r >= 2 * P else r


# ---- ops: name -> (the hook's op number, elements read, elements written) ---------------------------------

OPS = {
    "fe_add": (0, 2, 1), "fe_add_raw": (1, 2, 1), "fe_sub": (2, 2, 1), "fe_reduce_once": (3, 1, 1),
    "fe_csub2p": (4, 1, 1), "fe_bfly_lazy": (5, 2, 2), "fe_bfly_lazy_reduced": (6, 2, 2), "fe_reduce_lazy": (7, 1, 1),
    "fe_mul": (8, 2, 1), "fe_mul_lazy": (9, 2, 1), "fe_mul_lazy2": (10, 4, 2), "fe_mul_shoup": (11, 3, 1),
    "fe_mul_db": (12, 10, 1), "fe_mul_db_uniform": (13, 10, 1), "sub2p": (14, 1, 1), "csub2p_top": (15, 1, 1),
    "bfly_fast": (16, 2, 2), "bfly": (17, 2, 2), "csub2p_t_fast": (18, 1, 1), "csub2p_t": (19, 1, 1),
    "reduce_full_fast": (20, 1, 1), "reduce_full": (21, 1, 1), "fe_is_zero": (22, 1, 1),
}
N_OPS = 23

# A record is the tuple of the op's logical operands: (a, w) for the constant products, whose wq and
# digit-basis table `encode` derives.  PRE: the precondition the primitive's comment states.
PRE = {
    "fe_add": lambda a, b: a < P and b < P,
    "fe_add_raw": lambda a, b: a + b < R256,
    "fe_sub": lambda a, b: a < P and b < P,
    "fe_reduce_once": lambda t: t < 2 * P,
    "fe_csub2p": lambda t: t < 4 * P,
    "fe_bfly_lazy": lambda x, t: x < 4 * P and t < 2 * P,
    "fe_bfly_lazy_reduced": lambda x, t: x < 2 * P and t < 2 * P,
    "fe_reduce_lazy": lambda t: t < 4 * P,
    "fe_mul": lambda a, b: a < R256 and b < P,
    "fe_mul_lazy": lambda a, b: a < R256 and b < R256 and a * b < R256 * P,
    "fe_mul_lazy2": lambda a, b, c, d: max(a, b, c, d) < R256 and a * b < R256 * P and c * d < R256 * P,
    "fe_mul_shoup": lambda a, w: a < R256 and w < P,
    "fe_mul_db": lambda a, w: a < LAZY_R and w < P,
    "fe_mul_db_uniform": lambda a, w: a < LAZY_R and w < P,
    "sub2p": lambda t: 2 * P <= t < LAZY_R,
    "csub2p_top": lambda t: t < LAZY_R,
    "bfly_fast": lambda x, t: x < LAZY_R and t < 2 * P,
    "bfly": lambda x, t: x < 4 * P and t < 2 * P,          # (fe_bfly_lazy's X range)
    "csub2p_t_fast": lambda t: t < LAZY_R,
    "csub2p_t": lambda t: t < 4 * P,                       # (fe_csub2p's range)
    "reduce_full_fast": lambda t: t < LAZY_R,
    "reduce_full": lambda t: t < 4 * P,
    "fe_is_zero": lambda t: t < R256,
}

_SHOUP_OPS = _shoup_ops()

WANT = {
    "fe_add": lambda a, b: ((a + b) % P,),
    "fe_add_raw": lambda a, b: (a + b,),
    "fe_sub": lambda a, b: ((a - b) % P,),
    "fe_reduce_once": lambda t: (t % P,),
    "fe_csub2p": lambda t: (csub2p(t),),
    "fe_bfly_lazy": lambda x, t: (csub2p(x) + t, csub2p(x) + 2 * P - t),
    "fe_bfly_lazy_reduced": lambda x, t: (x + t, x + 2 * P - t),
    "fe_reduce_lazy": lambda t: (t % P,),
    "fe_mul": lambda a, b: (a * b * pow(R256, -1, P) % P,),
    "fe_mul_lazy": lambda a, b: (mont_lazy(a, b),),
    "fe_mul_lazy2": lambda a, b, c, d: (mont_lazy(a, b), mont_lazy(c, d)),
    "fe_mul_shoup": lambda a, w: (_shoup(_SHOUP_OPS, a, w),),
    "fe_mul_db": lambda a, w: (D.db_emulate(a, D.db_table(w)),),
    "fe_mul_db_uniform": lambda a, w: (D.db_emulate(a, D.db_table(w)),),
    "sub2p": lambda t: (t - 2 * P,),
    "csub2p_top": lambda t: (csub2p_top(t),),
    "bfly_fast": lambda x, t: (csub2p_top(x) + t, csub2p_top(x) + 2 * P - t),
    "bfly": lambda x, t: (csub2p(x) + t, csub2p(x) + 2 * P - t),
    "csub2p_t_fast": lambda t: (csub2p(csub2p_top(t)),),
    "csub2p_t": lambda t: (csub2p(t),),
    "reduce_full_fast": lambda t: (t % P,),
    "reduce_full": lambda t: (t % P,),
    "fe_is_zero": lambda t: (1 if t == 0 else 0,),
}


# ---- case tables -------------------------------------------------------------------------------------------

def _finish(recs, gen, seed, fill=64):
    """`fill` random records, more up to a multiple of 64, then 37: the last wave is partial."""
    rnd = random.Random(seed)
    recs = list(recs) + [gen(rnd) for _ in range(fill)]
    while len(recs) % 64:
        recs.append(gen(rnd))
    return recs + [gen(rnd) for _ in range(37)]


def _pad(recs, gen, rnd):
    while len(recs) % 64:
        recs.append(gen(rnd))


def _boundaries(limit):
    """0, 1, p - 1, the halves of p, 2^224 (- 1), the 32-bit word boundaries +- 1 and single all-ones words."""
    v = {0, 1, P - 1, (P - 1) // 2, (P + 1) // 2, 1 << 224, (1 << 224) - 1}
    for k in range(1, 8):
        v |= {(1 << (32 * k)) - 1, 1 << (32 * k), (1 << (32 * k)) + 1, M32 << (32 * k)}
    return sorted(x for x in v if x < limit)


def _canonical_pairs():
    """fe_add / fe_sub: every pair of boundary values (a == b, 0 against p - 1, 2^224 - 1 against 1 among them),
    a + b in {p - 1, p, p + 1, 2p - 2}, a = b -+ 1."""
    rnd = random.Random(21)
    v = _boundaries(P)
    pairs = [(a, b) for a in v for b in v]
    for a in v + [rnd.randrange(P) for _ in range(24)]:
        for s in (P - 1, P, P + 1, 2 * P - 2):
            if 0 <= s - a < P:
                pairs.append((a, s - a))
        if a:
            pairs += [(a - 1, a), (a, a - 1)]
        pairs.append((a, a))
    return pairs


def _rand_pair_canonical(rnd):
    return rnd.randrange(P), rnd.randrange(P)


def _rand_pair_raw(rnd):
    a = rnd.randrange(R256)
    return a, rnd.randrange(R256 - a)


def _word_steps(x, words):
    """x with one word one lower / one higher (x's words are neither 0 nor all ones where this is used)."""
    return [x + s * (1 << (32 * k)) for k in words for s in (-1, 1)]


def _lazy4_values():
    """fe_csub2p / fe_reduce_lazy: around p, 2p, 3p, 4p, and 2p's top word over lower words below, equal to and
    above 2p's."""
    top = TOP2P << 224
    v = [0, 2 * P - 1, 2 * P, 2 * P + 1, 3 * P, 4 * P - 1, 1, P - 1, P, P + 1, 3 * P - 1, 3 * P + 1]
    v += _word_steps(2 * P, range(7)) + [top, top + (1 << 224) - 1, top + (1 << 224)]
    return v


def _top_values():
    """The [0, 4p + 2^224) helpers: the top word below, at and above 2p's."""
    top = TOP2P << 224
    v = [0, 2 * P, top, top + (1 << 224) - 1, top + (1 << 224), 3 * P, 4 * P, LAZY_R - 1]
    v += [1, P - 1, P, P + 1, 2 * P - 1, 2 * P + 1, 3 * P - 1, 3 * P + 1, 4 * P - 1, 4 * P + 1, top + (2 << 224) - 1]
    return v + _word_steps(2 * P, range(7))


def _rand_top(rnd):
    return rnd.randrange(4 * P, LAZY_R) if rnd.random() < 0.5 else rnd.randrange(LAZY_R)


def _alternating(rnd, n_waves=2):
    """Waves whose lanes alternate between `top word above 2p's` and `not above`: the even lanes above in the
    first wave, the odd ones in the second."""
    out = []
    for wv in range(n_waves):
        for lane in range(64):
            above = (lane + wv) % 2 == 0
            out.append(rnd.randrange((TOP2P + 1) << 224, LAZY_R) if above else rnd.randrange((TOP2P + 1) << 224))
    return out


def _t_values(x):
    """A butterfly's T against X: 0, 1, p, 2p - 1 and X' = T (mod p and mod 2p), +- 1."""
    m = x % (2 * P)
    return sorted({t for t in (0, 1, P, 2 * P - 1, m, m - 1, m + 1, x % P, x % P + P) if 0 <= t < 2 * P})


def _unary(values, limit_gen, seed, alternating=False, keep=lambda t: True):
    rnd = random.Random(seed)
    recs = [(t,) for t in values if keep(t)]
    if alternating:
        _pad(recs, limit_gen, rnd)
        recs += [(t,) for t in _alternating(rnd) if keep(t)]
    return _finish(recs, limit_gen, seed + 1)


def _bfly_table(xs, gen_x, seed, alternating=False):
    rnd = random.Random(seed)

    def gen(r):
        return gen_x(r)[0], r.randrange(2 * P)
    recs = [(x, t) for x in xs for t in _t_values(x)]
    if alternating:
        _pad(recs, gen, rnd)
        recs += [(x, rnd.choice(_t_values(x) + [rnd.randrange(2 * P)])) for x in _alternating(rnd)]
    return _finish(recs, gen, seed + 1)


def _mont_narrow():
    c = _mont_cases()
    return c[:9] + c[9:509] + c[1509:1609]          # the edges, 500 in [0, 4p), 100 in [4p, 4p + 2^224)


def _mont_wide():
    c = _mont_wide_cases()
    return c[:16] + c[16:316] + c[716:1016]         # the edges, 300 against R^2 mod p, 300 against any b < p


def _rand_mont(rnd):
    return rnd.randrange(R256), rnd.randrange(P)


@functools.lru_cache(maxsize=None)
def shoup_pools():
    """test_generated_shoup_product's edges and random cases (no lane of which is flagged), constructed short
    quotients (a wq = 2^100 mod 2^256: the dropped columns carry) and constructed flagged lanes whose quotient
    is exact (a wq = -1 mod 2^256: the column-7 word is 2^32 - 1 - the dropped columns' top, nothing carries)."""
    rnd = random.Random(11)
    edges = [(0, 0), (R256 - 1, P - 1), (4 * P - 1, P - 1), (1, 1), (R256 - 1, 1)]
    plain = [(rnd.randrange(4 * P), rnd.randrange(P)) for _ in range(800)]
    plain += [(rnd.randrange(R256), rnd.randrange(P)) for _ in range(400)]
    short, exact, tried = [], [], 0
    while len(short) < 330 and tried < 1 << 16:
        tried += 1
        w = rnd.randrange(P)
        wq = w * R256 // P
        if wq % 2:
            a = (1 << 100) * pow(wq, -1, R256) % R256
            if _short_quotient(a, w):
                short.append((a, w))
            a = -pow(wq, -1, R256) % R256
            if len(exact) < 48 and shoup_flag(a, w) and not _short_quotient(a, w):
                exact.append((a, w))
    return edges, plain, short, exact


# fe_mul_shoup's table starts with these waves (wave index -> lanes holding a short quotient)
SHOUP_WAVES = {0: [], 1: list(range(64)), 2: [0], 3: [31], 4: [32], 5: [63], 6: list(range(0, 64, 2)),
               7: list(range(1, 64, 2))}
SHOUP_EXACT_WAVE, SHOUP_EXACT_LANES = 8, [5, 31, 40, 63]    # flagged lanes whose quotient is exact
SHOUP_TAIL_SHORT = [3, 10]                                  # short lanes of the partial last wave


def _shoup_table():
    edges, plain, short, exact = shoup_pools()
    plain = [c for c in plain if not shoup_flag(*c)]
    short, exact, pl = list(short), list(exact), iter(plain)
    recs = []
    for wv in range(9):
        lanes = SHOUP_WAVES.get(wv, [])
        for lane in range(64):
            if wv == SHOUP_EXACT_WAVE and lane in SHOUP_EXACT_LANES:
                recs.append(exact.pop())
            else:
                recs.append(short.pop() if lane in lanes else next(pl))
    recs += edges + list(pl) + short[:-len(SHOUP_TAIL_SHORT)] + exact
    rnd = random.Random(12)
    _pad(recs, _rand_mont, rnd)
    tail = [_rand_mont(rnd) for _ in range(37)]
    for k, lane in enumerate(SHOUP_TAIL_SHORT):
        tail[lane] = short[-1 - k]
    return recs + tail


DB_EDGES_A = [0, 1, P - 1, P, 2 * P - 1, 2 * P, 3 * P, 4 * P - 1, 1 << 255, (1 << 224) * 0xC19139CB, LAZY_R - 1]
DB_EDGES_W = [0, 1, 2, P - 1, (P + 1) // 2, pow(7, (P - 1) // 4, P)]


def _db_margin_cases():
    """tests/test_fe_db.py test_quotient_next_to_margin: a w = k p exactly, and just below."""
    rng = random.Random(12)
    exact = [(m * P, w) for w in (rng.randrange(1, P) for _ in range(300)) for m in (1, 2, 3)]
    below = []
    for _ in range(300):
        w = rng.randrange(1, P)
        below.append((rng.randrange(1, 4) * P - rng.randrange(1, 1 << 20), w))
    return exact, below


def _rand_db(rnd):
    return rnd.randrange(LAZY_R), rnd.randrange(P)


def _db_table():
    rng = random.Random(11)
    recs = [(a, w) for a in DB_EDGES_A for w in DB_EDGES_W]
    recs += [(rng.randrange(4 * P, LAZY_R), rng.randrange(P)) for _ in range(500)]
    exact, below = _db_margin_cases()
    return _finish(recs + exact + below, _rand_db, 14, fill=0)


DB_UNIFORM_MP_WAVES = 7      # waves (after the edge constants' six) whose 64 a values are p, 2p, 3p


def _db_uniform_table():
    """One w per wave: the edge constants over edge and random a, then waves of a = m p, then random."""
    rng = random.Random(15)
    recs = []
    for w in DB_EDGES_W:
        recs += [(a, w) for a in DB_EDGES_A + [_rand_top(rng) for _ in range(64 - len(DB_EDGES_A))]]
    for k in range(DB_UNIFORM_MP_WAVES):
        w = 1 if k == 0 else rng.randrange(1, P)
        recs += [((1 + lane % 3) * P, w) for lane in range(64)]
    for _ in range(8):
        w = rng.randrange(1, P)
        recs += [(rng.randrange(1, 5) * P - rng.randrange(1, 1 << 20) if lane % 2 else _rand_top(rng), w)
                 for lane in range(64)]
    w = rng.randrange(1, P)
    return recs + [((1 + lane % 3) * P if lane % 4 == 1 else _rand_top(rng), w) for lane in range(37)]


def _dual_pairs():
    """test_generated_dual_product's pairing: narrow with narrow, wide with wide, wide beside narrow both ways."""
    n, w = _mont_narrow(), _mont_wide()
    pairs = list(zip(n[:300], n[300:600])) + list(zip(w[:300], w[300:600]))
    pairs += list(zip(w[:300], n[:300])) + list(zip(n[300:600], w[300:600]))
    return [ab + cd for ab, cd in pairs]


def _is_zero_values():
    v = [0, 1, R256 - 1, P]
    for k in range(8):
        v += [1 << (32 * k), 1 << (32 * k + 31), M32 << (32 * k), R256 - 1 - (M32 << (32 * k))]
    return v


_TABLES = {
    "fe_add": lambda: _finish(_canonical_pairs(), _rand_pair_canonical, 31),
    "fe_sub": lambda: _finish(_canonical_pairs(), _rand_pair_canonical, 32),
    "fe_add_raw": lambda: _finish(
        _canonical_pairs() + [(4 * P - 1, 1 << 224), (LAZY_R - 1, R256 - LAZY_R), (R256 - 1, 0), (0, R256 - 1),
                              (R256 - 2, 1), (1 << 255, (1 << 255) - 1), (2 * P, 2 * P - 1), (2 * P - 1, 2 * P)] +
        [(R256 - 1 - x, x) for x in _boundaries(R256)], _rand_pair_raw, 33),
    "fe_reduce_once": lambda: _unary(
        [0, P - 1, P, P + 1, 2 * P - 1] + _word_steps(P, range(8)) + _boundaries(2 * P),
        lambda r: (r.randrange(2 * P),), 34),
    "fe_csub2p": lambda: _unary(_lazy4_values(), lambda r: (r.randrange(4 * P),), 35),
    "fe_reduce_lazy": lambda: _unary(_lazy4_values(), lambda r: (r.randrange(4 * P),), 36),
    "csub2p_t": lambda: _unary(_lazy4_values(), lambda r: (r.randrange(4 * P),), 37),
    "reduce_full": lambda: _unary(_lazy4_values(), lambda r: (r.randrange(4 * P),), 38),
    "sub2p": lambda: _unary(_top_values(), lambda r: (r.randrange(4 * P if r.random() < 0.5 else 2 * P, LAZY_R),), 39, True,
                            lambda t: t >= 2 * P),
    "csub2p_top": lambda: _unary(_top_values(), lambda r: (_rand_top(r),), 40, True),
    "csub2p_t_fast": lambda: _unary(_top_values(), lambda r: (_rand_top(r),), 41, True),
    "reduce_full_fast": lambda: _unary(_top_values(), lambda r: (_rand_top(r),), 42, True),
    "bfly_fast": lambda: _bfly_table(_top_values(), lambda r: (_rand_top(r),), 43, True),
    "bfly": lambda: _bfly_table(_lazy4_values(), lambda r: (r.randrange(4 * P),), 44),
    "fe_bfly_lazy": lambda: _bfly_table(_lazy4_values(), lambda r: (r.randrange(4 * P),), 45),
    "fe_bfly_lazy_reduced": lambda: _bfly_table(
        [x for x in _lazy4_values() if x < 2 * P] + _boundaries(2 * P), lambda r: (r.randrange(2 * P),), 46),
    "fe_mul": lambda: _finish(_mont_narrow() + _mont_wide(), _rand_mont, 47, fill=0),
    "fe_mul_lazy": lambda: _finish(_mont_narrow() + _mont_wide(), _rand_mont, 48, fill=0),
    "fe_mul_lazy2": lambda: _finish(_dual_pairs(), lambda r: _rand_mont(r) + _rand_mont(r), 49, fill=0),
    "fe_mul_shoup": _shoup_table,
    "fe_mul_db": _db_table,
    "fe_mul_db_uniform": _db_uniform_table,
    "fe_is_zero": lambda: _unary(_is_zero_values(), lambda r: (r.randrange(R256),), 50),
}
assert set(_TABLES) == set(OPS) == set(PRE) == set(WANT)


@functools.lru_cache(maxsize=None)
def table(op):
    """The op's records (tuples of Python integers), directed cases first."""
    return tuple(_TABLES[op]())


@functools.lru_cache(maxsize=None)
def expected(op):
    """The op's exact outputs, one tuple of integers per record of table(op)."""
    f = WANT[op]
    return tuple(f(*rec) for rec in table(op))


def _words(values, n_words=8):
    return np.frombuffer(b"".join(v.to_bytes(4 * n_words, "little") for v in values), dtype=np.uint32)


def encode(op, recs):
    """Records as the hook reads them: (n, 8 * elements) u32."""
    if op == "fe_mul_shoup":
        recs = [(a, w, w * R256 // P) for a, w in recs]
    if op in ("fe_mul_db", "fe_mul_db_uniform"):
        rows = [np.concatenate([_words([a]), np.array(D.db_table(w), dtype=np.uint32)]) for a, w in recs]
        return np.ascontiguousarray(np.stack(rows))
    return _words([v for rec in recs for v in rec]).reshape(len(recs), -1).copy()


@functools.lru_cache(maxsize=None)
def expected_array(op, mode):
    """(n, 8 * outputs) u32: mode 0 every lane runs the primitive; mode 1 only the odd lanes, the even ones
    copy their first input element to every output element."""
    n_out = OPS[op][2]
    want = list(expected(op))
    if mode:
        want = [w if i % 2 else (rec[0],) * n_out for i, (rec, w) in enumerate(zip(table(op), want))]
    out = _words([v for w in want for v in w]).reshape(len(want), 8 * n_out).copy()
    out.setflags(write=False)
    return out
