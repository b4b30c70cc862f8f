"""The tamper tables of the verifier's sweep, shared by the CPU tier (tests/test_verify_classes_cpu.py, on the
oracle's proofs) and the GPU tier (tests/test_gpu_verify_sweep.py, on the library's).

TEST INFRASTRUCTURE ONLY.  Each table is a deterministic list of (name, parts', public_wires') made from a proof's
parts (StarkProof.parts()' layout) and its public wires; parts' shares every untouched byte string with parts, so a
memoising classifier (verify_classes.py) pays for the tampered item alone.  No table says what a case must give:
the classifier decides that from the tampered proof.

  S1  every opening of every class: one bit of its leaf;
  S2  every level of every class's paths on openings {0, 63, 64, k - 1}, and one level of every opening;
  S3  every field of the four main leaves of positions {0, 15, 16, 63, 64, 79}: the lowest and the highest bit;
  S4  at every position, ten tamperings that each break one of the six equalities and leave five true;
  S5  encodings that change bytes and not values: v + 4p in every leaf of a class, w + p and w + 4p in the wires;
  S6  every root at its first and last byte, and one bit of every Last value.
"""
from __future__ import annotations

import random

from oracle import P, root_of_unity
import stark_verify as V

S3_POSITIONS = (0, 15, 16, 63, 64, 79)
S2_OPENINGS = (0, 63, 64)  # and k - 1
# S4: kind -> (role, field of that role's main leaf or None for the L leaf, the only equality that must fail, the
# L leaf's compensation as (k index, k index of the x^steps term) or None)
S4_KINDS = {
    "p_prev": (1, 0, "Q1", None), "p_w": (2, 0, "Q2", None), "p_2w": (3, 0, "Q2", None), "a_prev": (1, 1, "Q3", None),
    "D1": (0, 3, "Q1", (0, None)), "D2": (0, 4, "Q2", (1, None)), "D3": (0, 5, "Q3", (2, None)),
    "B2": (0, 6, "B2", (5, 6)), "B3": (0, 7, "B3", (7, 8)), "L": (None, None, "L", None),
}
# The fields of a position's four main leaves that some equality reads (verify.rs:185-206): all eight of role 0,
# p_prev and a_prev of role 1, p_w of role 2, p_2w of role 3.
S3_READ = {(0, c) for c in range(8)} | {(1, 0), (1, 1), (2, 0), (3, 0)}


def _with(parts: dict, path: tuple, key: str, value) -> dict:
    """parts with parts[path...][key] = value, copying only the containers on the way."""
    out = dict(parts)
    if not path:
        out[key] = value
        return out
    head, rest = path[0], path[1:]
    if isinstance(head, str) and rest and isinstance(rest[0], int):  # ("layers", l, ...)
        lst = list(parts[head])
        lst[rest[0]] = _with(lst[rest[0]], rest[1:], key, value)
        out[head] = lst
    else:
        out[head] = _with(parts[head], rest, key, value)
    return out


def _at(parts: dict, path: tuple):
    b = parts
    for k in path:
        b = b[k]
    return b


def _xor(b: bytes, at: int, mask: int) -> bytes:
    a = bytearray(b)
    a[at] ^= mask
    return bytes(a)


def _put(b: bytes, at: int, piece: bytes) -> bytes:
    return b[:at] + piece + b[at + len(piece):]


def _le(v: int) -> bytes:
    return v.to_bytes(32, "little")


def classes(parts: dict) -> list:
    """(label, path) of every set of openings: main, L, then each Middle layer's column and polynomial openings."""
    out = [("main", ("main",)), ("lcomb", ("lcomb",))]
    for l in range(len(parts["layers"])):
        out += [(f"column{l}", ("layers", l, "column")), (f"poly{l}", ("layers", l, "poly"))]
    return out


def s1(parts, pub) -> list:
    out = []
    for label, path in classes(parts):
        b = _at(parts, path)
        for q in range(b["k"]):
            at = q * b["leaf_len"] + (7 * q + 3) % b["leaf_len"]
            out.append((f"S1:{label}:opening{q}", _with(parts, path, "leaves", _xor(b["leaves"], at, 1 << (q % 8))), pub))
    return out


def s2(parts, pub) -> list:
    out, seen = [], set()
    for label, path in classes(parts):
        b = _at(parts, path)
        k, d = b["k"], b["depth"]
        pairs = [(q, l) for l in range(d) for q in sorted({q for q in S2_OPENINGS + (k - 1,) if q < k})]
        pairs += [(q, q % d) for q in range(k)]
        for q, l in pairs:
            name = f"S2:{label}:opening{q}:level{l}"
            if name in seen:
                continue
            seen.add(name)
            at = 32 * (q * d + l) + (5 * l + q) % 32
            out.append((name, _with(parts, path, "nodes", _xor(b["nodes"], at, 1 << ((q + l) % 8))), pub))
    return out


def s3(parts, pub) -> list:
    out = []
    main = parts["main"]
    for i in S3_POSITIONS:
        for j in range(4):
            for c in range(8):
                at = (4 * i + j) * main["leaf_len"] + 32 * c
                for what, byte, mask in (("low", 0, 0x01), ("high", 31, 0x80)):
                    out.append((f"S3:position{i}:role{j}:field{c}:{what}",
                                _with(parts, ("main",), "leaves", _xor(main["leaves"], at + byte, mask)), pub))
    return out


def s3_read(name: str) -> bool:
    """Whether some equality reads the field an S3 case touches."""
    _, _, role, field, _ = name.split(":")
    return (int(role[4:]), int(field[5:])) in S3_READ


def s4(parts, pub, steps: int) -> list:
    """delta = position + 1 added to one field; where the field enters the linear combination, the L leaf moves by
    the field's coefficient times delta (k from m_root, as verify.rs:168-175 derives it), so that L still holds."""
    precision = steps * V.EXTENSION_FACTOR
    log_precision = precision.bit_length() - 1
    g2 = root_of_unity(log_precision)
    positions = V.get_pseudorandom_indices(parts["l_root"], precision, V.SPOT_CHECK_SECURITY_FACTOR, V.EXTENSION_FACTOR)
    _, kk = V.challenges(parts["m_root"], parts["a_root"], precision)
    main, lc = parts["main"], parts["lcomb"]
    out = []
    for i, pos in enumerate(positions):
        delta = i + 1
        xst = pow(pow(g2, pos, P), steps, P)
        for kind, (role, field, _, comp) in S4_KINDS.items():
            q, l_move = parts, delta
            if role is not None:
                at = (4 * i + role) * main["leaf_len"] + 32 * field
                v = (V.fe(main["leaves"][at:at + 32]) + delta) % P
                q = _with(q, ("main",), "leaves", _put(main["leaves"], at, _le(v)))
                l_move = 0 if comp is None else (kk[comp[0]] + (kk[comp[1]] * xst if comp[1] is not None else 0)) * delta % P
            if l_move:
                v = (V.fe(lc["leaves"][32 * i:32 * i + 32]) + l_move) % P
                q = _with(q, ("lcomb",), "leaves", _put(lc["leaves"], 32 * i, _le(v)))
            out.append((f"S4:{kind}:position{i}", q, pub))
    return out


def s4_equality(name: str) -> str:
    return S4_KINDS[name.split(":")[1]][2]


def _plus_4p(b: bytes) -> bytes:
    """Every 32-byte value v of b (v < p) as v + 4p < 2^256: other bytes, the same field element."""
    out = bytearray()
    for i in range(0, len(b), 32):
        v = int.from_bytes(b[i:i + 32], "little")
        assert v < P
        out += _le(v + 4 * P)
    return bytes(out)


def s5(parts, pub) -> list:
    out = [("S5:main+4p", _with(parts, ("main",), "leaves", _plus_4p(parts["main"]["leaves"])), pub),
           ("S5:lcomb+4p", _with(parts, ("lcomb",), "leaves", _plus_4p(parts["lcomb"]["leaves"])), pub)]
    for l, x in enumerate(parts["layers"]):
        for which in ("column", "poly"):
            out.append((f"S5:{which}{l}+4p", _with(parts, ("layers", l, which), "leaves", _plus_4p(x[which]["leaves"])),
                        pub))
    out.append(("S5:last+4p", _with(parts, (), "last", _plus_4p(parts["last"])), pub))
    wires = [w if isinstance(w, int) else int.from_bytes(bytes(w), "little") for w in pub]
    assert all(w < P for w in wires)
    out.append(("S5:wires+p", parts, [w + P for w in wires]))
    out.append(("S5:wires+4p", parts, [w + 4 * P for w in wires]))
    return out


def s6(parts, pub) -> list:
    out = []
    for r in ("m_root", "l_root", "a_root"):
        for byte, mask in ((0, 0x01), (31, 0x80)):
            out.append((f"S6:{r}:byte{byte}", _with(parts, (), r, _xor(parts[r], byte, mask)), pub))
    for l, x in enumerate(parts["layers"]):
        for byte, mask in ((0, 0x01), (31, 0x80)):
            out.append((f"S6:root2_{l}:byte{byte}", _with(parts, ("layers", l), "root2", _xor(x["root2"], byte, mask)), pub))
    for v in range(len(parts["last"]) // 32):
        out.append((f"S6:last{v}", _with(parts, (), "last", _xor(parts["last"], 32 * v + (7 * v + 3) % 32, 1 << (v % 8))),
                    pub))
    return out


def tables(parts, pub, steps: int) -> dict:
    """Every sweep's cases by sweep name."""
    return {"S1": s1(parts, pub), "S2": s2(parts, pub), "S3": s3(parts, pub), "S4": s4(parts, pub, steps),
            "S5": s5(parts, pub), "S6": s6(parts, pub)}


def sample(tabs: dict, count: int, seed: int, keep=lambda name: False) -> list:
    """A fixed-seed sample of `count` cases drawn across the sweeps: every case `keep` names, then an equal share
    of each sweep (all of a smaller one), then more at random up to `count`."""
    rnd = random.Random(seed)
    chosen = {c[0]: c for t in tabs.values() for c in t if keep(c[0])}
    assert len(chosen) <= count
    share = (count - len(chosen)) // len(tabs)
    for t in tabs.values():
        rest = [c for c in t if c[0] not in chosen]
        for c in rnd.sample(rest, min(share, len(rest))):
            chosen[c[0]] = c
    rest = [c for t in tabs.values() for c in t if c[0] not in chosen]
    for c in rnd.sample(rest, min(count - len(chosen), len(rest))):
        chosen[c[0]] = c
    out = list(chosen.values())
    rnd.shuffle(out)
    return out
