"""Synthetic, satisfiable R1CS + witness in the circom binary formats the
reference reads (circom2bellman_core/src/reader.rs:4-89, r1cs-stark/src/reader.rs:7-42).

Stand-in for sha256_2_test, whose .r1cs the reference does not ship
(SURVEY.md 0.6): a chain of constraints with 3 terms per factor,

    (w[i] + a_i w[i-1] + 1) * (w[i] + b_i w[i-2] + 2) = w[i+1] + c_i w[1] + 3 w[0]

so that every constraint has n_coeff = 3 (9 trace slots).  original_steps =
9 * n_constraints; n_constraints = ceil(target / 9) gives steps = the next
power of two >= target.  Wire 0 is the constant 1; wire 1 is the public
output (the last chain value is copied into it by a final constraint) and
wire 2 the public input.
"""
from __future__ import annotations

import struct

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
P_LE = P.to_bytes(32, "little")


def _fe(x: int) -> bytes:
    return (x % P).to_bytes(32, "little")


def synth(n_constraints: int, seed: int = 1, inputs=None, n_public: int = 2):
    """Returns (r1cs_bytes, wtns_bytes).  inputs = (public output, public input) overrides
    the seeded ones: the same circuit (identical .r1cs) with another witness.

    n_public: the public wires the header declares (one output, n_public - 1 inputs; the prover's
    public_first_indices then has n_public + 1 entries, the constant wire 0 among them).  The inputs beyond
    wire 2 are wires 3 .. n_public with seeded values; each takes the place of one constant-or-output term of
    a chain constraint (three per constraint, in order: the 1 of the first factor and the 2 of the second
    become 1 w[q] and 2 w[q], the c w[1] of the product c w[q]), so every one of them is used.  The default
    is the circuit described above, byte for byte."""
    import random
    rnd = random.Random(seed)
    n_chain = n_constraints - 1
    extras = list(range(3, n_public + 1))
    if n_public < 2 or len(extras) >= 3 * n_chain:
        raise ValueError("n_public must be in [2, 3 (n_constraints - 1) + 2]")
    # wires: 0 = 1, 1 = public output, 2 .. n_public = public inputs, then the chain values
    base = n_public + 1
    n_wires = base + n_chain + 1
    w = [0] * n_wires
    w[0] = 1
    w[2] = rnd.randrange(P)
    w[base] = w[2]
    xrnd = random.Random(seed * 7919 + 13)  # (a stream of its own: the default circuit's draws stay as they are)
    for q in extras:
        w[q] = xrnd.randrange(P)
    seq = [2] + list(range(base, base + n_chain + 1))  # the chain, from the public input it starts at
    coef = [(rnd.randrange(1, P), rnd.randrange(1, P), rnd.randrange(1, P)) for _ in range(n_chain)]
    # the public output is a seeded value of its own; the chain is computed forward around it
    w[1] = rnd.randrange(P)
    if inputs is not None:
        w[1], w[2] = inputs[0] % P, inputs[1] % P
        w[base] = w[2]
    out = []
    for i, (a, b, c) in enumerate(coef):
        cur, p1, p2, nxt = seq[i + 1], seq[i], seq[max(i - 1, 0)], seq[i + 2]
        q = extras[3 * i:3 * i + 3]
        qa, qb, qc = q + [0, 0, 1][len(q):]  # the terms no extra input took: the constants (wire 0), c w[1]
        av = (w[cur] + a * w[p1] + w[qa]) % P
        bv = (w[cur] + b * w[p2] + 2 * w[qb]) % P
        w[nxt] = (av * bv - c * w[qc] - 3) % P
        A = [(cur, 1), (p1, a), (qa, 1)]
        B = [(cur, 1), (p2, b), (qb, 2)]
        C = [(nxt, 1), (qc, c), (0, 3)]
        out.append((A, B, C))
    # final constraint: w[last] * 1 = w[1] + 0 ... keep it non-trivial but satisfied: (w[last]) * (1) = (w[last])
    last = base + n_chain
    out.append(([(last, 1), (0, 0), (2, 0)], [(0, 1), (1, 0), (2, 0)], [(last, 1), (0, 0), (1, 0)]))
    body = bytearray()
    for A, B, C in out:
        for fac in (A, B, C):
            body += struct.pack("<I", len(fac))
            for wid, v in fac:
                body += struct.pack("<I", wid) + _fe(v)
    hdr = struct.pack("<I", 32) + P_LE + struct.pack("<IIIIQI", n_wires, 1, n_public - 1, 0, n_wires, len(out))
    r1cs = bytearray()
    r1cs += b"r1cs" + struct.pack("<II", 1, 3)
    r1cs += struct.pack("<IQ", 1, len(hdr)) + hdr
    r1cs += struct.pack("<IQ", 2, len(body)) + body
    wt = bytearray()
    wt += struct.pack("<I", 1936618615) + struct.pack("<IIIII", 2, 2, 1, 0, 0)
    wt += struct.pack("<I", 32) + P_LE
    wt += struct.pack("<IIII", n_wires, 0, 0, 0)
    for x in w:
        wt += _fe(x)
    return bytes(r1cs), bytes(wt)


def for_steps(log_steps: int, seed: int = 1, inputs=None, n_public: int = 2):
    """A circuit whose padded trace length is 2^log_steps (original_steps = 9 n_constraints)."""
    target = 1 << log_steps
    n = (target // 2) // 9 + 1            # original_steps in (2^(k-1), 2^k]
    return synth(n, seed, inputs, n_public=n_public)
