"""A verifier that classifies: which of the batched verifier's classes of checks (include/stark_hip.h
STARK_VERIFY_FAIL_*) a proof fails, and which items of each class.

TEST INFRASTRUCTURE ONLY.  Built from the pieces of the restated verifier (stark_verify.py: verify.rs:13-258,
fri.rs:226-404) over exact integers.  Where that verifier stops at the reference's first failed assertion, this one
evaluates every class on its own, from the proof as given, as the header words them:

  * PUBLIC_ONE (public_wires[0] != 1 after from_bytes_le's reduction) stands alone; nothing else is evaluated;
  * indices and challenges come from the roots as given, whatever else holds;
  * FRI_ROWS and SPOT are evaluated on the leaves' values whether or not their Merkle paths hold;
  * FRI_LAST is the Last layer's root or its degree.

classify() is handed the whole proof and never where it was tampered with.  Thousands of proofs that differ in one
item are cheap: every item's result is memoised on the item's own bytes (a path: root, index, leaf, nodes; a row:
its five leaves, the root that gives special_x, y; a position: its leaves, the roots its constants come from and
the public wires), a class's on the class's bytes, and what depends on the circuit alone -- the domain, K, F0, F1,
F2, IDX, PIDX over it, Zb2, I3 -- is computed once per circuit.

The proof must have the structure the circuit implies (StarkProof.parts()' layout: 320 main and 80 L openings, 40
column and 160 polynomial openings per Middle layer); any other is the single-proof verifier's business.
"""
from __future__ import annotations

from oracle import P, Oracle, to_limbs, from_limbs, root_of_unity
import stark_verify as V

PUBLIC_ONE, FRI_PATHS, FRI_ROWS, FRI_LAST, OPENING_PATHS, SPOT = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
SPOTS, ROWS = V.SPOT_CHECK_SECURITY_FACTOR, 40
MAIN_LEAF = 256


def parts_of_dict(proof: dict) -> dict:
    """A parsed StarkProof (serde_json's dict) in StarkProof.parts()' layout."""
    def uniform(brs):
        ll, d = len(brs[0]["leaf"]), len(brs[0]["nodes"])
        assert all(len(b["leaf"]) == ll and len(b["nodes"]) == d and all(len(n) == 32 for n in b["nodes"]) for b in brs)
        return {"leaves": b"".join(bytes(b["leaf"]) for b in brs),
                "nodes": b"".join(bytes(n) for b in brs for n in b["nodes"]), "k": len(brs), "leaf_len": ll, "depth": d}
    fri = proof["fri_proof"]
    last = [bytes(v) for v in fri[-1]["Last"]["last"]]
    assert all(len(v) == 32 for v in last)
    return {"m_root": bytes(proof["m_root"]), "l_root": bytes(proof["l_root"]), "a_root": bytes(proof["a_root"]),
            "main": uniform(proof["main_branches"]), "lcomb": uniform(proof["linear_comb_branches"]),
            "layers": [{"root2": bytes(x["Middle"]["root2"]), "column": uniform(x["Middle"]["column_branches"]),
                        "poly": uniform(x["Middle"]["poly_branches"])} for x in fri[:-1]],
            "last": b"".join(last)}


def dict_of_parts(parts: dict) -> dict:
    """The inverse: parts as the parsed StarkProof the restated verifier (and serde_json) reads."""
    def branches(b):
        ll, d = b["leaf_len"], b["depth"]
        return [{"leaf": list(b["leaves"][ll * i:ll * (i + 1)]),
                 "nodes": [list(b["nodes"][32 * (d * i + k):32 * (d * i + k + 1)]) for k in range(d)]}
                for i in range(b["k"])]
    fri = [{"Middle": {"root2": list(x["root2"]), "column_branches": branches(x["column"]),
                       "poly_branches": branches(x["poly"])}} for x in parts["layers"]]
    last = parts["last"]
    fri.append({"Last": {"last": [list(last[i:i + 32]) for i in range(0, len(last), 32)]}})
    return {"m_root": list(parts["m_root"]), "l_root": list(parts["l_root"]), "a_root": list(parts["a_root"]),
            "main_branches": branches(parts["main"]), "linear_comb_branches": branches(parts["lcomb"]), "fri_proof": fri}


def _field(ti, name):
    return ti[name] if isinstance(ti, dict) else getattr(ti, name)


def wire_value(w) -> int:
    """A public wire as given (an int, or its little-endian bytes) through from_bytes_le (ff_utils/src/fp.rs:70-77)."""
    return (w if isinstance(w, int) else int.from_bytes(bytes(w), "little")) % P


class Classifier:
    """The circuit's part of verify_r1cs_proof (verify.rs:27-84, 121-157), once, and the memos."""

    def __init__(self, orc: Oracle, trace_inputs):
        coefficients = list(_field(trace_inputs, "coefficients"))
        self.pfi = [tuple(x) for x in _field(trace_inputs, "public_first_indices")]
        os_ = self.original_steps = len(coefficients)
        assert os_ % 3 == 0
        log_steps = V._log2_ceil(os_ - 1)
        steps = self.steps = max(2 ** log_steps, 8)
        self.precision = steps * V.EXTENSION_FACTOR
        log_precision = log_steps + V.LOG_EXTENSION_FACTOR
        self.skips = self.precision // steps
        g2 = self.g2 = root_of_unity(log_precision)
        xs = [1] * self.precision
        for i in range(1, self.precision):
            xs[i] = xs[i - 1] * g2 % P
        self.xs = xs
        g1 = xs[self.skips]
        permuted = list(_field(trace_inputs, "permuted_indices")) + list(range(os_, steps))
        pad = [0] * (steps - os_)

        def extend(v):  # the column's polynomial over the whole precision domain
            return from_limbs(orc.best_fft(orc.inv_best_fft(to_limbs(v), g1, log_steps), g2, log_precision))
        self.cols = [extend(coefficients + pad)] + [extend(list(_field(trace_inputs, f)) + pad)
                                                    for f in ("flag0", "flag1", "flag2")]
        self.cols += [extend(range(steps)), extend(permuted)]
        self.bx = [xs[self.skips * w] for (_, w) in self.pfi]
        self.x_last = xs[(steps - 1) * self.skips]
        self.interp3 = V.lagrange_interp([xs[self.precision - self.skips]], [1])
        # FRI's layers (fri.rs:64-66): from degree precision / 4 down to the direct check
        self.layers = 0
        deg = self.precision // 4
        while deg > V.MIN_DEG_DIRECT_CHECKING:
            deg //= 4
            self.layers += 1
        self.depth = log_precision
        self._memo = {k: {} for k in ("indices", "path", "paths", "row", "rows", "last", "consts", "i2", "zb2", "spot",
                                      "spots")}

    # ---- memoised pieces ----

    def _cached(self, table, key, make):
        m = self._memo[table]
        if key not in m:
            m[key] = make()
        return m[key]

    def indices(self, seed: bytes, modulus: int, count: int) -> tuple:
        return self._cached("indices", (seed, modulus, count),
                            lambda: tuple(V.get_pseudorandom_indices(seed, modulus, count, self.skips)))

    def _bad_paths(self, root: bytes, indices: tuple, b: dict) -> tuple:
        """The openings of one set whose path does not reach `root` at its index."""
        leaves, nodes, ll, d = b["leaves"], b["nodes"], b["leaf_len"], b["depth"]

        def one(i, index):
            leaf, nd = leaves[ll * i:ll * (i + 1)], nodes[32 * d * i:32 * d * (i + 1)]
            return self._cached("path", (root, index, leaf, nd), lambda: V.path_root(
                index, leaf, [nd[32 * k:32 * k + 32] for k in range(d)]) == root)
        return self._cached("paths", (root, indices, leaves, nodes),
                            lambda: tuple(i for i, index in enumerate(indices) if not one(i, index)))

    def _bad_rows(self, layer: int, root_l: bytes, ys: tuple, col: bytes, poly: bytes) -> tuple:
        rou_deg = self.precision >> (2 * layer)
        w = pow(self.g2, 4 ** layer, P)

        def one(i, y):
            row, c = poly[128 * i:128 * (i + 1)], col[32 * i:32 * (i + 1)]
            return self._cached("row", (layer, root_l, y, row, c), lambda: V.fri_row_holds(
                w, V.quartic_roots(w, rou_deg), y, [row[32 * j:32 * j + 32] for j in range(4)], c, V.fe(root_l)))
        return self._cached("rows", (layer, root_l, ys, col, poly),
                            lambda: tuple(i for i, y in enumerate(ys) if not one(i, y)))

    def _bad_last(self, last: bytes, root: bytes) -> tuple:
        def make():
            vals = [last[i:i + 32] for i in range(0, len(last), 32)]
            rou_deg = self.precision >> (2 * self.layers)
            w = pow(self.g2, 4 ** self.layers, P)
            max_deg = (self.precision // 4) >> (2 * self.layers)
            bad = []
            if not (len(vals) > max_deg and len(vals) & (len(vals) - 1) == 0 and V.last_layer_root_holds(vals, root)):
                bad.append("root")
            if not (len(vals) > max_deg and len(vals) <= rou_deg
                    and V.last_layer_degree_holds(vals, w, rou_deg, max_deg, self.skips)):
                bad.append("degree")
            return tuple(bad)
        return self._cached("last", (last, root), make)

    def _interp2(self, pub: tuple) -> list:
        return self._cached("i2", pub, lambda: V.lagrange_interp(self.bx, [pub[k] for (k, _) in self.pfi]))

    def _zb2(self, pos: int) -> int:
        def make():
            z = 1
            for b in self.bx:
                z = z * (self.xs[pos] - b) % P
            return z
        return self._cached("zb2", pos, make)

    def _bad_spots(self, positions: tuple, m_root: bytes, a_root: bytes, pub: tuple, main: bytes, lcomb: bytes) -> tuple:
        def one(i, pos):
            main4, l_leaf = main[4 * MAIN_LEAF * i:4 * MAIN_LEAF * (i + 1)], lcomb[32 * i:32 * (i + 1)]

            def make():
                r, kk = self._cached("consts", (m_root, a_root), lambda: V.challenges(m_root, a_root, self.precision))
                x = self.xs[pos]
                k_x, f0, f1, f2, idx, pidx = (c[pos] for c in self.cols)
                eqs = V.spot_equalities([main4[MAIN_LEAF * q:MAIN_LEAF * (q + 1)] for q in range(4)], l_leaf,
                                        pow(x, self.steps, P), k_x, f0, f1, f2, idx, pidx, r, kk, self._zb2(pos),
                                        V.eval_poly_at(self._interp2(pub), x), (x - self.x_last) % P,
                                        V.eval_poly_at(self.interp3, x))
                return tuple(name for name, _, lhs, rhs in eqs if lhs != rhs)
            return self._cached("spot", (pos, m_root, a_root, pub, main4, l_leaf), make)

        def make_all():
            out = []
            for i, pos in enumerate(positions):
                bad = one(i, pos)
                if bad:
                    out.append((i, bad))
            return tuple(out)
        return self._cached("spots", (positions, m_root, a_root, pub, main, lcomb), make_all)

    # ---- the classes ----

    def _in_shape(self, parts) -> bool:
        def is_(b, k, leaf_len, depth):
            return (b["k"], b["leaf_len"], b["depth"]) == (k, leaf_len, depth) and \
                len(b["leaves"]) == k * leaf_len and len(b["nodes"]) == 32 * k * depth
        return len(parts["layers"]) == self.layers and is_(parts["main"], 4 * SPOTS, MAIN_LEAF, self.depth) and \
            is_(parts["lcomb"], SPOTS, 32, self.depth) and len(parts["last"]) % 32 == 0 and len(parts["last"]) > 0 and \
            all(is_(x["column"], ROWS, 32, self.depth - 2 * l - 2) and is_(x["poly"], 4 * ROWS, 32, self.depth - 2 * l)
                and len(x["root2"]) == 32 for l, x in enumerate(parts["layers"])) and \
            all(len(parts[r]) == 32 for r in ("m_root", "l_root", "a_root"))

    def classify(self, public_wires, parts):
        pub = tuple(wire_value(w) for w in public_wires)
        if pub[0] != 1:
            return PUBLIC_ONE, {"public_one": pub[0]}
        if not self._in_shape(parts):
            raise ValueError("the proof's structure is not what the circuit implies")
        m_root, l_root, a_root = parts["m_root"], parts["l_root"], parts["a_root"]
        detail = {}
        # verify_low_degree_proof (fri.rs:244-404)
        root_l = l_root
        fri_paths, fri_rows = [], []
        for l, x in enumerate(parts["layers"]):
            quarter = self.precision >> (2 * l + 2)
            ys = self.indices(x["root2"], quarter, ROWS)
            fri_paths += [(l, "column", i) for i in self._bad_paths(x["root2"], ys, x["column"])]
            poly_at = tuple(j * quarter + y for y in ys for j in range(4))
            fri_paths += [(l, "poly", i) for i in self._bad_paths(root_l, poly_at, x["poly"])]
            fri_rows += [(l, i) for i in self._bad_rows(l, root_l, ys, x["column"]["leaves"], x["poly"]["leaves"])]
            root_l = x["root2"]
        last = self._bad_last(parts["last"], root_l)
        # the openings and the spot checks (verify.rs:86-118, 185-254)
        positions = self.indices(l_root, self.precision, SPOTS)
        aug = tuple(r for j in positions for r in V.spot_rows(j, self.precision, self.skips, self.original_steps))
        openings = [("main", i) for i in self._bad_paths(m_root, aug, parts["main"])]
        openings += [("lcomb", i) for i in self._bad_paths(l_root, positions, parts["lcomb"])]
        spots = self._bad_spots(positions, m_root, a_root, pub, parts["main"]["leaves"], parts["lcomb"]["leaves"])
        mask = 0
        for bit, name, items in ((FRI_PATHS, "fri_paths", fri_paths), (FRI_ROWS, "fri_rows", fri_rows),
                                 (FRI_LAST, "fri_last", list(last)), (OPENING_PATHS, "opening_paths", openings),
                                 (SPOT, "spot", list(spots))):
            if items:
                mask |= bit
                detail[name] = items
        return mask, detail


_CLASSIFIERS = {}


def classifier(orc: Oracle, trace_inputs) -> Classifier:
    """The Classifier of a circuit, made once per trace_inputs object (an r1cs.Trace or r1cs.verifier_inputs' dict)."""
    key = id(trace_inputs)
    if key not in _CLASSIFIERS or _CLASSIFIERS[key][0] is not trace_inputs:
        _CLASSIFIERS[key] = (trace_inputs, Classifier(orc, trace_inputs))
    return _CLASSIFIERS[key][1]


def classify(orc: Oracle, trace_inputs, public_wires, parts):
    """(mask, detail): the OR of the failed STARK_VERIFY_FAIL_* classes, and the failing items by class --
    "fri_paths": [(layer, "column" | "poly", opening)], "fri_rows": [(layer, row)], "fri_last": ["root", "degree"],
    "opening_paths": [("main" | "lcomb", opening)], "spot": [(position, (failed equalities of Q1 Q2 Q3 B2 B3 L))]."""
    return classifier(orc, trace_inputs).classify(public_wires, parts)
