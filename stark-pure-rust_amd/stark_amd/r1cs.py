"""Python mirror of packages/r1cs-stark over libstark_hip.so.

    mk_r1cs_proof(ctx, ...)            prove.rs:14-378 (GPU-resident)
    R1csTrace.build(r1cs, wtns)        read_r1cs + read_witness + run.rs:310-437
    prove_with_witness(ctx, r1cs, wtns)   run.rs:310-452
    prove_with_file_path(ctx, ...)     run.rs:528-554 (writes the proof JSON)
    R1csCircuit(ctx, r1cs).prove(wtns) the same proofs, circuit-only work done once
    R1csCircuit.prove_batch(wtns_list) the same proofs for many witnesses through one launch chain
    StarkProof                         utils.rs:122-130 (serde_json text + roots)

Everything runs in libstark_hip.so; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import sys

import numpy as np

from . import Context, StarkError, _elems, _p64, _szp, _vp, load_library

# PyUnicode_DecodeASCII(const char*, Py_ssize_t, errors): one pass from the library's buffer to a str.
_decode_ascii = ctypes.pythonapi.PyUnicode_DecodeASCII
_decode_ascii.restype = ctypes.py_object
_decode_ascii.argtypes = [ctypes.c_void_p, ctypes.c_ssize_t, ctypes.c_char_p]


def ascii_at(ptr: int, n: int) -> str:
    """The n ASCII bytes at address ptr as a str (UnicodeDecodeError on a non-ASCII byte)."""
    return _decode_ascii(ptr, n, None) if n else ""


# PyUnicode_New(n, 127): a compact ASCII str whose n + 1 data bytes follow the object header, filled by
# the library in place (stark_r1cs_proof_json copies a multi-MB text on its host workers) instead of
# one decode pass on this thread.  The header size is checked once against a known string; when the
# layout is not the expected one, to_json decodes instead.
_unicode_new = ctypes.pythonapi.PyUnicode_New
_unicode_new.restype = ctypes.py_object
_unicode_new.argtypes = [ctypes.c_ssize_t, ctypes.c_uint32]


def _ascii_header():
    try:
        h = sys.getsizeof("") - 1
        probe = "".join(["stark", "-ascii-", "probe"])
        if ctypes.string_at(id(probe) + h, len(probe) + 1) == probe.encode() + b"\0":
            return h
    except Exception:
        pass
    return None


_ASCII_HEADER = _ascii_header()


class StarkProof:
    """StarkProof<BlakeDigest> held by the library (r1cs-stark/src/utils.rs:122-130)."""

    def __init__(self, lib, h):
        self.lib = lib
        self.h = h

    def __del__(self):
        try:
            if self.h:
                self.lib.stark_r1cs_proof_free(self.h)
        except Exception:
            pass

    def to_json(self) -> str:
        """serde_json::to_string(&proof) (run.rs:549), decoded straight from the proof's own
        text (stark_r1cs_proof_json_view: no intermediate buffers for a multi-MB proof)."""
        p = ctypes.c_void_p()
        n = ctypes.c_size_t(0)
        self.lib.stark_r1cs_proof_json_view(self.h, ctypes.byref(p), ctypes.byref(n))
        if _ASCII_HEADER is None or n.value < (1 << 20):
            return ascii_at(p.value, n.value)
        s = _unicode_new(n.value, 127)
        got = ctypes.c_size_t(0)
        dst = ctypes.cast(id(s) + _ASCII_HEADER, ctypes.c_char_p)
        rc = self.lib.stark_r1cs_proof_json(self.h, dst, n.value + 1, ctypes.byref(got))
        if rc != 0 or got.value != n.value:
            raise StarkError(rc, "stark_r1cs_proof_json", f"{got.value} of {n.value} bytes")
        return s

    def roots(self) -> dict:
        m, l, a = (ctypes.create_string_buffer(32) for _ in range(3))
        self.lib.stark_r1cs_proof_roots(self.h, m, l, a)
        return {"m_root": m.raw, "l_root": l.raw, "a_root": a.raw}

    def branches(self, which: int) -> dict:
        """stark_r1cs_proof_branches: main_branches (which = 0) or linear_comb_branches (1) as
        {"leaves": k x leaf_len bytes, "nodes": k x depth x 32 bytes, "k", "leaf_len", "depth"}."""
        k, ll, d = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        rc = self.lib.stark_r1cs_proof_branches(self.h, which, ctypes.byref(k), ctypes.byref(ll), ctypes.byref(d), None,
                                                0, None, 0)
        if rc != 0:
            raise StarkError(rc, "stark_r1cs_proof_branches")
        leaves = ctypes.create_string_buffer(max(k.value * ll.value, 1))
        nodes = ctypes.create_string_buffer(max(k.value * d.value * 32, 1))
        rc = self.lib.stark_r1cs_proof_branches(self.h, which, None, None, None, leaves, len(leaves), nodes, len(nodes))
        if rc != 0:
            raise StarkError(rc, "stark_r1cs_proof_branches")
        return {"leaves": leaves.raw[:k.value * ll.value], "nodes": nodes.raw[:k.value * d.value * 32], "k": k.value,
                "leaf_len": ll.value, "depth": d.value}

    def fri_layers(self) -> list:
        """The fri_proof through the stark_fri_proof_* accessors: a {"root2", "column", "poly"} dict per Middle
        layer (column and poly as branches() gives them, 32-B leaves) and {"last": n x 32 bytes} for a Last."""
        lib = self.lib
        fri = lib.stark_r1cs_proof_fri(self.h)
        out = []
        for i in range(lib.stark_fri_proof_num_layers(fri)):
            is_last = ctypes.c_int()
            root2 = ctypes.create_string_buffer(32)
            nc, cd, npl, pd, nl = (ctypes.c_size_t() for _ in range(5))
            rc = lib.stark_fri_proof_layer_info(fri, i, ctypes.byref(is_last), root2, ctypes.byref(nc), ctypes.byref(cd),
                                                ctypes.byref(npl), ctypes.byref(pd), ctypes.byref(nl))
            if rc != 0:
                raise StarkError(rc, "stark_fri_proof_layer_info")
            sizes = [32 * nc.value, 32 * nc.value * cd.value, 32 * npl.value, 32 * npl.value * pd.value, 32 * nl.value]
            bufs = [ctypes.create_string_buffer(max(n, 1)) for n in sizes]
            rc = lib.stark_fri_proof_layer_data(fri, i, *[x for b in bufs for x in (b, len(b))])
            if rc != 0:
                raise StarkError(rc, "stark_fri_proof_layer_data")
            cl, cn, pl, pn, lv = (b.raw[:n] for b, n in zip(bufs, sizes))
            if is_last.value:
                out.append({"last": lv})
            else:
                out.append({"root2": root2.raw,
                            "column": {"leaves": cl, "nodes": cn, "k": nc.value, "leaf_len": 32, "depth": cd.value},
                            "poly": {"leaves": pl, "nodes": pn, "k": npl.value, "leaf_len": 32, "depth": pd.value}})
        return out

    def parts(self) -> dict:
        """Everything from_parts takes, read through the accessors."""
        layers = self.fri_layers()
        last = b"".join(x["last"] for x in layers if "last" in x)
        return dict(self.roots(), main=self.branches(0), lcomb=self.branches(1),
                    layers=[x for x in layers if "last" not in x], last=last)

    @staticmethod
    def parts_of_dict(proof: dict) -> dict:
        """A parsed StarkProof (serde_json's dict) as from_parts' parts.  The openings of one set must have one
        shape, and a Last value 32 bytes (StarkError(3) otherwise): a handle holds uniform arrays."""
        def uniform(brs):
            ll = len(brs[0]["leaf"]) if brs else 32
            d = len(brs[0]["nodes"]) if brs else 0
            if any(len(b["leaf"]) != ll or len(b["nodes"]) != d or any(len(n) != 32 for n in b["nodes"]) for b in brs):
                raise StarkError(3, "StarkProof.from_parts", "openings of unequal shape")
            return {"leaves": b"".join(bytes(b["leaf"]) for b in brs),
                    "nodes": b"".join(bytes(n) for b in brs for n in b["nodes"]), "k": len(brs), "leaf_len": ll,
                    "depth": d}
        fri = proof["fri_proof"]
        if not fri or "Last" not in fri[-1] or any("Middle" not in x for x in fri[:-1]):
            raise StarkError(3, "StarkProof.from_parts", "Middle layers then one Last layer expected")
        last = [bytes(v) for v in fri[-1]["Last"]["last"]]
        if any(len(v) != 32 for v in last):
            raise StarkError(3, "StarkProof.from_parts", "a Last value is not 32 bytes")
        return {"m_root": bytes(proof["m_root"]), "l_root": bytes(proof["l_root"]), "a_root": bytes(proof["a_root"]),
                "main": uniform(proof["main_branches"]), "lcomb": uniform(proof["linear_comb_branches"]),
                "layers": [{"root2": bytes(x["Middle"]["root2"]), "column": uniform(x["Middle"]["column_branches"]),
                            "poly": uniform(x["Middle"]["poly_branches"])} for x in fri[:-1]],
                "last": b"".join(last)}

    @classmethod
    def from_parts(cls, parts, lib=None) -> "StarkProof":
        """A handle over copies of a StarkProof's parts (stark_r1cs_proof_from_parts; host only): `parts` is what
        parts() returns, or a parsed proof dict.  What R1csCircuit.verify_batch takes without any text."""
        from .verify import _Branches, _FriLayer
        lib = lib or load_library()
        if "main_branches" in parts:
            parts = cls.parts_of_dict(parts)

        def br(b):
            return _Branches(b["leaves"], b["nodes"], b["k"], b["leaf_len"], b["depth"])
        for r in ("m_root", "l_root", "a_root"):
            if len(parts[r]) != 32:
                raise StarkError(3, "StarkProof.from_parts", f"{r} is not 32 bytes")
        mb, lb = br(parts["main"]), br(parts["lcomb"])
        mids = parts["layers"]
        arr = (_FriLayer * max(len(mids), 1))()
        for i, m in enumerate(mids):
            if len(m["root2"]) != 32:
                raise StarkError(3, "StarkProof.from_parts", "root2 is not 32 bytes")
            arr[i] = _FriLayer(m["root2"], br(m["column"]), br(m["poly"]))
        last = parts["last"]
        h = _vp()
        rc = lib.stark_r1cs_proof_from_parts(parts["m_root"], parts["l_root"], parts["a_root"], ctypes.byref(mb),
                                             ctypes.byref(lb), ctypes.cast(arr, ctypes.c_void_p), len(mids), last,
                                             len(last) // 32, ctypes.byref(h))
        if rc != 0:
            raise StarkError(rc, "stark_r1cs_proof_from_parts")
        return cls(lib, h)


def _sz(v) -> np.ndarray:
    a = np.ascontiguousarray(np.asarray(v, dtype=np.uint64).reshape(-1))
    return a if a.size else np.zeros(1, dtype=np.uint64)


def mk_r1cs_proof(ctx: Context, witness_trace, computational_trace, public_wires, public_first_indices,
                  permuted_indices, coefficients, flag0, flag1, flag2, n_constraints: int,
                  n_wires: int) -> StarkProof:
    """prove.rs:14-26 argument order; field vectors as (n, 4) canonical limbs or int lists."""
    def el(x):
        if isinstance(x, np.ndarray):
            return _elems(x)
        from . import _limbs
        return _elems(np.array([_limbs(int(v)) for v in x], dtype=np.uint64).reshape(-1, 4)) if len(x) else \
            np.zeros((0, 4), dtype=np.uint64)
    w, ct, co = el(witness_trace), el(computational_trace), el(coefficients)
    f0, f1, f2, pw = el(flag0), el(flag1), el(flag2), el(public_wires)
    os_ = len(co)
    pfi = _sz([x for pair in public_first_indices for x in pair])
    perm = _sz(permuted_indices)
    szp = lambda a: a.ctypes.data_as(_szp)
    h = _vp()
    ctx.check(ctx.lib.stark_mk_r1cs_proof(ctx.h, _p64(w), _p64(ct), os_, _p64(pw), len(pw), szp(pfi),
                                          len(public_first_indices), szp(perm), _p64(co), _p64(f0), _p64(f1),
                                          _p64(f2), n_constraints, n_wires, ctypes.byref(h)), "mk_r1cs_proof")
    return StarkProof(ctx.lib, h)


class R1csTrace:
    """The mk_r1cs_proof arguments built by the library from .r1cs/.wtns bytes."""

    def __init__(self, r1cs: bytes, wtns: bytes):
        self.lib = load_library()
        self.h = _vp()
        rc = self.lib.stark_r1cs_trace_build(r1cs, len(r1cs), wtns, len(wtns), ctypes.byref(self.h))
        if rc != 0:
            self.h = None
            raise StarkError(rc, "r1cs_trace_build")

    def __del__(self):
        try:
            if self.h:
                self.lib.stark_r1cs_trace_free(self.h)
        except Exception:
            pass

    def dims(self) -> dict:
        v = [ctypes.c_size_t(0) for _ in range(5)]
        self.lib.stark_r1cs_trace_dims(self.h, *[ctypes.byref(x) for x in v])
        keys = ("original_steps", "n_public", "n_public_first", "n_constraints", "n_wires")
        return dict(zip(keys, (x.value for x in v)))

    def export(self) -> dict:
        d = self.dims()
        n = d["original_steps"]
        arrs = {k: np.zeros((n, 4), dtype=np.uint64) for k in ("witness_trace", "computational_trace",
                                                               "coefficients", "flag0", "flag1", "flag2")}
        perm = np.zeros(max(n, 1), dtype=np.uint64)
        pw = np.zeros((max(d["n_public"], 1), 4), dtype=np.uint64)
        pfi = np.zeros(max(2 * d["n_public_first"], 1), dtype=np.uint64)
        szp = lambda a: a.ctypes.data_as(_szp)
        self.lib.stark_r1cs_trace_export(self.h, *[_p64(arrs[k]) for k in ("witness_trace", "computational_trace",
                                                                           "coefficients", "flag0", "flag1",
                                                                           "flag2")],
                                         szp(perm), _p64(pw), szp(pfi))
        arrs["permuted_indices"] = [int(x) for x in perm[:n]]
        arrs["public_wires"] = pw[:d["n_public"]]
        arrs["public_first_indices"] = [(int(pfi[2 * i]), int(pfi[2 * i + 1])) for i in range(d["n_public_first"])]
        arrs.update(n_constraints=d["n_constraints"], n_wires=d["n_wires"])
        return arrs


def prove_with_witness(ctx: Context, r1cs: bytes, wtns: bytes) -> StarkProof:
    """run.rs:310-452, the trace built on the GPU (stark_prove_r1cs_bytes)."""
    h = _vp()
    ctx.check(ctx.lib.stark_prove_r1cs_bytes(ctx.h, r1cs, len(r1cs), wtns, len(wtns), ctypes.byref(h)),
              "prove_with_witness")
    return StarkProof(ctx.lib, h)


def prove_with_witness_host_trace(ctx: Context, r1cs: bytes, wtns: bytes) -> StarkProof:
    """run.rs:310-452 with the host trace builder (R1csTrace) feeding the same prover."""
    tr = R1csTrace(r1cs, wtns)
    h = _vp()
    ctx.check(ctx.lib.stark_prove_r1cs_trace(ctx.h, tr.h, ctypes.byref(h)), "prove_with_witness")
    return StarkProof(ctx.lib, h)


class R1csFailure(ctypes.Structure):
    """stark_r1cs_failure (include/stark_hip.h): one failing constraint with A.w, B.w and C.w."""
    _fields_ = [("constraint", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("a", ctypes.c_uint64 * 4),
                ("b", ctypes.c_uint64 * 4), ("c", ctypes.c_uint64 * 4)]


def _limbs_int(v) -> int:
    return sum(int(x) << (64 * i) for i, x in enumerate(v))


class WitnessCheck:
    """The report of a witness check (R1csCircuit.check): status (0 satisfied, 8 some constraint fails, 3 the
    witness was refused), n_failed (the exact count) and failures, the first max_failures failing constraints in
    ascending order as (constraint, a, b, c) with the values A.w, B.w and C.w mod p as Python ints."""

    def __init__(self, status: int, n_failed: int, failures: list):
        self.status = status
        self.n_failed = n_failed
        self.failures = failures

    @property
    def satisfied(self) -> bool:
        return self.status == 0

    def __eq__(self, other):
        return (isinstance(other, WitnessCheck) and
                (self.status, self.n_failed, self.failures) == (other.status, other.n_failed, other.failures))

    def __repr__(self):
        return f"WitnessCheck(status={self.status}, n_failed={self.n_failed}, failures={self.failures!r})"


class R1csCircuit:
    """A circuit prepared once for many proofs (stark_r1cs_circuit_new): everything of
    prove_with_witness (run.rs:310-452) that depends on the .r1cs alone, including the
    LDEs of K, F0-F2, IDX and PIDX, stays in HBM; prove(wtns) extends only S, P and A.
    The proofs equal prove_with_witness(ctx, r1cs, wtns)."""

    def __init__(self, ctx: Context, r1cs: bytes):
        self.ctx = ctx
        self.h = _vp()
        ctx.check(ctx.lib.stark_r1cs_circuit_new(ctx.h, r1cs, len(r1cs), ctypes.byref(self.h)), "r1cs_circuit_new")

    def __del__(self):
        try:
            if self.h:
                self.ctx.lib.stark_r1cs_circuit_free(self.h)
        except Exception:
            pass

    def prove(self, wtns: bytes) -> StarkProof:
        h = _vp()
        self.ctx.check(self.ctx.lib.stark_prove_r1cs_circuit(self.ctx.h, self.h, wtns, len(wtns), ctypes.byref(h)),
                       "prove_r1cs_circuit")
        return StarkProof(self.ctx.lib, h)

    def prove_batch(self, wtns_list, strict: bool = True) -> list:
        """prove(w) for every w of wtns_list through one chain of launches (stark_prove_r1cs_circuit_batch): the
        same proofs, byte for byte.  strict: the first failing witness raises StarkError (its .index tells
        which).  Otherwise the list holds a StarkError instance (with .index) in the place of each failed
        witness and a StarkProof everywhere else."""
        ws = [None if w is None else bytes(w) for w in wtns_list]
        n = len(ws)
        if n == 0:
            return []
        lib = self.ctx.lib
        ptrs = (ctypes.c_char_p * n)(*ws)
        lens = (ctypes.c_size_t * n)(*[0 if w is None else len(w) for w in ws])
        hs = (_vp * n)()
        sts = (ctypes.c_int * n)()
        self.ctx.check(lib.stark_prove_r1cs_circuit_batch(self.ctx.h, self.h, ptrs, lens, n, hs, sts),
                       "prove_r1cs_circuit_batch")
        out = []
        for b in range(n):
            if sts[b] == 0:
                out.append(StarkProof(lib, _vp(hs[b])))
            else:
                detail = lib.stark_ctx_last_error(self.ctx.h).decode() if sts[b] == 8 else ""
                e = StarkError(sts[b], f"prove_r1cs_circuit_batch, witness {b}", detail)
                e.index = b
                out.append(e)
        if strict:
            for x in out:
                if isinstance(x, StarkError):
                    raise x
        return out

    def check_batch(self, wtns_list, max_failures: int = 16) -> list:
        """A WitnessCheck for every w of wtns_list (stark_check_r1cs_circuit_batch): which constraints each witness
        fails, without proving anything.  None stands for a missing witness (status 3), as in prove_batch.  An
        unsatisfied witness does not raise: the report is the result.  Errors of the call as a whole raise
        StarkError."""
        ws = [None if w is None else bytes(w) for w in wtns_list]
        n = len(ws)
        if n == 0:
            return []
        cap = int(max_failures)
        if cap < 0 or cap > 0xFFFFFFFF:
            raise StarkError(3, "check_r1cs_circuit_batch", "max_failures out of range")
        lib = self.ctx.lib
        ptrs = (ctypes.c_char_p * n)(*ws)
        lens = (ctypes.c_size_t * n)(*[0 if w is None else len(w) for w in ws])
        sts = (ctypes.c_int * n)()
        nf = (ctypes.c_uint32 * n)()
        recs = (R1csFailure * (n * cap))() if cap else None
        self.ctx.check(lib.stark_check_r1cs_circuit_batch(self.ctx.h, self.h, ptrs, lens, n, sts, nf, recs, cap),
                       "check_r1cs_circuit_batch")
        out = []
        for b in range(n):
            fl = [(int(r.constraint), _limbs_int(r.a), _limbs_int(r.b), _limbs_int(r.c))
                  for r in (recs[b * cap + k] for k in range(min(int(nf[b]), cap)))]
            out.append(WitnessCheck(int(sts[b]), int(nf[b]), fl))
        return out

    def check(self, wtns: bytes, max_failures: int = 16) -> WitnessCheck:
        """check_batch of one witness."""
        return self.check_batch([wtns], max_failures)[0]

    def verify_batch(self, public_wires_list, proofs) -> list:
        """[(status, reasons)] of verify_circuit(public_wires, proof) for every pair, checked on the GPU through
        one chain of launches (stark_amd.verify.verify_circuit_batch).  `proofs` holds texts or parsed dicts, or
        StarkProof handles (verify_circuit_batch_proofs: no text on the way); None stands for a missing entry in
        either.  A list that mixes handles with texts is StarkError(3)."""
        from .verify import verify_circuit_batch, verify_circuit_batch_proofs
        handles = [isinstance(p, StarkProof) for p in proofs]
        if any(handles):
            if not all(h or p is None for h, p in zip(handles, proofs)):
                raise StarkError(3, "verify_batch", "StarkProof handles and proof texts in one list")
            return verify_circuit_batch_proofs(self.ctx, self, public_wires_list, proofs)
        return verify_circuit_batch(self.ctx, self, public_wires_list, proofs)


def check_with_witness(ctx: Context, r1cs: bytes, wtns: bytes, max_failures: int = 16) -> WitnessCheck:
    """Prepares the circuit and checks one witness (R1csCircuit.check)."""
    return R1csCircuit(ctx, r1cs).check(wtns, max_failures)


def prove_with_file_path(ctx: Context, r1cs_file_path: str, witness_file_path: str, proof_json_path: str) -> None:
    """run.rs:528-554."""
    with open(r1cs_file_path, "rb") as f:
        r1cs = f.read()
    with open(witness_file_path, "rb") as f:
        wtns = f.read()
    proof = prove_with_witness(ctx, r1cs, wtns)
    with open(proof_json_path, "w") as f:
        f.write(proof.to_json())
