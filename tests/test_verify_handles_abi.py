"""CPU: ABI 10 -- batched verification from proof handles, a handle made from a StarkProof's parts, and the
switch for who derives the batch's transcript -- is exported, declared and bound; the handle entry's whole-call
errors need no device; stark_r1cs_proof_from_parts round-trips the oracle's proof.  No GPU compute is called."""
import ctypes
import json
import os

import pytest

import r1cs as R
import stark_amd as S
from stark_amd.r1cs import R1csCircuit, StarkProof

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "r1cs")

NEW = ["stark_verify_r1cs_circuit_batch_proofs", "stark_r1cs_proof_from_parts",
       "stark_ctx_set_verify_batch_transcript"]


def test_handle_symbols_exported_declared_and_bound():
    lib = S.load_library()
    declared = S.header_symbols()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in declared, name
        assert name in S._SIGNATURES, name
        assert getattr(lib, name).argtypes == S._SIGNATURES[name][0], name
    assert S.header_abi_version() >= 10
    assert lib.stark_abi_version() == S.header_abi_version()


def test_handle_python_surface():
    from stark_amd import verify as V
    assert callable(V.verify_circuit_batch_proofs)
    assert callable(R1csCircuit.verify_batch)
    assert callable(S.Context.set_verify_batch_transcript)
    assert callable(StarkProof.from_parts) and callable(StarkProof.parts) and callable(StarkProof.parts_of_dict)


def test_handle_argument_errors_need_no_device():
    """tests/test_verify_batch_abi.py's list for the handle entry: the whole-call argument errors are decided
    before any device call and nothing is read or written then; an empty batch reads nothing, dummy handles
    included."""
    lib = S.load_library()
    one = (ctypes.c_char_p * 1)(b"\1" + b"\0" * 31)
    dummy = ctypes.create_string_buffer(64)
    h = ctypes.cast(dummy, ctypes.c_void_p)
    hs = (ctypes.c_void_p * 1)(h)
    sts = (ctypes.c_int * 1)(77)
    why = (ctypes.c_uint32 * 1)(77)
    fn = lib.stark_verify_r1cs_circuit_batch_proofs
    assert fn(None, None, one, 1, hs, 1, sts, why) == 3
    assert fn(None, None, None, 1, hs, 1, sts, why) == 3
    assert fn(None, None, one, 1, None, 1, sts, why) == 3
    assert fn(None, None, one, 0, hs, 1, sts, why) == 3
    assert fn(None, None, one, 1, hs, 65536, sts, why) == 3
    assert fn(None, None, one, 1, hs, 0, sts, why) == 3  # null handles come before the empty batch
    assert fn(h, h, None, 1, hs, 1, sts, why) == 3
    assert fn(h, h, one, 1, None, 1, sts, why) == 3
    assert fn(h, h, one, 0, hs, 1, sts, why) == 3
    assert fn(h, h, one, 1, hs, 65536, sts, why) == 3
    assert sts[0] == 77 and why[0] == 77
    assert fn(h, h, one, 1, hs, 0, sts, why) == 0
    assert fn(h, h, one, 1, hs, 0, None, None) == 0
    assert sts[0] == 77 and why[0] == 77 and dummy.raw == b"\0" * 64
    assert lib.stark_ctx_set_verify_batch_transcript(None, 0) == 3


@pytest.fixture(scope="module")
def oracle_proof(oracle):
    """The oracle's proof of `compute`, as tests/test_r1cs_cpu.py makes it."""
    return R.mk_r1cs_proof_json(oracle, R.build_trace(*R.load_fixture(FIX, "compute")))


def _concat(brs):
    return b"".join(bytes(b["leaf"]) for b in brs), b"".join(bytes(n) for b in brs for n in b["nodes"])


def test_from_parts_round_trip(oracle_proof):
    """The proof's text split into parts in Python, a handle made from them: its text is the original byte for
    byte (rendered on the first request), and every accessor returns the parts."""
    p = json.loads(oracle_proof)
    h = StarkProof.from_parts(p)
    assert h.to_json() == oracle_proof
    assert h.to_json() == oracle_proof  # (the second request reads the text kept by the first)
    lib = S.load_library()
    n = ctypes.c_size_t(0)
    assert lib.stark_r1cs_proof_json(h.h, None, 0, ctypes.byref(n)) == 0 and n.value == len(oracle_proof)
    buf = ctypes.create_string_buffer(n.value + 1)
    assert lib.stark_r1cs_proof_json(h.h, buf, n.value + 1, ctypes.byref(n)) == 0
    assert buf.value.decode() == oracle_proof
    assert h.roots() == {k: bytes(p[k]) for k in ("m_root", "l_root", "a_root")}
    for which, key, leaf_len in ((0, "main_branches", 256), (1, "linear_comb_branches", 32)):
        b = h.branches(which)
        leaves, nodes = _concat(p[key])
        assert (b["k"], b["leaf_len"], b["depth"]) == (len(p[key]), leaf_len, len(p[key][0]["nodes"]))
        assert b["leaves"] == leaves and b["nodes"] == nodes
    layers = h.fri_layers()
    assert len(layers) == len(p["fri_proof"])
    for got, want in zip(layers, p["fri_proof"]):
        if "Last" in want:
            assert got == {"last": b"".join(bytes(v) for v in want["Last"]["last"])}
            continue
        m = want["Middle"]
        assert got["root2"] == bytes(m["root2"])
        for part, key in (("column", "column_branches"), ("poly", "poly_branches")):
            leaves, nodes = _concat(m[key])
            assert (got[part]["k"], got[part]["depth"]) == (len(m[key]), len(m[key][0]["nodes"]))
            assert got[part]["leaves"] == leaves and got[part]["nodes"] == nodes
    # a handle rebuilt from a handle's own accessors is the same proof
    assert StarkProof.from_parts(h.parts()).to_json() == oracle_proof


def test_from_parts_argument_errors(oracle_proof):
    from stark_amd.verify import _Branches
    lib = S.load_library()
    parts = StarkProof.parts_of_dict(json.loads(oracle_proof))
    root = parts["m_root"]

    def call(main, lcomb, last=parts["last"], n_last=None, out=True):
        h = ctypes.c_void_p(1)
        rc = lib.stark_r1cs_proof_from_parts(root, root, root, ctypes.byref(main), ctypes.byref(lcomb), None, 0, last,
                                             len(parts["last"]) // 32 if n_last is None else n_last,
                                             ctypes.byref(h) if out else None)
        if out and rc != 0:
            assert h.value is None  # *out is NULL after an error
        if out and rc == 0:
            lib.stark_r1cs_proof_free(h)
        return rc

    def br(b, **kw):
        b = dict(b, **kw)
        return _Branches(b["leaves"], b["nodes"], b["k"], b["leaf_len"], b["depth"])
    good_m, good_l = br(parts["main"]), br(parts["lcomb"])
    assert call(good_m, good_l) == 0
    assert call(br(parts["main"], leaves=None), good_l) == 3  # null leaves, k > 0
    assert call(good_m, br(parts["lcomb"], nodes=None)) == 3  # null nodes, k x depth > 0
    assert call(br(parts["main"], leaf_len=0), good_l) == 3
    assert call(good_m, br(parts["lcomb"], leaf_len=0, k=0)) == 3
    assert call(br(parts["main"], k=1 << 62, leaf_len=8), good_l) == 3  # k x leaf_len overflows
    assert call(br(parts["main"], k=1, depth=1 << 62), good_l) == 3  # k x depth x 32 overflows
    assert call(good_m, good_l, last=None, n_last=4) == 3
    assert call(good_m, good_l, n_last=1 << 60) == 3  # 32 x n_last overflows
    assert call(good_m, good_l, out=False) == 3
    assert call(br(parts["main"], leaves=None, nodes=None, k=0), good_l, last=None, n_last=0) == 0  # counts of zero
