"""ABI 12 without a GPU: the three symbols of batched FRI verification, and stark_fri_proof_from_parts -- a
Vec<FriProof> handle over copies of a caller's parts -- against the oracle's proof text."""
import ctypes
import json

import pytest

import oracle as O
import stark_amd as S
from stark_amd.verify import _Branches, _FriLayer

NEW = ("stark_fri_proof_from_parts", "stark_verify_low_degree_batch", "stark_ctx_set_verify_batch_last")


def _proof_text(log_n, bound, excl, seed=1):
    n = 1 << log_n
    w = O.root_of_unity(log_n)
    vals = O.py_serial_fft(O.from_limbs(O.random_elements(bound, seed)) + [0] * (n - bound), w, log_n)
    return O.py_prove_low_degree_json(vals, w, bound, excl)


@pytest.fixture(scope="module")
def text():
    return _proof_text(7, 32, 8)  # one Middle layer, a Last of 32 values


def test_header_declares_and_library_exports():
    lib = S.load_library()
    syms = S.header_symbols()
    for name in NEW:
        assert name in syms, name
        assert hasattr(lib, name), name
        assert name in S._SIGNATURES, name


def test_abi_version():
    lib = S.load_library()
    assert S.header_abi_version() >= 12
    assert lib.stark_abi_version() == S.header_abi_version()


@pytest.mark.parametrize("log_n,bound,excl", [(7, 32, 8), (6, 16, 8), (8, 64, 0)])
def test_from_parts_round_trip(log_n, bound, excl):
    want = _proof_text(log_n, bound, excl, seed=log_n)
    h = S.FriProofList.from_parts(json.loads(want))
    assert h.to_json() == want
    assert len(h) == len(json.loads(want))
    # parts() reads everything from_parts takes back out of the handle
    again = S.FriProofList.from_parts(h.parts())
    assert again.to_json() == want


def test_from_parts_accessors(text):
    lib = S.load_library()
    proof = json.loads(text)
    h = S.FriProofList.from_parts(proof)
    is_last, root2 = ctypes.c_int(-1), ctypes.create_string_buffer(32)
    sz = [ctypes.c_size_t() for _ in range(5)]
    assert lib.stark_fri_proof_layer_info(h.h, 0, ctypes.byref(is_last), root2, *[ctypes.byref(x) for x in sz]) == 0
    mid = proof[0]["Middle"]
    assert is_last.value == 0 and root2.raw == bytes(mid["root2"])
    assert [x.value for x in sz] == [40, len(mid["column_branches"][0]["nodes"]), 160,
                                     len(mid["poly_branches"][0]["nodes"]), 0]
    assert lib.stark_fri_proof_layer_info(h.h, 1, ctypes.byref(is_last), None, *[ctypes.byref(x) for x in sz]) == 0
    assert is_last.value == 1 and sz[4].value == len(proof[1]["Last"]["last"])
    last = ctypes.create_string_buffer(32 * sz[4].value)
    assert lib.stark_fri_proof_layer_data(h.h, 1, None, 0, None, 0, None, 0, None, 0, last, len(last)) == 0
    assert last.raw == b"".join(bytes(v) for v in proof[1]["Last"]["last"])


def _call(lib, layers, n_layers, last, n_last, out):
    return lib.stark_fri_proof_from_parts(layers, n_layers, last, n_last, out)


def _layer_array(parts, keep, **change):
    """parts' first Middle layer as a one-entry stark_fri_layer_parts array, with fields of its column set changed."""
    m = parts["layers"][0]
    col = dict(m["column"], **change)
    arr = (_FriLayer * 1)()
    arr[0] = _FriLayer(change.get("root2", m["root2"]), _Branches(col["leaves"], col["nodes"], col["k"], col["leaf_len"],
                                                                  col["depth"]),
                       _Branches(m["poly"]["leaves"], m["poly"]["nodes"], m["poly"]["k"], m["poly"]["leaf_len"],
                                 m["poly"]["depth"]))
    keep.append(arr)
    return ctypes.cast(arr, ctypes.c_void_p)


def test_from_parts_bad_args(text):
    lib = S.load_library()
    parts = S.FriProofList.parts_of_list(json.loads(text))
    last, n_last = parts["last"], len(parts["last"]) // 32
    keep = []
    good = _layer_array(parts, keep)
    h = ctypes.c_void_p(0xdead)

    def refused(*args):
        h.value = 0xdead
        assert _call(lib, *args, ctypes.byref(h)) == 3
        assert h.value is None  # *out NULL

    assert _call(lib, good, 1, last, n_last, None) == 3                 # a null out
    refused(None, 1, last, n_last)                                       # a null layer array with a count
    refused(good, 1, None, n_last)                                       # null Last values with a count
    arr = (_FriLayer * 1)()
    ctypes.memmove(arr, good.value, ctypes.sizeof(_FriLayer))
    arr[0].root2 = None
    refused(ctypes.cast(arr, ctypes.c_void_p), 1, last, n_last)          # a null root2
    refused(_layer_array(parts, keep, leaf_len=0), 1, last, n_last)      # a leaf_len of 0
    refused(_layer_array(parts, keep, leaves=None), 1, last, n_last)     # null leaves with a count
    refused(_layer_array(parts, keep, nodes=None), 1, last, n_last)      # null nodes with a count and a depth
    big = ctypes.c_size_t(-1).value
    refused(_layer_array(parts, keep, k=big // 2), 1, last, n_last)      # k x leaf_len overflows
    refused(_layer_array(parts, keep, k=1 << 40, depth=1 << 40), 1, last, n_last)  # k x depth x 32 overflows
    refused(good, 1, last, big // 16)                                    # n_last x 32 overflows
    # and the good call, with an empty Last and with no layers
    assert _call(lib, good, 1, None, 0, ctypes.byref(h)) == 0 and h.value
    lib.stark_fri_proof_free(h)
    assert _call(lib, None, 0, last, n_last, ctypes.byref(h)) == 0 and h.value
    assert lib.stark_fri_proof_num_layers(h) == 1
    lib.stark_fri_proof_free(h)


def test_from_parts_judges_nothing_else(text):
    """Odd shapes are a verifier's business: 39 openings, 31-byte leaves and 48 Last values make handles whose
    text is the parts' text."""
    proof = json.loads(text)
    proof[0]["Middle"]["column_branches"].pop()
    for b in proof[0]["Middle"]["poly_branches"]:
        b["leaf"] = b["leaf"][:31]
    proof[1]["Last"]["last"] = (proof[1]["Last"]["last"] * 2)[:48]
    h = S.FriProofList.from_parts(proof)
    assert h.to_json() == json.dumps(proof, separators=(",", ":"))


def test_python_refuses_what_a_handle_cannot_hold(text):
    proof = json.loads(text)
    for bad in ([], proof[:1], [proof[1], proof[0], proof[1]]):
        with pytest.raises(S.StarkError) as e:
            S.FriProofList.from_parts(bad)
        assert e.value.code == 3


def test_set_verify_batch_last_null_ctx():
    assert S.load_library().stark_ctx_set_verify_batch_last(None, 1) == 3
    # whole-call errors of the batched entry need no device either
    lib = S.load_library()
    assert lib.stark_verify_low_degree_batch(None, b"\0" * 32, None, None, 1, 16, 8, None, None) == 3
