"""CPU: ABI 9's batched verification of a prepared circuit's proofs is exported, declared and bound.  No GPU
compute is called here."""
import ctypes

import stark_amd as S
from stark_amd.r1cs import R1csCircuit

NEW = ["stark_verify_r1cs_circuit_batch", "stark_ctx_set_verify_batch_limit"]


def test_verify_batch_symbols_exported_declared_and_bound():
    lib = S.load_library()
    declared = S.header_symbols()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in declared, name
        assert name in S._SIGNATURES, name
        assert getattr(lib, name).argtypes == S._SIGNATURES[name][0], name
    assert S.header_abi_version() >= 9
    assert lib.stark_abi_version() == S.header_abi_version()


def test_verify_batch_python_surface():
    from stark_amd import verify as V
    assert callable(V.verify_circuit_batch)
    assert callable(R1csCircuit.verify_batch)
    assert callable(S.Context.set_verify_batch_limit)
    masks = [V.FAIL_PUBLIC_ONE, V.FAIL_FRI_PATHS, V.FAIL_FRI_ROWS, V.FAIL_FRI_LAST, V.FAIL_OPENING_PATHS,
             V.FAIL_SPOT, V.FAIL_SINGLE]
    assert all(m and m & (m - 1) == 0 for m in masks) and len(set(masks)) == 7
    # the header's values
    import re
    text = open(S.HEADER_PATH).read()
    for name in ("PUBLIC_ONE", "FRI_PATHS", "FRI_ROWS", "FRI_LAST", "OPENING_PATHS", "SPOT", "SINGLE"):
        m = re.search(r"#define\s+STARK_VERIFY_FAIL_%s\s+(0x[0-9a-fA-F]+)u" % name, text)
        assert m and int(m.group(1), 16) == getattr(V, "FAIL_" + name), name


def test_verify_batch_argument_errors_need_no_device():
    """The whole-call argument errors are decided before any device call, and nothing is read or written then
    (the arrays passed here hold one entry); an empty batch is fine."""
    lib = S.load_library()
    one = (ctypes.c_char_p * 1)(b"\1" + b"\0" * 31)
    js = (ctypes.c_char_p * 1)(b"{}")
    lens = (ctypes.c_size_t * 1)(2)
    sts = (ctypes.c_int * 1)(77)
    why = (ctypes.c_uint32 * 1)(77)
    fn = lib.stark_verify_r1cs_circuit_batch
    # (a context and a circuit handle cannot exist without a device: null handles with every other argument set,
    # then each remaining null, the zero count and the oversized batch with null handles as well)
    assert fn(None, None, one, 1, js, lens, 1, sts, why) == 3
    assert fn(None, None, None, 1, js, lens, 1, sts, why) == 3
    assert fn(None, None, one, 1, None, lens, 1, sts, why) == 3
    assert fn(None, None, one, 1, js, None, 1, sts, why) == 3
    assert fn(None, None, one, 0, js, lens, 1, sts, why) == 3
    assert fn(None, None, one, 1, js, lens, 65536, sts, why) == 3
    assert fn(None, None, one, 1, js, lens, 0, sts, why) == 3  # null handles come before the empty batch
    assert sts[0] == 77 and why[0] == 77
    assert lib.stark_ctx_set_verify_batch_limit(None, 0) == 3
    # An empty batch reads nothing, the handles included: any non-null pointers do.
    dummy = ctypes.create_string_buffer(64)
    h = ctypes.cast(dummy, ctypes.c_void_p)
    assert fn(h, h, one, 1, js, lens, 0, sts, why) == 0
    assert fn(h, h, one, 1, js, lens, 0, None, None) == 0
    assert sts[0] == 77 and why[0] == 77 and dummy.raw == b"\0" * 64
