"""CPU: ABI 8's batched proofs of a prepared circuit are exported, declared and bound.  No GPU compute is
called here."""
import stark_amd as S
from stark_amd.r1cs import R1csCircuit

NEW = ["stark_prove_r1cs_circuit_batch", "stark_ctx_set_prove_batch_limit"]


def test_prove_batch_symbols_exported_declared_and_bound():
    lib = S.load_library()
    declared = S.header_symbols()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in declared, name
        assert name in S._SIGNATURES, name
        assert getattr(lib, name).argtypes == S._SIGNATURES[name][0], name
    assert S.header_abi_version() >= 8
    assert lib.stark_abi_version() == S.header_abi_version()


def test_prove_batch_python_surface():
    assert callable(R1csCircuit.prove_batch)
    assert callable(S.Context.set_prove_batch_limit)


def test_prove_batch_null_arguments_need_no_device():
    """The whole-call argument errors are decided before any device call: null handles, and a batch above the
    forests' 65,535 trees (nothing is read then: the arrays passed here hold one entry)."""
    import ctypes
    lib = S.load_library()
    one = (ctypes.c_char_p * 1)(b"")
    lens = (ctypes.c_size_t * 1)(0)
    out = (ctypes.c_void_p * 1)()
    assert lib.stark_prove_r1cs_circuit_batch(None, None, one, lens, 1, out, None) == 3
    assert lib.stark_ctx_set_prove_batch_limit(None, 0) == 3
    assert out[0] is None
