"""CPU: ABI 13's witness check is exported, declared and bound, its record has the header's size, and the
whole-call argument errors need no device."""
import ctypes

import stark_amd as S
from stark_amd.r1cs import R1csCircuit, R1csFailure, WitnessCheck

NEW = ["stark_check_r1cs_circuit_batch", "stark_check_r1cs_circuit"]


def test_witness_check_symbols_exported_declared_and_bound():
    lib = S.load_library()
    declared = S.header_symbols()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in declared, name
        assert name in S._SIGNATURES, name
        assert getattr(lib, name).argtypes == S._SIGNATURES[name][0], name
    assert S.header_abi_version() >= 13
    assert lib.stark_abi_version() == S.header_abi_version()


def test_failure_record_is_104_bytes():
    """uint32 constraint, uint32 reserved, three values of four uint64 limbs: no padding."""
    assert ctypes.sizeof(R1csFailure) == 104
    assert R1csFailure.a.offset == 8 and R1csFailure.b.offset == 40 and R1csFailure.c.offset == 72


def test_witness_check_python_surface():
    import stark_amd.r1cs as M
    assert callable(R1csCircuit.check) and callable(R1csCircuit.check_batch) and callable(M.check_with_witness)
    r = WitnessCheck(8, 2, [(3, 1, 2, 3)])
    assert not r.satisfied and r.n_failed == 2 and r.failures[0][0] == 3
    assert WitnessCheck(0, 0, []).satisfied


def test_witness_check_null_arguments_need_no_device():
    """Null handles, a batch above 65,535 and cap > 0 without `failures` are decided before any device call, and
    nothing is read or written: the arrays passed here hold one entry, the sentinels stay."""
    lib = S.load_library()
    one = (ctypes.c_char_p * 1)(b"")
    lens = (ctypes.c_size_t * 1)(0)
    sts = (ctypes.c_int * 1)(77)
    nf = (ctypes.c_uint32 * 1)(77)
    rec = (R1csFailure * 1)()
    ctypes.memset(rec, 0xA5, 104)
    for batch, cap, failures in ((1, 1, rec), (70000, 1, rec), (1, 1, None), (0, 0, None)):
        assert lib.stark_check_r1cs_circuit_batch(None, None, one, lens, batch, sts, nf, failures, cap) == 3
    assert lib.stark_check_r1cs_circuit(None, None, b"", 0, nf, rec, 1) == 3
    assert sts[0] == 77 and nf[0] == 77 and bytes(rec) == b"\xa5" * 104
