"""CPU: ABI 11's interpolation plans and the batched lagrange_interp are exported, declared and bound.  No GPU
compute is called here."""
import ctypes

import stark_amd as S

NEW = ["stark_interp_plan_new", "stark_interp_plan_new_domain", "stark_interp_plan_free", "stark_interp_plan_apply",
       "stark_interp_plan_apply_dev", "stark_lagrange_interp_batch"]


def test_interp_batch_symbols_exported_declared_and_bound():
    lib = S.load_library()
    declared = S.header_symbols()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in declared, name
        assert name in S._SIGNATURES, name
        assert getattr(lib, name).argtypes == S._SIGNATURES[name][0], name
    assert S.header_abi_version() >= 11
    assert lib.stark_abi_version() == S.header_abi_version()


def test_interp_batch_python_surface():
    assert callable(S.Context.interp_plan)
    assert callable(S.Context.lagrange_interp_batch)
    for name in ("apply", "apply_dev", "close"):
        assert callable(getattr(S.InterpPlan, name)), name


def test_interp_batch_null_arguments_need_no_device():
    """Null handles are argument errors decided before any device call; freeing a null plan is a no-op."""
    lib = S.load_library()
    out = ctypes.c_void_p()
    assert lib.stark_interp_plan_new(None, None, 0, ctypes.byref(out)) == 3
    assert lib.stark_interp_plan_new_domain(None, None, 0, None, 0, ctypes.byref(out)) == 3
    assert lib.stark_interp_plan_apply(None, None, 1, None) == 3
    assert lib.stark_interp_plan_apply_dev(None, None, 1, None, None) == 3
    assert lib.stark_lagrange_interp_batch(None, None, None, 1, 1, None) == 3
    assert lib.stark_interp_plan_free(None) == 0
    assert out.value is None
