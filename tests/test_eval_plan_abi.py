"""CPU: ABI 14's evaluation plans and the batched multi-point evaluation are exported, declared and bound.  No GPU
compute is called here."""
import ctypes

import stark_amd as S

NEW = ["stark_eval_plan_new", "stark_eval_plan_new_domain", "stark_eval_plan_free", "stark_eval_plan_apply",
       "stark_eval_plan_apply_dev", "stark_eval_poly_multipoint_batch"]


def test_eval_plan_symbols_exported_declared_and_bound():
    lib = S.load_library()
    declared = S.header_symbols()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in declared, name
        assert name in S._SIGNATURES, name
        assert getattr(lib, name).argtypes == S._SIGNATURES[name][0], name
    assert S.header_abi_version() >= 14
    assert lib.stark_abi_version() == S.header_abi_version()


def test_eval_plan_python_surface():
    assert callable(S.Context.eval_plan)
    assert callable(S.Context.eval_poly_multipoint_batch)
    for name in ("apply", "apply_dev", "close", "__enter__", "__exit__"):
        assert callable(getattr(S.EvalPlan, name)), name


def test_eval_plan_null_arguments_need_no_device():
    """Null handles are argument errors decided before any device call; freeing a null plan is a no-op."""
    lib = S.load_library()
    out = ctypes.c_void_p()
    assert lib.stark_eval_plan_new(None, None, 0, 1, ctypes.byref(out)) == 3
    assert lib.stark_eval_plan_new_domain(None, None, 0, None, 0, 1, ctypes.byref(out)) == 3
    assert lib.stark_eval_plan_apply(None, None, 1, 1, None) == 3
    assert lib.stark_eval_plan_apply_dev(None, None, 1, 1, 1, None, 1, None) == 3
    assert lib.stark_eval_poly_multipoint_batch(None, None, 1, 1, None, 1, None) == 3
    assert lib.stark_eval_plan_free(None) == 0
    assert out.value is None
