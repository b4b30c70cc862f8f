"""CPU tier of tests/ntt_pass_cases.py: the sparse case table covers what it claims, and the restatement of the
T-major first pass that tests/test_gpu_ntt_first_pass.py compares the kernel with is itself held to its
definition and to the oracle's transform."""
import numpy as np
import pytest

import ntt_pass_cases as N
import oracle as O
import stark_amd as S

P = O.P


def test_table_holds_every_pair():
    cases = N.sparse_cases()
    assert len(set(cases)) == len(cases)
    pairs = {(plan[0], z) for plan, z in cases if (plan, z) != N.PAD_CASE}
    assert pairs == {(r, z) for r in range(2, 10) for z in range(1, r + 1)}
    assert len(pairs) == 44
    for r, z in pairs:  # each pair in its three geometries
        assert {plan for plan, zz in cases if plan[0] == r and zz == z} >= {(r,), (r, 4), (r, 8)}
    assert len(cases) == 3 * 44 + 1
    plan, z = N.PAD_CASE
    assert plan == (4, 8) and z == 6 and z > plan[0] and N.PAD_CASE in cases


def test_table_reaches_every_radix_and_skip():
    """Every (radix, skip) sparse_first can give: skip has r's parity and 0 <= skip <= r; skip 0 is an even
    radix at zero_log 1, the dense instance on a compact source."""
    possible = {(r, k) for r in range(2, 10) for k in range(0, r + 1) if (k & 1) == (r & 1)}
    for tail in ((), (4,), (8,)):
        reached = {(plan[0], N.sparse_first(z, plan[0])) for plan, z in N.sparse_cases()
                   if plan[1:] == tail and z <= plan[0]}
        assert reached == possible
    assert all(N.sparse_first(1, r) == 0 for r in (2, 4, 6, 8))
    assert all(N.sparse_first(1, r) == 1 for r in (3, 5, 7, 9))
    assert [N.sparse_first(z, 9) for z in range(1, 10)] == [1, 1, 3, 3, 5, 5, 7, 7, 9]
    assert [N.sparse_first(z, 4) for z in range(1, 5)] == [0, 2, 2, 4]


def test_no_case_above_2_17():
    assert max(sum(plan) for plan, _ in N.sparse_cases()) == N.MAX_LOG_N == 17
    for plan, z in N.sparse_cases():
        assert 1 <= z <= sum(plan)


def test_tmajor_table_matches_the_plans():
    assert sorted(N.TMAJOR_FIRST) == [2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 16, 20]
    for log_n, t in N.TMAJOR_FIRST.items():
        assert S.ntt_plan(log_n)[0] == t, log_n
        assert (len(S.ntt_plan(log_n)) == 1) == (log_n <= 8)
        assert N.tmajor_zero_logs(log_n) == sorted({z for z in (1, 2, 3, t) if z <= t})
    assert [N.TMAJOR_FIRST[k] for k in (9, 10, 12, 14, 16, 20)] == [4, 5, 6, 7, 8, 8]


@pytest.mark.parametrize("log_n,zero_log", [(9, 1), (9, 4), (10, 3), (10, 5)])
def test_tmajor_restatement(oracle, log_n, zero_log):
    """out[t A + j] = sum_r src[j + r A] w_T^(r t) (tmajor_want, from the oracle's size-T transforms) against
    the sum itself at a few (t, j), and then, for every i < n,
    sum_j w^(i j) out[(i mod T) A + j] = the oracle's best_fft of the padded column at i."""
    n, log_t = 1 << log_n, N.TMAJOR_FIRST[log_n]
    T, A = 1 << log_t, n >> log_t
    w = O.root_of_unity(log_n)
    col = np.array(N.tmajor_input(log_n, zero_log)[:n >> zero_log])
    out = O.from_limbs(N.tmajor_want(oracle, col, log_n, log_t, threads=1))
    src = O.from_limbs(col) + [0] * (n - len(col))
    w_t = pow(w, A, P)
    for t, j in ((0, 0), (1, 0), (T - 1, A - 1), (3 % T, 5 % A), (T // 2, A // 2)):
        assert out[t * A + j] == sum(src[j + r * A] * pow(w_t, r * t, P) for r in range(T)) % P, (t, j)
    want = O.from_limbs(oracle.best_fft(col, w, log_n))
    wp = [1] * n
    for k in range(1, n):
        wp[k] = wp[k - 1] * w % P
    for i in range(n):
        base = (i % T) * A
        assert sum(wp[i * j % n] * out[base + j] for j in range(A)) % P == want[i], i


def test_sparse_reference_is_the_padded_transform(oracle):
    """sparse_want hands the oracle the compact column; the oracle pads it (fft.rs:327-357): same as padding here."""
    log_n, z = 8, 3
    m, n = 1 << (log_n - z), 1 << log_n
    for kind in N.INPUTS:
        x = N.sparse_input(log_n, z, kind)
        assert x.shape == (N.BATCH * m, 4)
        for inverse in (False, True):
            want = N.sparse_want(oracle, log_n, z, kind, inverse)
            f = oracle.inv_best_fft if inverse else oracle.best_fft
            for b in range(N.BATCH):
                padded = np.zeros((n, 4), dtype=np.uint64)
                padded[:m] = x[b * m:(b + 1) * m]
                assert np.array_equal(want[b * n:(b + 1) * n], f(padded, O.root_of_unity(log_n), log_n))
    pm1 = O.to_limbs([P - 1])[0]
    last = N.sparse_input(log_n, z, "last_pm1")
    assert [i for i in range(len(last)) if last[i].any()] == [m - 1, 2 * m - 1, 3 * m - 1]
    assert (N.sparse_input(log_n, z, "all_pm1") == pm1).all() and (last[m - 1] == pm1).all()
