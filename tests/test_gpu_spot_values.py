"""The cold verifier's spot evaluation (csrc/r1cs.hip circuit_spot_values: spot_setup_kernel, spot_eval_kernel,
spot_sum_kernel over the T-major first passes of the six circuit columns) value by value, through the test hook
stark_test_circuit_spot_values, which builds the cold circuit as stark_verify_r1cs_bytes does.

Reference: oracle/r1cs.py's step columns K, F0, F1, F2, IDX, PIDX, extended by the C oracle (inv_best_fft over the
steps, best_fft over the precision domain), read at the positions.  The kernel's sums may come back unreduced
(below 2^256) and are reduced below p here as verify_r1cs reduces them.  Bit for bit.

Positions (P the precision, T the plan's first radix): 0, 1, 7, 8, T - 1, T, T + 1, P / 2, P - T, P - 1 and one
per residue class mod T, in calls of 128 (kSpotMax) and one call of a single position.  The verifier itself never
samples a multiple of 8; there x^S is 1 or -1.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

import oracle as O
import r1cs as R
import r1cs_cases as C
import stark_amd as S

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

pytestmark = pytest.mark.gpu

P = O.P
SPOT_MAX = 128
BAD_ARG = 3
SYNTH = (6, 9, 13, 14)   # log2 steps: the first multi-pass plan; S = 16; S = 64; four workgroups per position


def _hook():
    fn = S.load_library().stark_test_circuit_spot_values
    fn.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t,
                   ctypes.c_void_p]
    fn.restype = ctypes.c_int
    return fn


def _spot(c, r1: bytes, positions):
    """(status, values[6][n] as integers below 2^256)."""
    n = len(positions)
    pos = (ctypes.c_uint64 * n)(*positions)
    out = np.full((6 * n + 2, 4), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)   # one guard element on either side
    rc = _hook()(c.h, r1, len(r1), pos, n, out[1:].ctypes.data)
    assert (out[0] == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and (out[-1] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    if rc != 0:
        assert (out == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "a refused call wrote its output"
        return rc, None
    vals = O.from_limbs(out[1:-1])
    return rc, [vals[k * n:(k + 1) * n] for k in range(6)]


def _synth(log_steps: int) -> bytes:
    import synth_r1cs
    return synth_r1cs.for_steps(log_steps)[0]


def _reference(oracle, r1: bytes):
    """(log_prec, the six extensions as limbs)."""
    circ = R.read_r1cs(r1)
    h = circ.header
    v = R.verifier_inputs(circ, [0] * (1 + h.n_public_inputs + h.n_public_outputs))
    os_ = len(v["coefficients"])
    log_steps = (os_ - 1).bit_length()    # log2_ceil of verify.rs / prove.rs; os >= 6, so at least 8 steps
    assert log_steps >= 3
    steps, log_prec = 1 << log_steps, log_steps + 3
    g2 = O.root_of_unity(log_prec)
    g1 = pow(g2, 8, P)
    pad = [0] * (steps - os_)
    cols = [v["coefficients"] + pad, v["flag0"] + pad, v["flag1"] + pad, v["flag2"] + pad, list(range(steps)),
            list(v["permuted_indices"]) + list(range(os_, steps))]
    def limbs(col):
        if max(col) >> 64:
            return O.to_limbs(col)
        a = np.zeros((len(col), 4), dtype=np.uint64)   # (flags and indices: one limb)
        a[:, 0] = col
        return a
    ext = [oracle.best_fft(oracle.inv_best_fft(limbs(col), g1, log_steps, cpus=4), g2, log_prec, cpus=4)
           for col in cols]
    return log_prec, ext


def _positions(log_prec: int):
    """The directed positions, then one per residue class mod T (class c at c + T k, k from a fixed generator),
    filled up with further generated positions to a multiple of 128."""
    prec, t = 1 << log_prec, 1 << S.ntt_plan(log_prec)[0]
    rng = np.random.default_rng(log_prec)
    out = [0, 1, 7, 8, t - 1, t % prec, (t + 1) % prec, prec // 2, prec - t, prec - 1]
    out += [c + t * int(rng.integers(0, prec // t)) for c in range(t)]
    while len(out) % SPOT_MAX:
        out.append(int(rng.integers(0, prec)))
    assert all(0 <= e < prec for e in out) and {e % t for e in out} == set(range(t))
    return out


def _check(ctx, oracle, r1: bytes):
    log_prec, ext = _reference(oracle, r1)
    positions = _positions(log_prec)
    calls = [positions[i:i + SPOT_MAX] for i in range(0, len(positions), SPOT_MAX)]
    calls.append([positions[8]])           # n = 1
    calls.append([(1 << log_prec) - 8])    # n = 1 at a multiple of 8
    assert any(len(c) == SPOT_MAX for c in calls)
    names = ("K", "F0", "F1", "F2", "IDX", "PIDX")
    for pos in calls:
        rc, got = _spot(ctx, r1, pos)
        assert rc == 0, rc
        for k in range(6):
            want = O.from_limbs(ext[k][pos])
            have = [g % P for g in got[k]]
            bad = [(e, i) for i, e in enumerate(pos) if have[i] != want[i]]
            assert not bad, (names[k], "n", len(pos), "wrong at (position, index)", bad[:8])


@pytest.mark.parametrize("name", C.SMALL)
def test_spot_values_directed_circuits(ctx, oracle, name):
    _check(ctx, oracle, C.CASES[name].circuit.r1cs)


@pytest.mark.parametrize("log_steps", SYNTH)
def test_spot_values_synthetic(ctx, oracle, log_steps):
    _check(ctx, oracle, _synth(log_steps))


def test_spot_values_refused(ctx):
    """129 positions, or a position at or above the precision: STARK_ERR_BAD_ARG and nothing written."""
    r1 = _synth(6)
    prec = 1 << 9
    assert _spot(ctx, r1, [3] * (SPOT_MAX + 1))[0] == BAD_ARG
    assert _spot(ctx, r1, [3, prec])[0] == BAD_ARG
    assert _spot(ctx, r1, [2 * prec + 1])[0] == BAD_ARG
    assert _spot(ctx, r1, [prec - 1])[0] == 0
