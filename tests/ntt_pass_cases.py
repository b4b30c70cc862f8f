"""The first-pass cases of tests/test_gpu_ntt_first_pass.py and what the CPU tier (tests/test_ntt_pass_cases_cpu.py)
holds them to: the sparse first passes of csrc/ntt.hip's ntt_pass_kernel, and the T-major first pass of the cold
verifier (ntt_first_pass_tmajor), restated from its definition.  Nothing here needs a GPU to import.

Sparse: a first pass of radix 2^r over columns whose rows >= 2^(r - z) are zero (z = zero_log) skips
skip = sparse_first(z, r) copy stages.  Every pair (r, z), 2 <= r <= 9, 1 <= z <= r, in three geometries:
  * plan (r,) at 2^r: the sparse pass is also the last pass (canonical store; the inverse multiplies by n^-1 in
    the store, do_scale);
  * plan (r, 4) at 2^(r + 4): 16 columns, a partial tile;
  * plan (r, 8) at 2^(r + 8): 256 columns, 2^(r - 2) tiles per transform for r > 2 (tile >> log_tiles selects
    the transform, tile & mask the columns);
and one case whose zero_log exceeds the first radix, which pads (pad_kernel) and runs dense.
"""
import ctypes
import functools

import numpy as np

import oracle as O

P = O.P
GUARD = 64          # elements of 0xFF on either side of a device buffer
MAX_LOG_N = 17      # no sparse case is larger than 2^17 points
RADICES = range(2, 10)
PAD_CASE = ((4, 8), 6)   # plan, zero_log > first radix


def sparse_first(zero_log: int, r: int) -> int:
    """Copy stages a first pass of radix 2^r skips (csrc/ntt.hip sparse_first): min(z, r), lowered by one when
    its parity differs from r's (odd radices pair stages (1,2), (3,4).. after a radix-2 stage 0, even (0,1)..)."""
    k = min(zero_log, r)
    if (k & 1) != (r & 1):
        k -= 1
    return k


def sparse_cases():
    """(plan, zero_log): the three geometries of every (r, z), then the pad case."""
    out = []
    for r in RADICES:
        for z in range(1, r + 1):
            for tail in ((), (4,), (8,)):
                out.append(((r,) + tail, z))
    out.append(PAD_CASE)
    return out


def case_id(case) -> str:
    plan, z = case
    return "x".join(map(str, plan)) + f"-z{z}"


# ---- inputs ------------------------------------------------------------------------------------------------

INPUTS = ("random", "all_pm1", "last_pm1")
BATCH = 3


@functools.lru_cache(maxsize=None)
def sparse_input(log_n: int, zero_log: int, kind: str) -> np.ndarray:
    """BATCH compact columns of 2^(log_n - zero_log) elements, (BATCH * m, 4) limbs.  random: distinct columns;
    all_pm1: every live element p - 1 (the copy stages feed equal operands into the first butterflies);
    last_pm1: p - 1 at the last live index alone."""
    m = 1 << (log_n - zero_log)
    if kind == "random":
        x = O.random_elements(BATCH * m, 0xF1257 + 64 * log_n + zero_log)
    else:
        x = np.zeros((BATCH * m, 4), dtype=np.uint64)
        pm1 = O.to_limbs([P - 1])[0]
        if kind == "all_pm1":
            x[:] = pm1
        else:
            x[m - 1::m] = pm1
    x.setflags(write=False)
    return x


def sparse_want(orc, log_n: int, zero_log: int, kind: str, inverse: bool) -> np.ndarray:
    """The oracle's best_fft / inv_best_fft of each compact column padded with zeros: (BATCH * 2^log_n, 4).
    (The oracle pads a short input itself, fft.rs:327-357; equal columns are transformed once.)"""
    x = sparse_input(log_n, zero_log, kind)
    m, w = 1 << (log_n - zero_log), O.root_of_unity(log_n)
    f = orc.inv_best_fft if inverse else orc.best_fft
    cols = []
    for b in range(BATCH):
        if kind != "random" and b > 0:
            cols.append(cols[0])
        else:
            cols.append(f(np.array(x[b * m:(b + 1) * m]), w, log_n, cpus=4))
    return np.concatenate(cols)


# ---- the T-major first pass ----------------------------------------------------------------------------------

# log_n -> first radix of the size's plan (csrc/ntt.hip plan_passes; a single pass up to 2^8)
TMAJOR_FIRST = {2: 2, 3: 3, 4: 4, 5: 5, 6: 6, 7: 7, 8: 8, 9: 4, 10: 5, 12: 6, 14: 7, 16: 8, 20: 8}
TMAJOR_BATCH = 6


def tmajor_zero_logs(log_n: int):
    t = TMAJOR_FIRST[log_n]
    return sorted({z for z in (1, 2, 3, t) if z <= t})


def tmajor_cases():
    return [(log_n, z) for log_n in TMAJOR_FIRST for z in tmajor_zero_logs(log_n)]


@functools.lru_cache(maxsize=None)
def tmajor_input(log_n: int, zero_log: int) -> np.ndarray:
    x = O.random_elements(TMAJOR_BATCH << (log_n - zero_log), 0x7A30 + 64 * log_n + zero_log)
    x.setflags(write=False)
    return x


def tmajor_want(orc, col: np.ndarray, log_n: int, log_t: int, threads: int = 8) -> np.ndarray:
    """ntt_first_pass_tmajor of one compact column by its definition: with T = 2^log_t, A = n / T and w_T = w^A,
    out[t A + j] = sum_r src[j + r A] w_T^(r t) over the column padded to n: the oracle's size-T transform of
    each strided column j (its zero tail left to the oracle's own padding)."""
    n, T = 1 << log_n, 1 << log_t
    A = n // T
    w_t = pow(O.root_of_unity(log_n), A, P)
    rows = -(-len(col) // A)             # live rows of each strided column
    src = np.zeros((rows * A, 4), dtype=np.uint64)
    src[:len(col)] = col
    strided = np.ascontiguousarray(src.reshape(rows, A, 4).transpose(1, 0, 2))   # [j][r]
    out = np.empty((T, A, 4), dtype=np.uint64)

    def run(j):
        out[:, j] = orc.best_fft(strided[j], w_t, log_t)

    if A >= 64 and threads > 1:          # (the oracle call releases the GIL)
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(run, range(A)))
    else:
        for j in range(A):
            run(j)
    return out.reshape(n, 4)


# ---- device buffers between guards -------------------------------------------------------------------------------

class Guarded:
    """A device buffer of n elements (32 bytes each) between two guard runs of GUARD elements of 0xFF; the
    region itself is 0xFF too until `put`.  A read of a row that should be an implicit zero then changes the
    output, and a store outside the region shows in `get`."""

    def __init__(self, ctx, n: int, data=None):
        self.ctx, self.n = ctx, n
        self.base = ctx.alloc((n + 2 * GUARD) * 32)
        self.ptr = self.base + GUARD * 32
        h = np.full((n + 2 * GUARD, 4), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
        if data is not None:
            assert data.shape == (n, 4)
            h[GUARD:GUARD + n] = data
        ctx.h2d(self.base, h)

    def get(self, what="") -> np.ndarray:
        """The region; both guards must still be 0xFF."""
        h = np.empty((self.n + 2 * GUARD, 4), dtype=np.uint64)
        self.ctx.d2h(h, self.base)
        ff = np.uint64(0xFFFFFFFFFFFFFFFF)
        assert (h[:GUARD] == ff).all(), f"{what}: the guard before the buffer was written"
        assert (h[GUARD + self.n:] == ff).all(), f"{what}: the guard after the buffer was written"
        return h[GUARD:GUARD + self.n]

    def free(self):
        if self.base:
            self.ctx.free(self.base)
            self.base = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def limbs_arg(x: int):
    return (ctypes.c_uint64 * 4)(*[(x >> (64 * k)) & (2**64 - 1) for k in range(4)])
