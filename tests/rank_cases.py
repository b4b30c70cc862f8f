"""Directed inputs for the per-rank kernels of the multi-GPU provers (csrc/dist.hip, the residue-class fold of
csrc/fri.hip, the interleave / top / multi-gather kernels of csrc/merkle.hip), op by op.

The golden circuits decide every shape the multi-process tests reach, so a fold never sees one row per rank, a
digest tree never has one digest per chunk and a value is never 0 or p - 1.  These tables sit at the edges of
each op's own argument space instead: the smallest sizes, the sizes on and next to a tile or workgroup edge,
exponents that wrap the twiddle mask, roots that reduce more than once.  tests/test_rank_cases_cpu.py holds the
host restatements of the ops to independent definitions on these tables; tests/test_gpu_rank_ops.py compares
each GPU op with its restatement on them, bit for bit.

No GPU and no oracle library here: only P, to_limbs and random_elements."""
import numpy as np

from oracle import P, random_elements, to_limbs

GENERATOR = 7  # of the field's multiplicative group (fp.rs:10)


def w_of(log_n: int) -> int:
    """The primitive 2^log_n-th root the provers use, 7^((p-1)/2^log_n) (prove.rs:71-82)."""
    return pow(GENERATOR, (P - 1) >> log_n, P)


def ints(limbs) -> list:
    a = np.asarray(limbs, dtype=np.uint64).reshape(-1, 4)
    return [int(r[0]) | (int(r[1]) << 64) | (int(r[2]) << 128) | (int(r[3]) << 192) for r in a]


def le32(values) -> bytes:
    """Field elements as the 32-byte little-endian strings the provers exchange."""
    return b"".join(int(v).to_bytes(32, "little") for v in values)


# ---- values ------------------------------------------------------------------------------------------------

KINDS = ("random", "pm1", "zero", "edge")


def VALUES(n: int, kind: str, seed: int = 0) -> np.ndarray:
    """n field elements as (n, 4) u64 limbs.  random; pm1: every element p - 1; zero; edge: random with 0, 1 and
    p - 1 at the first, middle and last positions (as many of them as n has room for)."""
    if kind == "zero":
        return np.zeros((n, 4), dtype=np.uint64)
    if kind == "pm1":
        return to_limbs([P - 1] * n)
    a = random_elements(n, 0x5EED0A00 + 977 * seed + n)
    if kind == "edge":
        for pos, v in ((0, 0), (n // 2, 1), (n - 1, P - 1)):  # (n = 1: p - 1 alone)
            a[pos] = to_limbs([v])[0]
    elif kind != "random":
        raise ValueError(kind)
    return a


def named(m: int, count: int) -> np.ndarray:
    """count elements whose limbs name (matrix m, position k): a misplaced element identifies itself."""
    a = np.zeros((count, 4), dtype=np.uint64)
    a[:, 0] = np.arange(count, dtype=np.uint64)
    a[:, 1] = m
    a[:, 2] = 0x7261_6E6B  # "rank"
    a[:, 3] = np.arange(count, dtype=np.uint64) ^ np.uint64(0x1555_5555)  # (< 2^61: below p's top limb)
    return a


# ---- stark_transpose_dev: (rows, cols, batch); the tile is 32 x 32 elements --------------------------------

TRANSPOSE = [(1, 1, 1), (1, 33, 1), (33, 1, 1), (31, 32, 1), (32, 32, 2), (33, 65, 3), (64, 96, 1), (37, 70, 5)]
TRANSPOSE_EMPTY = [(0, 5, 1), (5, 0, 1), (5, 5, 0)]

# ---- stark_twiddle2d_dev: (rows, cols, row_base, col_base, log_order) --------------------------------------
# The table is two-level with kb = (log_order + 1) / 2, so odd and even orders differ; the last case's bases
# exceed the order (and col_base + j 2^63) and are reduced by the mask before the product.

TWIDDLE = [(1, 1, 0, 0, 1), (5, 7, 0, 0, 3), (5, 7, 6, 7, 3), (4, 64, 0, 0, 12),
           (3, 300, 2**13 - 2, 2**13 - 150, 13), (3, 300, 2**20 - 2, 2**20 - 150, 20),
           (2, 257, 2**40 + 3, 2**63 + 5, 12)]
TWIDDLE_KINDS = ("edge", "pm1")

# ---- stark_ntt_strided_dev / _tw_dev: one thread per column, 256 per workgroup ------------------------------

STRIDED_LOG_G = (1, 2, 3, 4)
STRIDES = (1, 255, 256, 257)
STRIDED_KINDS = ("random", "pm1", "zero")


def strided_tw(log_g: int) -> list:
    """(log_order, base): a twiddle root of order exactly G; bases whose (base + i) wraps the mask inside the
    stride (2^13 - 100 + i passes 2^13 at i = 100) and the multi-process test's own pair."""
    return [(log_g, 0), (13, 2**13 - 100), (20, 123456)]


def tone_bins(log_g: int) -> list:
    G = 1 << log_g
    return sorted({1, G - 1})


def tone(log_g: int, stride: int, m: int, inverse: bool) -> np.ndarray:
    """(G, stride) matrix whose every column is the tone (p - 1) w^(-m j) (w^(+m j) for the inverse transform):
    its butterflies meet equal operands at every stage, and its transform is G (p - 1) (inverse: p - 1) at
    k = m and zero elsewhere."""
    G = 1 << log_g
    w = w_of(log_g)
    wm = pow(w, m if inverse else G - m, P)
    col = [(P - 1) * pow(wm, j, P) % P for j in range(G)]
    return to_limbs([col[j] for j in range(G) for _ in range(stride)])


def tone_transform(log_g: int, stride: int, m: int, inverse: bool) -> np.ndarray:
    G = 1 << log_g
    peak = (P - 1) if inverse else G * (P - 1) % P
    return to_limbs([peak if k == m else 0 for k in range(G) for _ in range(stride)])


# ---- stark_cyclic_ntt_local_dev: (log_n, log_g, rank), the edges of its argument check ---------------------

CYCLIC_LOCAL = [(2, 0, 0), (3, 1, 1), (8, 4, 0), (8, 4, 15)]
CYCLIC_LOCAL_BAD_LENGTH = [(2, 1, 0),   # log_n < log_g + 2
                           (5, 3, 0),   # log_n < 2 log_g (and >= log_g + 2)
                           (8, 2, 4)]   # rank = G

# ---- stark_fri_fold_dev / _dev_root -------------------------------------------------------------------------

FOLD_SIZES = [(n, world) for n in (4, 8, 32, 128) for world in (1, 2, 4, 8) if (n // 4) % world == 0] + \
             [(4096, 1), (4096, 8)]
FOLD_KINDS = ("random", "pm1", "zero", "cubic")
CUBIC = (3, 5, 7, 11)  # 3 + 5 X + 7 X^2 + 11 X^3


def cubic_at(x: int) -> int:
    return (CUBIC[0] + x * (CUBIC[1] + x * (CUBIC[2] + x * CUBIC[3]))) % P


def fold_roots(n: int) -> list:
    """(name, 32 bytes read as from_bytes_le): 0; an ordinary digest; 2^256 - 1 (five subtractions of p); p
    (reduces to 0), p - 1, p + 1; and w^3, a point of the layer, where the cubic is evaluated at one of its
    own nodes and must return that row's value."""
    w = w_of(n.bit_length() - 1)
    return [("zero", bytes(32)), ("digest", bytes(range(32))), ("ones", b"\xff" * 32),
            ("p", P.to_bytes(32, "little")), ("p-1", (P - 1).to_bytes(32, "little")),
            ("p+1", (P + 1).to_bytes(32, "little")), ("node", pow(w, 3, P).to_bytes(32, "little"))]


FOLD_ROOT_NAMES = ("zero", "digest", "ones", "p", "p-1", "p+1", "node")


def fold_layer(n: int, kind: str) -> list:
    """The n values of one FRI layer in natural order (ints)."""
    if kind == "cubic":
        w = w_of(n.bit_length() - 1)
        return [cubic_at(pow(w, i, P)) for i in range(n)]
    return ints(VALUES(n, kind, seed=3))


def rank_values(layer: list, world: int, rank: int) -> bytes:
    """What rank holds of a layer: the values at the points rank + world j."""
    return le32(layer[rank::world])


FOLD_BAD_ARG = [(32, 3, 0), (32, 4, 4)]        # (n, world, rank): world = 3; rank = world
FOLD_BAD_LENGTH = [(6, 1, 0), (8, 4, 0)]       # n = 6; (n / 4) % world != 0

# ---- digest trees, leaf digests, top ------------------------------------------------------------------------

DIGEST_TREES = [(1, 1), (2, 2), (8, 8), (8, 1), (16, 4), (1024, 8), (4096, 2)]  # (n, interleave)
LEAF_LENS = (32, 33, 256)
TOP_G = (1, 2, 4, 1024)


def tree_indices(n: int) -> list:
    return [0, n - 1, 1 % n, n // 2, 0]


def random_bytes(nbytes: int, seed: int) -> bytes:
    return bytes(np.random.default_rng(0x5EED0B00 + seed).integers(0, 256, size=nbytes, dtype=np.uint8))


def deinterleave(chunks: bytes, n: int, g: int) -> bytes:
    """Leaf order of n digests held as g residue-class chunks: leaf g m + r is chunk r's digest m."""
    a = np.frombuffer(chunks, dtype=np.uint8).reshape(g, n // g, 32)
    return a.transpose(1, 0, 2).tobytes()


DIGESTS_BAD_ARG = [(8, 0), (8, 3)]             # (n, interleave)
DIGESTS_BAD_LENGTH = [(0, 1), (6, 1), (2, 4)]
TOP_BAD_LENGTH = (3, 2048)

# ---- stark_open_batch ---------------------------------------------------------------------------------------

ROW_BYTES = (32, 256, 7, 36)
OPEN_TREES = [(64, 32), (16, 33), (8, 256)]    # (n, leaf_len) of the trees over leaves
OPEN_DIGEST_TREE = (32, 4)                     # (n, interleave)
OPEN_ROWS = 24                                 # rows of every row buffer


def index_lists(n: int, seed: int) -> list:
    """[0], [n - 1], duplicates, and 40 random indices of n."""
    rnd = np.random.default_rng(0x5EED0C00 + seed).integers(0, n, size=40)
    return [[0], [n - 1], [n // 2, 1 % n, n // 2, n // 2, 1 % n], [int(x) for x in rnd]]


# ---- rank state and L ---------------------------------------------------------------------------------------

RANK_STATE = [("compute", world, rank) for world in (1, 2, 4, 8) for rank in range(world)] + \
             [("poseidon3_test", 4, 3)]
