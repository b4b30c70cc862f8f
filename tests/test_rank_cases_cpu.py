"""CPU: the host restatements of the multi-GPU provers' per-rank ops at the edges of tests/rank_cases.py.

OracleProverOps and _PyTree (tests/test_dprove_cpu.py) and OracleOps (tests/test_distributed_cpu.py) are pinned,
through the real orchestration, to the golden proof digests and to the oracle's NTT -- at the golden circuits'
shapes.  tests/test_gpu_rank_ops.py uses them as the reference on directed shapes those circuits never reach,
so here each one is held to an independent definition on exactly those tables: the fold to the oracle's
multi_interp_4 + eval_quartic_multi over the whole layer and to its own world = 1 result, _PyTree to the
oracle's Merkle tree, the strided transforms to the DFT sum in Python integers, the twiddle and the transpose
to one-line definitions."""
import numpy as np
import pytest
import torch

import oracle as O
import rank_cases as C
from test_distributed_cpu import OracleOps
from test_dprove_cpu import OracleProverOps, _PyTree, _u8

P = O.P


def same(got, want, what, unit: int = 32) -> None:
    """got == want (bytes, or arrays of equal shape), told by the first differing element of `unit` bytes."""
    g = got if isinstance(got, bytes) else np.ascontiguousarray(got).tobytes()
    w = want if isinstance(want, bytes) else np.ascontiguousarray(want).tobytes()
    if g != w:
        k = next((i for i in range(min(len(g), len(w)) // unit + 1)
                  if g[unit * i:unit * (i + 1)] != w[unit * i:unit * (i + 1)]))
        pytest.fail(f"{what}: {len(g)} and {len(w)} bytes differ from element {k}: "
                    f"{g[unit * k:unit * (k + 1)].hex()} for {w[unit * k:unit * (k + 1)].hex()}", pytrace=False)


_OPS = []


def prover_ops() -> OracleProverOps:
    if not _OPS:
        _OPS.append(OracleProverOps())
    return _OPS[0]


_FOLDS = {}


def fold_columns(n: int, kind: str, root_name: str, world: int) -> list:
    """OracleProverOps.fold of every rank of `world` on the layer C.fold_layer(n, kind) with the named root of
    C.fold_roots(n): one column of n / 4 / world rows per rank (computed once per case)."""
    key = (n, kind, root_name, world)
    if key not in _FOLDS:
        layer, root = C.fold_layer(n, kind), dict(C.fold_roots(n))[root_name]
        w = C.w_of(n.bit_length() - 1)
        _FOLDS[key] = [prover_ops().fold(C.rank_values(layer, world, r), n, w, _u8(root), world, r)
                       for r in range(world)]
    return _FOLDS[key]


def fold_by_ranks(n: int, kind: str, root_name: str, world: int) -> bytes:
    """The ranks' columns back in natural row order (row r + world j)."""
    q = n // 4
    rows = [None] * q
    for r, col in enumerate(fold_columns(n, kind, root_name, world)):
        assert len(col) == 32 * (q // world)
        for j in range(q // world):
            rows[r + world * j] = col[32 * j:32 * (j + 1)]
    return b"".join(rows)


# ---- fold -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", C.FOLD_ROOT_NAMES)
@pytest.mark.parametrize("kind", C.FOLD_KINDS)
@pytest.mark.parametrize("n,world", C.FOLD_SIZES)
def test_fold_restatement_is_the_layer_interpolation(oracle, n, world, kind, name):
    """Rows x_i zeta^t interpolated by the oracle's multi_interp_4 and evaluated at special_x =
    from_bytes_le(root) mod p, as fri.rs:135-164 does over the whole layer; the world = 1 fold; and, for the
    cubic's own values, the cubic at special_x on every row."""
    w = C.w_of(n.bit_length() - 1)
    q = n // 4
    layer = C.fold_layer(n, kind)
    xs = O.to_limbs([pow(w, i + t * q, P) for i in range(q) for t in range(4)])
    ys = O.to_limbs([layer[i + t * q] for i in range(q) for t in range(4)])
    polys = oracle.multi_interp_4(xs, ys)
    sx = O.from_bytes_le(dict(C.fold_roots(n))[name])
    want = oracle.eval_quartic_multi(polys, O.to_limbs([sx] * q))
    got = fold_by_ranks(n, kind, name, world)
    same(got, want, f"fold n={n} world={world} {kind} root={name} vs multi_interp_4")
    if world > 1:
        same(got, fold_by_ranks(n, kind, name, 1), f"fold n={n} world={world} {kind} root={name} vs world 1")
    if kind == "cubic":
        same(got, C.le32([C.cubic_at(sx)] * q), f"fold n={n} world={world} root={name} vs the cubic")
    if name == "node" and kind == "random":   # special_x = w^3: row 3 mod q, point t = 3 div q
        assert got[32 * (3 % q):32 * (3 % q + 1)] == layer[3].to_bytes(32, "little")


def test_fold_roots_reduce_as_named():
    r = dict(C.fold_roots(32))
    assert tuple(r) == C.FOLD_ROOT_NAMES and all(len(b) == 32 for b in r.values())
    assert O.from_bytes_le(r["zero"]) == 0 and O.from_bytes_le(r["p"]) == 0
    assert O.from_bytes_le(r["p-1"]) == P - 1 and O.from_bytes_le(r["p+1"]) == 1
    assert (2**256 - 1) // P == 5 and O.from_bytes_le(r["ones"]) == 2**256 - 1 - 5 * P
    assert O.from_bytes_le(r["node"]) == pow(C.w_of(5), 3, P)


def test_fold_sizes_reach_one_row_per_rank():
    assert {(4, 1), (8, 2), (32, 8)} <= {(n, g) for n, g in C.FOLD_SIZES if n // 4 // g == 1}
    assert len(C.FOLD_SIZES) == 13


# ---- _PyTree ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("leaf_len", C.LEAF_LENS)
@pytest.mark.parametrize("n", [1, 2, 8, 1024])
def test_pytree_of_leaf_digests_is_the_oracle_tree(oracle, n, leaf_len):
    leaves = C.random_bytes(n * leaf_len, n + leaf_len)
    dig = prover_ops().leaf_digests(leaves, n, leaf_len)
    assert bytes(dig.numpy()) == b"".join(oracle.blake2s(leaves[leaf_len * i:leaf_len * (i + 1)]) for i in range(n))
    t = _PyTree()
    t.build(dig, n, 1)
    idx = C.tree_indices(n)
    root, paths = oracle.merkle(leaves, n, leaf_len, idx)
    assert bytes(t.root_tensor().numpy()) == root
    assert t.open(idx) == paths


@pytest.mark.parametrize("n,g", C.DIGEST_TREES)
def test_pytree_interleave_is_the_tree_of_the_deinterleaved_digests(n, g):
    chunks = C.random_bytes(32 * n, 100 + n + g)
    a, b = _PyTree(), _PyTree()
    a.build(_u8(chunks), n, g)
    natural = C.deinterleave(chunks, n, g)
    for r in range(g):   # the permutation, by its definition: leaf g m + r = chunk r's digest m
        for m in (0, n // g - 1):
            assert natural[32 * (g * m + r):32 * (g * m + r + 1)] == chunks[32 * (r * (n // g) + m):][:32]
    b.build(_u8(natural), n, 1)
    idx = C.tree_indices(n)
    same(b"".join(a.levels[0]), natural, f"leaf order of n={n} interleave={g}")
    assert bytes(a.root_tensor().numpy()) == bytes(b.root_tensor().numpy())
    for k, (pa, pb) in enumerate(zip(a.open(idx), b.open(idx))):
        same(b"".join(pa), b"".join(pb), f"path of index {idx[k]}, n={n} interleave={g}")


@pytest.mark.parametrize("g", C.TOP_G)
def test_merkle_top_restatement_is_the_oracle_tree_over_the_roots(oracle, g):
    """The g - 1 digests above g subtree roots: level by level the parents of a tree whose leaf digests are the
    roots; its last 32 bytes are that tree's root."""
    roots = C.random_bytes(32 * g, 200 + g)
    top = bytes(prover_ops().merkle_top(_u8(roots), g).numpy())
    assert len(top) == 32 * (g - 1)
    t = _PyTree()
    t.build(_u8(roots), g, 1)
    assert top == b"".join(b"".join(lv) for lv in t.levels[1:])


# ---- strided transforms -----------------------------------------------------------------------------------

def dft_columns(x: np.ndarray, log_g: int, stride: int, inverse: bool, pre=None) -> np.ndarray:
    """out[k][i] = sum_j x[j][i] w^(j k) (inverse: w^-1, times G^-1), after x[j][i] *= pre(j, i) when given."""
    G = 1 << log_g
    w = C.w_of(log_g)
    if inverse:
        w = pow(w, P - 2, P)
    wp = [pow(w, e, P) for e in range(G)]
    scale = pow(G, P - 2, P) if inverse else 1
    v = C.ints(x)
    out = [0] * (G * stride)
    for i in range(stride):
        col = [v[j * stride + i] * (pre(j, i) if pre else 1) % P for j in range(G)]
        for k in range(G):
            out[k * stride + i] = sum(col[j] * wp[j * k % G] for j in range(G)) * scale % P
    return O.to_limbs(out)


def strided_inputs(log_g: int, stride: int, inverse: bool) -> list:
    G = 1 << log_g
    ins = [(kind, C.VALUES(G * stride, kind, seed=log_g)) for kind in C.STRIDED_KINDS]
    return ins + [(f"tone{m}", C.tone(log_g, stride, m, inverse)) for m in C.tone_bins(log_g)]


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("log_g", C.STRIDED_LOG_G)
def test_ntt_strided_restatement_is_the_dft_sum(log_g, inverse):
    ops = OracleOps()
    for stride in C.STRIDES:
        for name, x in strided_inputs(log_g, stride, inverse):
            t = torch.from_numpy(x.copy().view(np.int64))
            ops.ntt_strided(t, log_g, stride, C.w_of(log_g), inverse)
            same(t.numpy(), dft_columns(x, log_g, stride, inverse), f"ntt_strided G=2^{log_g} stride={stride} {name}")
            if name.startswith("tone"):
                same(t.numpy(), C.tone_transform(log_g, stride, int(name[4:]), inverse), f"tone {name} closed form")


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("log_g", C.STRIDED_LOG_G)
def test_ntt_strided_tw_restatement_is_the_twiddled_dft_sum(log_g, inverse):
    ops = OracleOps()
    for log_order, base in C.strided_tw(log_g):
        tr = C.w_of(log_order)
        mask = (1 << log_order) - 1
        pre = lambda j, i: pow(tr, (j * (base + i)) & mask, P)  # noqa: E731
        for stride in C.STRIDES:
            x = C.VALUES((1 << log_g) * stride, "random", seed=log_g + log_order)
            t = torch.from_numpy(x.copy().view(np.int64))
            ops.ntt_strided_tw(t, log_g, stride, C.w_of(log_g), inverse, tr, log_order, base)
            same(t.numpy(), dft_columns(x, log_g, stride, inverse, pre),
                 f"ntt_strided_tw G=2^{log_g} stride={stride} order=2^{log_order} base={base}")


def test_strided_tw_bases_wrap_the_mask_inside_the_stride():
    wraps = [(lo, b) for lo, b in C.strided_tw(4) if (b & ((1 << lo) - 1)) + max(C.STRIDES) > (1 << lo)]
    assert (13, 2**13 - 100) in wraps


# ---- twiddle, transpose -----------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", C.TWIDDLE_KINDS)
@pytest.mark.parametrize("rows,cols,row_base,col_base,log_order", C.TWIDDLE)
def test_twiddle2d_restatement(rows, cols, row_base, col_base, log_order, kind):
    x = C.VALUES(rows * cols, kind, seed=log_order)
    t = torch.from_numpy(x.copy().view(np.int64))
    root = C.w_of(log_order)
    OracleOps().twiddle2d(t, rows, cols, row_base, col_base, root, log_order)
    want = [v * pow(root, ((row_base + k // cols) * (col_base + k % cols)) % (1 << log_order), P) % P
            for k, v in enumerate(C.ints(x))]
    same(t.numpy(), O.to_limbs(want), f"twiddle2d {rows}x{cols} bases {row_base},{col_base} order 2^{log_order}")


@pytest.mark.parametrize("rows,cols,batch", C.TRANSPOSE)
def test_transpose_restatement(rows, cols, batch):
    ops = OracleOps()
    for m in range(batch):
        x = C.named(m, rows * cols)
        src = torch.from_numpy(x.copy().view(np.int64))
        dst = torch.zeros_like(src)
        ops.transpose(src, dst, rows, cols)
        same(dst.numpy(), x.reshape(rows, cols, 4).transpose(1, 0, 2), f"transpose {rows}x{cols} matrix {m}")
    assert len({bytes(r) for r in np.concatenate([C.named(m, rows * cols) for m in range(batch)])}) == \
        batch * rows * cols   # every element of every matrix names itself


# ---- values ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 7, 4096])
def test_values(n):
    assert C.ints(C.VALUES(n, "zero")) == [0] * n
    assert C.ints(C.VALUES(n, "pm1")) == [P - 1] * n
    r, e = C.ints(C.VALUES(n, "random")), C.ints(C.VALUES(n, "edge"))
    assert all(v < P for v in r) and e[-1] == P - 1
    if n > 2:
        assert (e[0], e[n // 2]) == (0, 1) and e[1:n // 2] == r[1:n // 2]
