"""GPU: every per-rank op of the multi-GPU provers against its host restatement, op by op, in one process.

tests/test_gpu_dprove.py and tests/test_gpu_distributed.py run these kernels under 2-8 gloo processes at the
golden circuits' shapes and compare one digest at the end.  Here each entry point of csrc/dist.hip, the
residue-class fold of csrc/fri.hip and the leaf-digest / interleave / top / multi-gather kernels of
csrc/merkle.hip runs alone on the directed tables of tests/rank_cases.py and is compared, bit for bit, with
OracleProverOps / _PyTree / OracleOps (held to independent definitions on the same tables by
tests/test_rank_cases_cpu.py) or with a closed form.  Every device output sits between two 32-byte guards of
0xFF in a buffer of 0xFF, so a store outside the region the op may write, or a missing one inside it, shows;
a mismatch is reported by its first differing element."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import oracle as O
import rank_cases as C
import stark_amd as S
from stark_amd import _limbs, _p64
from stark_amd.distributed import GpuOps
from stark_amd.dprove import GpuProverOps, _OpenReq
from test_distributed_cpu import OracleOps
from test_dprove_cpu import _PyTree, _u8
from test_gpu_distributed import _local_step_want
from test_rank_cases_cpu import fold_columns, prover_ops, same, strided_inputs

pytestmark = pytest.mark.gpu

P = O.P
OK, BAD_LENGTH, BAD_ROOT, BAD_ARG, STATE = 0, 1, 2, 3, 7   # stark_status (include/stark_hip.h)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "r1cs")
FF = b"\xff" * 32


class Guarded:
    """nbytes of device memory between two 32-byte guards, everything 0xFF until `put`."""

    def __init__(self, nbytes: int, data=None):
        self.nbytes = nbytes
        self.t = torch.full((nbytes + 64,), 0xFF, dtype=torch.uint8, device="cuda")
        self.ptr = self.t.data_ptr() + 32
        if data is not None:
            self.put(data)

    @property
    def view(self) -> torch.Tensor:
        """The region as a tensor (data_ptr() = ptr), for the ops that take tensors."""
        return self.t[32:32 + self.nbytes]

    def put(self, data) -> None:
        raw = data if isinstance(data, bytes) else np.ascontiguousarray(data).tobytes()
        assert len(raw) == self.nbytes
        if raw:
            self.view.copy_(torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()))

    def get(self, what="") -> bytes:
        """The region's bytes once the device is idle; both guards must be untouched."""
        torch.cuda.synchronize()
        raw = self.t.cpu().numpy().tobytes()
        assert raw[:32] == FF, f"{what}: the 32 bytes before the output were written: {raw[:32].hex()}"
        assert raw[-32:] == FF, f"{what}: the 32 bytes after the output were written: {raw[-32:].hex()}"
        return raw[32:-32]


def dev(data) -> torch.Tensor:
    raw = data if isinstance(data, bytes) else np.ascontiguousarray(data).tobytes()
    return torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).cuda()


def stream() -> int:
    return S.torch_stream()


# ---- stark_transpose_dev -----------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,cols,batch", C.TRANSPOSE)
def test_transpose(ctx, rows, cols, batch):
    x = np.concatenate([C.named(m, rows * cols) for m in range(batch)])
    src, dst = Guarded(x.nbytes, x), Guarded(x.nbytes)
    if batch == 1:
        GpuOps(ctx).transpose(src.view, dst.view, rows, cols)
    else:
        ctx.transpose_dev(src.ptr, dst.ptr, rows, cols, batch, stream=stream())
    got = dst.get("transpose")
    assert src.get("transpose source") == x.tobytes()
    for m in range(batch):
        want = x.reshape(batch, rows, cols, 4)[m].transpose(1, 0, 2)
        same(got[m * want.nbytes:(m + 1) * want.nbytes], want, f"transpose {rows}x{cols} matrix {m} of {batch}")


def test_transpose_statuses(ctx):
    x = C.named(0, 25)
    src, dst = Guarded(x.nbytes, x), Guarded(x.nbytes)
    for rows, cols, batch in C.TRANSPOSE_EMPTY:
        assert ctx.lib.stark_transpose_dev(ctx.h, src.ptr, dst.ptr, rows, cols, batch, stream()) == OK
    assert dst.get("empty transpose") == b"\xff" * x.nbytes
    assert ctx.lib.stark_transpose_dev(ctx.h, src.ptr, src.ptr, 5, 5, 1, stream()) == BAD_ARG
    assert src.get("transpose onto itself") == x.tobytes()


# ---- stark_twiddle2d_dev -----------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", C.TWIDDLE_KINDS)
@pytest.mark.parametrize("rows,cols,row_base,col_base,log_order", C.TWIDDLE)
def test_twiddle2d(ctx, rows, cols, row_base, col_base, log_order, kind):
    x = C.VALUES(rows * cols, kind, seed=log_order)
    buf = Guarded(x.nbytes, x)
    root = C.w_of(log_order)
    GpuOps(ctx).twiddle2d(buf.view, rows, cols, row_base, col_base, root, log_order)
    want = [v * pow(root, ((row_base + k // cols) * (col_base + k % cols)) % (1 << log_order), P) % P
            for k, v in enumerate(C.ints(x))]
    same(buf.get("twiddle2d"), O.to_limbs(want),
         f"twiddle2d {rows}x{cols} bases {row_base},{col_base} order 2^{log_order} {kind}")


# ---- stark_ntt_strided_dev / stark_ntt_strided_tw_dev --------------------------------------------------------

def _host(x: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(x.copy().view(np.int64))


@pytest.mark.parametrize("stride", C.STRIDES)
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("log_g", C.STRIDED_LOG_G)
def test_ntt_strided(ctx, log_g, inverse, stride):
    ops, ref = GpuOps(ctx), OracleOps()
    w = C.w_of(log_g)
    for name, x in strided_inputs(log_g, stride, inverse):
        buf = Guarded(x.nbytes, x)
        ops.ntt_strided(buf.view, log_g, stride, w, inverse)
        want = _host(x)
        ref.ntt_strided(want, log_g, stride, w, inverse)
        got = buf.get("ntt_strided")
        same(got, want.numpy(), f"ntt_strided G=2^{log_g} stride={stride} inverse={inverse} {name}")
        if name.startswith("tone"):
            same(got, C.tone_transform(log_g, stride, int(name[4:]), inverse), f"ntt_strided {name} closed form")


@pytest.mark.parametrize("tw_case", [0, 1, 2])
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("log_g", C.STRIDED_LOG_G)
def test_ntt_strided_tw(ctx, log_g, inverse, tw_case):
    """The input twiddle t^(j (base + i) mod 2^log_order) before the transform; the tones are divided by it
    first, so the butterflies still meet them and the closed form still holds."""
    ops, ref = GpuOps(ctx), OracleOps()
    w = C.w_of(log_g)
    G = 1 << log_g
    log_order, base = C.strided_tw(log_g)[tw_case]
    tr = C.w_of(log_order)
    mask = (1 << log_order) - 1
    for stride in C.STRIDES:
        for name, x in strided_inputs(log_g, stride, inverse):
            if name.startswith("tone"):
                un = [pow(tr, (1 << log_order) - ((j * (base + i)) & mask), P) for j in range(G) for i in range(stride)]
                x = O.to_limbs([v * u % P for v, u in zip(C.ints(x), un)])
            buf = Guarded(x.nbytes, x)
            ops.ntt_strided_tw(buf.view, log_g, stride, w, inverse, tr, log_order, base)
            want = _host(x)
            ref.ntt_strided_tw(want, log_g, stride, w, inverse, tr, log_order, base)
            got = buf.get("ntt_strided_tw")
            what = (f"ntt_strided_tw G=2^{log_g} stride={stride} inverse={inverse} order=2^{log_order} "
                    f"base={base} {name}")
            same(got, want.numpy(), what)
            if name.startswith("tone"):
                same(got, C.tone_transform(log_g, stride, int(name[4:]), inverse), what + " closed form")


def test_ntt_strided_statuses(ctx):
    x = C.VALUES(32 * 5, "random")
    buf = Guarded(x.nbytes, x)
    lib, st = ctx.lib, stream()
    one = _limbs(1)
    assert lib.stark_ntt_strided_dev(ctx.h, buf.ptr, 0, 160, _p64(one), 0, st) == OK          # G = 1: the identity
    assert lib.stark_ntt_strided_tw_dev(ctx.h, buf.ptr, 0, 160, _p64(one), 0, _p64(one), 0, 7, st) == OK
    w5, w2, w3 = _limbs(C.w_of(5)), _limbs(C.w_of(2)), _limbs(C.w_of(3))
    assert lib.stark_ntt_strided_dev(ctx.h, buf.ptr, 5, 5, _p64(w5), 0, st) == BAD_LENGTH
    assert lib.stark_ntt_strided_dev(ctx.h, buf.ptr, 3, 20, _p64(w2), 0, st) == BAD_ROOT       # a root of order G / 2
    assert lib.stark_ntt_strided_dev(ctx.h, buf.ptr, 3, 20, _p64(w2), 1, st) == BAD_ROOT
    assert lib.stark_ntt_strided_tw_dev(ctx.h, buf.ptr, 3, 20, _p64(w3), 0, None, 13, 0, st) == BAD_ARG
    same(buf.get("strided statuses"), x, "data after calls that must not touch it")


# ---- stark_cyclic_ntt_local_dev ----------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["random", "edge", "pm1"])
@pytest.mark.parametrize("log_n,log_g,rank", C.CYCLIC_LOCAL)
def test_cyclic_ntt_local_argument_edges(ctx, oracle, log_n, log_g, rank, kind):
    """The smallest shard (M = 4), G = 1, M = G^2, the first and the last rank; rank 0's twiddle is all ones."""
    x = C.VALUES(1 << (log_n - log_g), kind, seed=log_n + rank)
    buf = Guarded(x.nbytes, x)
    GpuOps(ctx).cyclic_local(buf.view, log_n, log_g, rank, C.w_of(log_n), False)
    want = _local_step_want(oracle, x, log_n, log_g, rank)
    if rank == 0:
        assert want == O.from_limbs(oracle.best_fft(x, pow(C.w_of(log_n), 1 << log_g, P), log_n - log_g, cpus=1))
    same(buf.get("cyclic_ntt_local"), O.to_limbs(want), f"cyclic_ntt_local 2^{log_n} G=2^{log_g} rank {rank} {kind}")


def test_cyclic_ntt_local_statuses(ctx):
    x = C.VALUES(256, "random")
    buf = Guarded(x.nbytes, x)
    call = lambda log_n, log_g, rank, root: ctx.lib.stark_cyclic_ntt_local_dev(  # noqa: E731
        ctx.h, buf.ptr, log_n, log_g, rank, _p64(_limbs(root)), 0, stream())
    for log_n, log_g, rank in C.CYCLIC_LOCAL_BAD_LENGTH:
        assert call(log_n, log_g, rank, C.w_of(log_n)) == BAD_LENGTH, (log_n, log_g, rank)
    assert call(8, 2, 1, C.w_of(7)) == BAD_ROOT   # order n / 2: w^(n/2) = 1
    assert call(8, 2, 1, C.w_of(9)) == BAD_ROOT   # order 2 n: w^(n/2) = a fourth root
    same(buf.get("cyclic statuses"), x, "data after calls that must not touch it")


# ---- stark_fri_fold_dev / stark_fri_fold_dev_root ----------------------------------------------------------

def _fold(ctx, vals: torch.Tensor, out: Guarded, n, root: bytes, d_root, world, rank) -> int:
    rl = _limbs(C.w_of(n.bit_length() - 1))
    if d_root is None:
        return ctx.lib.stark_fri_fold_dev(ctx.h, vals.data_ptr(), out.ptr, n, _p64(rl), root, world, rank, stream())
    return ctx.lib.stark_fri_fold_dev_root(ctx.h, vals.data_ptr(), out.ptr, n, _p64(rl), d_root.data_ptr(), world, rank,
                                           stream())


@pytest.mark.parametrize("kind", C.FOLD_KINDS)
@pytest.mark.parametrize("n,world", C.FOLD_SIZES)
def test_fri_fold_every_rank(ctx, n, world, kind):
    """Both entry points, every rank, every root of the table, against OracleProverOps.fold on the rank's own
    values; the ranks' columns in residue order are the world = 1 column; the cubic's fold is the cubic."""
    layer = C.fold_layer(n, kind)
    q = n // 4
    ql = q // world
    vals = [dev(C.rank_values(layer, world, r)) for r in range(world)]
    whole = dev(C.le32(layer)) if world > 1 else None
    for name, root in C.fold_roots(n):
        d_root = dev(root)
        want = fold_columns(n, kind, name, world)
        natural = [None] * q
        for r in range(world):
            for entry, dr in (("fold_dev", None), ("fold_dev_root", d_root)):
                out = Guarded(32 * ql)
                assert _fold(ctx, vals[r], out, n, root, dr, world, r) == OK
                got = out.get(entry)
                same(got, want[r], f"{entry} n={n} world={world} rank={r} {kind} root={name}")
            for j in range(ql):
                natural[r + world * j] = got[32 * j:32 * (j + 1)]
        if world > 1:
            out = Guarded(32 * q)
            assert _fold(ctx, whole, out, n, root, d_root, 1, 0) == OK
            same(b"".join(natural), out.get("world 1"), f"ranks' columns vs world 1, n={n} world={world} {kind} {name}")
        if kind == "cubic":
            same(b"".join(natural), C.le32([C.cubic_at(O.from_bytes_le(root))] * q), f"cubic n={n} root={name}")
        elif kind == "random" and name == "node":
            assert natural[3 % q] == layer[3].to_bytes(32, "little")   # special_x = w^3: that point's own value


def test_fri_fold_statuses(ctx):
    vals = dev(C.le32(C.fold_layer(32, "random")))
    d_root = dev(bytes(range(32)))
    out = Guarded(32 * 8)
    for n, world, rank in C.FOLD_BAD_ARG:
        for dr in (None, d_root):
            assert _fold(ctx, vals, out, n, bytes(range(32)), dr, world, rank) == BAD_ARG, (n, world, rank)
    for n, world, rank in C.FOLD_BAD_LENGTH:
        for dr in (None, d_root):
            assert _fold(ctx, vals, out, n, bytes(range(32)), dr, world, rank) == BAD_LENGTH, (n, world, rank)
    assert out.get("fold statuses") == b"\xff" * 256


# ---- leaf digests, digest trees, top -------------------------------------------------------------------------

def _root_dev(ctx, tree) -> bytes:
    out = Guarded(32)
    assert ctx.lib.stark_merkle_root_dev(tree.h, out.ptr, stream()) == OK
    return out.get("merkle_root_dev")


def _tree_is(ctx, tree, n, want_root, want_paths, want_leaves, what):
    """root_dev, then gen_proofs (on the context's own stream: the device is idle by then) and get_root."""
    idx = C.tree_indices(n)
    assert _root_dev(ctx, tree) == want_root, f"{what}: root_dev"
    proofs = tree.gen_proofs(idx)
    assert tree.get_root() == want_root, f"{what}: get_root"
    assert tree.width() == n
    for k, (p, i) in enumerate(zip(proofs, idx)):
        assert p.leaf == want_leaves(i), f"{what}: leaf of proof {k} (index {i})"
        same(b"".join(p.nodes), b"".join(want_paths[k]), f"{what}: path of proof {k} (index {i})")


@pytest.mark.parametrize("n,g", C.DIGEST_TREES)
def test_digest_tree(ctx, n, g):
    chunks = C.random_bytes(32 * n, 100 + n + g)
    natural = C.deinterleave(chunks, n, g)
    ref = _PyTree()
    ref.build(_u8(chunks), n, g)
    tree = GpuProverOps(ctx).new_tree()
    tree.build(dev(chunks), n, g)
    want_root = bytes(ref.root_tensor().numpy())
    assert bytes(tree.root_tensor().cpu().numpy()) == want_root
    _tree_is(ctx, tree.t, n, want_root, ref.open(C.tree_indices(n)), lambda i: natural[32 * i:32 * (i + 1)],
             f"digest tree n={n} interleave={g}")


@pytest.mark.parametrize("leaf_len", C.LEAF_LENS)
def test_leaf_digests_then_digest_tree_is_the_tree_of_the_leaves(ctx, oracle, leaf_len):
    for n in (2, 512):
        leaves = C.random_bytes(n * leaf_len, n + leaf_len)
        d_leaves = dev(leaves)
        dig = Guarded(32 * n)
        assert ctx.lib.stark_merkle_leaf_digests_dev(ctx.h, d_leaves.data_ptr(), n, leaf_len, dig.ptr, stream()) == OK
        got = dig.get("leaf_digests")
        same(got, bytes(prover_ops().leaf_digests(leaves, n, leaf_len).numpy()), f"leaf digests n={n} len={leaf_len}")
        a, b = S.MerkleProofInPlace(ctx), S.MerkleProofInPlace(ctx)
        a.update_digests_dev(dig.ptr, n, 1, stream=stream())
        b.update_dev(d_leaves.data_ptr(), n, leaf_len, stream=stream())
        idx = C.tree_indices(n)
        root, paths = oracle.merkle(leaves, n, leaf_len, idx)
        _tree_is(ctx, a, n, root, paths, lambda i: got[32 * i:32 * (i + 1)], f"tree of digests len={leaf_len}")
        _tree_is(ctx, b, n, root, paths, lambda i: leaves[leaf_len * i:leaf_len * (i + 1)], f"tree len={leaf_len}")


def test_one_tree_rebuilt_four_ways(ctx, oracle):
    """update_bytes(256-byte leaves), update_digests_dev(fewer), update_bytes(40-byte leaves),
    update_digests_dev(more, interleave 4) on one tree: every root, path and leaf is the current build's, so
    no leaf pointer, leaf length, plane stride or depth of the build before it survives."""
    tree = S.MerkleProofInPlace(ctx)
    keep = []
    for step, (n, leaf_len, g) in enumerate([(64, 256, 0), (16, 32, 1), (32, 40, 0), (256, 32, 4)]):
        blob = C.random_bytes(n * leaf_len, 300 + step)
        if g == 0:
            tree.update_bytes(blob, n, leaf_len)
            root, paths = oracle.merkle(blob, n, leaf_len, C.tree_indices(n))
            leaf = lambda i, blob=blob, ll=leaf_len: blob[ll * i:ll * (i + 1)]  # noqa: E731
        else:
            keep.append(dev(blob))
            tree.update_digests_dev(keep[-1].data_ptr(), n, g, stream=stream())
            ref = _PyTree()
            ref.build(_u8(blob), n, g)
            root, paths = bytes(ref.root_tensor().numpy()), ref.open(C.tree_indices(n))
            leaf = lambda i, nat=C.deinterleave(blob, n, g): nat[32 * i:32 * (i + 1)]  # noqa: E731
        _tree_is(ctx, tree, n, root, paths, leaf, f"rebuild {step}: n={n} leaf_len={leaf_len} interleave={g}")


@pytest.mark.parametrize("g", C.TOP_G)
def test_merkle_top(ctx, g):
    roots = C.random_bytes(32 * g, 200 + g)
    d_roots = dev(roots)
    levels = Guarded(32 * (g - 1))
    assert ctx.lib.stark_merkle_top_dev(ctx.h, d_roots.data_ptr(), g, levels.ptr, stream()) == OK
    same(levels.get("merkle_top"), bytes(prover_ops().merkle_top(_u8(roots), g).numpy()), f"merkle_top g={g}")
    if g > 1:
        assert bytes(GpuProverOps(ctx).merkle_top(d_roots, g).cpu().numpy()) == levels.get("merkle_top")


def test_digest_tree_and_top_statuses(ctx):
    tree = S.MerkleProofInPlace(ctx)
    out = Guarded(32)
    assert ctx.lib.stark_merkle_root_dev(tree.h, out.ptr, stream()) == STATE   # never built
    d = dev(C.random_bytes(32 * 8, 1))
    for n, g in C.DIGESTS_BAD_ARG:
        assert ctx.lib.stark_merkle_update_digests_dev(tree.h, d.data_ptr(), n, g, stream()) == BAD_ARG, (n, g)
    for n, g in C.DIGESTS_BAD_LENGTH:
        assert ctx.lib.stark_merkle_update_digests_dev(tree.h, d.data_ptr(), n, g, stream()) == BAD_LENGTH, (n, g)
    assert ctx.lib.stark_merkle_root_dev(tree.h, out.ptr, stream()) == STATE   # still not
    for g in C.TOP_BAD_LENGTH:
        assert ctx.lib.stark_merkle_top_dev(ctx.h, d.data_ptr(), g, out.ptr, stream()) == BAD_LENGTH, g
    assert out.get("statuses") == FF


# ---- stark_open_batch ----------------------------------------------------------------------------------------

class _Source:
    """A tree or a row buffer that stark_open_batch reads: its request fields and the bytes an opening of idx
    must give -- the tree's own gen_proofs (pinned to the oracle by test_merkle_vs_oracle and the tests above),
    plain slices of the row bytes."""

    def __init__(self, name, n, leaf_len, tree=None, rows: bytes = None):
        self.name, self.n, self.leaf_len, self.tree, self.rows = name, n, leaf_len, tree, rows
        self.depth = n.bit_length() - 1 if tree is not None else 0
        self.d_rows = dev(rows) if rows is not None else None

    def want(self, idx):
        if self.tree is None:
            return b"".join(self.rows[self.leaf_len * i:self.leaf_len * (i + 1)] for i in idx), b""
        ps = self.tree.gen_proofs(idx)
        return b"".join(p.leaf for p in ps), b"".join(b"".join(p.nodes) for p in ps)


class _HostOut:
    """nbytes of host memory for an output of stark_open_batch, between two 32-byte guards of 0xFF."""

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.buf = ctypes.create_string_buffer(b"\xff" * (nbytes + 64), nbytes + 64)
        self.ptr = ctypes.addressof(self.buf) + 32

    def get(self, what) -> bytes:
        raw = self.buf.raw
        assert raw[:32] == FF and raw[32 + self.nbytes:] == FF, f"{what}: written outside its output"
        return raw[32:32 + self.nbytes]


def _open(ctx, plan):
    """plan: (source, idx, leaves wanted, nodes wanted) per request.  Returns (status, [(leaves, nodes)])."""
    reqs = (_OpenReq * max(len(plan), 1))()
    keep, outs = [], []
    for i, (src, idx, want_l, want_n) in enumerate(plan):
        arr = np.ascontiguousarray(idx, dtype=np.uint64)
        lo = _HostOut(len(idx) * src.leaf_len) if want_l else None
        no = _HostOut(len(idx) * src.depth * 32) if want_n else None
        keep.append(arr)
        outs.append((lo, no))
        reqs[i] = _OpenReq(src.tree.h if src.tree is not None else None,
                           src.d_rows.data_ptr() if src.d_rows is not None else None,
                           src.leaf_len if src.tree is None else 0, src.n if src.tree is None else 0,
                           arr.ctypes.data_as(S._szp) if len(idx) else None, len(idx),
                           lo.ptr if lo else None, no.ptr if no else None)
    torch.cuda.synchronize()
    rc = ctx.lib.stark_open_batch(ctx.h, ctypes.cast(reqs, ctypes.c_void_p) if plan else None, len(plan), stream())
    return rc, [(lo.get(f"request {i} leaves") if lo else None, no.get(f"request {i} nodes") if no else None)
                for i, (lo, no) in enumerate(outs)]


@pytest.fixture(scope="module")
def sources(ctx):
    out, keep = [], []
    for n, leaf_len in C.OPEN_TREES:
        t = S.MerkleProofInPlace(ctx)
        keep.append(dev(C.random_bytes(n * leaf_len, 400 + leaf_len)))
        t.update_dev(keep[-1].data_ptr(), n, leaf_len, stream=stream())
        out.append(_Source(f"tree of {leaf_len}-byte leaves", n, leaf_len, tree=t))
    n, g = C.OPEN_DIGEST_TREE
    t = S.MerkleProofInPlace(ctx)
    keep.append(dev(C.random_bytes(32 * n, 450)))
    t.update_digests_dev(keep[-1].data_ptr(), n, g, stream=stream())
    out.append(_Source("digest tree", n, 32, tree=t))
    for rb in C.ROW_BYTES:
        out.append(_Source(f"rows of {rb} bytes", C.OPEN_ROWS, rb, rows=C.random_bytes(C.OPEN_ROWS * rb, 500 + rb)))
    torch.cuda.synchronize()
    yield out
    del keep


def test_open_batch_mixed_requests(ctx, sources):
    """Trees of 32-, 33- (the byte copy path) and 256-byte leaves, a digest tree and row buffers of 32, 256, 7
    and 36 bytes in one call, empty requests in between; then the same call with one output of each request
    NULL, where the other must not change."""
    t32, t33, t256, tdig, r32, r256, r7, r36 = sources
    L = lambda s, which, seed=0: C.index_lists(s.n, seed)[which]  # noqa: E731
    plan = [(t32, L(t32, 0), True, True), (t32, [], False, False), (t33, L(t33, 3, 1), True, True),
            (t256, L(t256, 2), True, True), (r32, [], False, False), (tdig, L(tdig, 1), True, True),
            (r32, L(r32, 3, 2), True, True), (r256, L(r256, 0), True, True), (r7, L(r7, 2), True, True),
            (t33, [], False, False), (r36, L(r36, 1), True, True), (t32, L(t32, 3, 3), True, True),
            (r7, L(r7, 3, 4), True, True), (t256, L(t256, 1), True, True)]
    rc, got = _open(ctx, plan)
    assert rc == OK
    for i, ((src, idx, _, _), (leaves, nodes)) in enumerate(zip(plan, got)):
        if not idx:
            continue
        want_l, want_n = src.want(idx)
        same(leaves, want_l, f"request {i} ({src.name}, {len(idx)} indices): leaves", unit=src.leaf_len)
        same(nodes, want_n, f"request {i} ({src.name}, {len(idx)} indices): nodes")
    half, c = [], 0
    for src, idx, _, _ in plan:
        half.append((src, idx, bool(idx) and c % 2 == 1, bool(idx) and c % 2 == 0))
        c += bool(idx)
    rc, again = _open(ctx, half)
    assert rc == OK
    for i, ((_, _, want_l, want_n), (l1, n1), (l2, n2)) in enumerate(zip(half, got, again)):
        assert (l2 == l1) if want_l else (l2 is None), f"request {i}: leaves with nodes_out NULL"
        assert (n2 == n1) if want_n else (n2 is None), f"request {i}: nodes with leaves_out NULL"


def test_open_batch_seventy_requests(ctx, sources):
    """70 single-index requests over alternating trees and row buffers: past kGatherMaxReq = 64 the requests go
    to a second launch, whose descriptors number their proofs from 0 again."""
    order = [sources[i] for i in (0, 4, 1, 5, 2, 6, 3, 7)]
    plan = [(order[i % 8], [(3 * i + 1) % order[i % 8].n], True, True) for i in range(70)]
    rc, got = _open(ctx, plan)
    assert rc == OK
    for i, ((src, idx, _, _), (leaves, nodes)) in enumerate(zip(plan, got)):
        want_l, want_n = src.want(idx)
        same(leaves, want_l, f"request {i} ({src.name}, index {idx[0]}): leaf", unit=src.leaf_len)
        same(nodes, want_n, f"request {i} ({src.name}, index {idx[0]}): nodes")


def test_open_batch_statuses(ctx, sources):
    t32, r7 = sources[0], sources[6]
    assert _open(ctx, [])[0] == OK   # n_req = 0
    assert _open(ctx, [(t32, [0, t32.n], True, True)])[0] == BAD_ARG
    assert _open(ctx, [(r7, [0], True, True), (r7, [r7.n], True, True)])[0] == BAD_ARG
    unbuilt = _Source("unbuilt", 8, 32, tree=S.MerkleProofInPlace(ctx))
    assert _open(ctx, [(t32, [1], True, True), (unbuilt, [0], True, True)])[0] == STATE
    assert _open(ctx, [(t32, [1], False, False)])[0] == BAD_ARG


# ---- stark_dprove_begin_bytes / _info / _rows / _lincomb_dev ---------------------------------------------------

@pytest.mark.parametrize("name,world,rank", C.RANK_STATE)
def test_rank_state_rows_and_lincomb(ctx, name, world, rank):
    """The rank's sizes, g2 and a_root, its n_local x 256 bytes of constraint rows and, from the golden main
    root in device memory, its n_local x 32 bytes of L, against OracleProverOps (the oracle's rows of that
    residue class; L restated in Python integers)."""
    r1 = open(os.path.join(FIX, f"{name}.r1cs"), "rb").read()
    wt = open(os.path.join(FIX, f"{name}.wtns"), "rb").read()
    m_root = bytes.fromhex(json.load(open(os.path.join(ROOT, "tests", "golden", "r1cs_proofs.json")))[name]["m_root"])
    ref = prover_ops()
    want = ref.begin(r1, wt, world, rank)
    ops = GpuProverOps(ctx)
    h = ops.begin(r1, wt, world, rank)
    try:
        rc, info = ops.info(h)
        assert rc == OK
        assert info == ref.info(want)[1]
        n_local = info[1]
        assert n_local * world == info[0]
        same(ops.to_host(ops.rows(h), 8 * n_local), want["rows"], f"{name} rows of rank {rank} of {world}", unit=256)
        d_root = dev(m_root)
        got_l = ops.to_host(ops.lincomb(h, d_root), n_local)
        same(got_l, ref.lincomb(want, _u8(m_root)), f"{name} L of rank {rank} of {world}")
    finally:
        ops.end(h)
