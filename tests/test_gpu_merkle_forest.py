"""GPU parity: the Merkle forest (batch equal-shaped trees by one set of launches) against the oracle's tree,
called once per member tree; tiny trees against hashlib."""
import hashlib

import numpy as np
import pytest

import stark_amd as S

pytestmark = pytest.mark.gpu


def _blake(b: bytes) -> bytes:
    return hashlib.blake2s(b).digest()


def _py_root(leaves: list) -> bytes:
    lv = [_blake(x) for x in leaves]
    while len(lv) > 1:
        lv = [_blake(lv[i] + lv[i + 1]) for i in range(0, len(lv), 2)]
    return lv[0]


def _blob(n, leaf_len, batch, seed):
    return np.random.default_rng(seed).integers(0, 256, n * leaf_len * batch, dtype=np.uint8).tobytes()


def _indices(n, rng):
    return sorted(set(rng.integers(0, n, 6).tolist())) + [0, n - 1, 0, n - 1]


def _check_forest(f, oracle, blob, n, leaf_len, batch, seed, tag):
    """Every root, and the paths of the first, a middle and the last tree, against the oracle's tree of that
    member's leaves."""
    rng = np.random.default_rng(seed)
    roots = f.roots()
    assert len(roots) == batch
    tree_bytes = n * leaf_len
    for b in range(batch):
        mine = blob[b * tree_bytes:(b + 1) * tree_bytes]
        opened = b in (0, batch // 2, batch - 1)
        idx = _indices(n, rng) if opened else []
        root, paths = oracle.merkle(mine, n, leaf_len, idx, chunks=4)
        assert roots[b] == root, (tag, "root of tree", b)
        if opened:
            proofs = f.gen_proofs(b, idx)
            assert [p.nodes for p in proofs] == paths, (tag, "paths of tree", b)
            assert [p.leaf for p in proofs] == [mine[i * leaf_len:(i + 1) * leaf_len] for i in idx], (tag, b)
            S.verify_multi_branch(root, idx, proofs)


# Every boundary of the build: n = 1 (no pair level), 2 .. 8 (many trees per workgroup), 128 (a partly filled
# last workgroup), 256 / 512 (kTailBlock: one tree per workgroup from a first pair level of 256 nodes), 1024 .. 4096
# (kMerkleBlock; a tail launch of several workgroups per tree, then the packed one), 2^16 / 2^17 (kTailFrom: the
# leaf level takes the wide kernel with its two LDS levels), 2^19 (a wide pair level).
CASES = [(1, 32, 3), (2, 4, 5), (4, 33, 17), (8, 40, 2), (128, 32, 5), (256, 32, 17), (512, 32, 3), (512, 256, 2),
         (1024, 32, 5), (2048, 4, 2), (4096, 33, 3), (1 << 16, 32, 2), (1 << 17, 32, 3), (1 << 17, 40, 1),
         (1 << 19, 32, 1)]


@pytest.mark.parametrize("n,leaf_len,batch", CASES)
def test_forest_vs_oracle(ctx, oracle, n, leaf_len, batch):
    assert n * leaf_len * batch <= 32 << 20
    blob = _blob(n, leaf_len, batch, n * 131 + leaf_len * 7 + batch)
    f = S.MerkleForest(ctx)
    f.update_bytes(blob, n, leaf_len, batch)
    _check_forest(f, oracle, blob, n, leaf_len, batch, n + batch, (n, leaf_len, batch))


@pytest.mark.parametrize("n,batch", [(1, 2), (2, 3), (4, 5), (8, 17)])
def test_forest_tiny_vs_hashlib(ctx, n, batch):
    leaf_len = 33
    blob = _blob(n, leaf_len, batch, 900 + n)
    f = S.MerkleForest(ctx)
    f.update_bytes(blob, n, leaf_len, batch)
    want = [_py_root([blob[(b * n + i) * leaf_len:(b * n + i + 1) * leaf_len] for i in range(n)])
            for b in range(batch)]
    assert f.roots() == want


def test_forest_no_indices(ctx):
    f = S.MerkleForest(ctx)
    f.update_bytes(_blob(64, 32, 3, 5), 64, 32, 3)
    assert f.gen_proofs(1, []) == []


def test_forest_update_dev_unaligned(ctx, oracle):
    """32-byte leaves 8 bytes off a 16-byte boundary: the general leaf hash, not the 32-byte fast path; and the
    same leaves aligned."""
    n, batch = 1024, 3
    blob = _blob(n, 32, batch, 77)
    d = ctx.alloc(len(blob) + 16)
    try:
        f = S.MerkleForest(ctx)
        for off in (8, 0):
            ctx.h2d(d + off, np.frombuffer(blob, dtype=np.uint8))
            f.update_dev(d + off, n, 32, batch)
            _check_forest(f, oracle, blob, n, 32, batch, 3, ("dev", off))
    finally:
        ctx.free(d)


def test_forest_rebuilt_growing_and_shrinking(ctx, oracle):
    """One forest object over growing and shrinking (n, batch), three rounds: its node and leaf buffers are
    reallocated and reused; every root each time."""
    f = S.MerkleForest(ctx)
    shapes = [(512, 3), (1 << 14, 5), (64, 17), (4096, 2), (8, 1), (2048, 9)]
    for rnd in range(3):
        for n, batch in shapes:
            blob = _blob(n, 32, batch, 1000 * rnd + n + batch)
            f.update_bytes(blob, n, 32, batch)
            roots = f.roots()
            for b in range(batch):
                root, _ = oracle.merkle(blob[b * n * 32:(b + 1) * n * 32], n, 32, [], chunks=4)
                assert roots[b] == root, (rnd, n, batch, b)


def test_forest_errors(ctx):
    f = S.MerkleForest(ctx)
    f.batch = 1  # (the Python object sizes the roots' buffer from its last update)
    with pytest.raises(S.StarkError) as e:
        f.roots()  # before an update
    assert e.value.code == 7
    with pytest.raises(S.StarkError) as e:
        f.gen_proofs(0, [0])
    assert e.value.code == 7
    with pytest.raises(S.StarkError) as e:
        f.update_bytes(b"\0" * 192, 3, 32, 2)  # n not a power of two
    assert e.value.code == 1
    with pytest.raises(S.StarkError) as e:
        f.update_bytes(b"", 4, 32, 0)
    assert e.value.code == 3
    with pytest.raises(S.StarkError) as e:
        f.update_bytes(b"\0" * 65536, 1, 1, 65536)
    assert e.value.code == 3
    f.update_bytes(b"\0" * 256, 4, 32, 2)
    with pytest.raises(S.StarkError) as e:
        f.gen_proofs(0, [4])  # index >= n
    assert e.value.code == 3
    with pytest.raises(S.StarkError) as e:
        f.gen_proofs(2, [0])  # tree >= batch
    assert e.value.code == 3
