"""GPU parity of the Blake2s leaf hash (csrc/merkle_dev.h: hash_leaf, hash_leaf32) and of everything that
carries leaves of any byte length (the leaf-digest kernel, the single tree, the forest, both gathers) against
hashlib and a plain Python tree over it (blake_cases.py), at the lengths and alignments of blake_cases.LENS /
OFFSETS: every boundary of hash_leaf's four data paths (vector or byte loads x the full blocks or the last
one), the counter of every block, leaves of no bytes, each build regime with leaves that are not 32 bytes, and
the gather's word and byte paths with k * leaf_len on both sides of a multiple of 16.

Which tests run which path (ids are [leaf_len-offset] for test_leaf_digests):
  vector loads, full blocks    test_leaf_digests[80 96 112 128 144 176 192 256 320 - 0 16],
                               test_tree_build_regimes[n-80 n-144], test_wide_leaf_level_*[80]
  vector loads, last block     partial after a full one: the same at 80 96 112 144 176; alone: [16 48 - 0 16],
                               test_forest_lengths[16 48 80 144]
  byte loads, full blocks      test_leaf_digests[65 .. 1000 - every offset; 80 .. 320 - 1 4 8],
                               test_tree_build_regimes[n-65 n-193], test_gather_edges_*[65 127]
  byte loads, last block       test_leaf_digests[1 .. 63 and every length not a multiple of 16],
                               test_tree_every_length
  hash_leaf32                  test_leaf_digests[32-0 32-16], test_tree_update_dev_offsets[32-0 32-16]
                               (offsets 1 4 8: hash_leaf on the same leaves)
  leaf-digest kernel           test_leaf_digests
  wide leaf kernel             test_wide_leaf_level_tree, test_wide_leaf_level_forest
  gather, word copies          test_forest_lengths[16 48 80 144], test_forest_update_dev_offsets[offset 4]
  gather, byte copies          test_gather_edges_tree (the single tree's gather copies bytes only),
                               test_gather_edges_forest, test_forest_lengths[65 129],
                               test_forest_update_dev_offsets[offset 1]
  leaf_len = 0                 test_tree_of_empty_leaves, test_leaf_digests[0-*], test_tree_every_length[0],
                               test_forest_lengths[n-batch-0]"""
import numpy as np
import pytest

import blake_cases as B
import stark_amd as S

pytestmark = pytest.mark.gpu


class _DevLeaves:
    """blob on the device, its first leaf `offset` bytes from a 256-byte aligned allocation (B.device_image)."""

    def __init__(self, ctx, blob, offset):
        self.ctx = ctx
        img = B.device_image(blob, offset)
        self.base = ctx.alloc(img.nbytes)
        assert self.base % 256 == 0
        ctx.h2d(self.base, img)
        self.ptr = self.base + offset

    def __enter__(self):
        return self.ptr

    def __exit__(self, *exc):
        self.ctx.synchronize()
        self.ctx.free(self.base)


def _some(n, k, seed):
    """k indices below n, unsorted, with both ends and (from k = 2) a repeat."""
    idx = np.random.default_rng([seed, n, k]).integers(0, n, k).tolist()
    idx[0] = n - 1
    if k >= 3:
        idx[k // 2] = 0
    if k >= 2:
        idx[-1] = idx[0]
    return idx


def _ends(n):
    return [0, min(1, n - 1), n // 2, n - 1]


def _check_proofs(proofs, root, idx, levels, leaves, tag):
    assert [p.nodes for p in proofs] == [B.tree_path(levels, i) for i in idx], (tag, "paths")
    assert [p.leaf for p in proofs] == [leaves[i] for i in idx], (tag, "leaves")
    assert S.verify_multi_branch(root, idx, proofs) == [leaves[i] for i in idx], (tag, "verify")


def _check_tree(t, idx, levels, leaves, tag):
    proofs = t.gen_proofs(idx)
    assert t.get_root() == B.tree_root(levels), (tag, "root")
    _check_proofs(proofs, B.tree_root(levels), idx, levels, leaves, tag)


def _check_forest(f, n, leaf_len, batch, blob, trees, idx, tag):
    """Every root; the paths and leaves of the first and the last tree."""
    assert f.roots() == [B.tree_root(lv) for lv in trees], (tag, "roots")
    every = B.split(blob, n * batch, leaf_len)
    for b in sorted({0, batch - 1}):
        _check_proofs(f.gen_proofs(b, idx), B.tree_root(trees[b]), idx, trees[b], every[b * n:(b + 1) * n],
                      (tag, "tree", b))


# ---- a. leaf digests: every path of hash_leaf, and hash_leaf32, through merkle_leaf_digest_kernel ----

@pytest.mark.parametrize("offset", B.OFFSETS)
@pytest.mark.parametrize("leaf_len", B.LENS)
def test_leaf_digests(ctx, leaf_len, offset):
    """67 leaves: one partly filled workgroup, more than a wave, and enough leaves that their addresses take
    every residue mod 16 the length allows.  Offsets 0 and 1 hash the leaves that end in 0xFF."""
    n = 67
    blob = B.leaves_blob(n, leaf_len, 31 + offset, edge=offset in (0, 1))
    want = [B.blake(x) for x in B.split(blob, n, leaf_len)]
    d_out = ctx.alloc(32 * n + 32)
    try:
        with _DevLeaves(ctx, blob, offset) as d_leaves:
            tail = np.full(32, 0x5A, dtype=np.uint8)
            ctx.h2d(d_out + 32 * n, tail)
            ctx.check(ctx.lib.stark_merkle_leaf_digests_dev(ctx.h, d_leaves, n, leaf_len, d_out, None),
                      "leaf_digests")
            got = np.empty(32 * n + 32, dtype=np.uint8)
            ctx.d2h(got, d_out)
    finally:
        ctx.free(d_out)
    raw = got.tobytes()
    bad = [i for i in range(n) if raw[32 * i:32 * i + 32] != want[i]]
    assert not bad, (leaf_len, offset, "leaves with a wrong digest", bad)
    assert raw[32 * n:] == tail.tobytes(), "a digest written past the n-th"


# ---- b. one tree, every length ----

@pytest.mark.parametrize("leaf_len", B.LENS)
def test_tree_every_length(ctx, leaf_len):
    n = 8
    idx = [3, 0, 7, 1, 6, 2, 5, 4]
    t = S.MerkleProofInPlace(ctx)
    for edge in (False, True):
        blob, (levels,) = B.reference(n, leaf_len, 21, edge)
        t.update_bytes(blob, n, leaf_len)
        _check_tree(t, idx, levels, B.split(blob, n, leaf_len), (leaf_len, edge))


@pytest.mark.parametrize("offset", B.OFFSETS)
@pytest.mark.parametrize("leaf_len", [32, 48, 80, 81, 128, 192])
def test_tree_update_dev_offsets(ctx, leaf_len, offset):
    n = 8
    blob, (levels,) = B.reference(n, leaf_len, 21, True)
    with _DevLeaves(ctx, blob, offset) as d_leaves:
        t = S.MerkleProofInPlace(ctx)
        t.update_dev(d_leaves, n, leaf_len)
        _check_tree(t, list(range(n)), levels, B.split(blob, n, leaf_len), (leaf_len, offset))


@pytest.mark.parametrize("n", [1, 2, 8, 512])
def test_tree_of_empty_leaves(ctx, n):
    """leaf_len = 0: the tree of Blake2s(b"") leaves, and proofs whose leaves are empty; from host leaves and
    from a device pointer."""
    levels = B.tree_levels([b""] * n)
    idx = sorted(set(_ends(n))) + [n - 1]
    t = S.MerkleProofInPlace(ctx)
    t.update_bytes(b"", n, 0)
    _check_tree(t, idx, levels, [b""] * n, (n, "host"))
    with _DevLeaves(ctx, b"", 4) as d_leaves:
        t.update_dev(d_leaves, n, 0)
        _check_tree(t, idx, levels, [b""] * n, (n, "dev"))


# ---- c. each build regime with a leaf that is not 32 bytes ----
# n = 1 (no pair level), 2 (one workgroup), 256 / 512 (kTailBlock), 1024 / 4096 (kMerkleBlock, a tail launch of
# several workgroups); 65 = bytes + a full block, 80 / 144 = vector loads + full blocks, 193 = bytes + 3 blocks.

@pytest.mark.parametrize("leaf_len", [65, 80, 144, 193])
@pytest.mark.parametrize("n", [1, 2, 256, 512, 1024, 4096])
def test_tree_build_regimes(ctx, n, leaf_len):
    blob, (levels,) = B.reference(n, leaf_len, 41)
    t = S.MerkleProofInPlace(ctx)
    t.update_bytes(blob, n, leaf_len)
    _check_tree(t, _ends(n), levels, B.split(blob, n, leaf_len), (n, leaf_len))


# ---- d. the forest ----

@pytest.mark.parametrize("leaf_len", [0, 16, 48, 65, 80, 129, 144])
@pytest.mark.parametrize("n,batch", [(8, 3), (512, 2)])
def test_forest_lengths(ctx, n, batch, leaf_len):
    blob, trees = B.reference(n, leaf_len, 51, True, batch)
    f = S.MerkleForest(ctx)
    f.update_bytes(blob, n, leaf_len, batch)
    _check_forest(f, n, leaf_len, batch, blob, trees, _ends(n) + [n - 1, 0], (n, batch, leaf_len))


@pytest.mark.parametrize("offset", [4, 1])
@pytest.mark.parametrize("leaf_len", [32, 80])
@pytest.mark.parametrize("n,batch", [(8, 3), (512, 2)])
def test_forest_update_dev_offsets(ctx, n, batch, leaf_len, offset):
    """Leaves 4 bytes off a 16-byte boundary: the byte loads of hash_leaf and the gather's word copies; 1 byte
    off: its byte copies."""
    blob, trees = B.reference(n, leaf_len, 51, True, batch)
    with _DevLeaves(ctx, blob, offset) as d_leaves:
        f = S.MerkleForest(ctx)
        f.update_dev(d_leaves, n, leaf_len, batch)
        _check_forest(f, n, leaf_len, batch, blob, trees, _ends(n) + [n - 1, 0], (n, batch, leaf_len, offset))


# ---- e. gather edges: k * leaf_len on both sides of a multiple of 16 ----

GATHER_K = [1, 2, 5, 15, 16, 17, 64]


@pytest.mark.parametrize("k", GATHER_K)
@pytest.mark.parametrize("leaf_len", [1, 3, 33, 65, 127])
def test_gather_edges_tree(ctx, leaf_len, k):
    n = 64
    blob, (levels,) = B.reference(n, leaf_len, 61, True)
    t = S.MerkleProofInPlace(ctx)
    t.update_bytes(blob, n, leaf_len)
    _check_tree(t, _some(n, k, leaf_len), levels, B.split(blob, n, leaf_len), (leaf_len, k))


@pytest.mark.parametrize("k", GATHER_K)
@pytest.mark.parametrize("leaf_len", [3, 65])
def test_gather_edges_forest(ctx, leaf_len, k):
    n, batch = 64, 3
    blob, trees = B.reference(n, leaf_len, 61, True, batch)
    f = S.MerkleForest(ctx)
    f.update_bytes(blob, n, leaf_len, batch)
    _check_forest(f, n, leaf_len, batch, blob, trees, _some(n, k, leaf_len), (leaf_len, k))


# ---- f. the wide leaf kernel (a leaf level of 2^16 nodes and more, two levels in LDS) ----

@pytest.mark.parametrize("leaf_len", [33, 80])
@pytest.mark.parametrize("log_n", [16, 17])
def test_wide_leaf_level_tree(ctx, log_n, leaf_len):
    n = 1 << log_n
    blob, (levels,) = B.reference(n, leaf_len, 71)
    t = S.MerkleProofInPlace(ctx)
    t.update_bytes(blob, n, leaf_len)
    idx = [0, 1, n // 2 - 1, n // 2, 1023, n - 1]  # (1023: the last node of the first workgroup's block)
    _check_tree(t, idx, levels, B.split(blob, n, leaf_len), (n, leaf_len))


def test_wide_leaf_level_forest(ctx):
    n, leaf_len, batch = 1 << 16, 80, 2
    blob, trees = B.reference(n, leaf_len, 71, False, batch)
    f = S.MerkleForest(ctx)
    f.update_bytes(blob, n, leaf_len, batch)
    _check_forest(f, n, leaf_len, batch, blob, trees, [0, 1, n // 2 - 1, n // 2, 1024, n - 1], (n, leaf_len, batch))
