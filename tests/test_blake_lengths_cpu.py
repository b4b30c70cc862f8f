"""The host references at the leaf lengths of blake_cases.LENS, against hashlib: the library's host Blake2s
(stark_blake, and b2s_host under stark_merkle_verify), the oracle's C Blake2s and tree, and the oracle's Python
Blake2s.  test_gpu_blake_lengths.py checks the device leaf hash at the same lengths; with these passing, a
failure there points at the kernel."""
import pytest

import blake_cases as B
import oracle as O
import stark_amd as S

N = 8


def _messages(leaf_len):
    return B.split(B.leaves_blob(N, leaf_len, 11), N, leaf_len) + \
        B.split(B.leaves_blob(N, leaf_len, 12, edge=True), N, leaf_len)


@pytest.mark.parametrize("leaf_len", B.LENS)
def test_host_blake2s_vs_hashlib(oracle, leaf_len):
    for msg in _messages(leaf_len):
        want = B.blake(msg)
        assert S.blake(msg) == want, ("stark_blake", leaf_len)
        assert oracle.blake2s(msg) == want, ("oracle_blake2s", leaf_len)
        assert O.py_blake(msg) == want, ("py_blake", leaf_len)


@pytest.mark.parametrize("chunks", [1, 4])
@pytest.mark.parametrize("leaf_len", B.LENS)
def test_oracle_tree_vs_hashlib(oracle, leaf_len, chunks):
    for edge in (False, True):
        blob, (levels,) = B.reference(N, leaf_len, 21, edge)
        idx = [5, 0, 7, 3, 1, 6, 2, 4]
        root, paths = oracle.merkle(blob, N, leaf_len, idx, chunks=chunks)
        assert root == B.tree_root(levels), (leaf_len, chunks, edge)
        assert paths == [B.tree_path(levels, i) for i in idx], (leaf_len, chunks, edge)


@pytest.mark.parametrize("leaf_len", B.LENS)
def test_host_verify_accepts_hashlib_proofs(leaf_len):
    """stark_merkle_verify takes the hashlib tree's proof of every leaf, and refuses each one with one bit of the
    leaf flipped (of a node, where the leaf is empty)."""
    blob, (levels,) = B.reference(N, leaf_len, 21, True)
    leaves = B.split(blob, N, leaf_len)
    root = B.tree_root(levels)
    idx = list(range(N))
    proofs = [S.Proof(leaves[i], B.tree_path(levels, i)) for i in idx]
    assert S.verify_multi_branch(root, idx, proofs) == leaves
    for i in idx:
        if leaf_len:
            # the flipped byte walks over the leaf with i: its first, its last and some between
            at = [0, leaf_len - 1, leaf_len // 2, leaf_len // 3, 63 % leaf_len, 64 % leaf_len, 15 % leaf_len,
                  16 % leaf_len][i]
            leaf = bytearray(leaves[i])
            leaf[at] ^= 1 << (i % 8)
            bad = S.Proof(bytes(leaf), proofs[i].nodes)
        else:
            nodes = [bytearray(x) for x in proofs[i].nodes]
            nodes[i % len(nodes)][(5 * i) % 32] ^= 1 << (i % 8)
            bad = S.Proof(b"", [bytes(x) for x in nodes])
        with pytest.raises(AssertionError):
            S.verify_multi_branch(root, [i], [bad])
        if leaf_len:  # the right proof at another index (empty leaves are all one leaf: it would hold)
            with pytest.raises(AssertionError):
                S.verify_multi_branch(root, [i ^ 1], [proofs[i]])
