"""Shared data of test_blake_lengths_cpu.py and test_gpu_blake_lengths.py: the leaf lengths and alignments at
which the device leaf hash (csrc/merkle_dev.h, hash_leaf / hash_leaf32) changes its data path, a deterministic
leaf generator, and the reference tree over hashlib's Blake2s (independent of the library and of the oracle).

hash_leaf reads a leaf by 16-byte vector loads where the leaf's address and its length are both multiples of
16, and byte by byte otherwise; either way the 64-byte blocks before the last take one loop and the last block
(partial, full or empty) another.  LENS holds both residues mod 16 around every multiple of 64 up to 256, the
lengths between them that can take the vector path, and two longer ones."""
import functools
import hashlib

import numpy as np

LENS = [0, 1, 3, 4, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 96, 112, 127, 128, 129,
        144, 176, 191, 192, 193, 255, 256, 257, 320, 1000]

# Byte offsets of the first leaf from a 256-byte aligned device allocation.  0 and 16 keep a length that is a
# multiple of 16 on the vector path (and 32-byte leaves on hash_leaf32); 1, 4 and 8 force the byte path.
OFFSETS = [0, 1, 4, 8, 16]

GUARD = 64  # bytes of filler after the last leaf of a device image (device_image)


def blake(b: bytes) -> bytes:
    return hashlib.blake2s(b).digest()


def leaves_blob(n: int, leaf_len: int, seed: int, edge: bool = False) -> bytes:
    """n contiguous leaves of leaf_len random bytes, every leaf different wherever n leaves of that length can
    be.  edge: the last byte of every leaf is 0xFF (the byte after it is then the next leaf's first byte, which
    differs from leaf to leaf), so a read one byte short or one byte long changes the digest; leaves shorter
    than two bytes stay as they are."""
    rng = np.random.default_rng([seed, n, leaf_len, int(edge)])
    a = rng.integers(0, 256, (n, leaf_len), dtype=np.uint8)
    free = leaf_len  # the bytes that stay random
    if edge and leaf_len >= 2:
        a[:, -1] = 0xFF
        free -= 1
    if 0 < free < 4 and n <= 256 ** free:
        # short leaves: n different values of the leading bytes, drawn without repeats
        v = rng.choice(256 ** free, n, replace=False)
        for k in range(free):
            a[:, k] = (v >> (8 * k)) & 0xFF
    blob = a.tobytes()
    if 0 < free and n <= 256 ** min(free, 4):
        assert len({blob[i * leaf_len:(i + 1) * leaf_len] for i in range(n)}) == n, "equal leaves"
    return blob


def split(blob: bytes, n: int, leaf_len: int) -> list:
    return [blob[i * leaf_len:(i + 1) * leaf_len] for i in range(n)]


def device_image(blob: bytes, offset: int, seed: int = 0) -> np.ndarray:
    """The bytes of an allocation that holds blob at `offset`: filler that is never zero before it and GUARD
    bytes of it after it, so a read outside the leaves changes a digest and stays inside the allocation."""
    rng = np.random.default_rng([seed, offset, len(blob)])
    img = rng.integers(1, 256, offset + len(blob) + GUARD, dtype=np.uint8)
    img[offset:offset + len(blob)] = np.frombuffer(blob, dtype=np.uint8)
    return img


def tree_levels(leaves: list) -> list:
    """levels[0] = Blake2s(leaf), levels[d + 1][i] = Blake2s(levels[d][2 i] || levels[d][2 i + 1])."""
    assert leaves and len(leaves) & (len(leaves) - 1) == 0
    levels = [[blake(x) for x in leaves]]
    while len(levels[-1]) > 1:
        lv = levels[-1]
        levels.append([blake(lv[i] + lv[i + 1]) for i in range(0, len(lv), 2)])
    return levels


def tree_root(levels: list) -> bytes:
    return levels[-1][0]


def tree_path(levels: list, index: int) -> list:
    """The siblings of leaf `index`, leaf to root."""
    return [levels[d][(index >> d) ^ 1] for d in range(len(levels) - 1)]


@functools.lru_cache(maxsize=4)
def reference(n: int, leaf_len: int, seed: int, edge: bool = False, batch: int = 1):
    """(blob, [levels of tree b]) of `batch` trees of n leaves each over leaves_blob(n * batch, ...): computed
    once and shared by the tests that use the same shape; callers leave it unchanged."""
    blob = leaves_blob(n * batch, leaf_len, seed, edge)
    every = split(blob, n * batch, leaf_len)
    return blob, [tree_levels(every[b * n:(b + 1) * n]) for b in range(batch)]
