"""GPU: prove_low_degree over a device group (stark_group_prove_low_degree / _dev, csrc/group.hip) and the
two data-movement kernels it brings (stark_class_deal_dev / stark_class_merge_dev, csrc/dist.hip).  The G
members are G contexts on device 0, as in test_gpu_group.py.

Every proof is compared bit for bit with the oracle's restatement of fri.rs:46-224 (or, at 2^23, with its
committed digest), by length and SHA-256; a mismatch names the first differing layer."""
import ctypes
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "r1cs")
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "r1cs_proofs.json")))
BIG = json.load(open(os.path.join(ROOT, "tests", "golden", "large_digests.json")))

# (log_n, exclude, max_deg_plus_1): sizes the group distributes (G > 1, n > 2^16, max_deg_plus_1 > 16)
DISTRIBUTED = [
    (17, 8, 1 << 15),   # smallest n with a distributed layer; the tail starts at 2^15
    (18, 3, 1 << 16),   # the tail starts exactly at 2^16; an exclusion that is no power of two
    (19, 0, 1 << 17),   # two distributed layers; no exclusion
    (19, 8, 1 << 16),   # max degree n / 8
    (19, 8, 64),        # one distributed layer, then Last over 2^17 class-distributed values
]
# member 0's routes
SMALL = [(7, 8, 32), (12, 8, 1024), (16, 8, 1 << 13), (10, 2, 256)]


def _sha(s) -> str:
    return hashlib.sha256(s.encode() if isinstance(s, str) else s).hexdigest()


@functools.lru_cache(maxsize=None)
def _case(log_n, exclude, deg):
    """(values, root, the oracle's JSON), computed once per case and shared (never modified)."""
    o = O.Oracle()
    w = O.root_of_unity(log_n)
    vals = o.best_fft(O.random_elements(deg, log_n), w, log_n, cpus=8)
    vals.setflags(write=False)
    return vals, w, o.prove_low_degree_json(vals, w, deg, exclude, chunks=8)


def _layer_kind(layer) -> str:
    return next(iter(layer))


def _same_json(got: str, want: str, what=""):
    """Equal by length and SHA-256; on a mismatch the index and kind of the first differing layer."""
    if len(got) == len(want) and _sha(got) == _sha(want):
        return
    g, w = json.loads(got), json.loads(want)
    where = f"{len(g)} layers, expected {len(w)}"
    for i, (a, b) in enumerate(zip(g, w)):
        if a != b:
            where = f"first differing layer {i}: {_layer_kind(a)} (expected {_layer_kind(b)})"
            if _layer_kind(a) == _layer_kind(b) == "Middle":
                where += ", fields " + ",".join(k for k in b["Middle"] if a["Middle"].get(k) != b["Middle"][k])
            break
    pytest.fail(f"{what}: JSON of {len(got)} B differs from the expected {len(want)} B; {where}")


@pytest.fixture(scope="module")
def groups():
    """One group per member count, shared by the tests of this module (and so reused across shapes)."""
    from stark_amd.group import Group
    made = {}

    def get(G):
        if G not in made:
            made[G] = Group([0] * G)
        return made[G]
    yield get
    for g in made.values():
        g.close()


class _Shards:
    """x's residue classes on the members of g (stark_dev_alloc / stark_memcpy_h2d on the member contexts)."""

    def __init__(self, g, x):
        self.g, self.ptrs = g, []
        self.host = [np.ascontiguousarray(x[r::g.G]) for r in range(g.G)]
        for r in range(g.G):
            p = ctypes.c_void_p()
            assert g.lib.stark_dev_alloc(g.ctx_handle(r), max(self.host[r].nbytes, 32), ctypes.byref(p)) == 0
            self.ptrs.append(p.value)
            if self.host[r].nbytes:
                assert g.lib.stark_memcpy_h2d(g.ctx_handle(r), p.value, self.host[r].ctypes.data,
                                              self.host[r].nbytes) == 0

    def unchanged(self) -> bool:
        for r in range(self.g.G):
            back = np.empty_like(self.host[r])
            assert self.g.lib.stark_memcpy_d2h(self.g.ctx_handle(r), back.ctypes.data, self.ptrs[r], back.nbytes) == 0
            if not np.array_equal(back, self.host[r]):
                return False
        return True

    def free(self):
        for r, p in enumerate(self.ptrs):
            self.g.lib.stark_dev_free(self.g.ctx_handle(r), p)
        self.ptrs = []


@pytest.mark.parametrize("world", [1, 2, 4, 8])
def test_class_deal_merge(ctx, world):
    """chunk r, element j = block[r + world j], and back; n_block = world (one element per chunk), 24 world
    (no multiple of a workgroup's 128 elements) and 2^12 (several workgroups); twice on the same buffers."""
    rng = np.random.default_rng(0xC1A55 + world)
    for n_block in (world, 24 * world, 1 << 12):
        x = rng.integers(0, 1 << 63, (n_block, 4), dtype=np.uint64)
        d_in, d_chunks, d_back = (ctx.alloc(x.nbytes) for _ in range(3))
        try:
            ctx.h2d(d_in, x)
            for _ in range(2):
                ctx.class_deal_dev(d_in, d_chunks, n_block, world)
                ctx.class_merge_dev(d_chunks, d_back, n_block, world)
                ctx.synchronize()
                dealt, back = np.empty_like(x), np.empty_like(x)
                ctx.d2h(dealt, d_chunks)
                ctx.d2h(back, d_back)
                assert np.array_equal(dealt.reshape(world, -1, 4), x.reshape(-1, world, 4).transpose(1, 0, 2)), n_block
                assert np.array_equal(back, x), n_block
        finally:
            for p in (d_in, d_chunks, d_back):
                ctx.free(p)


def test_class_deal_merge_errors(ctx):
    a, b = ctx.alloc(64 * 32), ctx.alloc(64 * 32)
    try:
        for fn in (ctx.lib.stark_class_deal_dev, ctx.lib.stark_class_merge_dev):
            assert fn(ctx.h, a, b, 24, 3, None) == 3      # world not in {1, 2, 4, 8}
            assert fn(ctx.h, a, b, 32, 16, None) == 3
            assert fn(ctx.h, a, b, 0, 0, None) == 3
            assert fn(ctx.h, a, b, 26, 4, None) == 1      # world does not divide n_block
            assert fn(ctx.h, a, a, 32, 4, None) == 3      # the output is the input
            assert fn(ctx.h, a, a + 32 * 16, 32, 4, None) == 3   # ... or overlaps it
            assert fn(ctx.h, a, b, 0, 4, None) == 0       # nothing to move
        ctx.synchronize()
    finally:
        ctx.free(a)
        ctx.free(b)


@pytest.mark.parametrize("G", [2, 4, 8])
@pytest.mark.parametrize("log_n,exclude,deg", DISTRIBUTED)
def test_group_fri_vs_oracle(groups, G, log_n, exclude, deg):
    vals, w, want = _case(log_n, exclude, deg)
    _same_json(groups(G).prove_low_degree(vals, w, deg, exclude).to_json(), want, f"G={G}")


@pytest.mark.parametrize("G,log_n,exclude,deg", [(G, *c) for G in (1, 8) for c in SMALL] + [(1, 17, 8, 1 << 15)])
def test_group_fri_member0_routes(groups, G, log_n, exclude, deg):
    """Inputs the group does not distribute (n <= 2^16, or one member) are stark_prove_low_degree on member 0."""
    vals, w, want = _case(log_n, exclude, deg)
    _same_json(groups(G).prove_low_degree(vals, w, deg, exclude).to_json(), want, f"G={G}")


@pytest.mark.parametrize("G", [2, 8])
def test_group_fri_dev(groups, G):
    """The device entry: equal to the host entry's JSON at 2^17 with the shards left as they were; at 2^10
    the classes are gathered to member 0 and merged there, equal to the oracle."""
    g = groups(G)
    for log_n, exclude, deg, host_too in ((17, 8, 1 << 15, True), (10, 2, 256, False)):
        vals, w, want = _case(log_n, exclude, deg)
        sh = _Shards(g, vals)
        try:
            got = g.prove_low_degree_dev(sh.ptrs, 1 << log_n, w, deg, exclude).to_json()
            assert sh.unchanged(), log_n
        finally:
            sh.free()
        _same_json(got, want, f"_dev G={G} 2^{log_n}")
        if host_too:
            _same_json(got, g.prove_low_degree(vals, w, deg, exclude).to_json(), f"_dev vs host G={G}")


def test_group_fri_reuse(groups):
    """Two sizes, then the first again, on one group: the reused slots and trees give the first results; a
    proof of the whole prover on the same group still equals its golden digest."""
    g = groups(4)
    first = {}
    for log_n in (19, 17, 19):
        case = (19, 8, 1 << 16) if log_n == 19 else (17, 8, 1 << 15)
        vals, w, want = _case(*case)
        js = g.prove_low_degree(vals, w, case[2], case[1]).to_json()
        _same_json(js, first.setdefault(log_n, js), f"repeat of 2^{log_n}")
        _same_json(js, want, f"2^{log_n}")
    r1 = open(os.path.join(FIX, "compute.r1cs"), "rb").read()
    wt = open(os.path.join(FIX, "compute.wtns"), "rb").read()
    assert _sha(g.prove_with_witness(r1, wt).to_json()) == GOLD["compute"]["json_sha256"]


def test_group_fri_verifies(groups, oracle):
    """The product verifier (fri.rs:226-404) accepts the group's proof against the values' own Merkle root
    and rejects it with one leaf byte flipped."""
    from stark_amd.verify import verify_low_degree_proof
    log_n, exclude, deg = 19, 8, 1 << 17
    w = O.root_of_unity(log_n)
    vals = oracle.best_fft(O.random_elements(deg, log_n), w, log_n, cpus=8)
    root, _ = oracle.merkle(vals.tobytes(), 1 << log_n, 32, [], chunks=8)
    proof = json.loads(groups(4).prove_low_degree(vals, w, deg, exclude).to_json())
    assert [_layer_kind(x) for x in proof[:2]] == ["Middle", "Middle"]
    assert verify_low_degree_proof(root, w, proof, deg, exclude)
    proof[1]["Middle"]["poly_branches"][7]["leaf"][0] ^= 1
    with pytest.raises(AssertionError):
        verify_low_degree_proof(root, w, proof, deg, exclude)


def test_group_fri_2_23_digest(groups):
    """The bench's FRI input (precision 2^23) over 8 members equals the oracle's digest."""
    rec = BIG["fri_2^23"]
    lf = 23
    wf = O.root_of_unity(lf)
    g = groups(8)
    vals = g.best_fft(O.random_elements(1 << (lf - 2), 0x5EED0000 + lf), wf, lf)
    assert _sha(vals.tobytes()) == rec["values_sha256"]
    js = g.prove_low_degree(vals, wf, 1 << (lf - 2), 8).to_json()
    assert len(js) == rec["json_len"]
    assert _sha(js) == rec["json_sha256"]


def test_group_fri_errors(groups, ctx):
    """Argument errors carry the status the single-context call gives for the same input."""
    from stark_amd import StarkError
    g = groups(2)
    for log_n, deg in ((17, 1 << 15), (10, 256)):     # a distributed size and one of member 0's
        n = 1 << log_n
        vals = O.random_elements(n, 0xE44 + log_n)
        bad_root = O.root_of_unity(log_n + 1)          # len(values) != the order of the root
        with pytest.raises(StarkError) as single:
            ctx.prove_low_degree(vals, bad_root, deg, 8)
        with pytest.raises(StarkError) as e:
            g.prove_low_degree(vals, bad_root, deg, 8)
        assert e.value.code == single.value.code
        sh = _Shards(g, vals)
        try:
            with pytest.raises(StarkError) as e:
                g.prove_low_degree_dev(sh.ptrs, n, bad_root, deg, 8)
            assert e.value.code == single.value.code
            with pytest.raises(StarkError) as e:           # a null class pointer
                g.prove_low_degree_dev([sh.ptrs[0], None], n, O.root_of_unity(log_n), deg, 8)
            assert e.value.code == 3
        finally:
            sh.free()
        with pytest.raises(StarkError) as single:          # a column length the index sampler refuses
            ctx.prove_low_degree(vals, O.root_of_unity(log_n), deg, 1)
        with pytest.raises(StarkError) as e:
            g.prove_low_degree(vals, O.root_of_unity(log_n), deg, 1)
        assert e.value.code == single.value.code == 3
    g.synchronize()
