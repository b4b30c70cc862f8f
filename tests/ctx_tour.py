"""A tour of the single-GPU entry points for tests/test_gpu_ctx_tour.py (each on poisoned and on reused context
scratch) and tests/test_ctx_tour_cpu.py (the tables below against csrc/internal.h and the library's report).

BUFFERS classifies every buffer a stark_ctx owns, as stark_test_poison_ctx (csrc/api.hip) reports them: `scratch`
(the hook fills it: every call that reads it writes it first) or `kept` (its contents are an invariant between
calls).  DEVBUF_MEMBERS and PINNED_SLOTS restate csrc/internal.h; a member added there fails the CPU test until it
is classified here and in the hook.

OPS is the tour: per operation two shapes (B's scratch need is the smaller one, so B after A runs inside A's
buffers), a callable (ctx, shape, second) -> bytes and the expected bytes, computed once per session from the CPU
oracle or from the Python restatement the operation's own test uses -- never from a GPU run.  `second` (device
entries only) puts the call on a second torch stream instead of the context's.
"""
import functools
import json
import os
import random

import numpy as np

import oracle as O
import r1cs as R
import r1cs_cases as C
import stark_amd as S

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "r1cs")
P = O.P
NEVER = S.Context.MULTIPOINT_TREE_NEVER

SCRATCH, KEPT = "scratch", "kept"

# stark::DevBuf members of stark_ctx (csrc/internal.h), every one scratch: verify_arena / verify_lde hold the
# circuit stark_verify_r1cs_bytes builds anew on every call (kept for their allocations, not their contents).
DEVBUF_MEMBERS = ["scratch", "io", "io2", "fri_cols", "r1cs_arena", "trace_arena", "trace_raw", "lde_tmp",
                  "verify_arena", "verify_lde", "ext_idx_tmp", "inv_tmp", "spot", "poly", "fri_misc", "fri_batch",
                  "prove_batch", "verify_batch", "witness_check"]
PINNED_SLOTS = 8

BUFFERS = dict([(m, SCRATCH) for m in DEVBUF_MEMBERS] +
               [("pinned[%d]" % k, SCRATCH) for k in range(PINNED_SLOTS)] +
               # the digest areas of the context's trees and forests
               [("trees[%d]" % k, SCRATCH) for k in range(5)] +
               [("fri_trees", SCRATCH), ("fri_forests", SCRATCH)] +
               [("r1cs_forests[%d]" % k, SCRATCH) for k in range(3)] +
               [("verify_forest", SCRATCH)] +
               # kept: the tail kernels' workgroup counters (zero between launches), the caches and the plans
               [(k, KEPT) for k in ("tree_counters", "tw", "ext_idx", "post_tw", "interp_plans", "eval_plans",
                                    "long_lists")])

# scratch buffers no single-GPU entry point reaches, with the reason (test_tour_reaches_every_buffer)
UNREACHED = {
    "trees[0]": "no code creates slot 0 any more: prove_low_degree's layers are fri_trees",
    "trees[1]": "no code creates slot 1 any more: prove_low_degree's layers are fri_trees",
}


@functools.lru_cache(maxsize=None)
def oracle():
    return O.Oracle()


def state(ctx) -> dict:
    """What the tour keeps alive on a context between calls (circuits, plans, trees), so that a later call finds
    them as an earlier one left them; release() drops it before the context closes."""
    return ctx.__dict__.setdefault("_tour", {})


def release(ctx):
    for v in list(ctx.__dict__.pop("_tour", {}).values()):
        close = getattr(v, "close", None)
        if close:
            close()


def limbs(v):
    return O.to_limbs(v) if len(v) else np.empty((0, 4), dtype=np.uint64)


def _b(a) -> bytes:
    return np.ascontiguousarray(a).tobytes()


# ---- device buffers through torch ----------------------------------------------------------------------------------
_second = []


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _dev_empty(nbytes):
    import torch
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")


def _on_stream(ctx, second, body):
    """body(stream handle) on the context's stream or on a second torch stream, then a synchronisation: the
    tensors the body used may be read back after it."""
    import torch
    torch.cuda.synchronize()
    if second:
        if not _second:
            _second.append(torch.cuda.Stream())
        with torch.cuda.stream(_second[0]):
            body(S.torch_stream())
    else:
        body(0)
        ctx.synchronize()
    torch.cuda.synchronize()


def _host(t, nbytes) -> bytes:
    return t[:nbytes].cpu().numpy().tobytes()


# ---- NTT, LDE ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _coeffs(n, seed):
    return O.random_elements(max(n, 1), seed)[:n]


def _fft_run(inverse):
    def run(ctx, shape, second=False):
        log_n, length = shape
        f = ctx.inv_best_fft if inverse else ctx.best_fft
        return _b(f(_coeffs(length, 100 + log_n), O.root_of_unity(log_n), log_n))
    return run


def _fft_want(inverse):
    def want(shape):
        log_n, length = shape
        f = oracle().inv_best_fft if inverse else oracle().best_fft
        return _b(f(_coeffs(length, 100 + log_n), O.root_of_unity(log_n), log_n, cpus=4))
    return want


def _ntt_dev_run(ctx, shape, second=False):
    log_n, batch = shape
    c = _coeffs(batch << log_n, 110 + log_n)
    d = _dev(c)
    _on_stream(ctx, second, lambda s: ctx.ntt_dev(d.data_ptr(), log_n, batch, O.root_of_unity(log_n), stream=s))
    return _host(d, c.nbytes)


def _ntt_dev_want(shape):
    log_n, batch = shape
    n = 1 << log_n
    c = _coeffs(batch << log_n, 110 + log_n)
    return b"".join(_b(oracle().best_fft(c[b * n:(b + 1) * n], O.root_of_unity(log_n), log_n, cpus=4))
                    for b in range(batch))


def _lde_roots(log_steps, log_blowup):
    g2 = O.root_of_unity(log_steps + log_blowup)
    return pow(g2, 1 << log_blowup, P), g2


def _lde_run(ctx, shape, second=False):
    log_steps, log_blowup = shape
    g1, g2 = _lde_roots(log_steps, log_blowup)
    return _b(ctx.lde(_coeffs(1 << log_steps, 120 + log_steps), g1, log_blowup, g2))


def _lde_want_cols(v, log_steps, log_blowup, batch):
    g1, g2 = _lde_roots(log_steps, log_blowup)
    n = 1 << log_steps
    out = []
    for b in range(batch):
        co = oracle().inv_best_fft(v[b * n:(b + 1) * n], g1, log_steps, cpus=4)
        out.append(_b(oracle().best_fft(co, g2, log_steps + log_blowup, cpus=4)))
    return b"".join(out)


def _lde_want(shape):
    return _lde_want_cols(_coeffs(1 << shape[0], 120 + shape[0]), shape[0], shape[1], 1)


def _lde_dev_run(ctx, shape, second=False):
    log_steps, log_blowup, batch = shape
    g1, g2 = _lde_roots(log_steps, log_blowup)
    v = _coeffs(batch << log_steps, 130 + log_steps)
    d_in, nout = _dev(v), (batch << (log_steps + log_blowup)) * 32
    d_out = _dev_empty(nout)
    _on_stream(ctx, second, lambda s: ctx.lde_dev(d_in.data_ptr(), d_out.data_ptr(), log_steps, log_blowup, batch,
                                                 g1, g2, stream=s))
    return _host(d_out, nout)


def _lde_dev_want(shape):
    return _lde_want_cols(_coeffs(shape[2] << shape[0], 130 + shape[0]), *shape)


# ---- field vectors -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inv_in(n):
    v = O.random_elements(n, 140 + n % 97).copy()
    v[::7] = 0
    v[-1] = 0
    return v


@functools.lru_cache(maxsize=None)
def _interp4_in(rows):
    xs, ys = O.random_elements(4 * rows, 81 + rows).copy(), O.random_elements(4 * rows, 82 + rows)
    xs[4 * (rows // 2) + 3] = xs[4 * (rows // 2)]  # a repeated x: zero denominators map to zero
    return xs, ys


@functools.lru_cache(maxsize=None)
def _lincomb_in(shape):
    n_cols, n = shape
    return O.random_elements(n_cols * n, 93 + n_cols), O.random_elements(n_cols, 94 + n)


def _lincomb_want(shape):
    n_cols, n = shape
    cols, k = (O.from_limbs(a) for a in _lincomb_in(shape))
    return _b(O.to_limbs([sum(k[j] * cols[j * n + i] for j in range(n_cols)) % P for i in range(n)]))


# ---- polynomials (the restatements of tests/test_gpu_poly.py, test_gpu_divrem.py, test_gpu_interp_batch.py) --------
def py_zpoly(xs):
    z = [1]
    for x in xs:
        z = [((z[j - 1] if j else 0) - (z[j] * x if j < len(z) else 0)) % P for j in range(len(z) + 1)]
    return z


def py_interp(xs, ys):
    """lagrange_interp (poly_utils.rs:409-439) with 1 / 0 = 0, in O(n^2) on Python integers."""
    n = len(xs)
    z = py_zpoly(xs)
    out = [0] * n
    for x, y in zip(xs, ys):
        q, carry = [0] * n, z[n]
        for d in range(n, 0, -1):  # Z / (X - x) by synthetic division
            q[d - 1] = carry
            carry = (z[d - 1] + carry * x) % P
        den = 0
        for c in reversed(q):
            den = (den * x + c) % P
        if den == 0 or y == 0:
            continue
        s = y * pow(den, -1, P) % P
        for j in range(n):
            out[j] = (out[j] + q[j] * s) % P
    return out


def py_cyclic(a, b, n):
    out = [0] * n
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[(i + j) % n] = (out[(i + j) % n] + x * y) % P
    return out


def py_divrem(a, b):
    """div_polys and mod_polys (poly_utils.rs:235-295): (q, r), r of len(b) - 1 coefficients."""
    bb = list(b)
    while bb and bb[-1] == 0:
        bb.pop()
    c, q = list(a), []
    inv = pow(bb[-1], P - 2, P)
    for d in range(len(a) - len(bb), -1, -1):
        quot = c[d + len(bb) - 1] * inv % P
        q.append(quot)
        for i in range(len(bb)):
            c[d + i] = (c[d + i] - bb[i] * quot) % P
    q.reverse()
    return q, (c + [0] * len(b))[:len(b) - 1]


@functools.lru_cache(maxsize=None)
def _points(n, seed, repeat):
    """n field elements: 0 in the middle, distinct, or (repeat) with xs[1] again at the end."""
    rng = random.Random(seed)
    xs = []
    while len(xs) < n:
        x = rng.randrange(P)
        if x not in xs:
            xs.append(x)
    if n >= 3:
        xs[n // 2] = 0
        if repeat:
            xs[n - 1] = xs[1]
    return tuple(xs)


@functools.lru_cache(maxsize=None)
def _values(n, seed):
    rng = random.Random(seed)
    ys = [rng.randrange(P) for _ in range(n)]
    for i in range(0, n, 7):
        ys[i] = 0
    return tuple(ys)


def _tree_min(ctx, m, body):
    ctx.set_multipoint_tree_min(m)
    try:
        return body()
    finally:
        ctx.set_multipoint_tree_min(0)


@functools.lru_cache(maxsize=None)
def _mp_in(shape):
    n, d = shape
    return O.random_elements(d, 4000 + d), limbs(_points(n, 3000 + n, True))


def _mp_run(m):
    def run(ctx, shape, second=False):
        poly, xs = _mp_in(shape)
        return _tree_min(ctx, m, lambda: _b(ctx.eval_poly_multipoint(poly, xs)))
    return run


def _mp_dev_run(ctx, shape, second=False):
    poly, xs = _mp_in(shape)
    tp, tx, out = _dev(poly), _dev(xs), _dev_empty(xs.nbytes)
    _tree_min(ctx, 1, lambda: _on_stream(ctx, second, lambda s: ctx.eval_poly_multipoint_dev(
        tp.data_ptr(), len(poly), tx.data_ptr(), len(xs), out.data_ptr(), stream=s)))
    return _host(out, xs.nbytes)


def _mp_want(shape):
    poly, xs = _mp_in(shape)
    return _b(oracle().eval_poly_multi(poly, xs))


def _lagrange_run(m):
    def run(ctx, n, second=False):
        xs, ys = limbs(_points(n, 1000 + n, True)), limbs(_values(n, 2000 + n))
        return _tree_min(ctx, m, lambda: _b(ctx.lagrange_interp(xs, ys)))
    return run


@functools.lru_cache(maxsize=None)
def _lagrange_want(n):
    return _b(limbs(py_interp(_points(n, 1000 + n, True), _values(n, 2000 + n))))


@functools.lru_cache(maxsize=None)
def _domain_in(count):
    g = O.root_of_unity(10)
    w = random.Random(30 + count).sample(range(1 << 10), count)
    return g, tuple(w), tuple(pow(g, e, P) for e in w), _values(count, 40 + count)


def _lagrange_domain_run(ctx, count, second=False):
    g, w, _, ys = _domain_in(count)
    return _b(ctx.lagrange_interp(list(w), limbs(ys), root_of_unity=g, log_order_of_root=10))


def _lagrange_domain_want(count):
    _, _, xs, ys = _domain_in(count)
    return _b(limbs(py_interp(xs, ys)))


@functools.lru_cache(maxsize=None)
def _mul_in(shape):
    log_n, la, lb = shape
    return O.random_elements(la, 50 + la), O.random_elements(lb, 51 + lb)


def _mul_want(shape):
    a, b = _mul_in(shape)
    return _b(limbs(py_cyclic(O.from_limbs(a), O.from_limbs(b), 1 << shape[0])))


@functools.lru_cache(maxsize=None)
def _div_in(log_n):
    """(a b mod X^n - 1, b, a) for full-length a and b whose transform has no zero: the quotient is a."""
    n = 1 << log_n
    a, b = O.random_elements(n, 60 + log_n), O.random_elements(n, 61 + log_n)
    assert oracle().best_fft(b, O.root_of_unity(log_n), log_n, cpus=4).any(axis=1).all()
    return limbs(py_cyclic(O.from_limbs(a), O.from_limbs(b), n)), b, a


@functools.lru_cache(maxsize=None)
def _divrem_in(shape):
    la, lb = shape
    rng = random.Random(100 * la + lb)
    a, b = [rng.randrange(P) for _ in range(la)], [rng.randrange(1, P) for _ in range(lb)]
    return tuple(a), tuple(b)


def _divrem_run(ctx, shape, second=False):
    a, b = _divrem_in(shape)
    q, r = ctx.divrem_polys(limbs(a), limbs(b))
    return _b(q) + _b(r)


def _divrem_want(shape):
    q, r = py_divrem(*_divrem_in(shape))
    return _b(limbs(q)) + _b(limbs(r))


# ---- plans ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _interp_plan_in(n):
    rng = random.Random(11 * n)
    ys = [[rng.randrange(P) for _ in range(n)] for _ in range(3)]
    ys[0][1], ys[-1][n - 1] = 0, P - 1
    return _points(n, 7 * n, True), ys


def _interp_plan_run(dev):
    def run(ctx, n, second=False):
        xs, ys = _interp_plan_in(n)
        y = np.stack([O.to_limbs(v) for v in ys])
        plan = ctx.interp_plan(limbs(xs))  # (built on every call: the build takes ctx->poly too)
        try:
            if not dev:
                return _b(plan.apply(y))
            ty, out = _dev(y), _dev_empty(y.nbytes)
            _on_stream(ctx, second, lambda s: plan.apply_dev(ty.data_ptr(), 3, out.data_ptr(), stream=s))
            return _host(out, y.nbytes)
        finally:
            plan.close()
    return run


@functools.lru_cache(maxsize=None)
def _interp_plan_want(n):
    xs, ys = _interp_plan_in(n)
    return b"".join(_b(limbs(py_interp(xs, y))) for y in ys)


EVAL_PLAN_N, EVAL_PLAN_MAX = 129, 600


@functools.lru_cache(maxsize=None)
def _eval_plan_in(d):
    return (limbs(_points(EVAL_PLAN_N, 5000 + EVAL_PLAN_N, True)),
            np.ascontiguousarray(O.random_elements(3 * d, 6000 + d)).reshape(3, d, 4))


def _eval_plan_run(dev):
    def run(ctx, d, second=False):
        """One plan per context, built by the first call and kept (a `kept` buffer) across every later poisoning;
        d = 600 takes the plan's transform of alpha as it is, d = 100 a prefix of alpha."""
        xs, polys = _eval_plan_in(d)
        st = state(ctx)
        if "eval_plan" not in st:
            st["eval_plan"] = ctx.eval_plan(xs, EVAL_PLAN_MAX)
        plan = st["eval_plan"]
        if not dev:
            return _b(plan.apply(polys))
        tp, out = _dev(polys), _dev_empty(3 * EVAL_PLAN_N * 32)
        _on_stream(ctx, second, lambda s: plan.apply_dev(tp.data_ptr(), d, d, 3, out.data_ptr(), EVAL_PLAN_N,
                                                        stream=s))
        return _host(out, 3 * EVAL_PLAN_N * 32)
    return run


def _eval_plan_want(d):
    xs, polys = _eval_plan_in(d)
    return b"".join(_b(oracle().eval_poly_multi(p, xs)) for p in polys)


# ---- Merkle --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _merkle_in(shape, batch):
    log_n, leaf_len = shape
    n = 1 << log_n
    rng = np.random.default_rng(log_n * 1000 + leaf_len + batch)
    blob = rng.integers(0, 256, n * leaf_len * batch, dtype=np.uint8).tobytes()
    idx = sorted(set(rng.integers(0, n, 12).tolist())) + [0, n - 1, 0]
    return blob, n, leaf_len, idx


def _proof_bytes(root, proofs):
    return root + b"".join(p.leaf + b"".join(p.nodes) for p in proofs)


def _merkle_run(dev):
    def run(ctx, shape, second=False):
        """One tree object per context: shape B is built in the node buffer shape A left."""
        blob, n, leaf_len, idx = _merkle_in(shape, 1)
        key = "merkle_dev" if dev else "merkle"
        t = state(ctx).get(key) or S.MerkleProofInPlace(ctx)
        state(ctx)[key] = t
        if dev:
            d = _dev(np.frombuffer(blob, dtype=np.uint8))
            _on_stream(ctx, second, lambda s: t.update_dev(d.data_ptr(), n, leaf_len, stream=s))
        else:
            t.update_bytes(blob, n, leaf_len)
        proofs = t.gen_proofs(idx)
        return _proof_bytes(t.get_root(), proofs)
    return run


def _merkle_want_of(blob, n, leaf_len, idx):
    root, paths = oracle().merkle(blob, n, leaf_len, idx, chunks=4)
    return root + b"".join(blob[i * leaf_len:(i + 1) * leaf_len] + b"".join(p) for i, p in zip(idx, paths))


def _merkle_want(shape):
    return _merkle_want_of(*_merkle_in(shape, 1))


def _forest_run(ctx, shape, second=False):
    blob, n, leaf_len, idx = _merkle_in(shape, 3)
    f = state(ctx).get("forest") or S.MerkleForest(ctx)
    state(ctx)["forest"] = f
    f.update_bytes(blob, n, leaf_len, 3)
    roots = f.roots()
    return b"".join(_proof_bytes(roots[b], f.gen_proofs(b, idx)) for b in range(3))


def _forest_want(shape):
    blob, n, leaf_len, idx = _merkle_in(shape, 3)
    tb = n * leaf_len
    return b"".join(_merkle_want_of(blob[b * tb:(b + 1) * tb], n, leaf_len, idx) for b in range(3))


# ---- FRI -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fri_in(log_n, deg_div, b=0):
    w = O.root_of_unity(log_n)
    n = 1 << log_n
    return w, oracle().best_fft(O.random_elements(n // deg_div, 7000 + 100 * log_n + b), w, log_n, cpus=4)


def _fri_run(ctx, shape, second=False):
    log_n, excl, deg_div = shape
    w, v = _fri_in(log_n, deg_div)
    return ctx.prove_low_degree(v, w, (1 << log_n) // deg_div, excl).to_json().encode()


@functools.lru_cache(maxsize=None)
def _fri_json(log_n, excl, deg_div, b=0):
    w, v = _fri_in(log_n, deg_div, b)
    return oracle().prove_low_degree_json(v, w, (1 << log_n) // deg_div, excl, chunks=4)


def _fri_want(shape):
    return _fri_json(*shape).encode()


def _fri_batch_run(dev):
    def run(ctx, shape, second=False):
        log_n, batch = shape
        n = 1 << log_n
        vs = np.ascontiguousarray(np.stack([_fri_in(log_n, 4, b)[1] for b in range(batch)]))
        w = O.root_of_unity(log_n)
        if dev:
            d = _dev(vs)
            import torch
            torch.cuda.synchronize()
            proofs = ctx.prove_low_degree_batch_dev(d.data_ptr(), n, batch, w, n // 4, 8)
        else:
            proofs = ctx.prove_low_degree_batch(vs, w, n // 4, 8)
        return b"\n".join(p.to_json().encode() for p in proofs)
    return run


def _fri_batch_want(shape):
    return b"\n".join(_fri_json(shape[0], 8, 4, b).encode() for b in range(shape[1]))


@functools.lru_cache(maxsize=None)
def _fri_verify_in(shape):
    """Three oracle proofs of (log_n, bound, exclusion 8); the middle one's last admissible Last value has one bit
    flipped, which is FAIL_FRI_LAST for it alone (tests/test_gpu_fri_verify_batch.py's table case)."""
    log_n, bound = shape
    w = O.root_of_unity(log_n)
    n = 1 << log_n
    roots, proofs = [], []
    for b in range(3):
        v = oracle().best_fft(O.random_elements(bound, 9000 + 64 * log_n + b), w, log_n, cpus=4)
        roots.append(oracle().merkle(_b(v), n, 32, [], chunks=4)[0])
        proofs.append(json.loads(oracle().prove_low_degree_json(v, w, bound, 8, chunks=4)))
    last = proofs[1][-1]["Last"]["last"]
    at = max(p for p in range(len(last)) if p % 8)
    last[at] = list(bytes(last[at]))
    last[at][1] ^= 2
    return w, roots, proofs


def _fri_verify_run(mode):
    def run(ctx, shape, second=False):
        from stark_amd.verify import verify_low_degree_batch
        w, roots, proofs = _fri_verify_in(shape)
        ctx.set_verify_batch_last(mode)
        try:
            got = verify_low_degree_batch(ctx, roots, w, proofs, shape[1], 8)
        finally:
            ctx.set_verify_batch_last(0)
        return repr(got).encode()
    return run


def _fri_verify_want(shape):
    from stark_amd.verify import FAIL_FRI_LAST
    return repr([(0, 0), (8, FAIL_FRI_LAST), (0, 0)]).encode()


# ---- R1CS ----------------------------------------------------------------------------------------------------------
CIRCUIT = "long_a"   # tests/r1cs_cases.py: os 963, 512 steps, four public wires, long factors


def _read(name, ext):
    with open(os.path.join(FIX, f"{name}.{ext}"), "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def _r1cs_in(name, seed=1):
    """(r1cs, wtns) of the fixture `compute` (one witness) or of a directed case."""
    if name == "compute":
        return _read("compute", "r1cs"), _read("compute", "wtns")
    case = C.CASES[name]
    return case.circuit.r1cs, case.wtns(seed)


@functools.lru_cache(maxsize=None)
def _trace(name, seed=1):
    r1, wt = _r1cs_in(name, seed)
    return R.build_trace(R.read_r1cs(r1), R.read_witness(wt))


@functools.lru_cache(maxsize=None)
def _proof_json(name, seed=1):
    return R.mk_r1cs_proof_json(oracle(), _trace(name, seed))


def _circuit(ctx, name):
    """The case's prepared circuit on this context, prepared by the first call that needs it and kept."""
    from stark_amd.r1cs import R1csCircuit
    st = state(ctx)
    if ("circuit", name) not in st:
        st["circuit", name] = R1csCircuit(ctx, _r1cs_in(name)[0])
    return st["circuit", name]


def _column_min(ctx, m, body):
    ctx.set_public_column_min(m)
    try:
        return body()
    finally:
        ctx.set_public_column_min(0)


def _prove_run(how, column_min=0):
    def run(ctx, name, second=False):
        from stark_amd.r1cs import prove_with_witness, prove_with_witness_host_trace
        r1, wt = _r1cs_in(name)
        call = {"device": lambda: prove_with_witness(ctx, r1, wt),
                "host": lambda: prove_with_witness_host_trace(ctx, r1, wt),
                "circuit": lambda: _circuit(ctx, name).prove(wt)}[how]
        return _column_min(ctx, column_min, lambda: call().to_json().encode())
    return run


def _prove_want(name):
    return _proof_json(name).encode()


def _seeds(name):
    return (1, 1, 1, 1) if name == "compute" else (1, 2, 3, 4)


def _prove_batch_run(column_min=0):
    def run(ctx, name, second=False):
        wts = [_r1cs_in(name, s)[1] for s in _seeds(name)]
        return _column_min(ctx, column_min, lambda: b"\n".join(
            p.to_json().encode() for p in _circuit(ctx, name).prove_batch(wts)))
    return run


def _prove_batch_want(name):
    return b"\n".join(_proof_json(name, s).encode() for s in _seeds(name))


def _idx_tmp_run(ctx, name, second=False):
    """A cache cap of 0: IDX's extension lives in ext_idx_tmp for this proof only, F0's and 1 / Zb3 are made with
    the proof's other columns."""
    from stark_amd.r1cs import prove_with_witness
    r1, wt = _r1cs_in(name)
    ctx.set_cache_limit(0)
    try:
        return prove_with_witness(ctx, r1, wt).to_json().encode()
    finally:
        ctx.set_cache_limit(4 << 30)  # (stark::kDefaultCacheLimit)


@functools.lru_cache(maxsize=None)
def _public_sets(name):
    """[the proof's public wires, wire 1 changed, wire 0 changed] and the restated verifier's verdict on each
    (verify.rs:13-258; wire 0 other than 1 is refused before it, run.rs:480)."""
    from stark_verify import verify_r1cs_proof
    tr = _trace(name)
    pub = list(tr.public_wires)
    sets = [pub]
    for k in (1, 0):
        bad = list(pub)
        bad[k] = (bad[k] + 1) % P
        sets.append(bad)
    verdict = []
    for k, w in enumerate(sets):
        if k == 2:
            verdict.append(False)
            continue
        try:
            verdict.append(bool(verify_r1cs_proof(oracle(), _proof_json(name), w, tr.public_first_indices,
                                                  tr.permuted_indices, tr.coefficients, tr.flag0, tr.flag1, tr.flag2,
                                                  tr.n_constraints, tr.n_wires)))
        except AssertionError:
            verdict.append(False)
    assert verdict[0] and not verdict[2]
    return sets, verdict


def _verify_single_run(ctx, name, second=False):
    """stark_verify_with_witness, then stark_verify_r1cs_bytes on each set of public wires: the verifier's own
    circuit build (verify_arena, verify_lde, spot) every time."""
    from stark_amd.verify import verify_with_witness, verify_with_wtns
    r1, wt = _r1cs_in(name)
    proof = _proof_json(name)
    out = [verify_with_wtns(ctx, r1, wt, proof)]
    for w in _public_sets(name)[0]:
        try:
            out.append(verify_with_witness(ctx, r1, w, proof))
        except AssertionError:
            out.append(False)
    return repr(out).encode()


def _verify_single_want(name):
    return repr([True] + _public_sets(name)[1]).encode()


def _verify_batch_run(handles, transcript):
    def run(ctx, name, second=False):
        from stark_amd.r1cs import StarkProof
        sets, _ = _public_sets(name)
        proof = _proof_json(name)
        proofs = [StarkProof.from_parts(json.loads(proof)) for _ in sets] if handles else [proof] * len(sets)
        ctx.set_verify_batch_transcript(transcript)
        try:
            got = _circuit(ctx, name).verify_batch(sets, proofs)
        finally:
            ctx.set_verify_batch_transcript(0)
        assert got[0] == (0, 0), got
        return repr([s for s, _ in got]).encode()
    return run


def _verify_batch_want(name):
    return repr([0 if ok else 8 for ok in _public_sets(name)[1]]).encode()


CHECK_A, CHECK_B = "long_a", "ragged"


@functools.lru_cache(maxsize=None)
def _check_in(name):
    """Three witnesses, the middle one with a wire raised by one, and R1CS satisfaction in Python integers
    (tests/test_gpu_witness_check.py failing())."""
    case = C.CASES[name]
    c = case.circuit
    def failing(raw):
        rep = []
        for i, fac in enumerate(c.cons):
            a, b, cc = (sum(v * raw[w] for w, v in fc) % P for fc in fac)
            if (a * b - cc) % P:
                rep.append((i, a, b, cc))
        return rep

    raws = [list(C.solve(c, seed, case.values, case.wire0)) for seed in (1, 2, 3)]
    for w in range(c.n_wires // 2, c.n_wires):  # the first wire from the middle on that some constraint reads
        bad = list(raws[1])
        bad[w] = (bad[w] + 1) % P
        if failing(bad):
            raws[1] = bad
            break
    reports = [failing(raw) for raw in raws]
    assert reports[1] and not reports[0] and not reports[2]
    return [C.wtns_bytes(r) for r in raws], reports


def _check_run(ctx, name, second=False):
    ws, _ = _check_in(name)
    got = _circuit(ctx, name).check_batch(ws, max_failures=16)
    return repr([(g.status, g.n_failed, g.failures) for g in got]).encode()


def _check_want(name):
    _, reports = _check_in(name)
    return repr([(8 if r else 0, len(r), r[:16]) for r in reports]).encode()


# ---- the table -----------------------------------------------------------------------------------------------------
class Op:
    def __init__(self, name, a, b, run, want, source, dev=False):
        self.name, self.shapes, self.run, self.source, self.dev = name, {"A": a, "B": b}, run, source, dev
        self._want = want

    @functools.lru_cache(maxsize=None)
    def want(self, which) -> bytes:
        return self._want(self.shapes[which])

    def call(self, ctx, which, second=False) -> bytes:
        return self.run(ctx, self.shapes[which], second and self.dev)


ORACLE, PYTHON = "oracle", "python restatement"

OPS = [
    Op("best_fft", (12, 1000), (5, 32), _fft_run(False), _fft_want(False), ORACLE),
    Op("best_fft_sparse", (12, 1024), (5, 8), _fft_run(False), _fft_want(False), ORACLE),
    Op("inv_best_fft", (12, 4096), (5, 20), _fft_run(True), _fft_want(True), ORACLE),
    Op("ntt_dev", (11, 3), (5, 1), _ntt_dev_run, _ntt_dev_want, ORACLE, dev=True),
    Op("lde", (12, 2), (7, 3), _lde_run, _lde_want, ORACLE),
    # a blow-up beyond the plan's first radix (2^6 and 2^5 here): pad_kernel writes the zero-extended input
    Op("lde_pad", (4, 8), (3, 8), _lde_run, _lde_want, ORACLE),
    Op("lde_dev", (11, 3, 3), (7, 3, 1), _lde_dev_run, _lde_dev_want, ORACLE, dev=True),
    Op("multi_inv", 4097, 257, lambda ctx, n, second=False: _b(ctx.multi_inv(_inv_in(n))),
       lambda n: _b(oracle().multi_inv(_inv_in(n))), ORACLE),
    Op("multi_interp_4", 1000, 40, lambda ctx, r, second=False: _b(ctx.multi_interp_4(*_interp4_in(r))),
       lambda r: _b(oracle().multi_interp_4(*_interp4_in(r))), ORACLE),
    Op("eval_quartic_multi", 333, 40,
       lambda ctx, n, second=False: _b(ctx.eval_quartic_multi(_coeffs(4 * n, 91 + n), _coeffs(n, 92 + n))),
       lambda n: _b(oracle().eval_quartic_multi(_coeffs(4 * n, 91 + n), _coeffs(n, 92 + n))), ORACLE),
    Op("lincomb", (9, 4096), (1, 10), lambda ctx, s, second=False: _b(ctx.lincomb(*_lincomb_in(s))), _lincomb_want,
       PYTHON),
    Op("eval_poly_at_multi", (5000, 37), (100, 5),
       lambda ctx, s, second=False: _b(ctx.eval_poly_at_multi(*_mp_in(s))), _mp_want, ORACLE),
    Op("multipoint_tree", (129, 3 * 256 + 7), (33, 33), _mp_run(1), _mp_want, ORACLE),
    Op("multipoint_tree_dev", (129, 3 * 256 + 7), (33, 33), _mp_dev_run, _mp_want, ORACLE, dev=True),
    Op("multipoint_split", (3, 65539), (80, 4097), _mp_run(NEVER), _mp_want, ORACLE),
    Op("zpoly", 257, 33, lambda ctx, n, second=False: _b(ctx.zpoly(limbs(_points(n, 1000 + n, True)))),
       lambda n: _b(limbs(py_zpoly(_points(n, 1000 + n, True)))), PYTHON),
    Op("lagrange_interp_tree", 257, 33, _lagrange_run(1), _lagrange_want, PYTHON),
    Op("lagrange_interp_horner", 257, 33, _lagrange_run(NEVER), _lagrange_want, PYTHON),
    Op("lagrange_interp_domain", 257, 33, _lagrange_domain_run, _lagrange_domain_want, PYTHON),
    Op("mul_polys", (8, 256, 256), (6, 20, 17),
       lambda ctx, s, second=False: _b(ctx.mul_polys(*_mul_in(s), O.root_of_unity(s[0]), s[0])), _mul_want, PYTHON),
    Op("div_polys", 8, 4,
       lambda ctx, k, second=False: _b(ctx.div_polys(_div_in(k)[0], _div_in(k)[1], O.root_of_unity(k), k)),
       lambda k: _b(_div_in(k)[2]), PYTHON),
    Op("divrem_polys", (257, 129), (6, 3), _divrem_run, _divrem_want, PYTHON),
    Op("interp_plan", 257, 33, _interp_plan_run(False), _interp_plan_want, PYTHON),
    Op("interp_plan_dev", 257, 33, _interp_plan_run(True), _interp_plan_want, PYTHON, dev=True),
    Op("eval_plan", 600, 100, _eval_plan_run(False), _eval_plan_want, ORACLE),
    Op("eval_plan_dev", 600, 100, _eval_plan_run(True), _eval_plan_want, ORACLE, dev=True),
    Op("merkle_33", (12, 33), (5, 40), _merkle_run(False), _merkle_want, ORACLE),
    Op("merkle_256", (9, 256), (5, 40), _merkle_run(False), _merkle_want, ORACLE),
    Op("merkle_dev", (12, 33), (9, 256), _merkle_run(True), _merkle_want, ORACLE, dev=True),
    Op("forest_33", (12, 33), (5, 40), _forest_run, _forest_want, ORACLE),
    Op("forest_256", (9, 256), (5, 40), _forest_run, _forest_want, ORACLE),
    Op("prove_low_degree", (12, 8, 4), (7, 8, 4), _fri_run, _fri_want, ORACLE),
    Op("prove_low_degree_excl2", (10, 2, 4), (7, 8, 4), _fri_run, _fri_want, ORACLE),
    Op("prove_low_degree_batch", (10, 3), (7, 2), _fri_batch_run(False), _fri_batch_want, ORACLE),
    # (a device entry, but not dev=True: stark_prove_low_degree_batch_dev takes no stream, it runs on the context's)
    Op("prove_low_degree_batch_dev", (10, 3), (7, 2), _fri_batch_run(True), _fri_batch_want, ORACLE),
    Op("verify_low_degree_batch_host_last", (12, 16), (7, 32), _fri_verify_run(1), _fri_verify_want, ORACLE),
    Op("verify_low_degree_batch_device_last", (12, 16), (7, 32), _fri_verify_run(2), _fri_verify_want, ORACLE),
    Op("prove_with_witness", CIRCUIT, "compute", _prove_run("device"), _prove_want, ORACLE),
    Op("prove_with_witness_host_trace", CIRCUIT, "compute", _prove_run("host"), _prove_want, ORACLE),
    Op("circuit_prove", CIRCUIT, "compute", _prove_run("circuit"), _prove_want, ORACLE),
    Op("prove_batch", CIRCUIT, "compute", _prove_batch_run(), _prove_batch_want, ORACLE),
    Op("prove_public_column", CIRCUIT, "compute", _prove_run("device", 1), _prove_want, ORACLE),
    Op("circuit_prove_public_column", CIRCUIT, "compute", _prove_run("circuit", 1), _prove_want, ORACLE),
    Op("prove_batch_public_column", CIRCUIT, "compute", _prove_batch_run(1), _prove_batch_want, ORACLE),
    Op("prove_idx_tmp", CIRCUIT, "compute", _idx_tmp_run, _prove_want, ORACLE),
    Op("verify_with_wtns", CIRCUIT, "compute", _verify_single_run, _verify_single_want, ORACLE),
    Op("verify_batch_texts_host_transcript", CIRCUIT, "compute", _verify_batch_run(False, 1), _verify_batch_want,
       ORACLE),
    Op("verify_batch_texts_device_transcript", CIRCUIT, "compute", _verify_batch_run(False, 2), _verify_batch_want,
       ORACLE),
    Op("verify_batch_handles_host_transcript", CIRCUIT, "compute", _verify_batch_run(True, 1), _verify_batch_want,
       ORACLE),
    Op("verify_batch_handles_device_transcript", CIRCUIT, "compute", _verify_batch_run(True, 2), _verify_batch_want,
       ORACLE),
    Op("check_batch", CHECK_A, CHECK_B, _check_run, _check_want, PYTHON),
]

BY_NAME = {op.name: op for op in OPS}
assert len(BY_NAME) == len(OPS)
