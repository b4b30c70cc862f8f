"""A/B of the interpolation plans (ABI 11) against the parent commit's library, both loaded into one process
through tools/ab_libs.py's bind (own ctypes handle, own context each), in alternating rounds:

    python tools/interp_batch_ab.py parent.so this.so [--reps 10] [--out profiles/interp_batch_ab.txt]

Cases, ms per proof (or per interpolated vector):
  prove     stark_prove_r1cs_circuit_batch on `bits` (B = 8, 2) and on a synthetic circuit of 2^13 steps with 1,024
            public wires (B = 16, 2), default thresholds: the column route's I2 coefficients per witness (parent)
            against one plan application (this build);
  verify    stark_verify_r1cs_circuit_batch_proofs on `bits` (B = 8, 2; 1,062 points, above the verification
            threshold) and on `compute` at B = 64 with stark_ctx_set_public_column_min(2): verify_interp2 per proof
            (parent) against one plan application;
  interp    B calls of stark_lagrange_interp over one point set (both builds: the parent's form) against one
            stark_lagrange_interp_batch (this build only), n = 1,024, B = 16 and 64; the row of the B calls in
            this build is a control (the single entry is unchanged) and carries no verdict.

Every case runs its forms as two interleaved series of --reps rounds, the order rotating: a form's time is the
median over both series, its spread the difference between the medians of its two series.  The new form wins a
case when it is lower per proof than the parent's by more than three times the parent build's own spread.  Before
any timing the proofs' JSON digests, the verdicts and the interpolants must be equal across the builds; the tool
stops otherwise."""
import argparse
import ctypes
import hashlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")]
FIX = os.path.join(ROOT, "tests", "golden", "r1cs")

vp, u64p, szp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_size_t)


def series(variants, reps):
    """tools/verify_batch_ab.py's scheme: name -> (median over both series in ms, |median - median'|)."""
    ts = {k: ([], []) for k in variants}
    order = list(variants.items())
    for _ in range(reps):
        for half in (0, 1):
            for k, f in order:
                t = time.perf_counter()
                f()
                ts[k][half].append((time.perf_counter() - t) * 1e3)
            order = order[1:] + order[:1]
    return {k: (statistics.median(a + b), abs(statistics.median(a) - statistics.median(b))) for k, (a, b) in ts.items()}


class Build:
    def __init__(self, path):
        from ab_libs import bind
        self.lib, self.h = bind(path)
        self.new = hasattr(self.lib, "stark_lagrange_interp_batch")
        L = self.lib
        L.stark_r1cs_circuit_new.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(vp)]
        L.stark_r1cs_circuit_free.argtypes = [vp]
        L.stark_r1cs_circuit_free.restype = None
        L.stark_prove_r1cs_circuit_batch.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_char_p), szp, ctypes.c_uint32,
                                                     ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_int)]
        L.stark_r1cs_proof_json_view.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), szp]
        L.stark_r1cs_proof_free.argtypes = [vp]
        L.stark_r1cs_proof_free.restype = None
        L.stark_verify_r1cs_circuit_batch_proofs.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_char_p), ctypes.c_size_t,
                                                             ctypes.POINTER(vp), ctypes.c_uint32,
                                                             ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint32)]
        L.stark_ctx_set_public_column_min.argtypes = [vp, ctypes.c_size_t]
        L.stark_lagrange_interp.argtypes = [vp, u64p, u64p, ctypes.c_size_t, u64p]
        if self.new:
            L.stark_lagrange_interp_batch.argtypes = [vp, u64p, u64p, ctypes.c_size_t, ctypes.c_uint32, u64p]

    def circuit(self, r1):
        c = vp()
        assert self.lib.stark_r1cs_circuit_new(self.h, r1, len(r1), ctypes.byref(c)) == 0
        return c

    def prove_batch(self, c, wts):
        """The handles (the caller frees them)."""
        n = len(wts)
        ptrs = (ctypes.c_char_p * n)(*wts)
        lens = (ctypes.c_size_t * n)(*[len(w) for w in wts])
        out, sts = (vp * n)(), (ctypes.c_int * n)()
        assert self.lib.stark_prove_r1cs_circuit_batch(self.h, c, ptrs, lens, n, out, sts) == 0 and not any(sts)
        return [vp(h) for h in out]

    def digest(self, proof):
        p, n = ctypes.c_char_p(), ctypes.c_size_t()
        assert self.lib.stark_r1cs_proof_json_view(proof, ctypes.byref(p), ctypes.byref(n)) == 0
        return hashlib.sha256(ctypes.string_at(p, n.value)).hexdigest()[:16]

    def free(self, proofs):
        for p in proofs:
            self.lib.stark_r1cs_proof_free(p)

    def verify_batch(self, c, pub, proofs):
        n = len(proofs)
        pubs = (ctypes.c_char_p * n)(*[pub] * n)
        hs = (vp * n)(*[p.value for p in proofs])
        sts, why = (ctypes.c_int * n)(), (ctypes.c_uint32 * n)()
        rc = self.lib.stark_verify_r1cs_circuit_batch_proofs(self.h, c, pubs, len(pub) // 32, hs, n, sts, why)
        return [rc] + list(sts) + list(why)


def fixture(name):
    with open(os.path.join(FIX, name + ".r1cs"), "rb") as f:
        r1 = f.read()
    with open(os.path.join(FIX, name + ".wtns"), "rb") as f:
        return r1, f.read()


def public_bytes(r1, wt):
    import r1cs as R
    h = R.read_r1cs(r1).header
    return b"".join(bytes(w).ljust(32, b"\0") for w in R.read_witness(wt)[:1 + h.n_public_inputs + h.n_public_outputs])


def report(say, what, batch, res, old, new, control=False):
    """control: the row compares unchanged code in the two builds (no plan runs): it carries no verdict."""
    per = {k: (v[0] / batch, v[1] / batch) for k, v in res.items()}
    gain, bar = per[old][0] - per[new][0], 3 * per[old][1]
    verdict = "control" if control else "plan" if gain > bar else ("parent" if -gain > bar else "tie")
    say(f"{what:>28} {batch:>3} {per[old][0]:>12.4f} {per[old][1]:>9.4f} {per[new][0]:>12.4f} {per[new][1]:>9.4f} "
        f"{gain:>9.4f} {bar:>9.4f} {per[old][0] / per[new][0]:>6.2f} {verdict:>7}")


def main():
    import synth_r1cs
    import oracle as O
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("this")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    old, new = Build(a.parent), Build(a.this)
    assert new.new and not old.new, "usage: parent.so this.so"
    say("# interpolation plans against the parent commit's library, one process, alternating rounds; ms per proof:")
    say("# median over two interleaved series of `reps` rounds per build; spread = the difference between the medians")
    say("# of a build's two series; the plan wins when parent - this exceeds three times the parent's spread")
    say(f"# reps {a.reps}")
    say()
    say(f"{'case':>28} {'B':>3} {'parent/proof':>12} {'(spread)':>9} {'this/proof':>12} {'(spread)':>9} {'gain':>9} "
        f"{'3 spread':>9} {'ratio':>6} {'verdict':>7}")
    circuits = {"bits": fixture("bits"), "synth13x1024": synth_r1cs.for_steps(13, n_public=1024),
                "compute": fixture("compute")}
    for name, sizes in (("bits", (8, 2)), ("synth13x1024", (16, 2))):
        r1, wt = circuits[name]
        co, cn = old.circuit(r1), new.circuit(r1)
        for batch in sizes:
            po, pn = old.prove_batch(co, [wt] * batch), new.prove_batch(cn, [wt] * batch)  # warm, and the digests
            do, dn = [old.digest(p) for p in po], [new.digest(p) for p in pn]
            old.free(po)
            new.free(pn)
            assert do == dn and len(set(do)) == 1, f"{name}: JSON digests differ"
            res = series({"parent": lambda: old.free(old.prove_batch(co, [wt] * batch)),
                          "this": lambda: new.free(new.prove_batch(cn, [wt] * batch))}, a.reps)
            report(say, f"prove_batch {name}", batch, res, "parent", "this")
        if name == "bits":
            pub = public_bytes(r1, wt)
            for batch in sizes:
                po, pn = old.prove_batch(co, [wt] * batch), new.prove_batch(cn, [wt] * batch)
                vo, vn = old.verify_batch(co, pub, po), new.verify_batch(cn, pub, pn)
                assert vo == vn and not any(vo), f"{name}: verdicts differ or a proof is refused"
                res = series({"parent": lambda: old.verify_batch(co, pub, po),
                              "this": lambda: new.verify_batch(cn, pub, pn)}, a.reps)
                report(say, f"verify_batch handles {name}", batch, res, "parent", "this")
                old.free(po)
                new.free(pn)
        old.lib.stark_r1cs_circuit_free(co)
        new.lib.stark_r1cs_circuit_free(cn)
    r1, wt = circuits["compute"]
    co, cn, pub = old.circuit(r1), new.circuit(r1), public_bytes(r1, wt)
    for b in (old, new):
        b.lib.stark_ctx_set_public_column_min(b.h, 2)
    po, pn = old.prove_batch(co, [wt] * 64), new.prove_batch(cn, [wt] * 64)
    vo, vn = old.verify_batch(co, pub, po), new.verify_batch(cn, pub, pn)
    assert vo == vn and not any(vo), "compute: verdicts differ or a proof is refused"
    res = series({"parent": lambda: old.verify_batch(co, pub, po), "this": lambda: new.verify_batch(cn, pub, pn)}, a.reps)
    report(say, "verify_batch compute, min 2", 64, res, "parent", "this")
    old.free(po)
    new.free(pn)
    for b, c in ((old, co), (new, cn)):
        b.lib.stark_ctx_set_public_column_min(b.h, 0)
        b.lib.stark_r1cs_circuit_free(c)
    n = 1024
    xs = O.random_elements(n, 0x1A7E)
    p64 = lambda arr: arr.ctypes.data_as(u64p)
    for batch in (16, 64):
        ys = np.ascontiguousarray(O.random_elements(batch * n, 0x1A7F + batch)).reshape(batch, n, 4)
        outs = {k: np.empty_like(ys) for k in ("parent", "this", "plan")}

        def loop(b, out):
            for i in range(batch):
                assert b.lib.stark_lagrange_interp(b.h, p64(xs), p64(ys[i]), n, p64(out[i])) == 0

        def plan():
            assert new.lib.stark_lagrange_interp_batch(new.h, p64(xs), p64(ys), n, batch, p64(outs["plan"])) == 0

        forms = {"parent": lambda: loop(old, outs["parent"]), "this": lambda: loop(new, outs["this"]), "plan": plan}
        for f in forms.values():
            f()
        assert outs["parent"].tobytes() == outs["this"].tobytes() == outs["plan"].tobytes(), "interpolants differ"
        res = series(forms, a.reps)
        report(say, f"B x lagrange_interp (this build), n {n}", batch, res, "parent", "this", control=True)
        report(say, f"lagrange_interp_batch, n {n}", batch, res, "parent", "plan")
    say()
    say("# equal across the builds before every timed case: the proofs' JSON digests, the verdicts (all accepted),")
    say("# the interpolants' bytes")


if __name__ == "__main__":
    main()
