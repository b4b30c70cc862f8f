"""A/B of the two routes for the public points (stark_ctx_set_public_column_min), and the no-regression A/B
against another build of the library, in one process:

    python tools/public_inputs_ab.py [--parent other/libstark_hip.so] [--reps 10] [--out profiles/public_column_ab.txt]

Threshold.  Synthetic circuits (tools/synth_r1cs.py, n_public) of 2^13 and 2^17 steps with m = 8, 32, 128,
   1,024 and 8,192 boundary points (m < steps): stark_prove_r1cs_bytes and stark_verify_with_witness with the
   column route (threshold 1) and the Horner route (SIZE_MAX) alternating, each route as two interleaved
   series of --reps calls.  A route's time is the median over both series; the spread is the largest
   difference between the medians of two series of one route (the same code, the same inputs).  The column
   route wins at m when Horner's median exceeds its by more than three spreads; the default threshold is the
   smallest such m.
Regression, run first (--parent: the library of the commit before the column route).  compute, poseidon3_test,
   pedersen_test and the 2^17-step two-public-wire circuit, which stay on the Horner route under the default
   threshold: this build against the other one and a second context of the other one (the control: two
   contexts of one build differ by more than two series of one context), alternating, two series each, on
   fresh contexts; within three spreads or not.

Both libraries are called through ctypes directly (two builds cannot share stark_amd's one loaded library)."""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "stark-pure-rust_amd"), os.path.join(ROOT, "tools")]
FIX = os.path.join(ROOT, "tests", "golden", "r1cs")
NEVER = ctypes.c_size_t(-1).value
_vp = ctypes.c_void_p


class Lib:
    """One build of libstark_hip.so with one context."""

    def __init__(self, path):
        self.lib = ctypes.CDLL(os.path.abspath(path))
        L = self.lib
        L.stark_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(_vp)]
        L.stark_ctx_destroy.argtypes = [_vp]
        L.stark_prove_r1cs_bytes.argtypes = [_vp, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                             ctypes.POINTER(_vp)]
        L.stark_r1cs_proof_json_view.argtypes = [_vp, ctypes.POINTER(_vp), ctypes.POINTER(ctypes.c_size_t)]
        L.stark_r1cs_proof_free.argtypes = [_vp]
        L.stark_verify_with_witness.argtypes = [_vp, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                                ctypes.c_char_p, ctypes.c_size_t]
        self.ctx = _vp()
        rc = L.stark_ctx_create(0, ctypes.byref(self.ctx))
        if rc:
            raise RuntimeError(f"{path}: stark_ctx_create = {rc}")
        if hasattr(L, "stark_ctx_set_public_column_min"):
            L.stark_ctx_set_public_column_min.argtypes = [_vp, ctypes.c_size_t]

    def close(self):
        self.lib.stark_ctx_destroy(self.ctx)

    def route(self, m):
        rc = self.lib.stark_ctx_set_public_column_min(self.ctx, m)
        assert rc == 0, rc

    def prove(self, r1, wt):
        """The proof's JSON text (the call's time is the caller's to take)."""
        h = _vp()
        rc = self.lib.stark_prove_r1cs_bytes(self.ctx, r1, len(r1), wt, len(wt), ctypes.byref(h))
        if rc:
            raise RuntimeError(f"stark_prove_r1cs_bytes = {rc}")
        p, n = _vp(), ctypes.c_size_t()
        self.lib.stark_r1cs_proof_json_view(h, ctypes.byref(p), ctypes.byref(n))
        js = ctypes.string_at(p.value, n.value)
        self.lib.stark_r1cs_proof_free(h)
        return js

    def time_prove(self, r1, wt):
        h = _vp()
        t = time.perf_counter()
        rc = self.lib.stark_prove_r1cs_bytes(self.ctx, r1, len(r1), wt, len(wt), ctypes.byref(h))
        dt = time.perf_counter() - t
        if rc:
            raise RuntimeError(f"stark_prove_r1cs_bytes = {rc}")
        self.lib.stark_r1cs_proof_free(h)
        return dt

    def time_verify(self, r1, wt, js):
        t = time.perf_counter()
        rc = self.lib.stark_verify_with_witness(self.ctx, r1, len(r1), wt, len(wt), js, len(js))
        dt = time.perf_counter() - t
        if rc:
            raise RuntimeError(f"stark_verify_with_witness = {rc}")
        return dt


def series(variants, reps, warm=2):
    """variants: name -> a call returning seconds.  Each runs as two series, all interleaved
    (a b a' b' b a b' a' ...: the order rotates); returns name -> (median over both in ms, |median - median'| in ms)."""
    for f in variants.values():
        for _ in range(warm):
            f()
    ts = {k: ([], []) for k in variants}
    order = list(variants.items())
    for _ in range(reps):
        for half in (0, 1):
            for k, f in order:
                ts[k][half].append(f() * 1e3)
            order = order[1:] + order[:1]  # every variant follows every other equally often
    return {k: (statistics.median(a + b), abs(statistics.median(a) - statistics.median(b))) for k, (a, b) in ts.items()}


def fixture(name):
    return open(f"{FIX}/{name}.r1cs", "rb").read(), open(f"{FIX}/{name}.wtns", "rb").read()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "stark-pure-rust_amd", "libstark_hip.so"))
    ap.add_argument("--parent", default="")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--log-steps", type=int, nargs="*", default=[13, 17])
    ap.add_argument("--points", type=int, nargs="*", default=[8, 32, 128, 1024, 8192])
    a = ap.parse_args()
    import synth_r1cs
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    new = None
    if a.parent:
        # This build between two contexts of the parent, made in that order: when a context was made counts
        # (a context made after another one of the process was destroyed measured 0.1-0.2 ms slower per
        # proof, whatever the build; hence first in the process, and the control on both sides).
        old, new, ctl = Lib(a.parent), Lib(a.lib), Lib(a.parent)
        say(f"# no regression below the threshold: this build (default threshold) against {os.path.basename(a.parent)},")
        say(f"# alternating in one process, {a.reps} calls per series, two series per context, ms; parent' = a second")
        say("# context of the parent build; spread = the largest difference between two series of one context or")
        say("# between the parent's two contexts")
        say("%16s %10s %10s %10s %8s %12s %22s" % ("circuit", "this", "parent", "parent'", "spread", "this-parent", "verdict"))
        cases = [(n, fixture(n)) for n in ("compute", "poseidon3_test", "pedersen_test")]
        cases.append(("synthetic 2^17", synth_r1cs.for_steps(17)))
        for name, (r1, wt) in cases:
            if not new.prove(r1, wt) == old.prove(r1, wt) == ctl.prove(r1, wt):
                raise RuntimeError(f"{name}: the two builds' proofs differ")
            res = series({"parent": lambda: old.time_prove(r1, wt), "this": lambda: new.time_prove(r1, wt),
                          "control": lambda: ctl.time_prove(r1, wt)}, a.reps)
            spread = max(res["this"][1], res["parent"][1], res["control"][1], abs(res["parent"][0] - res["control"][0]))
            diff = res["this"][0] - res["parent"][0]
            verdict = "within three spreads" if abs(diff) <= 3 * spread else ("slower" if diff > 0 else "faster")
            say(f"{name:>16} {res['this'][0]:>10.3f} {res['parent'][0]:>10.3f} {res['control'][0]:>10.3f} "
                f"{spread:>8.3f} {diff:>12.3f} {verdict:>22}")
        old.close()
        ctl.close()
        say()
    new = new or Lib(a.lib)
    wins = {}
    if a.log_steps and a.points:
        say(f"# public points: column route against Horner route, {a.reps} calls per series, two series per route, ms")
        say("# (median over both series; spread = the larger difference between a route's two series' medians)")
        say(f"{'steps':>6} {'m':>6} {'call':>7} {'column':>10} {'horner':>10} {'spread':>8} {'horner-column':>14} "
            f"{'verdict':>10}")
    for ls in a.log_steps:
        for m in a.points:
            if m >= 1 << ls or m < 3:
                continue
            r1, wt = synth_r1cs.for_steps(ls, n_public=m - 1)
            new.route(1)
            js = new.prove(r1, wt)
            new.route(NEVER)
            if new.prove(r1, wt) != js:
                raise RuntimeError(f"2^{ls} steps, m = {m}: the two routes' proofs differ")

            def timed(route, call):
                def f():
                    new.route(route)
                    return call()
                return f
            for what, call in (("prove", lambda: new.time_prove(r1, wt)), ("verify", lambda: new.time_verify(r1, wt, js))):
                res = series({"column": timed(1, call), "horner": timed(NEVER, call)}, a.reps)
                spread = max(res["column"][1], res["horner"][1])
                gain = res["horner"][0] - res["column"][0]
                verdict = "column" if gain > 3 * spread else ("horner" if -gain > 3 * spread else "tie")
                if what == "prove":
                    wins.setdefault(m, []).append(verdict == "column")
                say(f"{'2^%d' % ls:>6} {m:>6} {what:>7} {res['column'][0]:>10.3f} {res['horner'][0]:>10.3f} {spread:>8.3f} "
                    f"{gain:>14.3f} {verdict:>10}")
    always = sorted(m for m, w in wins.items() if all(w))
    # the smallest m from which the column route wins at every size measured, and at every larger m
    best = None
    for m in reversed(sorted(wins)):
        if m in always:
            best = m
        else:
            break
    if wins:
        say(f"# smallest m from which the column route wins the proof at every size measured: {best}")
        new.route(0)
    new.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
