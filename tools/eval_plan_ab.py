"""A/B of the evaluation plans (ABI 14) against the parent commit's library, both loaded into one process through
tools/ab_libs.py's bind (own ctypes handle, own context each), in alternating rounds:

    python tools/eval_plan_ab.py parent.so this.so [--reps 10] [--out profiles/eval_plan_ab.txt]

Per shape (n points, deg+1 coefficients; the shapes of profiles/multipoint_eval_ab.txt) and batch B in {1, 16, 64},
ms per polynomial, host buffers in and out in every form:
  parent    B calls of stark_eval_poly_multipoint, default routing, in the parent's library;
  this      the same B calls in this build: a control (the single entry is unchanged), no verdict;
  plan      one stark_eval_plan_apply of B polynomials on a plan built before the timed rounds
            (max_deg_plus_1 = deg+1).
The `_dev` rows are the same three forms on device-resident coefficients and values (stark_eval_poly_multipoint_dev,
stark_eval_plan_apply_dev), each ended by stark_ctx_synchronize: what the launch chains cost without the staging
copies, which at 2^20 coefficients (32 MiB a polynomial) are most of a host-buffer call.
The plan's build (stark_eval_plan_new .. stark_eval_plan_free, which ends synchronised) is timed on its own: the
median of five.

Every case runs its forms as two interleaved series of --reps rounds, the order rotating: a form's time is the
median over both series, its spread the difference between the medians of its two series.  The plan wins a case
when it is lower per polynomial than the parent's B calls by more than three times the parent build's own spread,
and loses when it is higher by as much.  Before any timing the values must be equal across the three forms; the
tool stops otherwise."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")]

vp, u64p, sz, u32 = ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t, ctypes.c_uint32
SHAPES = [(80, 1 << 20), (1024, 1024), (1024, 1 << 20), (8192, 1 << 17), (65536, 1 << 13), (65536, 1 << 20)]
BATCHES = [1, 16, 64]


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
        self.new = hasattr(self.lib, "stark_eval_plan_new")
        L = self.lib
        L.stark_eval_poly_multipoint.argtypes = [vp, u64p, sz, u64p, sz, u64p]
        L.stark_eval_poly_multipoint_dev.argtypes = [vp, vp, sz, vp, sz, vp, vp]
        L.stark_ctx_synchronize.argtypes = [vp]
        if self.new:
            L.stark_eval_plan_new.argtypes = [vp, u64p, sz, sz, ctypes.POINTER(vp)]
            L.stark_eval_plan_free.argtypes = [vp]
            L.stark_eval_plan_apply.argtypes = [vp, u64p, sz, u32, u64p]
            L.stark_eval_plan_apply_dev.argtypes = [vp, vp, sz, sz, u32, vp, sz, vp]


def p64(arr):
    return arr.ctypes.data_as(u64p)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def report(say, n, d, batch, res, old, new, control=False, dev=False):
    """control: the row compares unchanged code in the two builds (no plan runs): it carries no verdict."""
    per = {k: (v[0] / batch, v[1] / batch) for k, v in res.items()}
    gain, bar = per[old][0] - per[new][0], 3 * per[old][1]
    verdict = "control" if control else "plan" if gain > bar else ("parent" if -gain > bar else "tie")
    say(f"{n:>6} {d:>8} {batch:>3} {new + ('_dev' if dev else ''):>8} {per[old][0]:>12.4f} {per[old][1]:>9.4f} {per[new][0]:>12.4f} "
        f"{per[new][1]:>9.4f} {gain:>9.4f} {bar:>9.4f} {per[old][0] / per[new][0]:>7.2f} {verdict:>7}")


def main():
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
    say("# evaluation plans against B single stark_eval_poly_multipoint calls (default routing) of the parent commit's")
    say("# library, one process, alternating rounds; host buffers in and out; ms per polynomial: median over two")
    say("# interleaved series of `reps` rounds per form; spread = the difference between the medians of a form's two")
    say("# series; the plan wins when parent - plan exceeds three times the parent's spread, loses when plan - parent does;")
    say("# `this` rows: the same B single calls in this build (a control: the single entry is unchanged);")
    say("# `_dev` rows: the device-resident forms of the three, each ended by the context's synchronise (no staging)")
    say(f"# reps {a.reps}")
    say()
    say(f"{'n':>6} {'deg+1':>8} {'B':>3} {'form':>8} {'parent/poly':>12} {'(spread)':>9} {'form/poly':>12} {'(spread)':>9} "
        f"{'gain':>9} {'3 spread':>9} {'ratio':>7} {'verdict':>7}")
    builds = []
    for n, d in SHAPES:
        xs = O.random_elements(n, 0xE7A1 + n)
        base = O.random_elements(d + max(BATCHES), 0xE7A2 + d)
        plan = vp()
        assert new.lib.stark_eval_plan_new(new.h, p64(xs), n, d, ctypes.byref(plan)) == 0
        for batch in BATCHES:
            polys = np.ascontiguousarray(np.stack([base[b:b + d] for b in range(batch)]))  # polynomial b: a window
            outs = {k: np.empty((batch, n, 4), dtype=np.uint64) for k in ("parent", "this", "plan")}

            def loop(b, out):
                for i in range(batch):
                    assert b.lib.stark_eval_poly_multipoint(b.h, p64(polys[i]), d, p64(xs), n, p64(out[i])) == 0

            def apply():
                assert new.lib.stark_eval_plan_apply(plan, p64(polys), d, batch, p64(outs["plan"])) == 0

            forms = {"parent": lambda: loop(old, outs["parent"]), "this": lambda: loop(new, outs["this"]), "plan": apply}
            for f in forms.values():  # warm, and the values
                f()
            assert outs["parent"].tobytes() == outs["this"].tobytes() == outs["plan"].tobytes(), "values differ"
            res = series(forms, a.reps)
            report(say, n, d, batch, res, "parent", "this", control=True)
            report(say, n, d, batch, res, "parent", "plan")
            # the device-resident forms, each ended by its context's synchronise: no staging in any of them
            d_xs, d_polys = dev(xs), dev(polys)
            d_outs = {k: torch.zeros(batch * n * 32, dtype=torch.uint8, device="cuda") for k in ("parent", "this", "plan")}
            torch.cuda.synchronize()

            def loop_dev(b, out):
                for i in range(batch):
                    assert b.lib.stark_eval_poly_multipoint_dev(b.h, d_polys.data_ptr() + 32 * d * i, d, d_xs.data_ptr(),
                                                                n, out.data_ptr() + 32 * n * i, None) == 0
                assert b.lib.stark_ctx_synchronize(b.h) == 0

            def apply_dev():
                assert new.lib.stark_eval_plan_apply_dev(plan, d_polys.data_ptr(), d, d, batch, d_outs["plan"].data_ptr(),
                                                         n, None) == 0
                assert new.lib.stark_ctx_synchronize(new.h) == 0

            forms = {"parent": lambda: loop_dev(old, d_outs["parent"]), "this": lambda: loop_dev(new, d_outs["this"]),
                     "plan": apply_dev}
            for f in forms.values():
                f()
            for k, t in d_outs.items():
                assert t.cpu().numpy().tobytes() == outs["parent"].tobytes(), f"device form {k}: values differ"
            res = series(forms, a.reps)
            report(say, n, d, batch, res, "parent", "this", control=True, dev=True)
            report(say, n, d, batch, res, "parent", "plan", dev=True)
            del d_xs, d_polys, d_outs
        assert new.lib.stark_eval_plan_free(plan) == 0
        ts = []
        for _ in range(5):
            t = time.perf_counter()
            assert new.lib.stark_eval_plan_new(new.h, p64(xs), n, d, ctypes.byref(plan)) == 0
            ts.append((time.perf_counter() - t) * 1e3)
            assert new.lib.stark_eval_plan_free(plan) == 0
        builds.append((n, d, statistics.median(ts), max(ts) - min(ts)))
    say()
    say("# the plan's build (stark_eval_plan_new, ends synchronised), outside the rounds above; ms, median of five")
    say("# (max - min)")
    for n, d, med, spread in builds:
        say(f"# build {n:>6} {d:>8} {med:>10.3f} ({spread:.3f})")
    say()
    say("# equal across the three forms before every timed case: the values' bytes")
    for b in (old, new):
        b.lib.stark_ctx_destroy(b.h)


if __name__ == "__main__":
    main()
