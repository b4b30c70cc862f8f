"""A/B of the three multi-point evaluation routes in one process, alternating:

    python tools/multipoint_ab.py [--reps 10] [--shape-limit 60] [--out profiles/multipoint_eval_ab.txt]

horner   stark_eval_poly_at_multi: the untouched kernel, one thread per point (the yardstick: the code of the
         commit before the other two existed);
split    stark_eval_poly_multipoint with the tree switched off (threshold SIZE_MAX);
tree     stark_eval_poly_multipoint with the tree forced (threshold 1).

Every shape (n points, deg_plus_1 coefficients) runs each route as two interleaved series of --reps host-buffer
calls (tools/public_inputs_ab.py's scheme): a route's time is the median over both series, the spread the larger
difference between the medians of two series of one route.  The tree wins a shape when the split Horner's median
exceeds its by more than three spreads.  The default threshold is the smallest measured min(n, deg_plus_1) from
which the tree wins every measured shape; none: "never".  A shape whose calls would take longer than
--shape-limit seconds runs fewer calls per series (the column `reps` says how many).  The three routes' values
are compared first; the tool stops at the first difference or error.

Then lagrange_interp at --interp-points (8,192) arbitrary points with the descent on and off, and divrem_polys at
(2^20, 2^19).  An empty --points skips the table and runs these two alone."""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "stark-pure-rust_amd"), os.path.join(ROOT, "oracle")]

import numpy as np  # noqa: E402


def series(variants, reps, warm=1):
    """variants: name -> a call.  Two series each, all interleaved, the order rotating; returns
    name -> (median over both in ms, |median - median'| in ms)."""
    for f in variants.values():
        for _ in range(warm):
            f()
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shape-limit", type=float, default=60.0, help="seconds of calls per shape")
    ap.add_argument("--points", type=int, nargs="*", default=[80, 256, 1024, 8192, 65536])
    ap.add_argument("--log-deg", type=int, nargs="*", default=[10, 13, 17, 20])
    ap.add_argument("--interp-points", type=int, nargs="*", default=[8192])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import oracle as O
    import stark_amd as S
    ctx = S.Context(0)
    never = S.Context.MULTIPOINT_TREE_NEVER
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    def routed(m, call):
        def f():
            ctx.set_multipoint_tree_min(m)
            return call()
        return f

    if a.points and a.log_deg:
        say("# multi-point evaluation, host-buffer calls, ms: median over two interleaved series of `reps` calls per route;")
        say("# spread = the largest difference between the medians of two series of one route; the tree wins when")
        say("# split - tree exceeds three spreads")
        say(f"{'n':>6} {'deg+1':>8} {'reps':>4} {'horner':>11} {'split':>11} {'tree':>11} {'spread':>8} "
            f"{'split-tree':>11} {'verdict':>8}")
    verdicts = {}
    for n in a.points:
        xs = O.random_elements(n, 7000 + n)
        for ld in a.log_deg:
            d = 1 << ld
            poly = O.random_elements(d, 8000 + ld)
            calls = {"horner": lambda: ctx.eval_poly_at_multi(poly, xs),
                     "split": routed(never, lambda: ctx.eval_poly_multipoint(poly, xs)),
                     "tree": routed(1, lambda: ctx.eval_poly_multipoint(poly, xs))}
            once = {}
            outs = {}
            for k, f in calls.items():  # the first calls: tables, buffers, and the values
                f()
                t = time.perf_counter()
                outs[k] = f()
                once[k] = time.perf_counter() - t
            if not (np.array_equal(outs["horner"], outs["split"]) and np.array_equal(outs["horner"], outs["tree"])):
                flush()
                raise RuntimeError(f"n = {n}, deg_plus_1 = {d}: the routes' values differ")
            reps = max(1, min(a.reps, int(a.shape_limit / (2 * sum(once.values()) + 1e-9))))
            res = series(calls, reps, warm=0)
            spread = max(v[1] for v in res.values())
            gain = res["split"][0] - res["tree"][0]
            verdict = "tree" if gain > 3 * spread else ("split" if -gain > 3 * spread else "tie")
            verdicts[(n, d)] = verdict
            say(f"{n:>6} {d:>8} {reps:>4} {res['horner'][0]:>11.3f} {res['split'][0]:>11.3f} {res['tree'][0]:>11.3f} "
                f"{spread:>8.3f} {gain:>11.3f} {verdict:>8}")
            flush()
    best = None
    for m in sorted({min(k) for k in verdicts}, reverse=True):
        if all(v == "tree" for k, v in verdicts.items() if min(k) >= m):
            best = m
        else:
            break
    if verdicts:
        say(f"# smallest measured min(n, deg+1) from which the tree wins every measured shape: {best if best else 'never'}")
        say()

    # lagrange_interp at arbitrary points: Z'(x_i) down the tree against the one-thread-per-point Horner
    for n in a.interp_points:
        xs, ys = O.random_elements(n, 9001), O.random_elements(n, 9002)
        calls = {"descent": routed(1, lambda: ctx.lagrange_interp(xs, ys)),
                 "horner": routed(never, lambda: ctx.lagrange_interp(xs, ys))}
        if not np.array_equal(calls["descent"](), calls["horner"]()):
            flush()
            raise RuntimeError("lagrange_interp: the two routes' interpolants differ")
        res = series(calls, a.reps)
        say(f"# lagrange_interp, {n} arbitrary points, ms (median, spread): descent {res['descent'][0]:.3f} "
            f"({res['descent'][1]:.3f}), horner {res['horner'][0]:.3f} ({res['horner'][1]:.3f})")
    # divrem_polys
    la, lb = 1 << 20, 1 << 19
    pa, pb = O.random_elements(la, 9003), O.random_elements(lb, 9004)
    # (into the same output arrays every call: fresh ones cost their page faults, 48 MB here)
    q, r, nq = np.zeros((la, 4), dtype=np.uint64), np.zeros((lb - 1, 4), dtype=np.uint64), ctypes.c_size_t(0)

    def divrem():
        ctx.check(ctx.lib.stark_divrem_polys(ctx.h, S._p64(pa), la, S._p64(pb), lb, S._p64(q), ctypes.byref(nq),
                                             S._p64(r)), "divrem_polys")
    res = series({"divrem": divrem}, a.reps, warm=2)
    say(f"# divrem_polys, la = {la}, lb = {lb}, ms (median, spread): {res['divrem'][0]:.3f} ({res['divrem'][1]:.3f})")
    ctx.set_multipoint_tree_min(0)
    ctx.close()
    flush()


if __name__ == "__main__":
    main()
