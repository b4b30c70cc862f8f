"""A/B of `batch` sequential prove_low_degree_dev calls against one prove_low_degree_batch_dev on the same device
values, in one process, alternating:

    python tools/fri_batch_ab.py [--reps 10] [--out profiles/fri_batch_ab.txt]

seq      `batch` calls of stark_prove_low_degree_dev, one per vector: the untouched single-proof entry point (the
         yardstick: the code of the commit before the batch existed);
batch    one stark_prove_low_degree_batch_dev over the same vectors.

Every shape (n values, batch vectors) runs the two forms as two interleaved series of --reps rounds
(tools/multipoint_ab.py's scheme): a form's time is the median over both series, its spread the difference
between the medians of its two series.  The batch wins a shape when its time per proof is lower than the
sequential form's by more than three times the larger spread (both per proof).  The proofs' JSON texts are
compared first (sha256 per proof); the tool stops at a difference.  Handles are freed outside the timed calls.

After the table, --sweep (on by default) halves the batch at the small shapes down to 2 and reports the smallest
batch that still wins at each n."""
import argparse
import ctypes
import hashlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "stark-pure-rust_amd"), os.path.join(ROOT, "oracle")]

import numpy as np  # noqa: E402

SHAPES = [(12, 64), (14, 32), (16, 16), (20, 4), (23, 1)]


def series(variants, reps):
    """variants: name -> a call returning what to release after the clock stops.  Two series each, interleaved,
    the order rotating; returns name -> (median over both in ms, |median - median'| in ms)."""
    ts = {k: ([], []) for k in variants}
    order = list(variants.items())
    for _ in range(reps):
        for half in (0, 1):
            for k, f in order:
                t = time.perf_counter()
                held = f()
                ts[k][half].append((time.perf_counter() - t) * 1e3)
                del held
            order = order[1:] + order[:1]
    return {k: (statistics.median(a + b), abs(statistics.median(a) - statistics.median(b))) for k, (a, b) in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="", help="log_n:batch,... (default: the five of the table)")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import oracle as O
    import stark_amd as S
    shapes = [tuple(int(x) for x in s.split(":")) for s in a.shapes.split(",")] if a.shapes else SHAPES
    ctx = S.Context(0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    def forms(d, n, batch, w):
        def seq():
            return [ctx.prove_low_degree_dev(d + 32 * n * b, n, w, n // 4, 8) for b in range(batch)]

        def one():
            return ctx.prove_low_degree_batch_dev(d, n, batch, w, n // 4, 8)
        return {"seq": seq, "batch": one}

    def measure(d, n, batch, w):
        f = forms(d, n, batch, w)
        for g in f.values():  # warm: tables, buffers
            g()
        res = series(f, a.reps)
        per = {k: (v[0] / batch, v[1] / batch) for k, v in res.items()}
        spread = max(v[1] for v in per.values())
        gain = per["seq"][0] - per["batch"][0]
        verdict = "batch" if gain > 3 * spread else ("seq" if -gain > 3 * spread else "tie")
        return res, per, spread, gain, verdict

    say("# prove_low_degree on device values (max_deg_plus_1 = n / 4, exclude 8), ms: median over two interleaved")
    say("# series of `reps` rounds per form; spread = the difference between the medians of a form's two series;")
    say("# per proof = / batch; the batch wins when seq - batch per proof exceeds three times the larger spread")
    head = (f"{'log_n':>5} {'batch':>5} {'seq':>10} {'(spread)':>9} {'one batch':>10} {'(spread)':>9} "
            f"{'seq/proof':>10} {'batch/proof':>11} {'gain':>8} {'3 spread':>9} {'verdict':>7}")
    say(head)
    small = []
    for log_n, batch in shapes:
        n = 1 << log_n
        w = O.root_of_unity(log_n)
        vals = np.zeros((batch, n, 4), dtype=np.uint64)
        for b in range(batch):
            vals[b, :n // 4] = O.random_elements(n // 4, 4200 + 64 * log_n + b)
        d = ctx.alloc(vals.nbytes)
        ctx.h2d(d, vals)
        del vals
        ctx.ntt_dev(d, log_n, batch, w)  # the vectors: evaluations of polynomials of degree < n / 4
        ctx.synchronize()
        f = forms(d, n, batch, w)
        sha = {k: [hashlib.sha256(p.to_json().encode()).hexdigest() for p in g()] for k, g in f.items()}
        if sha["seq"] != sha["batch"]:
            raise RuntimeError(f"log_n = {log_n}, batch = {batch}: the two forms' proofs differ")
        res, per, spread, gain, verdict = measure(d, n, batch, w)
        say(f"{log_n:>5} {batch:>5} {res['seq'][0]:>10.3f} {res['seq'][1]:>9.3f} {res['batch'][0]:>10.3f} "
            f"{res['batch'][1]:>9.3f} {per['seq'][0]:>10.4f} {per['batch'][0]:>11.4f} {gain:>8.4f} {3 * spread:>9.4f} "
            f"{verdict:>7}   # sha256 equal ({batch})")
        if not a.no_sweep and batch > 2 and log_n <= 16:
            rows = []
            bb = batch // 2
            while bb >= 2:
                r2, p2, s2, g2, v2 = measure(d, n, bb, w)
                rows.append((bb, p2, g2, s2, v2))
                bb //= 2
            small.append((log_n, batch, verdict, rows))
        ctx.free(d)
    for log_n, batch, verdict, rows in small:
        say()
        say(f"# log_n = {log_n}: smaller batches (per proof, ms)")
        say(f"{'batch':>5} {'seq/proof':>10} {'batch/proof':>11} {'gain':>8} {'3 spread':>9} {'verdict':>7}")
        pays = batch if verdict == "batch" else None
        ok = verdict == "batch"
        for bb, p2, g2, s2, v2 in rows:
            say(f"{bb:>5} {p2['seq'][0]:>10.4f} {p2['batch'][0]:>11.4f} {g2:>8.4f} {3 * s2:>9.4f} {v2:>7}")
            ok = ok and v2 == "batch"
            if ok:
                pays = bb
        say(f"# log_n = {log_n}: the batch wins at every measured batch from {pays if pays else 'none'} up")
    ctx.close()


if __name__ == "__main__":
    main()
