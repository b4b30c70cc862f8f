"""A/B of batched FRI verification against the loop of single calls, over the same proofs, in one process,
alternating:

    python tools/time_fri_verify_batch.py [--reps 10] [--logs 12,16] [--batches 1,16,64,256] [--out FILE]

(a) batch/host  stark_verify_low_degree_batch with the Last elements on the host workers (set_verify_batch_last(1));
(b) batch/dev   the same with the Last elements on the device (set_verify_batch_last(2));
(c) loop        stark_verify_low_degree_proof once per proof over the same parts: the only way before the batched
                entry.

Sizes 2^12 and 2^16 points with the bound n / 4, batches 1, 16, 64 and 256.  Every form is called on the library
directly with its arguments encoded beforehand.  Every case runs the three forms as two interleaved series of
--reps rounds (tools/verify_batch_ab.py's scheme): a form's time is the median over both series, its spread the
difference between the medians of its two series; all per proof.  Every status of every form must be 0 first; the
tool stops otherwise.  A size's proofs are of 64 different vectors; a batch of 256 holds each four times.

The default Last mode is the device unless, at batch 64, it is slower than the host mode by more than three times
the host mode's spread: the last lines say which it is."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "stark-pure-rust_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")]

from verify_batch_ab import series  # noqa: E402

LOGS = (12, 16)
BATCHES = (1, 16, 64, 256)
DISTINCT = 64
EXCL = 8


def proofs_of(ctx, log_n):
    """(w, roots, handles, parsed proofs) of DISTINCT vectors of 2^log_n values of degree < n / 4."""
    import numpy as np
    import oracle as O
    import stark_amd as S
    n = 1 << log_n
    w = O.root_of_unity(log_n)
    vs = np.stack([ctx.best_fft(O.random_elements(n // 4, 5000 + 97 * log_n + b), w, log_n) for b in range(DISTINCT)])
    forest = S.MerkleForest(ctx)
    forest.update_bytes(np.ascontiguousarray(vs).tobytes(), n, 32, DISTINCT)
    roots = forest.roots()
    handles = ctx.prove_low_degree_batch(vs, w, n // 4, EXCL)
    return w, roots, handles, [h.layers() for h in handles]


def forms(ctx, w, roots, handles, parsed, log_n, batch):
    import stark_amd as S
    from stark_amd.verify import _Branches, _FriLayer, _uniform_branches
    lib = ctx.lib
    n = 1 << log_n
    pick = [b % DISTINCT for b in range(batch)]
    blob = b"".join(roots[b] for b in pick)
    hs = (ctypes.c_void_p * batch)(*[handles[b].h for b in pick])
    sts = (ctypes.c_int * batch)()
    rou = S._limbs(w)
    p_rou = rou.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    keep = [rou]
    singles = []  # the single call's arguments per distinct proof
    for b in sorted(set(pick)):
        proof = parsed[b]
        mids = [x["Middle"] for x in proof[:-1]]
        arr = (_FriLayer * max(len(mids), 1))()
        for i, m in enumerate(mids):
            root2 = bytes(m["root2"])
            keep.append(root2)
            arr[i] = _FriLayer(root2, _uniform_branches(m["column_branches"], keep),
                               _uniform_branches(m["poly_branches"], keep))
        last = [bytes(v) for v in proof[-1]["Last"]["last"]]
        ptrs = (ctypes.c_char_p * len(last))(*last)
        lens = (ctypes.c_size_t * len(last))(*[32] * len(last))
        keep += [arr, last, ptrs, lens]
        singles.append((roots[b], ctypes.cast(arr, ctypes.c_void_p), len(mids), ctypes.cast(ptrs, ctypes.c_void_p), lens,
                        len(last)))

    def batch_form(mode):
        def call():
            lib.stark_ctx_set_verify_batch_last(ctx.h, mode)
            rc = lib.stark_verify_low_degree_batch(ctx.h, blob, p_rou, hs, batch, n // 4, EXCL, sts, None)
            return [rc] + list(sts)
        return call

    def loop():
        return [lib.stark_verify_low_degree_proof(*singles[b % len(singles)][:1], p_rou, *singles[b % len(singles)][1:],
                                                  n // 4, EXCL) for b in range(batch)]
    return {"batch/host": batch_form(1), "batch/dev": batch_form(2), "loop": loop}, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--logs", default=",".join(map(str, LOGS)), help="log2 sizes, comma separated")
    ap.add_argument("--batches", default=",".join(map(str, BATCHES)), help="batch sizes, comma separated")
    a = ap.parse_args()
    logs, batches = [int(x) for x in a.logs.split(",")], [int(x) for x in a.batches.split(",")]
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    import stark_amd as S
    ctx = S.Context(0)
    say("# verify_low_degree_proof of B proofs of 2^log_n values, bound n / 4, exclusion 8; ms per proof.")
    say("# (a) batch/host = stark_verify_low_degree_batch, Last elements on the host workers; (b) batch/dev = the same,")
    say("# Last elements on the device; (c) loop = stark_verify_low_degree_proof per proof, the only way before.")
    say("# Median over two interleaved series of `reps` rounds per form; spread = the difference between the medians of")
    say("# a form's two series; (n.nn x) = loop / batch form per proof.  reps = %d." % a.reps)
    say()
    names = ("batch/host", "batch/dev", "loop")
    say(f"{'log_n':>5} {'B':>4} " + " ".join(f"{k + '/proof':>17} {'(spread)':>9}" for k in names) +
        "   loop / (a), loop / (b), (b) - (a) against 3 spread (a)")
    at64 = {}
    for log_n in logs:
        w, roots, handles, parsed = proofs_of(ctx, log_n)
        for batch in batches:
            f, keep = forms(ctx, w, roots, handles, parsed, log_n, batch)
            for k, g in f.items():  # warm (buffers), and every status 0
                if any(g()):
                    raise RuntimeError(f"2^{log_n}, B = {batch}: the {k} form refuses a proof")
            res = series(f, a.reps)
            per = {k: (v[0] / batch, v[1] / batch) for k, v in res.items()}
            diff, bar = per["batch/dev"][0] - per["batch/host"][0], 3 * per["batch/host"][1]
            say(f"{log_n:>5} {batch:>4} " + " ".join(f"{per[k][0]:>17.4f} {per[k][1]:>9.4f}" for k in names) +
                f"   {per['loop'][0] / per['batch/host'][0]:.2f}x, {per['loop'][0] / per['batch/dev'][0]:.2f}x, "
                f"{diff:+.4f} against {bar:.4f}")
            if batch == 64:
                at64[log_n] = (diff, bar)
            del keep
        del handles, parsed
    ctx.set_verify_batch_last(0)
    say()
    slower = [log_n for log_n, (diff, bar) in at64.items() if diff > bar]
    for log_n, (diff, bar) in at64.items():
        say(f"# 2^{log_n} at B = 64: batch/dev - batch/host = {diff:+.4f} ms per proof, three host spreads = {bar:.4f}: "
            f"the device is {'slower' if diff > bar else 'not slower'}")
    say(f"# default Last mode by this run: {'1 (host)' if slower else '2 (device)'}")
    ctx.close()


if __name__ == "__main__":
    main()
