"""A/B of B sequential stark_verify_r1cs_circuit calls against one stark_verify_r1cs_circuit_batch over the same
proofs of one prepared circuit, in one process, alternating:

    python tools/verify_batch_ab.py [--reps 10] [--out profiles/verify_batch_ab.txt]

seq      B calls of stark_verify_r1cs_circuit, one per proof: the untouched single-proof entry point (the
         yardstick: the code path of the commit before the batch existed);
batch    one stark_verify_r1cs_circuit_batch over the same proofs.

Both forms are called on the library directly with the texts and wires encoded beforehand.  Every case (circuit,
B) runs the two forms as two interleaved series of --reps rounds (tools/prove_batch_ab.py's scheme): a form's
time is the median over both series, its spread the difference between the medians of its two series.  The batch
wins a case when its time per proof is lower than the sequential form's by more than three times the larger
spread (both per proof).  Every status of both forms must be 0 first; the tool stops otherwise.

Four parts: the table for the library as it is; the same table with every batch read one proof per host worker
and with every batch read one proof after another through the reader's own parallel passes
(STARK_VERIFY_BATCH_PARSE=worker|inner, child processes: the library reads the variable once), which is the
measurement behind the library's choice between the two; and the library's phase clock (STARK_PROFILE=1, a child
process) once per form at each circuit's larger B, where the share of the JSON parse shows.  The fixtures hold one
witness each, so their batches repeat one proof."""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "stark-pure-rust_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")]
FIX = os.path.join(ROOT, "tests", "golden", "r1cs")
CASES = [("compute", 64), ("poseidon3_test", 16), ("pedersen_test", 8)]


def load(name):
    with open(os.path.join(FIX, name + ".r1cs"), "rb") as f:
        r1 = f.read()
    with open(os.path.join(FIX, name + ".wtns"), "rb") as f:
        wt = f.read()
    return r1, wt


def series(variants, reps):
    """variants: name -> a call.  Two series each, interleaved, the order rotating; returns name -> (median over
    both in ms, |median - median'| in ms)."""
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


def forms(ctx, circuit, pub: bytes, js: bytes, batch: int):
    """The two forms over `batch` copies of one proof, as calls returning their statuses."""
    lib = ctx.lib
    n_public = len(pub) // 32
    pubs = (ctypes.c_char_p * batch)(*[pub] * batch)
    texts = (ctypes.c_char_p * batch)(*[js] * batch)
    lens = (ctypes.c_size_t * batch)(*[len(js)] * batch)
    sts = (ctypes.c_int * batch)()

    def seq():
        return [lib.stark_verify_r1cs_circuit(ctx.h, circuit.h, pub, n_public, js, len(js)) for _ in range(batch)]

    def one_batch():
        rc = lib.stark_verify_r1cs_circuit_batch(ctx.h, circuit.h, pubs, n_public, texts, lens, batch, sts, None)
        return [rc] + list(sts)
    return {"seq": seq, "batch": one_batch}


def cases_of(a):
    return [(s.split(":")[0], int(s.split(":")[1])) for s in a.cases.split(",")] if a.cases else CASES


def prepared(ctx, name):
    import r1cs as R
    from stark_amd.r1cs import R1csCircuit
    from stark_amd.verify import _wire_bytes
    r1, wt = load(name)
    circuit = R1csCircuit(ctx, r1)
    h = R.read_r1cs(r1).header
    pub = _wire_bytes(R.read_witness(wt)[:1 + h.n_public_inputs + h.n_public_outputs])
    return circuit, pub, circuit.prove(wt).to_json().encode()


def table(a, say):
    import stark_amd as S
    ctx = S.Context(0)
    say(f"{'circuit':>15} {'B':>3} {'seq':>10} {'(spread)':>9} {'one batch':>10} {'(spread)':>9} "
        f"{'seq/proof':>10} {'batch/proof':>11} {'gain':>8} {'3 spread':>9} {'ratio':>6} {'verdict':>7}")
    for name, big in cases_of(a):
        circuit, pub, js = prepared(ctx, name)
        for batch in sorted({2, big}, reverse=True):
            f = forms(ctx, circuit, pub, js, batch)
            for k, g in f.items():  # warm (buffers), and every status 0
                if any(g()):
                    raise RuntimeError(f"{name}, B = {batch}: the {k} form refuses a proof")
            res = series(f, a.reps)
            per = {k: (v[0] / batch, v[1] / batch) for k, v in res.items()}
            spread = max(v[1] for v in per.values())
            gain = per["seq"][0] - per["batch"][0]
            verdict = "batch" if gain > 3 * spread else ("seq" if -gain > 3 * spread else "tie")
            say(f"{name:>15} {batch:>3} {res['seq'][0]:>10.3f} {res['seq'][1]:>9.3f} {res['batch'][0]:>10.3f} "
                f"{res['batch'][1]:>9.3f} {per['seq'][0]:>10.4f} {per['batch'][0]:>11.4f} {gain:>8.4f} "
                f"{3 * spread:>9.4f} {per['seq'][0] / per['batch'][0]:>6.2f} {verdict:>7}   # {len(js)} B of JSON per proof")
        del circuit
    ctx.close()


def phases(a):
    """(child, STARK_PROFILE=1) each form once per circuit at its larger B: the library's clock goes to stderr."""
    import stark_amd as S
    ctx = S.Context(0)
    for name, big in cases_of(a):
        print(f"[ab] {name}: the circuit, a proof and warm-up calls of both forms (not the figures)", file=sys.stderr,
              flush=True)
        circuit, pub, js = prepared(ctx, name)
        f = forms(ctx, circuit, pub, js, big)
        for g in f.values():
            g()
        for k in ("seq", "batch"):
            print(f"[ab] {name} B = {big}: {k}" + (" (the first of its B calls)" if k == "seq" else ""), file=sys.stderr,
                  flush=True)
            if k == "seq":
                forms(ctx, circuit, pub, js, 1)["seq"]()
            else:
                f[k]()
        del circuit
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cases", default="", help="name:B,... (default: the three of the table)")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="", help="(internal) table | phases")
    a = ap.parse_args()
    if a.child == "table":
        table(a, lambda s="": print(s, flush=True))
        return
    if a.child == "phases":
        phases(a)
        return
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    def child(kind, env):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--reps", str(a.reps)]
        if a.cases:
            cmd += ["--cases", a.cases]
        r = subprocess.run(cmd, env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                           check=True, timeout=900)
        return r.stdout, r.stderr

    say("# verifications of one prepared circuit's proofs: B calls of stark_verify_r1cs_circuit (seq) against one")
    say("# stark_verify_r1cs_circuit_batch (one batch), ms: median over two interleaved series of `reps` rounds per")
    say("# form; spread = the difference between the medians of a form's two series; per proof = / B; ratio =")
    say("# seq / batch per proof; the batch wins when seq - batch per proof exceeds three times the larger spread")
    say()
    say("# the library as it is: a chunk of at least half as many proofs as host workers is read one proof per")
    say("# worker, a smaller one through the reader's parallel passes")
    table(a, say)
    say()
    say("# every batch read one proof per host worker, each serially (STARK_VERIFY_BATCH_PARSE=worker)")
    for line in child("table", {"STARK_VERIFY_BATCH_PARSE": "worker"})[0].splitlines():
        say(line)
    say()
    say("# every batch read one proof after another, each through the reader's parallel passes")
    say("# (STARK_VERIFY_BATCH_PARSE=inner)")
    for line in child("table", {"STARK_VERIFY_BATCH_PARSE": "inner"})[0].splitlines():
        say(line)
    say()
    say("# (the three tables are three processes: compare a table's ratio column, not its times, with another's)")
    say()
    say("# the library's phase clock (STARK_PROFILE=1), once per form at each circuit's larger B")
    warm = False
    for line in child("phases", {"STARK_PROFILE": "1"})[1].splitlines():
        if line.startswith("[ab]"):
            warm = "not the figures" in line
        if not warm and (line.startswith("[stark]") or line.startswith("[ab]")):
            say(line)


if __name__ == "__main__":
    main()
