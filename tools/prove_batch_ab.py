"""A/B of B sequential stark_prove_r1cs_circuit calls against one stark_prove_r1cs_circuit_batch over the same
witnesses of one prepared circuit, in one process, alternating:

    python tools/prove_batch_ab.py [--reps 10] [--out profiles/prove_batch_ab.txt]

seq      B calls of R1csCircuit.prove, one per witness: the untouched single-proof entry point (the yardstick: the
         code path of the commit before the batch existed);
batch    one R1csCircuit.prove_batch over the same witnesses.

Every case (circuit, B) runs the two forms as two interleaved series of --reps rounds (tools/fri_batch_ab.py's
scheme): a form's time is the median over both series, its spread the difference between the medians of its two
series.  The batch wins a case when its time per proof is lower than the sequential form's by more than three
times the larger spread (both per proof).  The proofs' JSON texts are compared first (sha256 per proof); the tool
stops at a difference.  Handles are freed outside the timed calls.  Each circuit also runs at B = 2.

Two figures per case, reported separately:

end to end    the calls as a caller sees them, proof handles with their rendered JSON included;
device chain  the same calls up to the last download: the wall time minus the host's JSON render behind it.  The
              render's time is what the library's own phase clock (STARK_PROFILE=1) prints for the phases after
              the last download ("proof head JSON (beside them)" and "proof JSON"), so this part runs in a child
              process with the clock on (--chain-child; it costs a few stderr lines per proof, on both forms).

The fixtures hold one witness each, so their batches repeat it; the 2^17-step synthetic circuit gets two."""
import argparse
import hashlib
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "stark-pure-rust_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")]
FIX = os.path.join(ROOT, "tests", "golden", "r1cs")
CASES = [("compute", 64), ("poseidon3_test", 16), ("pedersen_test", 8), ("synth17", 2)]
PHASE = re.compile(r"\[stark\]\s{3}(.+?)\s+([\d.]+) us \(at\s+[\d.]+\)")
AFTER_LAST_DOWNLOAD = ("proof head JSON (beside them)", "proof JSON")


def load(name, batch):
    """(r1cs bytes, `batch` witnesses) of a case."""
    if name.startswith("synth"):
        import synth_r1cs
        log_steps = int(name[5:])
        r1, _ = synth_r1cs.for_steps(log_steps)
        return r1, [synth_r1cs.for_steps(log_steps, inputs=(31 + b, 7 * b + 5))[1] for b in range(batch)]
    with open(os.path.join(FIX, name + ".r1cs"), "rb") as f:
        r1 = f.read()
    with open(os.path.join(FIX, name + ".wtns"), "rb") as f:
        wt = f.read()
    return r1, [wt] * batch


class StderrCapture:
    """The process's stderr (fd 2: the library's phase clock writes there) into a file, read back per call."""

    def __init__(self):
        self.f = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.f.fileno(), 2)

    def take(self) -> str:
        self.f.seek(0)
        text = self.f.read().decode(errors="replace")
        self.f.seek(0)
        self.f.truncate()
        return text

    def close(self):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.f.close()


def series(variants, reps, capture=None):
    """variants: name -> a call returning what to release after the clock stops.  Two series each, interleaved,
    the order rotating; returns name -> (median over both in ms, |median - median'| in ms).  With `capture` the
    time of the phases after the last download, as the library printed them, is taken off each call."""
    ts = {k: ([], []) for k in variants}
    order = list(variants.items())
    for _ in range(reps):
        for half in (0, 1):
            for k, f in order:
                if capture:
                    capture.take()
                t = time.perf_counter()
                held = f()
                ms = (time.perf_counter() - t) * 1e3
                if capture:
                    ms -= sum(float(us) for ph, us in PHASE.findall(capture.take()) if ph in AFTER_LAST_DOWNLOAD) / 1e3
                ts[k][half].append(ms)
                del held
            order = order[1:] + order[:1]
    return {k: (statistics.median(a + b), abs(statistics.median(a) - statistics.median(b))) for k, (a, b) in ts.items()}


def measure(circuit, wts, reps, capture=None):
    f = {"seq": lambda: [circuit.prove(w) for w in wts], "batch": lambda: circuit.prove_batch(wts)}
    for g in f.values():  # warm: tables, buffers
        g()
    res = series(f, reps, capture)
    per = {k: (v[0] / len(wts), v[1] / len(wts)) for k, v in res.items()}
    spread = max(v[1] for v in per.values())
    gain = per["seq"][0] - per["batch"][0]
    verdict = "batch" if gain > 3 * spread else ("seq" if -gain > 3 * spread else "tie")
    return res, per, spread, gain, verdict


def run(a, say, capture=None):
    import stark_amd as S
    from stark_amd.r1cs import R1csCircuit
    cases = [(s.split(":")[0], int(s.split(":")[1])) for s in a.cases.split(",")] if a.cases else CASES
    ctx = S.Context(0)
    say(f"{'circuit':>15} {'B':>3} {'seq':>10} {'(spread)':>9} {'one batch':>10} {'(spread)':>9} "
        f"{'seq/proof':>10} {'batch/proof':>11} {'gain':>8} {'3 spread':>9} {'ratio':>6} {'verdict':>7}")
    for name, big in cases:
        r1, all_wts = load(name, big)
        circuit = R1csCircuit(ctx, r1)
        for batch in sorted({2, big}, reverse=True):
            wts = all_wts[:batch]
            sha = [[hashlib.sha256(p.to_json().encode()).hexdigest() for p in g()]
                   for g in (lambda: [circuit.prove(w) for w in wts], lambda: circuit.prove_batch(wts))]
            if sha[0] != sha[1]:
                raise RuntimeError(f"{name}, B = {batch}: the two forms' proofs differ")
            res, per, spread, gain, verdict = measure(circuit, wts, a.reps, capture)
            say(f"{name:>15} {batch:>3} {res['seq'][0]:>10.3f} {res['seq'][1]:>9.3f} {res['batch'][0]:>10.3f} "
                f"{res['batch'][1]:>9.3f} {per['seq'][0]:>10.4f} {per['batch'][0]:>11.4f} {gain:>8.4f} "
                f"{3 * spread:>9.4f} {per['seq'][0] / per['batch'][0]:>6.2f} {verdict:>7}   # sha256 equal ({batch})")
        del circuit
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cases", default="", help="name:B,... (default: the four of the table; synthN = 2^N steps)")
    ap.add_argument("--out", default="")
    ap.add_argument("--chain-child", action="store_true", help="(internal) the device-chain part, phase clock on")
    a = ap.parse_args()
    if a.chain_child:
        cap = StderrCapture()
        try:
            run(a, lambda s="": print(s, flush=True), cap)
        finally:
            cap.close()
        return
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    say("# proofs of one prepared circuit: B calls of stark_prove_r1cs_circuit (seq) against one")
    say("# stark_prove_r1cs_circuit_batch (one batch), ms: median over two interleaved series of `reps` rounds per")
    say("# form; spread = the difference between the medians of a form's two series; per proof = / B; ratio =")
    say("# seq / batch per proof; the batch wins when seq - batch per proof exceeds three times the larger spread")
    say()
    say("# end to end (proof handles with their rendered JSON)")
    run(a, say)
    say()
    say("# device chain alone: up to the last download (the wall time minus the phases after it, proof head JSON")
    say("# and proof JSON, as the library's phase clock printed them; a child process with STARK_PROFILE=1)")
    env = dict(os.environ, STARK_PROFILE="1")
    cmd = [sys.executable, os.path.abspath(__file__), "--chain-child", "--reps", str(a.reps)]
    if a.cases:
        cmd += ["--cases", a.cases]
    child = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, check=True)
    for line in child.stdout.splitlines():
        say(line)


if __name__ == "__main__":
    main()
