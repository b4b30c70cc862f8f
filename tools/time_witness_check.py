"""What a witness check costs against the proof it saves, over the same witnesses of one prepared circuit, in one
process, alternating:

    python tools/time_witness_check.py [--reps 10] [--out profiles/witness_check_ab.txt]

prove    one R1csCircuit.prove_batch(strict=False): the only way the library answered "does this witness satisfy
         the circuit" before the check existed, and an entry point the check leaves untouched (the yardstick);
check    one R1csCircuit.check_batch over the same witnesses (max_failures = 16).

The cases are tools/prove_batch_ab.py's (circuit x B), each with every witness good and again with the last
witness of the batch bad (its last value raised by one; the tool stops if that does not fail a constraint, or if
the two forms' statuses differ).  Every case runs the two forms as two interleaved series of --reps rounds
(tools/prove_batch_ab.py's scheme): a form's time is the median over both series, its spread the difference between
the medians of its two series.  The check passes a case when its time per witness is lower than the proof's by more
than three times the larger spread (both per witness).

Two figures per case, reported separately:

end to end    the calls as a caller sees them, Python's report objects included;
device chain  the check's upload, launches and download alone: what the library's own phase clock (STARK_PROFILE=1)
              prints for "upload + launches enqueued" and "chain + download (synced)", so this part runs in a child
              process with the clock on (--chain-child).

Last, the largest batch of pedersen_test witnesses one chunk takes under the default prove-batch limit, from the
working set include/stark_hip.h states (n_wires x 64 B, one bit per constraint in 64-bit words, min(cap, n_c)
records of 104 B, a 4-B count; grid.y caps a chunk at 65,535)."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "stark-pure-rust_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")]
import prove_batch_ab as AB  # noqa: E402

CAP = 16
CHAIN = ("upload + launches enqueued", "chain + download (synced)")
STAGE = ("witnesses staged (host)",)


def raise_last_value(wt: bytes) -> bytes:
    fs = int.from_bytes(wt[24:28], "little")
    v = (int.from_bytes(wt[-fs:], "little") + 1) % (1 << (8 * fs))
    return wt[:-fs] + v.to_bytes(fs, "little")


def phases(text, names):
    return sum(float(us) for ph, us in AB.PHASE.findall(text) if ph in names) / 1e3


def chunk_capacity(r1: bytes, cap: int, limit: int = 6 << 30) -> int:
    import r1cs as R
    h = R.read_r1cs(r1).header
    per = h.n_wires * 64 + 2 * ((h.n_constraints + 63) // 64) * 4 + min(cap, h.n_constraints) * 104 + 4
    return min(65535, (limit - 6 * 256) // per)


def run(a, say, capture=None):
    import stark_amd as S
    from stark_amd.r1cs import R1csCircuit
    cases = [(s.split(":")[0], int(s.split(":")[1])) for s in a.cases.split(",")] if a.cases else AB.CASES
    ctx = S.Context(0)
    if capture:
        say(f"{'circuit':>15} {'B':>3} {'bad':>3} {'staging':>9} {'chain':>9} {'(spread)':>9} {'chain/witness':>13}")
    else:
        say(f"{'circuit':>15} {'B':>3} {'bad':>3} {'prove':>10} {'(spread)':>9} {'check':>10} {'(spread)':>9} "
            f"{'prove/wit':>10} {'check/wit':>10} {'saved':>9} {'3 spread':>9} {'ratio':>7} {'verdict':>7}")
    for name, batch in cases:
        r1, wts = AB.load(name, batch)
        circuit = R1csCircuit(ctx, r1)
        for n_bad in (0, 1):
            ws = list(wts)
            if n_bad:
                ws[-1] = raise_last_value(ws[-1])
            reports = circuit.check_batch(ws, CAP)
            proved = [p.code if hasattr(p, "code") else 0 for p in circuit.prove_batch(ws, strict=False)]
            if [r.status for r in reports] != proved:
                raise RuntimeError(f"{name}: check says {[r.status for r in reports]}, the prover {proved}")
            if [r.status for r in reports] != [0] * (batch - n_bad) + [8] * n_bad:
                raise RuntimeError(f"{name}: statuses {[r.status for r in reports]} with {n_bad} bad witness(es)")
            if capture:
                ts = ([], [])
                stage = []
                for _ in range(a.reps):
                    for half in (0, 1):
                        capture.take()
                        circuit.check_batch(ws, CAP)
                        text = capture.take()
                        ts[half].append(phases(text, CHAIN))
                        stage.append(phases(text, STAGE))
                med = statistics.median(ts[0] + ts[1])
                spread = abs(statistics.median(ts[0]) - statistics.median(ts[1]))
                say(f"{name:>15} {batch:>3} {n_bad:>3} {statistics.median(stage):>9.3f} {med:>9.3f} {spread:>9.3f} "
                    f"{med / batch:>13.4f}")
                continue
            f = {"prove": lambda: circuit.prove_batch(ws, strict=False), "check": lambda: circuit.check_batch(ws, CAP)}
            res = AB.series(f, a.reps)
            per = {k: (v[0] / batch, v[1] / batch) for k, v in res.items()}
            spread = max(v[1] for v in per.values())
            saved = per["prove"][0] - per["check"][0]
            verdict = "check" if saved > 3 * spread else "MISSES"
            say(f"{name:>15} {batch:>3} {n_bad:>3} {res['prove'][0]:>10.3f} {res['prove'][1]:>9.3f} "
                f"{res['check'][0]:>10.3f} {res['check'][1]:>9.3f} {per['prove'][0]:>10.4f} {per['check'][0]:>10.4f} "
                f"{saved:>9.4f} {3 * spread:>9.4f} {per['prove'][0] / per['check'][0]:>7.1f} {verdict:>7}")
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
        cap = AB.StderrCapture()
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

    say("# witness check against the proof it saves: one stark_prove_r1cs_circuit_batch (prove, statuses only) and")
    say(f"# one stark_check_r1cs_circuit_batch (check, cap {CAP}) over the same B witnesses of one prepared circuit,")
    say("# bad of them unsatisfied; ms: median over two interleaved series of `reps` rounds per form; spread = the")
    say("# difference between the medians of a form's two series; per witness = / B; saved = prove - check per")
    say("# witness; the check passes when saved exceeds three times the larger spread")
    say()
    say("# end to end")
    run(a, say)
    say()
    say("# the check's device chain alone (upload, launches, download, up to the synchronisation behind it) and the")
    say("# host's staging before it, ms, as the library's phase clock printed them (a child process with")
    say("# STARK_PROFILE=1; a batch of one chunk)")
    env = dict(os.environ, STARK_PROFILE="1")
    cmd = [sys.executable, os.path.abspath(__file__), "--chain-child", "--reps", str(a.reps)]
    if a.cases:
        cmd += ["--cases", a.cases]
    child = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, check=True)
    for line in child.stdout.splitlines():
        say(line)
    say()
    r1, _ = AB.load("pedersen_test", 1)
    say(f"# largest batch of pedersen_test witnesses in one chunk under the default 6 GiB limit (cap {CAP}): "
        f"{chunk_capacity(r1, CAP)}")


if __name__ == "__main__":
    main()
