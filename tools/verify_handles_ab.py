"""A/B of batched verification from proof handles and of the transcript derived on the device, against the JSON
entry as it is, over the same proofs of one prepared circuit, in one process, alternating:

    python tools/verify_handles_ab.py [--reps 10] [--out profiles/verify_handles_ab.txt]

(a) json/host     stark_verify_r1cs_circuit_batch, the host's transcript: the entry as it was (the baseline);
(b) handles/host  stark_verify_r1cs_circuit_batch_proofs on the handles the texts came from, the host's transcript;
(c) handles/dev   the same with the transcript kernel (stark_ctx_set_verify_batch_transcript(2));
(d) json/dev      the JSON entry with the transcript kernel.

Every form is called on the library directly with its arguments encoded beforehand; the transcript mode is set
by each form's call (a store in the context).  Every case (circuit, B) runs the four forms as two interleaved
series of --reps rounds (tools/verify_batch_ab.py's scheme): a form's time is the median over both series, its
spread the difference between the medians of its two series.  A form beats another when its time per proof is
lower by more than three times the baseline form's spread (per proof).  Every status of every form must be 0
first; the tool stops otherwise.

Then the library's phase clock (STARK_PROFILE=1, a child process) once for (a), (b) and (c) on `compute` at 64,
and for (a) with the boundary interpolants formed per proof by verify_interp2's GPU branch
(stark_ctx_set_public_column_min(2)) against the basis-matrix launch.  The fixtures hold one witness each, so their batches repeat one proof."""
import argparse
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "stark-pure-rust_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")]

from verify_batch_ab import load, series  # noqa: E402

CASES = [("compute", 64), ("poseidon3_test", 16), ("pedersen_test", 8)]
FORMS = [("json/host", False, 1), ("handles/host", True, 1), ("handles/dev", True, 2), ("json/dev", False, 2)]


def prepared(ctx, name):
    import r1cs as R
    from stark_amd.r1cs import R1csCircuit
    from stark_amd.verify import _wire_bytes
    r1, wt = load(name)
    circuit = R1csCircuit(ctx, r1)
    h = R.read_r1cs(r1).header
    pub = _wire_bytes(R.read_witness(wt)[:1 + h.n_public_inputs + h.n_public_outputs])
    return circuit, pub, circuit.prove(wt)


def forms(ctx, circuit, pub: bytes, proof, batch: int):
    """The four forms over `batch` copies of one proof, as calls returning their statuses."""
    lib = ctx.lib
    n_public = len(pub) // 32
    js = proof.to_json().encode()
    pubs = (ctypes.c_char_p * batch)(*[pub] * batch)
    texts = (ctypes.c_char_p * batch)(*[js] * batch)
    lens = (ctypes.c_size_t * batch)(*[len(js)] * batch)
    hs = (ctypes.c_void_p * batch)(*[proof.h] * batch)
    sts = (ctypes.c_int * batch)()

    def form(handles, mode):
        def call():
            lib.stark_ctx_set_verify_batch_transcript(ctx.h, mode)
            if handles:
                rc = lib.stark_verify_r1cs_circuit_batch_proofs(ctx.h, circuit.h, pubs, n_public, hs, batch, sts, None)
            else:
                rc = lib.stark_verify_r1cs_circuit_batch(ctx.h, circuit.h, pubs, n_public, texts, lens, batch, sts, None)
            return [rc] + list(sts)
        return call
    return {k: form(h, m) for k, h, m in FORMS}, len(js)


def table(a, say):
    import stark_amd as S
    ctx = S.Context(0)
    say(f"{'circuit':>15} {'B':>3} " + " ".join(f"{k + '/proof':>18} {'(spread)':>9}" for k, _, _ in FORMS) +
        f" {'3 spread (a)':>13}  verdicts: b vs a, c vs b, d vs a")
    for name, big in CASES:
        circuit, pub, proof = prepared(ctx, name)
        for batch in sorted({2, big}, reverse=True):
            f, n_js = forms(ctx, circuit, pub, proof, batch)
            for k, g in f.items():  # warm (buffers), and every status 0
                if any(g()):
                    raise RuntimeError(f"{name}, B = {batch}: the {k} form refuses a proof")
            res = series(f, a.reps)
            per = {k: (v[0] / batch, v[1] / batch) for k, v in res.items()}
            bar = 3 * per["json/host"][1]

            def verdict(new, old):
                gain = per[old][0] - per[new][0]
                return f"{new if gain > bar else (old if -gain > bar else 'tie')} ({per[old][0] / per[new][0]:.2f}x)"
            say(f"{name:>15} {batch:>3} " + " ".join(f"{per[k][0]:>18.4f} {per[k][1]:>9.4f}" for k, _, _ in FORMS) +
                f" {bar:>13.4f}  {verdict('handles/host', 'json/host')}, {verdict('handles/dev', 'handles/host')}, "
                f"{verdict('json/dev', 'json/host')}   # {n_js} B of JSON per proof")
        del circuit, proof
    ctx.close()


def phases():
    """(child, STARK_PROFILE=1) the forms once on compute at 64: the library's clock goes to stderr."""
    import stark_amd as S
    ctx = S.Context(0)
    name, big = CASES[0]
    print(f"[ab] {name}: the circuit, a proof and warm-up calls of every form (not the figures)", file=sys.stderr,
          flush=True)
    circuit, pub, proof = prepared(ctx, name)
    f, _ = forms(ctx, circuit, pub, proof, big)
    for g in f.values():
        g()
    ctx.set_public_column_min(2)
    f["json/host"]()
    ctx.set_public_column_min(0)
    for k in ("json/host", "handles/host", "handles/dev"):
        print(f"[ab] {name} B = {big}: {k}", file=sys.stderr, flush=True)
        f[k]()
    print(f"[ab] {name} B = {big}: json/host with the boundary interpolants formed per proof on the GPU "
          "(set_public_column_min(2): verify_interp2's stark_lagrange_interp_domain branch)", file=sys.stderr, flush=True)
    ctx.set_public_column_min(2)
    f["json/host"]()
    ctx.set_public_column_min(0)
    del circuit, proof
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="", help="(internal) phases")
    a = ap.parse_args()
    if a.child == "phases":
        phases()
        return
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    say("# batched verification of one prepared circuit's proofs, ms per proof: (a) json/host = the JSON entry as it")
    say("# was, (b) handles/host = stark_verify_r1cs_circuit_batch_proofs, (c) handles/dev = the same with the")
    say("# transcript kernel, (d) json/dev = the JSON entry with the transcript kernel.  Median over two interleaved")
    say("# series of `reps` rounds per form; spread = the difference between the medians of a form's two series; a form")
    say("# beats another when it is lower by more than three times (a)'s spread; (n.nn x) = old / new per proof")
    say()
    table(a, say)
    say()
    say("# the library's phase clock (STARK_PROFILE=1), once per form on compute at 64")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "phases"],
                       env=dict(os.environ, STARK_PROFILE="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       check=True, timeout=600)
    warm = False
    for line in r.stderr.splitlines():
        if line.startswith("[ab]"):
            warm = "not the figures" in line
        if not warm and (line.startswith("[stark]") or line.startswith("[ab]")):
            say(line)


if __name__ == "__main__":
    main()
