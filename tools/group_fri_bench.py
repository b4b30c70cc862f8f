"""Timings around the group FRI (stark_group_prove_low_degree, csrc/group.hip).

    python tools/group_fri_bench.py --ab parent.so new.so [--members 8] [--rounds 4] [--reps 10]
        Same-box A/B of the group prover across library builds (raw ctypes: any ABI revision): the
        synthetic 2^20-step proof over `members` contexts on device 0, cold (stark_group_prove_r1cs_bytes)
        and prepared (stark_group_circuit_new + stark_group_prove_r1cs_circuit), one child process per
        build per round, rounds alternating.  Prints every round's median, per build the median of the
        round medians, the first build's round-to-round spread (max - min of its round medians) and whether
        the second build is slower than the first by more than three times that spread.

    python tools/group_fri_bench.py [--members 8] [--log-n 23] [--reps 10]
        Information: prove_low_degree at 2^log_n (max_deg_plus_1 = n / 4, exclude 8) on one context and
        over the group through the host and the device entry points, host wall-clock medians; and the
        achieved GB/s of stark_class_deal_dev / stark_class_merge_dev at 2^log_n elements (64 B moved per
        element).  The members share one device here: the group figures time the code path, they are not
        a scaling figure.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import ctypes, hashlib, json, os, statistics, sys, time
lib = ctypes.CDLL(os.path.abspath(sys.argv[1]))
root, G, reps = sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
vp, sz, cp = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p
lib.stark_group_create.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_uint32, ctypes.POINTER(vp)]
lib.stark_group_destroy.argtypes = [vp]
lib.stark_group_prove_r1cs_bytes.argtypes = [vp, cp, sz, cp, sz, ctypes.POINTER(vp)]
lib.stark_group_circuit_new.argtypes = [vp, cp, sz, ctypes.POINTER(vp)]
lib.stark_group_prove_r1cs_circuit.argtypes = [vp, ctypes.POINTER(vp), cp, sz, ctypes.POINTER(vp)]
lib.stark_r1cs_circuit_free.argtypes = [vp]
lib.stark_r1cs_proof_json_view.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(sz)]
lib.stark_r1cs_proof_free.argtypes = [vp]
sys.path.insert(0, os.path.join(root, "tools"))
import synth_r1cs
r, w = synth_r1cs.for_steps(20)
g = vp()
assert lib.stark_group_create((ctypes.c_int * G)(*([0] * G)), G, ctypes.byref(g)) == 0
circ = (vp * G)()
assert lib.stark_group_circuit_new(g, r, len(r), circ) == 0

def proof(p):
    q, n = vp(), sz()
    lib.stark_r1cs_proof_json_view(p, ctypes.byref(q), ctypes.byref(n))
    js = ctypes.string_at(q.value, n.value)
    lib.stark_r1cs_proof_free(p)
    return js

def cold():
    p = vp()
    assert lib.stark_group_prove_r1cs_bytes(g, r, len(r), w, len(w), ctypes.byref(p)) == 0
    return proof(p)

def prepared():
    p = vp()
    assert lib.stark_group_prove_r1cs_circuit(g, circ, w, len(w), ctypes.byref(p)) == 0
    return proof(p)

out = {}
for name, fn in (("cold", cold), ("prepared", prepared)):
    ts = []
    for i in range(reps + 2):
        t = time.perf_counter()
        js = fn()
        ts.append(time.perf_counter() - t)
    out[name] = {"ms": [round(x * 1e3, 4) for x in ts[2:]], "digest": hashlib.sha256(js).hexdigest()[:16]}
for c in circ:
    lib.stark_r1cs_circuit_free(c)
lib.stark_group_destroy(g)
print(json.dumps(out))
'''


def ab(args):
    libs = args.ab
    rounds = {lib: {"cold": [], "prepared": []} for lib in libs}
    digests = {}
    for rnd in range(args.rounds):
        for lib in libs:
            r = subprocess.run([sys.executable, "-c", CHILD, lib, ROOT, str(args.members), str(args.reps)],
                               capture_output=True, text=True, timeout=600)
            if r.returncode != 0:  # (a child that died on the GPU is not followed by more GPU programs)
                print(f"{lib}: rc {r.returncode} {r.stderr[-500:]}", flush=True)
                sys.exit(1)
            for name, v in json.loads(r.stdout.strip().splitlines()[-1]).items():
                med = statistics.median(v["ms"])
                rounds[lib][name].append(med)
                digests.setdefault(name, set()).add(v["digest"])
                print(f"round {rnd} {os.path.basename(lib):12s} {name:9s} median {med:8.3f} ms  best "
                      f"{min(v['ms']):8.3f} ms  n={len(v['ms'])}  digest {v['digest']}", flush=True)
    base, new = libs[0], libs[-1]
    for name in ("cold", "prepared"):
        b, n = rounds[base][name], rounds[new][name]
        spread = max(b) - min(b)
        mb, mn = statistics.median(b), statistics.median(n)
        verdict = "slower" if mn - mb > 3 * spread else "not slower"
        print(f"{name:9s} {os.path.basename(base)} {mb:8.3f} ms (round-to-round spread {spread:.3f} ms)  "
              f"{os.path.basename(new)} {mn:8.3f} ms  difference {mn - mb:+.3f} ms vs bar {3 * spread:.3f} ms: "
              f"{verdict}; digests agree: {len(digests[name]) == 1}", flush=True)


def med_wall(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1000.0


def info(args):
    sys.path.insert(0, os.path.join(ROOT, "stark-pure-rust_amd"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import numpy as np
    import oracle as O
    import stark_amd as S
    from stark_amd.group import Group
    G, log_n = args.members, args.log_n
    n = 1 << log_n
    w = O.root_of_unity(log_n)
    out = {"members": G, "devices": [0] * G, "log_n": log_n,
           "note": "all members are contexts on one device: the group figures time the code path, not scaling"}
    ctx = S.Context(0)
    vals = ctx.best_fft(O.random_elements(n // 4, 0x5EED0000 + log_n), w, log_n)
    # one context, device-resident values (what bench.py times)
    d = ctx.alloc(vals.nbytes)
    ctx.h2d(d, vals)
    ref = ctx.prove_low_degree_dev(d, n, w, n // 4, 8).to_json()
    out["single_ctx_dev_ms"] = round(med_wall(lambda: ctx.prove_low_degree_dev(d, n, w, n // 4, 8), args.reps), 4)
    out["single_ctx_host_ms"] = round(med_wall(lambda: ctx.prove_low_degree(vals, w, n // 4, 8), args.reps), 4)
    # deal / merge: `launches` back to back, one synchronisation
    d2 = ctx.alloc(vals.nbytes)
    launches = 20
    for name, fn, a, b in (("deal", ctx.class_deal_dev, d, d2), ("merge", ctx.class_merge_dev, d2, d)):
        for world in (2, 8):
            fn(a, b, n, world)
            ctx.synchronize()

            def run():
                for _ in range(launches):
                    fn(a, b, n, world)
                ctx.synchronize()
            ms = med_wall(run, 5) / launches
            out[f"class_{name}_world{world}_2^{log_n}_GBps"] = round(64.0 * n / (ms * 1e-3) / 1e9, 1)
    ctx.free(d2)
    ctx.free(d)
    g = Group([0] * G)
    out["group_host_bitexact_vs_single"] = g.prove_low_degree(vals, w, n // 4, 8).to_json() == ref
    out["group_host_ms"] = round(med_wall(lambda: g.prove_low_degree(vals, w, n // 4, 8), args.reps), 4)
    ptrs = []
    for r in range(G):
        p = ctypes.c_void_p()
        g.check(g.lib.stark_dev_alloc(g.ctx_handle(r), n // G * 32, ctypes.byref(p)), "dev_alloc")
        x = np.ascontiguousarray(vals[r::G])
        g.check(g.lib.stark_memcpy_h2d(g.ctx_handle(r), p.value, x.ctypes.data, x.nbytes), "h2d")
        ptrs.append(p.value)
    out["group_dev_bitexact_vs_single"] = g.prove_low_degree_dev(ptrs, n, w, n // 4, 8).to_json() == ref
    out["group_dev_ms"] = round(med_wall(lambda: g.prove_low_degree_dev(ptrs, n, w, n // 4, 8), args.reps), 4)
    for r, p in enumerate(ptrs):
        g.lib.stark_dev_free(g.ctx_handle(r), p)
    g.close()
    ctx.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", nargs=2, metavar=("PARENT_SO", "NEW_SO"))
    ap.add_argument("--members", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--log-n", type=int, default=23)
    args = ap.parse_args()
    if args.ab:
        ab(args)
    else:
        info(args)


if __name__ == "__main__":
    main()
