"""tests/abi_client_check/check_flow.cpp, a C++ caller built against include/stark_hip.h alone: it prepares
`compute`, checks its witness with stark_check_r1cs_circuit, then [the witness, the witness with its last value
raised by one] with stark_check_r1cs_circuit_batch, and prints the reports.  The lines must be the ones Python's
R1csCircuit.check_batch gives, and those R1CS satisfaction in Python integers."""
import os
import subprocess

import pytest

import r1cs as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "r1cs")
CLIENT = os.path.join(HERE, "abi_client_check")
BIN = os.path.join(CLIENT, "check_flow")
P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
CAP = 4   # check_flow.cpp's

pytestmark = pytest.mark.gpu


def _lines(b, status, n_failed, failures):
    out = [f"witness {b}: status {status} n_failed {n_failed}"]
    return out + [f"  constraint {i} a {a:x} b {x:x} c {c:x}" for i, a, x, c in failures[:CAP]]


def test_check_client_builds_runs_and_reports(ctx):
    from stark_amd.r1cs import R1csCircuit
    subprocess.run(["make", "-s", "-C", CLIENT], check=True)
    out = subprocess.run(["ldd", BIN], capture_output=True, text=True, check=True).stdout
    assert "libstark_hip.so" in out and "not found" not in out.split("libstark_hip.so")[1].splitlines()[0]
    r1, wt = os.path.join(FIX, "compute.r1cs"), os.path.join(FIX, "compute.wtns")
    r = subprocess.run([BIN, r1, wt], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = r.stdout.rstrip("\n").split("\n")

    r1b, good = open(r1, "rb").read(), open(wt, "rb").read()
    raw = [int.from_bytes(v, "little") for v in R.read_witness(good)]
    fs = int.from_bytes(good[24:28], "little")   # the field size, behind the 24-byte prologue
    bad = good[:-fs] + ((raw[-1] + 1) % (1 << (8 * fs))).to_bytes(fs, "little")
    cons = [[[(w, int.from_bytes(v, "little")) for w, v in fc] for fc in fac] for fac in R.read_r1cs(r1b).constraints]

    def failing(values):
        out = []
        for i, fac in enumerate(cons):
            a, b, c = (sum(v * values[w] for w, v in fc) % P for fc in fac)
            if (a * b - c) % P:
                out.append((i, a, b, c))
        return out

    want_good, want_bad = failing(raw), failing(raw[:-1] + [raw[-1] + 1])
    assert want_good == [] and want_bad, "compute's witness holds, and its last value matters"
    want = (["single"] + _lines(0, 0, 0, []) + ["batch"] + _lines(0, 0, 0, []) +
            _lines(1, 8, len(want_bad), want_bad))
    assert got == want, r.stdout
    # and Python's surface gives the same reports
    reports = R1csCircuit(ctx, r1b).check_batch([good, bad], CAP)
    py = ["single"] + _lines(0, reports[0].status, reports[0].n_failed, reports[0].failures) + ["batch"]
    for b, rep in enumerate(reports):
        py += _lines(b, rep.status, rep.n_failed, rep.failures)
    assert got == py
