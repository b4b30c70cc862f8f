"""tests/abi_client_verify/verify_flow.cpp, a C++ caller built against include/stark_hip.h alone: it prepares
`compute`, proves a batch of 3, verifies the handles, rebuilds proof 1 with stark_r1cs_proof_from_parts from its
accessors, flips one byte of a main leaf in a second rebuilt copy and verifies [original, rebuilt, tampered] --
no proof text anywhere."""
import os
import subprocess

import pytest

import r1cs as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "r1cs")
CLIENT = os.path.join(HERE, "abi_client_verify")
BIN = os.path.join(CLIENT, "verify_flow")

pytestmark = pytest.mark.gpu

OPENING_PATHS, SPOT = 0x10, 0x20


def test_verify_client_builds_runs_and_reports(tmp_path):
    subprocess.run(["make", "-s", "-C", CLIENT], check=True)
    out = subprocess.run(["ldd", BIN], capture_output=True, text=True, check=True).stdout
    assert "libstark_hip.so" in out and "not found" not in out.split("libstark_hip.so")[1].splitlines()[0]
    r1, wt = os.path.join(FIX, "compute.r1cs"), os.path.join(FIX, "compute.wtns")
    h = R.read_r1cs(open(r1, "rb").read()).header
    wires = R.read_witness(open(wt, "rb").read())[:1 + h.n_public_inputs + h.n_public_outputs]
    (tmp_path / "public.bin").write_bytes(b"".join(bytes(w).ljust(32, b"\0") for w in wires))
    r = subprocess.run([BIN, r1, wt, str(tmp_path / "public.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = dict(x.split(": ") for x in r.stdout.strip().splitlines())
    assert lines["handles"] == "0/0 0/0 0/0", r.stdout
    assert lines["rebuilt"] == f"0/0 0/0 8/{OPENING_PATHS | SPOT:x}", r.stdout
