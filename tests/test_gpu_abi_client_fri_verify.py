"""tests/abi_client_fri_verify/fri_verify_flow.cpp, a C++ caller built against include/stark_hip.h alone: it proves
a batch of 3 low-degree vectors, verifies the handles in one call, rebuilds proof 1 with stark_fri_proof_from_parts
from its accessors, flips one bit of a polynomial leaf in a second rebuilt copy and verifies
[original, rebuilt, tampered]."""
import os
import subprocess

import numpy as np
import pytest

import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
CLIENT = os.path.join(HERE, "abi_client_fri_verify")
BIN = os.path.join(CLIENT, "fri_verify_flow")

pytestmark = pytest.mark.gpu

FRI_PATHS, FRI_ROWS = 0x02, 0x04


def test_fri_verify_client_builds_runs_and_reports(tmp_path):
    subprocess.run(["make", "-s", "-C", CLIENT], check=True)
    out = subprocess.run(["ldd", BIN], capture_output=True, text=True, check=True).stdout
    assert "libstark_hip.so" in out and "not found" not in out.split("libstark_hip.so")[1].splitlines()[0]
    log_n, bound, excl, batch = 10, 256, 8, 3
    (tmp_path / "root.bin").write_bytes(O.to_limbs([O.root_of_unity(log_n)]).tobytes())
    (tmp_path / "coeffs.bin").write_bytes(np.ascontiguousarray(O.random_elements(batch * bound, 31)).tobytes())
    r = subprocess.run([BIN, str(log_n), str(bound), str(excl), str(tmp_path / "root.bin"), str(tmp_path / "coeffs.bin")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = dict(x.split(": ") for x in r.stdout.strip().splitlines())
    assert lines["handles"] == "0/0 0/0 0/0", r.stdout
    assert lines["rebuilt"] == f"0/0 0/0 8/{FRI_PATHS | FRI_ROWS:x}", r.stdout
