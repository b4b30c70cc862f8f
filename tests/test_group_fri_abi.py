"""The group FRI entry points on the C ABI (include/stark_hip.h stark_group_prove_low_degree / _dev,
stark_class_deal_dev / stark_class_merge_dev) and their C++ client tests/abi_client_group_fri/group_fri_flow.cpp
(best_fft -> prove_low_degree on a group).
CPU: the symbols and the Python methods exist, the client builds against the header and links the library.
GPU: the client's proof at G = 4, as the library serialises it and as rebuilt from the structured parts,
equals the oracle's JSON (fri.rs:46-224)."""
import hashlib
import json
import os
import struct
import subprocess

import pytest

import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
CLIENT = os.path.join(HERE, "abi_client_group_fri")
BIN = os.path.join(CLIENT, "group_fri_flow")
SYMBOLS = ["stark_group_prove_low_degree", "stark_group_prove_low_degree_dev", "stark_class_deal_dev",
           "stark_class_merge_dev"]


def test_library_exports_group_fri_symbols():
    import stark_amd as S
    lib = S.load_library()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in S._SIGNATURES and s in S.header_symbols(), s
    assert lib.stark_abi_version() == S.header_abi_version() >= 4


def test_group_has_fri_methods():
    from stark_amd.group import Group
    assert callable(getattr(Group, "prove_low_degree", None))
    assert callable(getattr(Group, "prove_low_degree_dev", None))


def test_client_builds_and_links():
    subprocess.run(["make", "-s", "-C", CLIENT], check=True)
    out = subprocess.run(["ldd", BIN], capture_output=True, text=True, check=True).stdout
    assert "libstark_hip.so" in out and "not found" not in out.split("libstark_hip.so")[1].splitlines()[0]


@pytest.mark.gpu
def test_group_fri_client_matches_oracle(oracle, tmp_path):
    assert os.path.exists(BIN), "build() compiles tests/abi_client_group_fri/group_fri_flow"
    G, log_n, exclude = 4, 17, 8
    n = 1 << log_n
    coeffs = O.random_elements(n // 4, 0x5EED0900 + log_n)
    w = O.root_of_unity(log_n)
    blob = struct.pack("<4I", log_n, len(coeffs), 0, exclude) + O.to_limbs([w]).tobytes() + coeffs.tobytes()
    (tmp_path / "in.bin").write_bytes(blob)
    r = subprocess.run([BIN, str(G), str(tmp_path / "in.bin"), str(tmp_path)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    want = oracle.prove_low_degree_json(oracle.best_fft(coeffs, w, log_n, cpus=8), w, n // 4, exclude, chunks=8)
    for name in ("fri.json", "fri_parts.json"):
        got = (tmp_path / name).read_bytes()
        if len(got) != len(want) or hashlib.sha256(got).digest() != hashlib.sha256(want.encode()).digest():
            a, b = json.loads(got), json.loads(want)
            diff = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            kind = next(iter(b[diff])) if diff < len(b) else "none"
            pytest.fail(f"{name}: {len(got)} B, expected {len(want)} B; first differing layer {diff} ({kind})")
