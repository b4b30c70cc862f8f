"""Resources of the batched verifier's three kernels from the code object's notes of a gfx950 cross-compile (no
GPU needed):

    python tools/verify_batch_kernel_meta.py [--out profiles/verify_batch_kernel_meta.txt]

csrc/verify_batch.hip is compiled device-only to assembly (hipcc -O3 -std=c++17 --offload-arch=gfx950
--cuda-device-only -S), and every kernel's VGPRs, SGPRs, LDS bytes and scratch bytes are read from the
.amdgpu_metadata notes.  The single-proof verifier has no kernels of its own (its checks run on the host), so
there is no parent column.  Exit status 1 when a kernel is missing or has scratch."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["verify_paths_batch_kernel", "verify_fri_rows_batch_kernel", "verify_spot_batch_kernel"]
KEYS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels(tmp: str) -> dict:
    """kernel name -> (vgpr, sgpr, lds, scratch)."""
    asm = os.path.join(tmp, "verify_batch.s")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950",
                    "--cuda-device-only", "-S", "-w", "-I" + os.path.join(ROOT, "include"), "-o", asm,
                    os.path.join(ROOT, "stark-pure-rust_amd", "csrc", "verify_batch.hip")], check=True)
    out = {}
    for blk in re.findall(r"(- \.agpr_count.*?\.wavefront_size)", open(asm).read(), re.S):
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        for k in KERNELS:
            if f"{len(k)}{k}E" in name:  # (Itanium mangling: <length><name>)
                out[k] = tuple(int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1)) for key in KEYS)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        got = kernels(tmp)
    lines = ["Batched verification of one circuit's proofs: resources of its kernels, gfx950 cross-compile",
             "(hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S of csrc/verify_batch.hip;",
             "tools/verify_batch_kernel_meta.py).  vgpr / sgpr / lds bytes / scratch bytes from the code object's",
             "notes (.vgpr_count, .sgpr_count, .group_segment_fixed_size, .private_segment_fixed_size).", ""]
    fmt = "{:32s} vgpr {:>4} sgpr {:>4} lds {:>6} scratch {:>4}"
    missing = [k for k in KERNELS if k not in got]
    for k in KERNELS:
        if k in got:
            lines.append(fmt.format(k, *got[k]))
    spills = [k for k in KERNELS if k in got and got[k][3]]
    path_vgprs = got.get(KERNELS[0], ("?",))[0]
    lines += ["", f"One path, row or position per lane in all three.  At {path_vgprs} VGPRs the path kernel keeps a whole",
              "compression's state per lane at full occupancy (eight waves per SIMD up to 64 VGPRs), so the quad form",
              "(hash_pair_quad, a compression spread over four lanes with its message in LDS) was not taken.",
              f"kernels with scratch: {', '.join(spills) if spills else 'none'}"]
    if missing:
        lines.append(f"kernels not found: {', '.join(missing)}")
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(1 if spills or missing else 0)


if __name__ == "__main__":
    main()
