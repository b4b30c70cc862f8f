"""Resources of the two kernels that batched verification from handles adds (the transcript and the boundary
interpolants on the device), from the code object's notes of a gfx950 cross-compile (no GPU needed):

    python tools/verify_handles_kernel_meta.py [--out profiles/verify_handles_kernel_meta.txt]

Read as tools/verify_batch_kernel_meta.py reads the three check kernels' rows (the same compile of
csrc/verify_batch.hip); those rows are printed beside the new ones so that one run shows the whole file.  Exit
status 1 when a new kernel is missing or has scratch."""
import argparse
import sys
import tempfile

import verify_batch_kernel_meta as M

NEW = ["verify_transcript_batch_kernel", "verify_interp2_batch_kernel"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    old = list(M.KERNELS)
    M.KERNELS[:] = old + NEW  # (kernels() collects the names listed there)
    with tempfile.TemporaryDirectory() as tmp:
        got = M.kernels(tmp)
    M.KERNELS[:] = old
    lines = ["Batched verification from proof handles: resources of its two kernels, gfx950 cross-compile",
             "(hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S of csrc/verify_batch.hip;",
             "tools/verify_handles_kernel_meta.py).  vgpr / sgpr / lds bytes / scratch bytes from the code object's",
             "notes (.vgpr_count, .sgpr_count, .group_segment_fixed_size, .private_segment_fixed_size).", ""]
    fmt = "{:32s} vgpr {:>4} sgpr {:>4} lds {:>6} scratch {:>4}"
    lines.append("== new ==")
    lines += [fmt.format(k, *got[k]) for k in NEW if k in got]
    lines += ["", "== the three check kernels of the same file (tools/verify_batch_kernel_meta.py's rows) =="]
    lines += [fmt.format(k, *got[k]) for k in old if k in got]
    missing = [k for k in NEW if k not in got]
    spills = [k for k in NEW if k in got and got[k][3]]
    lines += ["", "verify_transcript_batch_kernel: one wave per proof; its LDS holds the chains' words (28 chains of 80",
              "words at most), the 80 positions and the layers' 40 rows.  Each Blake2s chain runs on a lane of its own",
              "with the whole compression's state in registers (b2s_short, as the prover's r1cs_r_kernel).",
              "verify_interp2_batch_kernel: one lane per (proof, coefficient), a product and a sum per term.",
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
