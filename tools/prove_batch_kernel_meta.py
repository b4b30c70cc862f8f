"""Resources of the kernels the batched prover touched, this tree against its parent's, from the code objects'
notes of a gfx950 cross-compile (no GPU needed):

    git worktree add /tmp/parent HEAD~1      # or any checkout of the parent commit
    python tools/prove_batch_kernel_meta.py --parent /tmp/parent [--out profiles/prove_batch_kernel_meta.txt]

Each of csrc/r1cs.hip and csrc/r1cs_trace_dev.hip is compiled device-only to assembly in both trees
(hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S), and every kernel's VGPRs, SGPRs, LDS bytes
and scratch bytes are read from the .amdgpu_metadata notes.  The single-proof kernels that now share their code
with a batched form (a __device__ body, or a template on a batched flag whose <false> instantiation is the kernel
as it was) must show the parent's four numbers; the batched kernels are listed after them.
Exit status 1 when a single-proof kernel differs or the batched constraint kernel has scratch."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ["r1cs.hip", "r1cs_trace_dev.hip"]
# single-proof kernels that share their code with a batched form: a __device__ body, or a template on a batched
# flag (the single proof's instantiation is <false>; the parent's kernel has the plain name)
TOUCHED = ["r1cs_r_kernel<false>", "r1cs_k_kernel", "r1cs_index_kernel", "r1cs_a_vals_kernel",
           "scan_block_kernel<false>", "scan_tot_kernel", "scan_apply_kernel", "r1cs_constraint_kernel<false>",
           "r1cs_lincomb_kernel", "wit_fill_kernel", "running_sum_kernel", "running_sum_long_kernel<false>"]
# single-proof kernels the batch launches as they are, over the proofs' arrays laid back to back
REUSED = ["r1cs_l_root_kernel", "r1cs_a_mini_kernel", "wit_decode_kernel"]
NEW = ["r1cs_r_kernel<true>", "r1cs_k_batch_kernel", "r1cs_l_root_batch_kernel", "r1cs_tr_init_batch_kernel",
       "r1cs_index_batch_kernel", "r1cs_a_vals_batch_kernel", "scan_block_kernel<true>", "scan_tot_batch_kernel",
       "scan_apply_batch_kernel", "r1cs_constraint_kernel<true>", "r1cs_lincomb_batch_kernel",
       "wit_fill_batch_kernel", "running_sum_batch_kernel", "running_sum_long_kernel<true>"]
KEYS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels(tree: str, tmp: str, tag: str) -> dict:
    """short kernel name -> (vgpr, sgpr, lds, scratch) for the FILES of the package under `tree`."""
    pkg = os.path.join(tree, "stark-pure-rust_amd")
    out = {}
    for f in FILES:
        asm = os.path.join(tmp, f"{tag}_{f}.s")
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950",
                        "--cuda-device-only", "-S", "-w", "-I" + os.path.join(tree, "include"), "-o", asm,
                        os.path.join(pkg, "csrc", f)], check=True)
        text = open(asm).read()
        for blk in re.findall(r"(- \.agpr_count.*?\.wavefront_size)", text, re.S):
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            vals = tuple(int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1)) for k in KEYS)
            for k in TOUCHED + REUSED + NEW:  # (Itanium mangling: <length><name>, then the template argument)
                base, _, flag = k.partition("<")
                arg = {"": "E", "false>": "ILb0EE", "true>": "ILb1EE"}[flag]
                if f"{len(base)}{base}{arg}" in name:
                    out[k] = vals
                if flag == "false>" and f"{len(base)}{base}E" in name:  # the parent's untemplated kernel
                    out[k] = vals
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="a checkout of the parent commit")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        old, new = kernels(a.parent, tmp, "parent"), kernels(ROOT, tmp, "this")
    lines = ["Batched proofs of one prepared circuit: resources of the kernels it touched, gfx950 cross-compile",
             "(hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S of csrc/r1cs.hip and",
             "csrc/r1cs_trace_dev.hip; tools/prove_batch_kernel_meta.py).  vgpr / sgpr / lds bytes / scratch bytes",
             "from the code objects' notes (.vgpr_count, .sgpr_count, .group_segment_fixed_size,",
             ".private_segment_fixed_size).",
             "", "== single-proof kernels that now share their code with a batched form: parent | this tree =="]
    fmt = "{:36s} vgpr {:>4} sgpr {:>4} lds {:>6} scratch {:>4}"
    bad = 0
    for k in TOUCHED + REUSED:
        same = old[k] == new[k]
        bad += not same
        lines.append(fmt.format(k, *old[k]) + "  |" + fmt.format("", *new[k])[36:] +
                     ("  equal" if same else "  DIFFERENT"))
    lines += ["", "(the last three are launched by the batch as they are, over the proofs' arrays laid back to back)",
              "", "== batched kernels (new) =="]
    for k in NEW:
        lines.append(fmt.format(k, *new[k]))
    scratch = new["r1cs_constraint_kernel<true>"][3]
    lines += ["",
              f"r1cs_constraint_kernel<true> (the batched form) at __launch_bounds__(256, 3): scratch {scratch} bytes",
              f"single-proof kernels that differ from the parent: {bad}"]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(1 if bad or scratch else 0)


if __name__ == "__main__":
    main()
