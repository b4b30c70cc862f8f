"""GPU: one StarkProof shared by `world` ranks (stark_amd/dprove.py with
libstark_hip's per-rank steps).  On the one-GPU test box the ranks share GPU 0
and exchange through gloo; the 8-GPU bench runs the same code over RCCL.
The proof must equal the single-GPU / oracle proof byte for byte."""
import datetime
import hashlib
import json
import os
import sys

import pytest
import torch
import torch.distributed as dist
from ranks import run_ranks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "r1cs")


def _worker(rank, world, port, name, log_synth, tail_log, out_q):
    import faulthandler
    faulthandler.dump_traceback_later(90, exit=True)   # a stuck rank prints its stack and exits
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=80))
    import stark_amd as S
    from stark_amd.dprove import GpuProverOps, prove_distributed
    from stark_amd.r1cs import prove_with_witness
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = S.Context(0)
    if name:
        r1 = open(os.path.join(FIX, f"{name}.r1cs"), "rb").read()
        wt = open(os.path.join(FIX, f"{name}.wtns"), "rb").read()
    else:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import synth_r1cs
        r1, wt = synth_r1cs.for_steps(log_synth)
    js = prove_distributed(GpuProverOps(ctx), r1, wt, fri_tail_log=tail_log)
    single = prove_with_witness(ctx, r1, wt).to_json() if rank == 0 and not name else None
    digest = lambda s: hashlib.sha256(s.encode()).hexdigest() if s is not None else None
    out_q.put((rank, digest(js), digest(single)))
    dist.barrier()
    ctx.close()
    dist.destroy_process_group()


def _run(world, name, log_synth=0, tail_log=16):
    res = {r: (a, b) for r, a, b in run_ranks(_worker, world, (name, log_synth, tail_log), timeout=110)}
    assert all(res[r][0] is None for r in range(1, world))
    return res[0]


@pytest.mark.parametrize("name,world,tail_log", [("compute", 2, 0), ("compute", 8, 16), ("poseidon3_test", 4, 0),
                                                 ("pedersen_test", 2, 16), ("pedersen_test", 8, 12), ("bits", 4, 0)])
def test_prove_distributed_gpu(name, world, tail_log):
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "r1cs_proofs.json")))
    got, _ = _run(world, name, tail_log=tail_log)
    assert got == golden[name]["json_sha256"]


@pytest.mark.parametrize("world", [1, 4])
def test_prove_distributed_gpu_synthetic(world):
    """A 2^14-step synthetic circuit: the distributed proof equals the single-GPU proof."""
    got, single = _run(world, None, 14)
    assert got == single


def _worker_circuit(rank, world, port, out_q):
    import faulthandler
    faulthandler.dump_traceback_later(90, exit=True)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=80))
    import stark_amd as S
    from stark_amd.dprove import DistCircuit, GpuProverOps, prove_distributed
    from stark_amd.r1cs import prove_with_witness
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth_r1cs
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = S.Context(0)
    r1, _ = synth_r1cs.for_steps(13)
    circ = DistCircuit(ctx, r1)
    got = []
    for inputs in [(5, 6), (7, 8)]:
        _, wt = synth_r1cs.for_steps(13, inputs=inputs)
        js = prove_distributed(GpuProverOps(ctx), None, wt, circuit=circ)
        if rank == 0:
            got.append(hashlib.sha256(js.encode()).hexdigest() ==
                       hashlib.sha256(prove_with_witness(ctx, r1, wt).to_json().encode()).hexdigest())
    r1p, wtp = open(os.path.join(FIX, "pedersen_test.r1cs"), "rb").read(), open(os.path.join(FIX, "pedersen_test.wtns"), "rb").read()
    js = prove_distributed(GpuProverOps(ctx), None, wtp, circuit=DistCircuit(ctx, r1p))
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "r1cs_proofs.json")))
    if rank == 0:
        got.append(hashlib.sha256(js.encode()).hexdigest() == golden["pedersen_test"]["json_sha256"])
    out_q.put((rank, got))
    dist.barrier()
    del circ
    ctx.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [1, 4])
def test_prove_distributed_prepared_circuit(world):
    """DistCircuit: two witnesses of one synthetic circuit equal the single-GPU proofs; pedersen_test
    equals the golden digest."""
    res = dict(run_ranks(_worker_circuit, world, (), timeout=110))
    assert res[0] == [True, True, True]


def _worker_synth20(rank, world, port, prepared, out_q):
    """The sha256_2_test stand-in (synthetic 2^20-step circuit, precision 2^23) through the multi-rank
    prover: rank 0's StarkProof JSON digest, to be compared with the oracle's
    (tests/golden/large_digests.json, mk_r1cs_proof restated in oracle/r1cs.c, prove.rs:14-378)."""
    import faulthandler
    faulthandler.dump_traceback_later(200, exit=True)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=180))
    import stark_amd as S
    from stark_amd.dprove import DistCircuit, GpuProverOps, prove_distributed
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth_r1cs
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = S.Context(0)
    r1, wt = synth_r1cs.for_steps(20)
    if prepared:
        circ = DistCircuit(ctx, r1)
        js = prove_distributed(GpuProverOps(ctx), None, wt, circuit=circ)
    else:
        circ = None
        js = prove_distributed(GpuProverOps(ctx), r1, wt)
    out_q.put((rank, js if rank == 0 else None))
    dist.barrier()
    del circ
    ctx.close()
    dist.destroy_process_group()


def _differing_fields(js, ctx):
    """On a wrong digest: which StarkProof fields differ from the single-GPU proof, and where."""
    from stark_amd.r1cs import prove_with_witness
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth_r1cs
    r1, wt = synth_r1cs.for_steps(20)
    a, b = json.loads(js), json.loads(prove_with_witness(ctx, r1, wt).to_json())
    out = []
    for key in b:
        if a.get(key) != b[key]:
            va, vb = a.get(key), b[key]
            if isinstance(va, list) and isinstance(vb, list):
                idx = [i for i in range(min(len(va), len(vb))) if va[i] != vb[i]]
                out.append(f"{key}: {len(idx)} of {len(vb)} entries differ, first {idx[:6]}")
            else:
                out.append(f"{key}: differs")
    return "; ".join(out)


@pytest.mark.parametrize("world,prepared", [(4, False), (8, False), (8, True)])
def test_prove_distributed_synth_2_20_vs_oracle_digest(world, prepared):
    """BASELINE config 5's stand-in at its size: one proof of the synthetic 2^20-step circuit over
    `world` ranks (cold, and from a DistCircuit) equals the oracle's StarkProof byte for byte
    (the digest tests/test_gpu_large.py pins the single-GPU prover to)."""
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "large_digests.json")))["prove_synth_2^20_steps"]
    res = dict(run_ranks(_worker_synth20, world, (prepared,), timeout=230))
    got = hashlib.sha256(res[0].encode()).hexdigest()
    if got != want["json_sha256"]:
        import stark_amd as S
        c = S.Context(0)
        try:
            detail = _differing_fields(res[0], c)
        finally:
            c.close()
        pytest.fail(f"digest {got} != {want['json_sha256']}: {detail}")


# ---- the host-array entry points (stark_dprove_begin, stark_dprove_lincomb), in one process ----------
#
# stark_dprove_begin takes the prove.rs-level trace as host arrays with the flags as field elements (seven
# extended columns, no shared F0); stark_dprove_lincomb takes the main root as host bytes.  The reference
# for both is the path every other test here pins to the golden digests: stark_dprove_begin_bytes (the
# device trace builder, flag bytes) and stark_dprove_lincomb_dev, on the same context.

_TRACES = {}


def _python_trace(name):
    """The Python-built trace of a fixture as the arrays stark_dprove_begin takes (built once per name)."""
    if name not in _TRACES:
        import numpy as np
        import r1cs as R
        from oracle import to_limbs
        from stark_amd import _elems
        tr = R.build_trace(*R.load_fixture(FIX, name))
        u64 = lambda v: np.ascontiguousarray(np.asarray(v, dtype=np.uint64).reshape(-1))
        _TRACES[name] = dict(
            wit=_elems(to_limbs(tr.witness_trace)), comp=_elems(to_limbs(tr.computational_trace)),
            pub=_elems(to_limbs(tr.public_wires)), coef=_elems(to_limbs(tr.coefficients)),
            f0=_elems(to_limbs(tr.flag0)), f1=_elems(to_limbs(tr.flag1)), f2=_elems(to_limbs(tr.flag2)),
            pfi=u64([x for pair in tr.public_first_indices for x in pair]), n_pfi=len(tr.public_first_indices),
            perm=u64(tr.permuted_indices), n_constraints=tr.n_constraints, n_wires=tr.n_wires)
    return _TRACES[name]


def _begin_pair(ctx, name, world, rank):
    """(handle of stark_dprove_begin on the Python trace, handle of stark_dprove_begin_bytes on the fixture's
    bytes) for one rank, both on the context's own stream.  The caller frees them (_free)."""
    import ctypes
    from stark_amd import _p64, _szp, _vp
    t = _python_trace(name)
    szp = lambda a: a.ctypes.data_as(_szp)
    ha, hb = _vp(), _vp()
    try:
        ctx.check(ctx.lib.stark_dprove_begin(ctx.h, world, rank, _p64(t["wit"]), _p64(t["comp"]), len(t["coef"]),
                                             _p64(t["pub"]), len(t["pub"]), szp(t["pfi"]), t["n_pfi"],
                                             szp(t["perm"]), _p64(t["coef"]), _p64(t["f0"]), _p64(t["f1"]),
                                             _p64(t["f2"]), t["n_constraints"], t["n_wires"], None,
                                             ctypes.byref(ha)), "dprove_begin")
        r1 = open(os.path.join(FIX, f"{name}.r1cs"), "rb").read()
        wt = open(os.path.join(FIX, f"{name}.wtns"), "rb").read()
        ctx.check(ctx.lib.stark_dprove_begin_bytes(ctx.h, world, rank, r1, len(r1), wt, len(wt), None,
                                                   ctypes.byref(hb)), "dprove_begin_bytes")
    except Exception:
        _free(ctx, ha, hb)
        raise
    return ha, hb


def _free(ctx, *handles):
    for h in handles:
        if h:
            ctx.lib.stark_dprove_free(h)


def _info(ctx, h):
    """(precision, n_local, original_steps, g2 limbs, a_root) of stark_dprove_info."""
    import ctypes
    import numpy as np
    from stark_amd import _p64
    v = [ctypes.c_size_t(0) for _ in range(3)]
    g2 = np.zeros(4, dtype=np.uint64)
    a_root = ctypes.create_string_buffer(32)
    ctx.check(ctx.lib.stark_dprove_info(h, *[ctypes.byref(x) for x in v], _p64(g2), a_root), "dprove_info")
    return v[0].value, v[1].value, v[2].value, tuple(int(x) for x in g2), a_root.raw


def _device_bytes(ctx, ptr, nbytes):
    import numpy as np
    out = np.empty(nbytes, dtype=np.uint8)
    ctx.d2h(out, ptr)   # stark_memcpy_d2h, as GpuProverOps.to_host
    return out


def _rows_ptr(ctx, h):
    import ctypes
    from stark_amd import _vp
    p = _vp()
    ctx.check(ctx.lib.stark_dprove_rows(h, ctypes.byref(p)), "dprove_rows")
    return p.value


@pytest.mark.parametrize("name,world,rank", [("compute", 2, 0), ("compute", 2, 1), ("compute", 8, 5),
                                             ("poseidon3_test", 4, 3)])
def test_dprove_begin_host_arrays_equals_bytes(ctx, name, world, rank):
    """stark_dprove_begin on the Python-built trace gives the rank state of stark_dprove_begin_bytes: the
    same sizes, g2 and a_root, and the same n_local x 256 bytes of constraint rows.  (compute at world 8:
    P = steps = 16, the edge of degree < steps <= P; poseidon3_test: 6684 steps padded to 8192.)"""
    import numpy as np
    ha, hb = _begin_pair(ctx, name, world, rank)
    try:
        ia, ib = _info(ctx, ha), _info(ctx, hb)
        assert ia == ib
        prec, n_local, os_ = ia[:3]
        assert n_local == prec // world and os_ == len(_python_trace(name)["coef"])
        ra = _device_bytes(ctx, _rows_ptr(ctx, ha), n_local * 256)
        rb = _device_bytes(ctx, _rows_ptr(ctx, hb), n_local * 256)
        assert np.array_equal(ra, rb)
    finally:
        _free(ctx, ha, hb)


def test_dprove_lincomb_host_root_equals_device_root(ctx):
    """stark_dprove_lincomb (the main root as host bytes) gives the L of stark_dprove_lincomb_dev (the same
    32 bytes in device memory), on the handle pair of compute at (2, 0) with the golden m_root."""
    import ctypes
    import numpy as np
    from stark_amd import _vp
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "r1cs_proofs.json")))
    m_root = bytes.fromhex(golden["compute"]["m_root"])
    assert len(m_root) == 32
    ha, hb = _begin_pair(ctx, "compute", 2, 0)
    d_root = ctx.alloc(32)
    try:
        n_local = _info(ctx, ha)[1]
        assert _info(ctx, hb)[1] == n_local
        la, lb = _vp(), _vp()
        ctx.check(ctx.lib.stark_dprove_lincomb(ha, m_root, ctypes.byref(la)), "dprove_lincomb")
        ctx.h2d(d_root, np.frombuffer(m_root, dtype=np.uint8))
        ctx.check(ctx.lib.stark_dprove_lincomb_dev(hb, d_root, ctypes.byref(lb)), "dprove_lincomb_dev")
        ctx.synchronize()
        a = _device_bytes(ctx, la.value, n_local * 32)
        b = _device_bytes(ctx, lb.value, n_local * 32)
        assert a.any() and np.array_equal(a, b)
    finally:
        ctx.free(d_root)
        _free(ctx, ha, hb)
