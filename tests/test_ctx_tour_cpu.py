"""CPU: the tables of tests/ctx_tour.py against csrc/internal.h and against the report of the library's poison
hook, so that a buffer added to stark_ctx fails here until someone classifies it; and the tour table's shape."""
import os
import re

import pytest

import ctx_tour as T
import stark_amd as S

HERE = os.path.dirname(os.path.abspath(__file__))
INTERNAL_H = os.path.join(os.path.dirname(HERE), "stark-pure-rust_amd", "csrc", "internal.h")


def _ctx_struct() -> str:
    text = open(INTERNAL_H).read()
    m = re.search(r"^struct stark_ctx \{\n(.*?)^\};", text, re.S | re.M)
    assert m, "struct stark_ctx not found in csrc/internal.h"
    return re.sub(r"//[^\n]*", "", m.group(1))


def test_every_devbuf_member_is_classified_once():
    members = []
    for decl in re.findall(r"stark::DevBuf\s+([^;]+);", _ctx_struct()):
        members += [name.strip() for name in decl.split(",")]
    assert len(members) >= 19 and len(set(members)) == len(members)
    assert sorted(members) == sorted(T.DEVBUF_MEMBERS)
    assert len(set(T.DEVBUF_MEMBERS)) == len(T.DEVBUF_MEMBERS)
    for m in members:
        assert T.BUFFERS[m] in (T.SCRATCH, T.KEPT), m


def test_pinned_slot_count():
    body = _ctx_struct()
    ptrs = re.search(r"void\*\s+pinned\[(\d+)\]", body)
    sizes = re.search(r"size_t\s+pinned_bytes\[(\d+)\]", body)
    assert ptrs and sizes and int(ptrs.group(1)) == int(sizes.group(1)) == T.PINNED_SLOTS
    assert [k for k in T.BUFFERS if k.startswith("pinned[")] == ["pinned[%d]" % k for k in range(T.PINNED_SLOTS)]


def test_trees_forests_and_tables_are_classified():
    """The context's other owners of device memory: each is in the table under the name the report gives it."""
    body = _ctx_struct()
    n_trees = int(re.search(r"stark_merkle_tree\*\s+trees\[(\d+)\]", body).group(1))
    n_forests = int(re.search(r"stark_merkle_forest\*\s+r1cs_forests\[(\d+)\]", body).group(1))
    want = ["trees[%d]" % k for k in range(n_trees)] + ["r1cs_forests[%d]" % k for k in range(n_forests)]
    for name in ("fri_trees", "fri_forests", "verify_forest", "tw", "ext_idx", "post_tw", "interp_plans",
                 "eval_plans", "long_lists"):
        assert re.search(r"\b%s\b" % name, body), name
        want.append(name)
    for name in want:
        assert name in T.BUFFERS, name
    # every vector, map and handle the struct holds is one of them
    held = re.findall(r"std::(?:vector|map)<[^;]*>\s+(\w+);", body) + \
        re.findall(r"stark_merkle_(?:tree|forest)\*\s+(\w+)", body)
    assert sorted(set(held)) == sorted({n.split("[")[0] for n in want}), held
    assert set(T.UNREACHED) <= {k for k, c in T.BUFFERS.items() if c == T.SCRATCH}


def test_report_names_equal_the_table():
    """stark_test_poison_ctx with no context reports every name and class with 0 bytes (no device needed)."""
    try:
        report = S.poison_ctx(None, 0)
    except (OSError, RuntimeError) as e:  # (test_abi.py fails where the library does not load)
        pytest.fail(f"libstark_hip.so does not load: {e}")
    assert [n for n, _, _ in report] == list(T.BUFFERS)
    assert {n: c for n, _, c in report} == T.BUFFERS
    assert all(b == 0 for _, b, _ in report)


def test_tour_table_is_complete():
    assert len(T.OPS) >= 40
    for op in T.OPS:
        assert set(op.shapes) == {"A", "B"} and op.shapes["A"] != op.shapes["B"], op.name
        assert op.source in (T.ORACLE, T.PYTHON), op.name
        assert callable(op.run) and callable(op._want), op.name

