"""CPU: ABI 7's Merkle forest and batched prove_low_degree are exported, declared and bound.  No GPU compute
is called here."""
import stark_amd as S

NEW = ["stark_merkle_forest_new", "stark_merkle_forest_free", "stark_merkle_forest_update",
       "stark_merkle_forest_update_dev", "stark_merkle_forest_roots", "stark_merkle_forest_gen_proofs",
       "stark_prove_low_degree_batch", "stark_prove_low_degree_batch_dev"]


def test_batch_symbols_exported_and_declared():
    lib = S.load_library()
    declared = S.header_symbols()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in declared, name
        assert name in S._SIGNATURES, name
    assert S.header_abi_version() >= 7
    assert lib.stark_abi_version() == S.header_abi_version()


def test_batch_python_surface():
    for name in ("update_bytes", "update_dev", "roots", "gen_proofs"):
        assert callable(getattr(S.MerkleForest, name)), name
    assert callable(S.Context.prove_low_degree_batch)
    assert callable(S.Context.prove_low_degree_batch_dev)
