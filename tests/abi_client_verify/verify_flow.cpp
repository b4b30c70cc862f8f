// A non-Python caller of batched verification from proof handles (include/stark_hip.h), built
// against the header alone, making the calls a Rust host makes that has just proved a batch, or that holds
// StarkProof values received over the wire:
//   prove_with_witness x 3 (run.rs:310-452)   -> stark_r1cs_circuit_new + stark_prove_r1cs_circuit_batch
//   verify_with_witness x 3 (run.rs:454-526)  -> stark_verify_r1cs_circuit_batch_proofs on the handles
//   a StarkProof value (utils.rs:122-130)     -> stark_r1cs_proof_from_parts, from proof 1's accessors; and a second
//                                                copy with one byte of a main leaf flipped
//   verify [original, rebuilt, tampered]      -> stark_verify_r1cs_circuit_batch_proofs
// No proof text is rendered or parsed on the way.  Test infrastructure (tests/test_gpu_abi_client_verify.py).
//   usage: verify_flow <circuit.r1cs> <witness.wtns> <public.bin>
//   public.bin: the public wires, 32 little-endian bytes each
//   stdout: "handles: s/r s/r s/r" and "rebuilt: s/r s/r s/r" (status/reasons, reasons in hex)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "stark_hip.h"

static stark_ctx* g_ctx = nullptr;

static void check(stark_status rc, const char* what) {
  if (rc != STARK_OK) {
    fprintf(stderr, "%s: %s (%s)\n", what, stark_status_str(rc), g_ctx ? stark_ctx_last_error(g_ctx) : "");
    exit(2);
  }
}

static std::vector<uint8_t> read_file(const char* path) {
  std::vector<uint8_t> v;
  FILE* f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "cannot read %s\n", path);
    exit(3);
  }
  uint8_t buf[65536];
  for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + n);
  fclose(f);
  return v;
}

// One set of openings read through its accessor, and the stark_branches over it.
struct Openings {
  std::vector<uint8_t> leaves, nodes;
  size_t k = 0, leaf_len = 0, depth = 0;
  stark_branches view() const { return stark_branches{leaves.data(), nodes.data(), k, leaf_len, depth}; }
};

// A StarkProof value's parts, as a host that built them itself (or deserialised them) holds them.
struct Parts {
  uint8_t m_root[32], l_root[32], a_root[32];
  Openings main, lcomb;
  struct Layer {
    uint8_t root2[32];
    Openings column, poly;
  };
  std::vector<Layer> layers;
  std::vector<uint8_t> last;
};

static Parts parts_of(const stark_r1cs_proof* p) {
  Parts q;
  check(stark_r1cs_proof_roots(p, q.m_root, q.l_root, q.a_root), "proof_roots");
  for (int which = 0; which < 2; ++which) {
    Openings& o = which ? q.lcomb : q.main;
    check(stark_r1cs_proof_branches(p, which, &o.k, &o.leaf_len, &o.depth, nullptr, 0, nullptr, 0), "proof_branches");
    o.leaves.resize(o.k * o.leaf_len);
    o.nodes.resize(o.k * o.depth * 32);
    check(stark_r1cs_proof_branches(p, which, nullptr, nullptr, nullptr, o.leaves.data(), o.leaves.size(),
                                    o.nodes.data(), o.nodes.size()),
          "proof_branches (data)");
  }
  const stark_fri_proof* fri = stark_r1cs_proof_fri(p);
  for (size_t i = 0; i < stark_fri_proof_num_layers(fri); ++i) {
    int is_last = 0;
    Parts::Layer L;
    size_t n_last = 0;
    L.column.leaf_len = L.poly.leaf_len = 32;
    check(stark_fri_proof_layer_info(fri, i, &is_last, L.root2, &L.column.k, &L.column.depth, &L.poly.k, &L.poly.depth,
                                     &n_last),
          "layer_info");
    L.column.leaves.resize(32 * L.column.k);
    L.column.nodes.resize(32 * L.column.k * L.column.depth);
    L.poly.leaves.resize(32 * L.poly.k);
    L.poly.nodes.resize(32 * L.poly.k * L.poly.depth);
    std::vector<uint8_t> last(32 * n_last);
    check(stark_fri_proof_layer_data(fri, i, L.column.leaves.data(), L.column.leaves.size(), L.column.nodes.data(),
                                     L.column.nodes.size(), L.poly.leaves.data(), L.poly.leaves.size(),
                                     L.poly.nodes.data(), L.poly.nodes.size(), last.data(), last.size()),
          "layer_data");
    if (is_last) q.last = last;
    else q.layers.push_back(L);
  }
  return q;
}

static stark_r1cs_proof* handle_of(const Parts& q) {
  std::vector<stark_fri_layer_parts> layers;
  for (const Parts::Layer& L : q.layers) layers.push_back(stark_fri_layer_parts{L.root2, L.column.view(), L.poly.view()});
  const stark_branches mb = q.main.view(), lb = q.lcomb.view();
  stark_r1cs_proof* h = nullptr;
  check(stark_r1cs_proof_from_parts(q.m_root, q.l_root, q.a_root, &mb, &lb, layers.data(), layers.size(), q.last.data(),
                                    q.last.size() / 32, &h),
        "r1cs_proof_from_parts");
  return h;
}

static void verify_and_print(const char* what, const stark_r1cs_circuit* circuit, const std::vector<uint8_t>& pub,
                             const stark_r1cs_proof* const* proofs) {
  const uint8_t* pubs[3] = {pub.data(), pub.data(), pub.data()};
  stark_status st[3];
  uint32_t why[3];
  check(stark_verify_r1cs_circuit_batch_proofs(g_ctx, circuit, pubs, pub.size() / 32, proofs, 3, st, why), what);
  printf("%s: %d/%x %d/%x %d/%x\n", what, (int)st[0], why[0], (int)st[1], why[1], (int)st[2], why[2]);
}

int main(int argc, char** argv) {
  if (argc != 4) {
    fprintf(stderr, "usage: verify_flow <circuit.r1cs> <witness.wtns> <public.bin>\n");
    return 1;
  }
  const std::vector<uint8_t> r1cs = read_file(argv[1]), wtns = read_file(argv[2]), pub = read_file(argv[3]);
  if (stark_abi_version() != STARK_ABI_VERSION) {
    fprintf(stderr, "library ABI %u, header %u\n", stark_abi_version(), STARK_ABI_VERSION);
    return 4;
  }
  check(stark_ctx_create(0, &g_ctx), "ctx_create");
  stark_r1cs_circuit* circuit = nullptr;
  check(stark_r1cs_circuit_new(g_ctx, r1cs.data(), r1cs.size(), &circuit), "r1cs_circuit_new");

  const uint8_t* ws[3] = {wtns.data(), wtns.data(), wtns.data()};
  const size_t lens[3] = {wtns.size(), wtns.size(), wtns.size()};
  stark_r1cs_proof* proofs[3] = {nullptr, nullptr, nullptr};
  check(stark_prove_r1cs_circuit_batch(g_ctx, circuit, ws, lens, 3, proofs, nullptr), "prove_r1cs_circuit_batch");
  verify_and_print("handles", circuit, pub, proofs);

  Parts parts = parts_of(proofs[1]);
  stark_r1cs_proof* rebuilt = handle_of(parts);
  parts.main.leaves[5 * parts.main.leaf_len + 40] ^= 1;  // one byte of main leaf 5
  stark_r1cs_proof* tampered = handle_of(parts);
  const stark_r1cs_proof* mixed[3] = {proofs[1], rebuilt, tampered};
  verify_and_print("rebuilt", circuit, pub, mixed);

  stark_r1cs_proof_free(rebuilt);
  stark_r1cs_proof_free(tampered);
  for (stark_r1cs_proof* p : proofs) stark_r1cs_proof_free(p);
  stark_r1cs_circuit_free(circuit);
  stark_ctx_destroy(g_ctx);
  return 0;
}
