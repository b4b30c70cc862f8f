// A C++ caller of batched FRI verification, built against include/stark_hip.h alone:
//   fri_verify_flow <log_n> <max_deg_plus_1> <exclude> <root.bin> <coeffs.bin>
// root.bin: the root of unity of order 2^log_n (4 little-endian u64); coeffs.bin: batch x max_deg_plus_1
// coefficients (32 B each).  It evaluates the polynomials (stark_best_fft), commits the vectors (a Merkle
// forest), proves the batch (stark_prove_low_degree_batch), verifies the handles (stark_verify_low_degree_batch),
// rebuilds proof 1 from its accessors with stark_fri_proof_from_parts, flips one bit of a polynomial leaf in a
// second rebuilt copy and verifies [original, rebuilt, tampered] against proof 1's root.  Prints
//   handles: <status>/<reasons hex> ...
//   rebuilt: <status>/<reasons hex> x 3
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "stark_hip.h"

#define CHECK(call)                                                              \
  do {                                                                           \
    stark_status st_ = (call);                                                   \
    if (st_ != STARK_OK) {                                                       \
      fprintf(stderr, "%s: %s\n", #call, stark_status_str(st_));                 \
      return 1;                                                                  \
    }                                                                            \
  } while (0)

static std::vector<uint8_t> read_file(const char* path) {
  std::vector<uint8_t> v;
  FILE* f = fopen(path, "rb");
  if (!f) return v;
  fseek(f, 0, SEEK_END);
  v.resize((size_t)ftell(f));
  fseek(f, 0, SEEK_SET);
  if (fread(v.data(), 1, v.size(), f) != v.size()) v.clear();
  fclose(f);
  return v;
}

// A proof's parts read through the accessors, and the stark_fri_layer_parts over them.
struct Parts {
  struct Layer {
    uint8_t root2[32];
    size_t n_col, col_depth, n_poly, poly_depth;
    std::vector<uint8_t> col_leaves, col_nodes, poly_leaves, poly_nodes;
  };
  std::vector<Layer> layers;
  std::vector<uint8_t> last;
  stark_status read(const stark_fri_proof* p) {
    const size_t n = stark_fri_proof_num_layers(p);
    for (size_t i = 0; i < n; ++i) {
      int is_last = 0;
      Layer L;
      size_t n_last = 0;
      stark_status st = stark_fri_proof_layer_info(p, i, &is_last, L.root2, &L.n_col, &L.col_depth, &L.n_poly,
                                                   &L.poly_depth, &n_last);
      if (st != STARK_OK) return st;
      if (is_last) {
        last.resize(32 * n_last);
        st = stark_fri_proof_layer_data(p, i, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, last.data(), last.size());
      } else {
        L.col_leaves.resize(32 * L.n_col);
        L.col_nodes.resize(32 * L.n_col * L.col_depth);
        L.poly_leaves.resize(32 * L.n_poly);
        L.poly_nodes.resize(32 * L.n_poly * L.poly_depth);
        st = stark_fri_proof_layer_data(p, i, L.col_leaves.data(), L.col_leaves.size(), L.col_nodes.data(),
                                        L.col_nodes.size(), L.poly_leaves.data(), L.poly_leaves.size(),
                                        L.poly_nodes.data(), L.poly_nodes.size(), nullptr, 0);
        layers.push_back(L);
      }
      if (st != STARK_OK) return st;
    }
    return STARK_OK;
  }
  stark_status handle(stark_fri_proof** out) const {
    std::vector<stark_fri_layer_parts> v;
    for (const Layer& L : layers)
      v.push_back({L.root2,
                   {L.col_leaves.data(), L.col_nodes.data(), L.n_col, 32, L.col_depth},
                   {L.poly_leaves.data(), L.poly_nodes.data(), L.n_poly, 32, L.poly_depth}});
    return stark_fri_proof_from_parts(v.data(), v.size(), last.data(), last.size() / 32, out);
  }
};

int main(int argc, char** argv) {
  if (argc != 6) {
    fprintf(stderr, "usage: fri_verify_flow log_n max_deg_plus_1 exclude root.bin coeffs.bin\n");
    return 2;
  }
  if (stark_abi_version() != STARK_ABI_VERSION) {
    fprintf(stderr, "library ABI %u, header %u\n", stark_abi_version(), STARK_ABI_VERSION);
    return 1;
  }
  const uint32_t log_n = (uint32_t)atoi(argv[1]);
  const size_t bound = (size_t)atol(argv[2]), n = (size_t)1 << log_n;
  const uint32_t excl = (uint32_t)atoi(argv[3]);
  const std::vector<uint8_t> root_b = read_file(argv[4]), coeffs = read_file(argv[5]);
  if (root_b.size() != 32 || coeffs.empty() || coeffs.size() % (32 * bound)) {
    fprintf(stderr, "bad input files\n");
    return 2;
  }
  const uint64_t* root = reinterpret_cast<const uint64_t*>(root_b.data());
  const uint32_t batch = (uint32_t)(coeffs.size() / (32 * bound));
  if (batch < 2) return 2;
  stark_ctx* ctx = nullptr;
  CHECK(stark_ctx_create(0, &ctx));
  std::vector<uint64_t> values((size_t)batch * n * 4);
  for (uint32_t b = 0; b < batch; ++b)
    CHECK(stark_best_fft(ctx, reinterpret_cast<const uint64_t*>(coeffs.data()) + (size_t)b * bound * 4, bound, root, log_n,
                         values.data() + (size_t)b * n * 4));
  stark_merkle_forest* forest = nullptr;
  CHECK(stark_merkle_forest_new(ctx, &forest));
  CHECK(stark_merkle_forest_update(forest, reinterpret_cast<const uint8_t*>(values.data()), n, 32, batch));
  std::vector<uint8_t> roots(32 * (size_t)batch);
  CHECK(stark_merkle_forest_roots(forest, roots.data()));
  std::vector<stark_fri_proof*> proofs(batch, nullptr);
  CHECK(stark_prove_low_degree_batch(ctx, values.data(), n, batch, root, bound, excl, proofs.data()));
  std::vector<stark_status> sts(batch);
  std::vector<uint32_t> why(batch);
  CHECK(stark_verify_low_degree_batch(ctx, roots.data(), root, proofs.data(), batch, bound, excl, sts.data(),
                                      why.data()));
  printf("handles:");
  for (uint32_t b = 0; b < batch; ++b) printf(" %d/%x", (int)sts[b], why[b]);
  printf("\n");
  Parts parts;
  CHECK(parts.read(proofs[1]));
  stark_fri_proof *rebuilt = nullptr, *tampered = nullptr;
  CHECK(parts.handle(&rebuilt));
  if (parts.layers.empty()) return 2;
  parts.layers[0].poly_leaves[32 * 9 + 2] ^= 0x10;
  CHECK(parts.handle(&tampered));
  const stark_fri_proof* three[3] = {proofs[1], rebuilt, tampered};
  uint8_t roots3[96];
  for (int k = 0; k < 3; ++k)
    for (int i = 0; i < 32; ++i) roots3[32 * k + i] = roots[32 + i];
  CHECK(stark_verify_low_degree_batch(ctx, roots3, root, three, 3, bound, excl, sts.data(), why.data()));
  printf("rebuilt:");
  for (int b = 0; b < 3; ++b) printf(" %d/%x", (int)sts[b], why[b]);
  printf("\n");
  stark_fri_proof_free(rebuilt);
  stark_fri_proof_free(tampered);
  for (stark_fri_proof* p : proofs) stark_fri_proof_free(p);
  stark_merkle_forest_free(forest);
  stark_ctx_destroy(ctx);
  return 0;
}
