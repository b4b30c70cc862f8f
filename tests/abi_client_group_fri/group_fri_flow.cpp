// A non-Python caller of the group FRI entry point (include/stark_hip.h), built
// against the header alone, making the calls a Rust host with a group configured makes:
//   fri::fft::best_fft (fft.rs:327)           -> stark_group_best_fft
//   fri::fri::prove_low_degree (fri.rs:46)    -> stark_group_prove_low_degree + stark_fri_proof_json
// and rebuilding the Vec<FriProof> from stark_fri_proof_layer_info / _layer_data, as the shim does when it
// builds FriProof<H> values without serde: the structured route on a group's proof.
// Test infrastructure (tests/test_group_fri_abi.py): the test compares both texts with the oracle's.
//   usage: group_fri_flow <G> <in.bin> <out_dir>
//   in.bin (as shim_flow): u32 log_n, u32 n_coeffs, u32 k, u32 exclude; u64 root[4]; u64 coeffs[4 * n_coeffs];
//   u64 idx[k] (not used here)
//   out: fri.json (the library's text), fri_parts.json (rebuilt from the parts)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "stark_hip.h"

static stark_group* g_group = nullptr;

static void check(stark_status rc, const char* what) {
  if (rc != STARK_OK) {  // the shim's ok(): a non-zero status is a panic
    fprintf(stderr, "%s: %s (%s)\n", what, stark_status_str(rc), g_group ? stark_group_last_error(g_group) : "");
    exit(2);
  }
}

static void write_file(const std::string& path, const void* data, size_t len) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || fwrite(data, 1, len, f) != len) {
    fprintf(stderr, "cannot write %s\n", path.c_str());
    exit(3);
  }
  fclose(f);
}

// serde_json of Vec<u8>
static void json_u8s(std::string& o, const uint8_t* p, size_t n) {
  o += '[';
  for (size_t i = 0; i < n; ++i) {
    if (i) o += ',';
    o += std::to_string((unsigned)p[i]);
  }
  o += ']';
}

// serde_json of Vec<Proof<Vec<u8>, BlakeDigest>> (merkle_tree.rs:14-18)
static void json_branches(std::string& o, const std::vector<uint8_t>& leaves, const std::vector<uint8_t>& nodes,
                          size_t k, size_t depth) {
  o += '[';
  for (size_t i = 0; i < k; ++i) {
    if (i) o += ',';
    o += "{\"leaf\":";
    json_u8s(o, leaves.data() + 32 * i, 32);
    o += ",\"nodes\":[";
    for (size_t d = 0; d < depth; ++d) {
      if (d) o += ',';
      json_u8s(o, nodes.data() + 32 * (i * depth + d), 32);
    }
    o += "]}";
  }
  o += ']';
}

int main(int argc, char** argv) {
  if (argc != 4) {
    fprintf(stderr, "usage: group_fri_flow <G> <in.bin> <out_dir>\n");
    return 1;
  }
  const uint32_t G = (uint32_t)atoi(argv[1]);
  FILE* f = fopen(argv[2], "rb");
  if (!f) return 1;
  uint32_t hdr[4];
  uint64_t root[4];
  if (fread(hdr, 4, 4, f) != 4 || fread(root, 8, 4, f) != 4) return 1;
  const uint32_t log_n = hdr[0], n_coeffs = hdr[1], exclude = hdr[3];
  const size_t n = (size_t)1 << log_n;
  std::vector<uint64_t> coeffs(4 * (size_t)n_coeffs);
  if (fread(coeffs.data(), 8, coeffs.size(), f) != coeffs.size()) return 1;
  fclose(f);
  const std::string out = argv[3];

  if (stark_abi_version() != STARK_ABI_VERSION) {
    fprintf(stderr, "library ABI %u, header %u\n", stark_abi_version(), STARK_ABI_VERSION);
    return 4;
  }
  std::vector<int> devices(G, 0);  // G members on device 0
  check(stark_group_create(devices.data(), G, &g_group), "stark_group_create");

  std::vector<uint64_t> evals(4 * n);
  check(stark_group_best_fft(g_group, coeffs.data(), n_coeffs, root, log_n, evals.data()), "group best_fft");

  // prove_low_degree::<Fp, BlakeDigest>(&values, root, n / 4, exclude) with the group as the worker pool
  stark_fri_proof* proof = nullptr;
  check(stark_group_prove_low_degree(g_group, evals.data(), n, root, n / 4, exclude, &proof), "group prove_low_degree");
  size_t len = 0;
  check(stark_fri_proof_json(proof, nullptr, 0, &len), "fri_proof_json (size)");
  std::string json(len + 1, '\0');
  check(stark_fri_proof_json(proof, &json[0], json.size(), &len), "fri_proof_json");
  write_file(out + "/fri.json", json.data(), len);

  // the same Vec<FriProof> from its parts (fri.rs:16-26)
  std::string parts = "[";
  const size_t layers = stark_fri_proof_num_layers(proof);
  for (size_t i = 0; i < layers; ++i) {
    int is_last = 0;
    uint8_t root2[32];
    size_t n_col = 0, col_depth = 0, n_poly = 0, poly_depth = 0, n_last = 0;
    check(stark_fri_proof_layer_info(proof, i, &is_last, root2, &n_col, &col_depth, &n_poly, &poly_depth, &n_last),
          "layer_info");
    std::vector<uint8_t> cl(32 * n_col), cn(32 * n_col * col_depth), pl(32 * n_poly), pn(32 * n_poly * poly_depth),
        last(32 * n_last);
    check(stark_fri_proof_layer_data(proof, i, cl.data(), cl.size(), cn.data(), cn.size(), pl.data(), pl.size(),
                                     pn.data(), pn.size(), last.data(), last.size()),
          "layer_data");
    if (i) parts += ',';
    if (is_last) {
      parts += "{\"Last\":{\"last\":[";
      for (size_t v = 0; v < n_last; ++v) {
        if (v) parts += ',';
        json_u8s(parts, last.data() + 32 * v, 32);
      }
      parts += "]}}";
    } else {
      parts += "{\"Middle\":{\"root2\":";
      json_u8s(parts, root2, 32);
      parts += ",\"column_branches\":";
      json_branches(parts, cl, cn, n_col, col_depth);
      parts += ",\"poly_branches\":";
      json_branches(parts, pl, pn, n_poly, poly_depth);
      parts += "}}";
    }
  }
  parts += ']';
  write_file(out + "/fri_parts.json", parts.data(), parts.size());

  stark_fri_proof_free(proof);
  stark_group_destroy(g_group);
  printf("group_fri_flow ok: G=%u n=%zu layers=%zu json=%zu B\n", G, n, layers, len);
  return 0;
}
