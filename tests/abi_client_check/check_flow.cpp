// A non-Python caller of the witness check (include/stark_hip.h), built against the header alone,
// making the calls a Rust host makes that screens witnesses before it proves them:
//   stark_r1cs_circuit_new                    the circuit, prepared once
//   stark_check_r1cs_circuit                  the witness as it is
//   stark_check_r1cs_circuit_batch            [the witness, the witness with its last value raised by one]
// Test infrastructure (tests/test_gpu_abi_client_check.py).
//   usage: check_flow <circuit.r1cs> <witness.wtns>
//   stdout, one report per witness: "witness <b>: status <s> n_failed <n>", then one line per listed failure,
//   "  constraint <i> a <hex> b <hex> c <hex>" (the values as big-endian hex numbers without leading zeros)
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

static std::string hex(const uint64_t v[4]) {
  char buf[65];
  snprintf(buf, sizeof buf, "%016llx%016llx%016llx%016llx", (unsigned long long)v[3], (unsigned long long)v[2],
           (unsigned long long)v[1], (unsigned long long)v[0]);
  std::string s(buf);
  const size_t k = s.find_first_not_of('0');
  return k == std::string::npos ? "0" : s.substr(k);
}

static void report(uint32_t b, stark_status st, uint32_t n_failed, const stark_r1cs_failure* f, uint32_t cap) {
  printf("witness %u: status %d n_failed %u\n", b, (int)st, n_failed);
  for (uint32_t k = 0; k < n_failed && k < cap; ++k)
    printf("  constraint %u a %s b %s c %s\n", f[k].constraint, hex(f[k].a).c_str(), hex(f[k].b).c_str(),
           hex(f[k].c).c_str());
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s <circuit.r1cs> <witness.wtns>\n", argv[0]);
    return 1;
  }
  if (stark_abi_version() != STARK_ABI_VERSION) {
    fprintf(stderr, "library ABI %u, header %u\n", stark_abi_version(), STARK_ABI_VERSION);
    return 1;
  }
  const std::vector<uint8_t> r1cs = read_file(argv[1]), good = read_file(argv[2]);
  // the last value of a .wtns file is its last field_size bytes; the field size sits behind the 24-byte prologue
  std::vector<uint8_t> bad = good;
  if (bad.size() < 28) return 1;
  const uint32_t fs = bad[24] | bad[25] << 8 | bad[26] << 16 | (uint32_t)bad[27] << 24;
  if (fs == 0 || fs > 32 || bad.size() < 28 + (size_t)fs) return 1;
  for (size_t i = bad.size() - fs; i < bad.size() && ++bad[i] == 0; ++i) {
  }
  check(stark_ctx_create(0, &g_ctx), "ctx_create");
  stark_r1cs_circuit* circuit = nullptr;
  check(stark_r1cs_circuit_new(g_ctx, r1cs.data(), r1cs.size(), &circuit), "r1cs_circuit_new");

  const uint32_t cap = 4;
  uint32_t n1 = 99;
  std::vector<stark_r1cs_failure> f1(cap);
  const stark_status s1 = stark_check_r1cs_circuit(g_ctx, circuit, good.data(), good.size(), &n1, f1.data(), cap);
  if (s1 != STARK_OK && s1 != STARK_ERR_CHECK) check(s1, "check_r1cs_circuit");
  printf("single\n");
  report(0, s1, n1, f1.data(), cap);

  const uint8_t* ws[2] = {good.data(), bad.data()};
  const size_t lens[2] = {good.size(), bad.size()};
  stark_status sts[2];
  uint32_t nf[2];
  std::vector<stark_r1cs_failure> f2(2 * cap);
  check(stark_check_r1cs_circuit_batch(g_ctx, circuit, ws, lens, 2, sts, nf, f2.data(), cap), "check_r1cs_circuit_batch");
  printf("batch\n");
  for (uint32_t b = 0; b < 2; ++b) report(b, sts[b], nf[b], f2.data() + (size_t)b * cap, cap);

  stark_r1cs_circuit_free(circuit);
  stark_ctx_destroy(g_ctx);
  return 0;
}
