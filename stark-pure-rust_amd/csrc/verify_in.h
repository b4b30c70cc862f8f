// The verifier's parsed proof and the pieces of verify.hip that the batched verifier (verify_batch.hip) shares
// with the single-proof one: the reader, the sampler, the transcript values and the Last layer's check.
#pragma once
#include <memory>
#include <vector>

#include "internal.h"

namespace stark {

// ---- the proof, as serde_json writes it (utils.rs:122-130, merkle_tree.rs:14-18, fri.rs:16-26) ----

// Bytes held elsewhere: the proof text's arena (ProofIn::arena) or the caller's arrays.  A parsed proof
// makes no allocation per opening (freeing ~3,600 small vectors written by 16 threads took ~0.27 ms of a
// 1.35 ms pedersen verify, profiles/r05_verify_phases.txt).
struct Bytes {
  const uint8_t* p = nullptr;
  size_t n = 0;
  const uint8_t* data() const { return p; }
  size_t size() const { return n; }
  const uint8_t* begin() const { return p; }
  const uint8_t* end() const { return p + n; }
};

struct Branch {  // commitment::merkle_tree::Proof
  Bytes leaf;
  Bytes nodes;  // 32 B each, leaf -> root
};

struct FriIn {  // FriProof::Middle { root2, column_branches, poly_branches } | Last { last }
  bool last = false;
  uint8_t root2[32] = {0};
  std::vector<Branch> col, poly;
  std::vector<std::vector<uint8_t>> last_vals;
};

struct ProofIn {
  uint8_t m_root[32], l_root[32], a_root[32];
  std::vector<Branch> main, lcomb;
  std::vector<FriIn> fri;
  // The openings' bytes: the opening whose text starts at offset t is written from arena + t / 2 (a
  // number takes two characters at least, so an opening's bytes end before its text's end / 2 and
  // openings side by side never overlap; pre_parse_branches bounds each parallel parse by the next
  // candidate's start, so a candidate nested inside another opening cannot write into it).
  std::unique_ptr<uint8_t[]> arena;
};

// The StarkProof JSON into pr; false where serde_json::from_reader fails (run.rs:579).  serial: the whole text
// on the calling thread (no host_parallel inside: the caller runs one proof per host worker); the parse is the
// same either way.
bool read_proof(const char* proof_json, size_t json_len, ProofIn& pr, bool serial = false);
// get_pseudorandom_indices (fri/src/utils.rs:75-117) as size_t; false where the reference panics.
bool sampler(const uint8_t seed[32], size_t modulus, uint32_t count, uint32_t excl, std::vector<size_t>& out);
// verify_r1cs_proof (verify.rs:13-258) for a prepared circuit; `pub_bytes` holds the public wires as 32-byte
// little-endian integers (from_bytes_le, run.rs:477-480).
stark_status verify_r1cs(stark_ctx* ctx, const PreparedCircuit& c, const uint8_t* pub_bytes, size_t n_public,
                         const ProofIn& pr);
// The trace's sizes as verify_r1cs_proof derives them (verify.rs:40-63): steps, precision = 8 steps, and
// g2 = 7^((p - 1) / precision).
struct VerifyDomain {
  uint64_t steps, prec, skips;
  HostFp g2;
};
VerifyDomain verify_domain(size_t os);
// The boundary points x_k = g2^(skips slot_k) of the public wires' first uses (Zb2's roots), and I2's
// coefficients through the wires' values there (verify.rs:151-155, utils.rs:421-474): host lagrange_interp
// below the context's public-column threshold, stark_lagrange_interp_domain from it on.
std::vector<HostFp> verify_boundary_points(const PreparedCircuit& c, const VerifyDomain& d);
stark_status verify_interp2(stark_ctx* ctx, const PreparedCircuit& c, const std::vector<HostFp>& pub,
                            const VerifyDomain& d, const std::vector<HostFp>& bx, std::vector<HostFp>& interp2);
// r from a_root (utils.rs:272-290) and k from m_root (verify.rs:164-173); false where the sampler panics.
bool verify_challenges(const ProofIn& pr, uint64_t prec, HostFp r[3], HostFp kk[11]);
// verify_low_degree_proof (fri.rs:226-404) on a parsed Vec<FriProof>: what stark_verify_low_degree_proof returns
// for these parts (root: the root of unity's Montgomery image).
stark_status verify_fri_single(const uint8_t merkle_root[32], const HostFp& root, const std::vector<FriIn>& proof,
                               size_t max_deg_plus_1, uint32_t excl);
// The FriProof::Last element's checks (fri.rs:346-403) against the tree root, root of unity and degree bound
// that the Middle layers before it leave.
stark_status fri_last_check(const FriIn& last, const uint8_t m_root[32], const HostFp& root, size_t max_deg_plus_1,
                            uint32_t excl);

}  // namespace stark
