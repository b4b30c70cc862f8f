// Fiat-Shamir pieces that the prover's transcript kernels (r1cs.hip) and the batched verifier's
// (verify_batch.hip) share: a short message's Blake2s, the byte-order handling of the sampler's words and
// the reductions of a 256-bit integer below p.
#pragma once
#include "blake2s.h"
#include "internal.h"

namespace stark {

__device__ __forceinline__ uint32_t bswap32(uint32_t x) { return __builtin_bswap32(x); }

// Digest of a 32- or 33-byte message (words LE, zero padded).
__device__ __forceinline__ void b2s_short(const uint32_t* w, uint32_t extra_byte, uint32_t len, uint32_t out[8]) {
  uint32_t m[16];
#pragma unroll
  for (int i = 0; i < 8; ++i) m[i] = w[i];
  m[8] = extra_byte;
#pragma unroll
  for (int i = 9; i < 16; ++i) m[i] = 0;
  b2s_init(out);
  b2s_compress(out, m, len, 0, true);
}

// One of get_random_ff_values' elements (utils.rs:272-290): eight of the sampler's words (the digest bytes read
// big-endian, mod precision = 2^k) written back as big-endian bytes and read with from_bytes_le, canonical.
__device__ __forceinline__ fe challenge_r(const uint32_t* words, uint32_t prec_mask) {
  fe r;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t v = bswap32(words[i]) & prec_mask;  // BE word mod 2^k
    r.w[i] = bswap32(v);                               // BE bytes read as LE words
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) fe_reduce_once(r);
  return r;
}

// k_i = from_str(mk_seed([m_root, [i]])) (prove.rs:274-283, utils.rs:25-27, 51-57): the digest as a big-endian
// integer mod p, canonical.
__device__ __forceinline__ fe challenge_k(const uint32_t h[8]) {
  fe k;
#pragma unroll
  for (int j = 0; j < 8; ++j) k.w[j] = bswap32(h[7 - j]);
#pragma unroll
  for (int t = 0; t < 5; ++t) fe_reduce_once(k);
  return k;
}

}  // namespace stark
