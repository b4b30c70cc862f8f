// mk_r1cs_proof (packages/r1cs-stark/src/prove.rs:14-378) resident on one
// gfx950 GPU.
//
// Everything of size `steps` or `precision` lives in HBM from upload to
// proof; the host runs only the transcript (a_root -> r, m_root -> k,
// l_root -> positions, the FRI layer roots) and serialises the proof.
//
//   upload 6 step columns + permuted indices
//   index/accumulator kernel      IDX, PIDX, 40-B accumulator leaves
//   acc Merkle tree               -> a_root -> r (host, utils.rs:272-290)
//   batched iNTT(steps, g1) x 8 -> zero-pad -> batched NTT(precision, g2) x 8
//   A column: a_vals kernel, two product scans, multi_inv, iNTT/NTT
//   zb kernel + multi_inv         inverse Zb2 / Zb3 (0 -> 0)
//   constraint kernel             Q1..Q3 -> D1..D3, B2, B3 (with the
//                                 reference's divisibility asserts) written as
//                                 the 256-B main-tree rows P|A|S|D1|D2|D3|B2|B3
//   main Merkle tree (256-B leaves) -> m_root -> k (host, prove.rs:274-283)
//   linear-combination kernel     L, then its Merkle tree -> l_root
//   proof gathers + prove_low_degree on the resident L.
//
// Values are canonical in HBM; constants are Montgomery images so that
// fe_mul(data, const) is the canonical product (see fp_dev.h).
#include <string.h>

#include <string>
#include <vector>

#include "internal.h"
#include "blake2s.h"
#include "fe_db.h"
#include "transcript_dev.h"

namespace stark {
void json_bytes(std::string& o, const uint8_t* p, size_t n);
void json_branches(std::string& o, const std::vector<uint8_t>& leaves, size_t leaf_len,
                   const std::vector<uint8_t>& nodes, size_t k, size_t depth);
void fri_proof_json_string(const stark_fri_proof* proof, std::string& o);
}  // namespace stark

namespace stark {

static inline fe fe_zero_host() {
  fe r;
  for (int i = 0; i < 8; ++i) r.w[i] = 0;
  return r;
}

constexpr int kExtensionFactor = 8;     // utils.rs:135
constexpr int kLogExtensionFactor = 3;  // utils.rs:134
constexpr int kSpotChecks = 80;         // utils.rs:136
constexpr uint32_t kScanBlock = 1024;   // elements per workgroup in the product scan

// Montgomery image of R (montmul(x, r2) = Montgomery image of x) and of 1.
struct Mont {
  fe r2, one, unit;  // unit = canonical 1 (montmul(x_m, unit) = canonical x)
  fe rinv;           // R^-1 as a canonical value (montmul(x_m, rinv) = x R^-1)
};

static Mont mont() {
  const FieldHost& F = FieldHost::get();
  Mont m;
  HostFp one = F.one();
  m.r2 = to_dev(F.from_canonical(one.v));
  m.one = to_dev(one);
  m.unit = fe_zero_host();
  m.unit.w[0] = 1;
  const HostFp rv = F.from_canonical(one.v);  // the value R
  m.rinv = to_dev(F.inv(F.mul(rv, rv)));      // the value R^-2, whose Montgomery image is R^-1
  return m;
}

__device__ __forceinline__ fe fe_from_u64(uint64_t v) {
  fe r = fe_zero();
  r.w[0] = (uint32_t)v;
  r.w[1] = (uint32_t)(v >> 32);
  return r;
}

// Fiat-Shamir values derived on the device from the tree roots, so the proof
// is enqueued end to end without waiting for the host.
constexpr int kLincombConsts = 29;
struct Transcript {
  fe r0;       // canonical r[0]
  fe r1_m;     // Montgomery r[1], r[2]
  fe r2_m;
  fe k_m[11];  // Montgomery k[0..10]
  fe kx_m[8][3];  // Montgomery k3 + k4 xs_t, k5 + k6 xs_t, k7 + k8 xs_t (t = i mod 8)
  uint32_t roots[3][8];  // a_root, m_root, l_root (LE words = the digest bytes)
  int err;
  // Digit-basis tables (fe_db.h) of L's constants: k0, k1, k2, k9, k10, then kx[t][c] at 5 + 3 t + c.
  uint32_t k_db[kLincombConsts][72];
  // The constraint kernel's constants as digit-basis tables: r[1], r[2] (r1cs_r_kernel), and from the
  // host (upload_constraint_tables) R^-1 (the x R^-1 scalings) and the partial-fraction coefficients a_k.
  uint32_t r_db[2][72];
  uint32_t c_db[33][72];  // R^-1 | a_0..a_7 | inv(Z) R^k at t = i mod 8, table 9 + 8 k + t (invz_m)
};

// (bswap32, b2s_short, challenge_r and challenge_k: transcript_dev.h, shared with the batched verifier.)

// The digit-basis table of a canonical constant c: limb j of c 2^(32 i) mod p at 9 i + j, each row one
// product by the Montgomery image of 2^(32 i) (Pow32), one row per thread.
__device__ __forceinline__ void db_limbs(const fe& c, uint32_t* __restrict__ out) {  // 9 x 29-bit limbs of c
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    const int bit = 29 * j, w = bit >> 5, sh = bit & 31;
    uint32_t v = c.w[w] >> sh;
    if (sh > 3 && w < 7) v |= c.w[w + 1] << (32 - sh);
    out[j] = v & STARK_DB_M29;
  }
}

// Montgomery images of 2^(32 i) mod p, i < 8: a digit-basis table's rows as independent products.
struct Pow32 {
  fe m[8];
};

// The trees of a forest as a batched kernel reads their roots: tree b's root words at nodes + b stride + root_at
// (forest_nodes_dev).
struct ForestRoots {
  const uint32_t* nodes;
  uint64_t stride, root_at;
  __device__ __forceinline__ const uint32_t* root(uint64_t b) const { return nodes + b * stride + root_at; }
};

// r = get_random_ff_values(a_root, precision, 3, 0) (utils.rs:272-290):
// get_pseudorandom_indices(seed, precision, 24, 0) (fri/src/utils.rs:82-109)
// expands seed || B(seed) || B(B(seed)), reads 24 big-endian words mod
// precision; each group of 8 is written as big-endian bytes and read back
// with from_bytes_le (mod p).
// (BATCH: for proof blockIdx.x of a batch, its accumulator tree's root in the forest `acc` and its transcript
// tr[blockIdx.x]; the single proof's instantiation is the kernel as it was, `acc` unread.)
template <bool BATCH>
__global__ void r1cs_r_kernel(const uint32_t* __restrict__ a_root, uint32_t prec_mask, fe r2, Pow32 p32,
                              Transcript* __restrict__ tr, ForestRoots acc) {
  if constexpr (BATCH) {
    a_root = acc.root(blockIdx.x);
    tr += blockIdx.x;
  }
  __shared__ fe rs[2];
  if (threadIdx.x == 0) {
    uint32_t data[24];
#pragma unroll
    for (int i = 0; i < 8; ++i) data[i] = a_root[i];
    b2s_short(data, 0, 32, data + 8);
    b2s_short(data + 8, 0, 32, data + 16);
    fe r[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = challenge_r(data + 8 * c, prec_mask);
    tr->r0 = r[0];
    tr->r1_m = fe_mul(r[1], r2);
    tr->r2_m = fe_mul(r[2], r2);
    rs[0] = r[1];
    rs[1] = r[2];
#pragma unroll
    for (int i = 0; i < 8; ++i) tr->roots[0][i] = a_root[i];
  }
  __syncthreads();
  // The digit-basis tables of r[1], r[2] (the constraint kernel's): one row r 2^(32 i) per thread.
  const uint32_t t = threadIdx.x;
  if (t < 16) db_limbs(fe_mul(rs[t >> 3], p32.m[t & 7]), tr->r_db[t >> 3] + 9 * (t & 7));
}

// (g2^steps)^t, t < 8: the x^steps factor of L at the points i = t mod 8 (prove.rs:287-291).
struct XsPowers {
  fe v[8];
};

constexpr uint32_t kKThreads = 256;  // r1cs_k_kernel: kLincombConsts x 8 table rows
static_assert(kLincombConsts * 8 <= kKThreads, "r1cs_k_kernel rows");
// k_0 = 1, k_i = from_str(mk_seed([m_root, [i]])) = BE integer of
// Blake2s(m_root || i) mod p (prove.rs:274-283, utils.rs:25-27, 51-57); then the
// three per-residue coefficients of L, kx[t] = (k3 + k4 xs_t, k5 + k6 xs_t,
// k7 + k8 xs_t), so the L kernel needs 8 products per point instead of 14.
__device__ __forceinline__ void r1cs_k_body(const uint32_t* __restrict__ m_root, const fe& r2, const fe& one_m,
                                            const XsPowers& xs, const Pow32& p32, Transcript* __restrict__ tr) {
  __shared__ fe ks[11];
  __shared__ fe kx[8][3];
  const uint32_t i = threadIdx.x;
  if (i == 0) {
    ks[0] = one_m;
    tr->k_m[0] = one_m;
#pragma unroll
    for (int j = 0; j < 8; ++j) tr->roots[1][j] = m_root[j];
  } else if (i <= 10) {
    uint32_t h[8];
    b2s_short(m_root, i, 33, h);
    ks[i] = fe_mul(challenge_k(h), r2);
    tr->k_m[i] = ks[i];
  }
  __syncthreads();
  if (i < 8) {
    kx[i][0] = fe_add(ks[3], fe_mul(ks[4], xs.v[i]));
    kx[i][1] = fe_add(ks[5], fe_mul(ks[6], xs.v[i]));
    kx[i][2] = fe_add(ks[7], fe_mul(ks[8], xs.v[i]));
    tr->kx_m[i][0] = kx[i][0];
    tr->kx_m[i][1] = kx[i][1];
    tr->kx_m[i][2] = kx[i][2];
  }
  __syncthreads();
  // The constants' digit-basis tables, one row c 2^(32 r) mod p per thread (kKThreads threads)
  if (i < kLincombConsts * 8) {
    static constexpr int kIdx[5] = {0, 1, 2, 9, 10};
    const uint32_t c = i >> 3, r = i & 7;
    const fe m = c < 5 ? ks[kIdx[c]] : kx[(c - 5) / 3][(c - 5) % 3];
    fe unit = fe_zero();
    unit.w[0] = 1;
    const fe canon = fe_mul(m, unit);  // canonical constant (Montgomery image x R^-1)
    db_limbs(fe_mul(canon, p32.m[r]), tr->k_db[c] + 9 * r);
  }
}
__global__ void r1cs_k_kernel(const uint32_t* __restrict__ m_root, fe r2, fe one_m, XsPowers xs, Pow32 p32,
                              Transcript* __restrict__ tr) {
  r1cs_k_body(m_root, r2, one_m, xs, p32, tr);
}
// r1cs_k_kernel for proof blockIdx.x of a batch: its main tree's root, its transcript.
__global__ void r1cs_k_batch_kernel(ForestRoots mt, fe r2, fe one_m, XsPowers xs, Pow32 p32,
                                    Transcript* __restrict__ tr) {
  r1cs_k_body(mt.root(blockIdx.x), r2, one_m, xs, p32, tr + blockIdx.x);
}

__global__ void r1cs_l_root_kernel(const uint32_t* __restrict__ l_root, Transcript* __restrict__ tr) {
  if (threadIdx.x < 8) tr->roots[2][threadIdx.x] = l_root[threadIdx.x];
}
// The same for proof blockIdx.x of a batch (the L forest's root launch writes special_x only).
__global__ void r1cs_l_root_batch_kernel(ForestRoots lt, Transcript* __restrict__ tr) {
  if (threadIdx.x < 8) tr[blockIdx.x].roots[2][threadIdx.x] = lt.root(blockIdx.x)[threadIdx.x];
}

// A batch's transcripts before its chain: everything ahead of c_db zeroed (the constraint flags among it), and
// the host-built constants (upload_constraint_tables, in tr[0]) copied to every other proof's, so that the
// batched kernels read tr[b] as the single proof's read tr.
__global__ void r1cs_tr_init_batch_kernel(Transcript* __restrict__ tr) {
  constexpr uint32_t kHeadWords = offsetof(Transcript, c_db) / 4, kDbWords = sizeof(Transcript::c_db) / 4;
  uint32_t* mine = reinterpret_cast<uint32_t*>(tr + blockIdx.x);
  for (uint32_t k = threadIdx.x; k < kHeadWords; k += blockDim.x) mine[k] = 0;
  if (blockIdx.x == 0) return;  // (uniform)
  const uint32_t* src = &tr->c_db[0][0];
  uint32_t* dst = &tr[blockIdx.x].c_db[0][0];
  for (uint32_t k = threadIdx.x; k < kDbWords; k += blockDim.x) dst[k] = src[k];
}

// Montgomery image of g^i from the two-level tables of g.
__device__ __forceinline__ fe pow_tab(const fe* __restrict__ lo, const fe* __restrict__ hi, uint32_t kb, uint64_t i) {
  return fe_mul(lo[i & (((uint64_t)1 << kb) - 1)], hi[i >> kb]);
}

// IDX / PIDX step columns (prove.rs:160-167 with the identity tail of
// prove.rs:55-56) and the accumulator leaves u64 LE index || to_bytes_le(w)
// (utils.rs:254-263).
// (IDX itself is not written: its extension is the context's shared ext_index_column.)
// (dig non-null: each 40-B leaf's Blake2s too, the accumulator tree's level 0 (merkle_level0), 8 words.)
__device__ __forceinline__ void r1cs_index_row(const uint64_t* __restrict__ perm, uint64_t os, uint64_t steps,
                                               const fe* __restrict__ w, fe* __restrict__ pidx,
                                               uint64_t* __restrict__ acc_leaves, uint32_t* __restrict__ dig) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= steps) return;
  const uint64_t p = i < os ? perm[i] : i;
  fe_store(pidx + i, fe_from_u64(p));
  const fe x = fe_load(w + i);
  uint64_t* leaf = acc_leaves + 5 * i;
  leaf[0] = p;
#pragma unroll
  for (int k = 0; k < 4; ++k) leaf[1 + k] = (uint64_t)x.w[2 * k] | ((uint64_t)x.w[2 * k + 1] << 32);
  if (dig) {  // (uniform) one zero-padded block of the 40 leaf bytes
    uint32_t h[8], m[16];
    b2s_init(h);
    m[0] = (uint32_t)p;
    m[1] = (uint32_t)(p >> 32);
#pragma unroll
    for (int k = 0; k < 8; ++k) m[2 + k] = x.w[k];
#pragma unroll
    for (int k = 10; k < 16; ++k) m[k] = 0;
    b2s_compress(h, m, 40, 0, true);
    uint4* d = reinterpret_cast<uint4*>(dig + 8 * i);
    d[0] = make_uint4(h[0], h[1], h[2], h[3]);
    d[1] = make_uint4(h[4], h[5], h[6], h[7]);
  }
}
__global__ void r1cs_index_kernel(const uint64_t* __restrict__ perm, uint64_t os, uint64_t steps,
                                  const fe* __restrict__ w, fe* __restrict__ pidx, uint64_t* __restrict__ acc_leaves,
                                  uint32_t* __restrict__ dig) {
  r1cs_index_row(perm, os, steps, w, pidx, acc_leaves, dig);
}
// r1cs_index_kernel for proof blockIdx.y of a batch: the circuit's permutation (one copy), the proof's witness
// column at w + y steps, its PIDX column and leaves likewise, and its tree's level 0 at dig + y dig_stride words.
__global__ void r1cs_index_batch_kernel(const uint64_t* __restrict__ perm, uint64_t os, uint64_t steps,
                                        const fe* __restrict__ w, fe* __restrict__ pidx,
                                        uint64_t* __restrict__ acc_leaves, uint32_t* __restrict__ dig,
                                        uint64_t dig_stride) {
  const uint64_t b = blockIdx.y;
  r1cs_index_row(perm, os, steps, w + b * steps, pidx + b * steps, acc_leaves + b * 5 * steps, dig + b * dig_stride);
}

// Flag columns F0, F1, F2 (run.rs:283-308) from bytes: dst[f * steps + i] = fb[f * os + i].
__global__ void r1cs_flags_kernel(const uint8_t* __restrict__ fb, uint64_t os, uint64_t steps, fe* __restrict__ dst) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= 3 * os) return;
  const uint64_t f = g / os, i = g - f * os;
  fe_store(dst + f * steps + i, fe_from_u64(fb[g]));
}

// The proof's input columns from device-resident trace columns in one launch (the device trace builder's
// output, stark_prove_r1cs_bytes), in place of a dozen copies and fills: raw[c] (c < 6: K F0 F1 F2 S P) =
// the column zero-padded to `steps` (F0-F2 widened from their 0/1 bytes), wcopy = S, perm copied, and
// the transcript zeroed.
struct PackArgs {
  const fe* col[6];     // K, (F0, F1, F2 when given as elements), S, P
  const uint8_t* fb;    // F0-F2 as 3 x os bytes (or null)
  const uint64_t* perm_in;
  uint64_t os, steps;
  fe* raw;
  fe* wcopy;
  uint64_t* perm;
  uint32_t* tr;         // the transcript, tr_words u32
  uint32_t tr_words;
  uint32_t k_slot;      // K's raw slot: 0, or 1 when F0's extension is the shared one (F0 not written)
};
__global__ void r1cs_pack_kernel(PackArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < a.tr_words) a.tr[i] = 0;
  if (i >= a.steps) return;
  const bool in = i < a.os;
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    if (c == 1 && a.k_slot) continue;  // (uniform)
    fe v = fe_zero();
    if (in) {
      if (a.fb && c >= 1 && c <= 3) v = fe_from_u64(a.fb[(uint64_t)(c - 1) * a.os + i]);
      else v = fe_load(a.col[c] + i);
    }
    fe_store(a.raw + (uint64_t)(c == 0 ? a.k_slot : c) * a.steps + i, v);
    if (c == 4) fe_store(a.wcopy + i, v);
  }
  if (in) a.perm[i] = a.perm_in[i];
}

// val_nmr / val_dnm of calc_a_mini_evaluations (utils.rs:317-318), written as
// Montgomery images for the product scans.
// ext_idx[8 j] = IDX[j] = j and ext_pidx[8 j] = PIDX[j] (the LDE interpolates the step
// values); with ext_idx == nullptr (distributed prover: the extended columns are
// sharded) they are taken from the step-domain permutation instead.
__device__ __forceinline__ void r1cs_a_vals_row(const fe* __restrict__ ext_idx, const fe* __restrict__ ext_pidx,
                                                const uint64_t* __restrict__ perm, uint64_t os,
                                                const fe* __restrict__ w, uint64_t steps,
                                                const Transcript* __restrict__ tr, const fe& mr2,
                                                fe* __restrict__ nmr_m, fe* __restrict__ dnm_m) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= steps) return;
  const fe r0 = tr->r0, r1_m = tr->r1_m, r2_m = tr->r2_m;
  const fe rw = fe_mul(fe_load(w + j), r2_m);
  const fe xi = ext_idx ? fe_load(ext_idx + j * kExtensionFactor) : fe_from_u64(j);
  const fe xp = ext_idx ? fe_load(ext_pidx + j * kExtensionFactor) : fe_from_u64(j < os ? perm[j] : j);
  const fe vn = fe_add(fe_add(r0, fe_mul(xi, r1_m)), rw);
  const fe vd = fe_add(fe_add(r0, fe_mul(xp, r1_m)), rw);
  fe_store(nmr_m + j, fe_mul(vn, mr2));
  fe_store(dnm_m + j, fe_mul(vd, mr2));
}
__global__ void r1cs_a_vals_kernel(const fe* __restrict__ ext_idx, const fe* __restrict__ ext_pidx,
                                   const uint64_t* __restrict__ perm, uint64_t os,
                                   const fe* __restrict__ w, uint64_t steps, const Transcript* __restrict__ tr, fe mr2,
                                   fe* __restrict__ nmr_m, fe* __restrict__ dnm_m) {
  r1cs_a_vals_row(ext_idx, ext_pidx, perm, os, w, steps, tr, mr2, nmr_m, dnm_m);
}
// r1cs_a_vals_kernel for proof blockIdx.y of a batch (IDX and PIDX from the step-domain permutation, which is the
// circuit's): its witness column, transcript and the two product arrays, each `steps` from a proof to the next.
__global__ void r1cs_a_vals_batch_kernel(const uint64_t* __restrict__ perm, uint64_t os, const fe* __restrict__ w,
                                         uint64_t steps, const Transcript* __restrict__ tr, fe mr2,
                                         fe* __restrict__ nmr_m, fe* __restrict__ dnm_m) {
  const uint64_t b = blockIdx.y;
  r1cs_a_vals_row(nullptr, nullptr, perm, os, w + b * steps, steps, tr + b, mr2, nmr_m + b * steps, dnm_m + b * steps);
}

// Inclusive product scan, phase 1: each workgroup scans kScanBlock Montgomery
// values in place (4 per thread, then a 256-entry scan of the thread
// products in LDS) and writes the block product to tot[blockIdx].
// The scans run over one or two arrays at once (blockIdx.y picks the array: the A column's numerators and
// denominators, one launch per phase for both).
struct ScanArrays {
  fe* v[2];
  fe* tot[2];
  fe* canon[2];
};

// (BATCH: the three scan phases take proof blockIdx.z of a batch, whose arrays are n elements and nb block
// products behind the previous proof's, so no scan runs across two proofs.)
template <bool BATCH>
__global__ __launch_bounds__(256) void scan_block_kernel(ScanArrays a, uint64_t n, fe one_m, uint32_t nb) {
  __shared__ fe part[256];
  fe* __restrict__ v = a.v[blockIdx.y];
  fe* __restrict__ tot = a.tot[blockIdx.y];
  if constexpr (BATCH) {
    v += (uint64_t)blockIdx.z * n;
    tot += (uint64_t)blockIdx.z * nb;
  }
  const uint64_t base = (uint64_t)blockIdx.x * kScanBlock + 4 * threadIdx.x;
  fe x[4];
  fe acc = one_m;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    x[k] = base + k < n ? fe_load(v + base + k) : one_m;
    acc = fe_mul(acc, x[k]);
    x[k] = acc;
  }
  part[threadIdx.x] = acc;
  __syncthreads();
  // Hillis-Steele over the 256 thread products.
  for (uint32_t off = 1; off < 256; off <<= 1) {
    fe t = part[threadIdx.x];
    if (threadIdx.x >= off) t = fe_mul(part[threadIdx.x - off], t);
    __syncthreads();
    part[threadIdx.x] = t;
    __syncthreads();
  }
  const fe pre = threadIdx.x ? part[threadIdx.x - 1] : one_m;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (base + k < n) fe_store(v + base + k, threadIdx.x ? fe_mul(pre, x[k]) : x[k]);
  if (threadIdx.x == 255) tot[blockIdx.x] = part[255];
}

// Phase 2: exclusive scan of the block products (one workgroup; each thread
// owns a contiguous run).
__device__ __forceinline__ void scan_tot_body(fe* __restrict__ tot, uint32_t nb, const fe& one_m) {
  __shared__ fe part[256];
  const uint32_t per = (nb + 255) / 256;
  const uint32_t lo = threadIdx.x * per, hi = lo + per < nb ? lo + per : nb;
  fe acc = one_m;
  for (uint32_t i = lo; i < hi; ++i) acc = fe_mul(acc, tot[i]);
  part[threadIdx.x] = acc;
  __syncthreads();
  // Inclusive Hillis-Steele scan of the 256 run products (8 dependent
  // products instead of a 256-long serial chain), then shift to exclusive.
  for (uint32_t off = 1; off < 256; off <<= 1) {
    fe t = part[threadIdx.x];
    if (threadIdx.x >= off) t = fe_mul(part[threadIdx.x - off], t);
    __syncthreads();
    part[threadIdx.x] = t;
    __syncthreads();
  }
  const fe excl = threadIdx.x ? part[threadIdx.x - 1] : one_m;
  __syncthreads();
  part[threadIdx.x] = excl;
  __syncthreads();
  acc = part[threadIdx.x];
  for (uint32_t i = lo; i < hi; ++i) {
    const fe t = tot[i];
    tot[i] = acc;
    acc = fe_mul(acc, t);
  }
}
__global__ __launch_bounds__(256) void scan_tot_kernel(ScanArrays a, uint32_t nb, fe one_m) {
  scan_tot_body(a.tot[blockIdx.y], nb, one_m);
}
// Phase 2 for proof blockIdx.z of a batch (its nb block products behind the previous proof's).
__global__ __launch_bounds__(256) void scan_tot_batch_kernel(ScanArrays a, uint32_t nb, fe one_m) {
  scan_tot_body(a.tot[blockIdx.y] + (uint64_t)blockIdx.z * nb, nb, one_m);
}

// Phase 3: block b (> 0) times the product of blocks before it; also emits
// the canonical value into `canon` when given.
__device__ __forceinline__ void scan_apply_body(fe* __restrict__ v, const fe* __restrict__ tot,
                                                fe* __restrict__ canon, uint64_t n, const fe& unit) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fe x = fe_load(v + i);
  const uint64_t b = i / kScanBlock;
  if (b) x = fe_mul(x, tot[b]);
  fe_store(v + i, x);
  if (canon) fe_store(canon + i, fe_mul(x, unit));
}
__global__ void scan_apply_kernel(ScanArrays a, uint64_t n, fe unit) {
  scan_apply_body(a.v[blockIdx.y], a.tot[blockIdx.y], a.canon[blockIdx.y], n, unit);
}
// Phase 3 for proof blockIdx.z of a batch.
__global__ void scan_apply_batch_kernel(ScanArrays a, uint64_t n, uint32_t nb, fe unit) {
  const uint64_t z = blockIdx.z;
  fe* const canon = a.canon[blockIdx.y];
  scan_apply_body(a.v[blockIdx.y] + z * n, a.tot[blockIdx.y] + z * nb, canon ? canon + z * n : nullptr, n, unit);
}

// a_mini[j] = acc_nmr[j] * inv(acc_dnm[j]) (utils.rs:331-336); nmr Montgomery, inv canonical.
__global__ void r1cs_a_mini_kernel(const fe* __restrict__ nmr_m, const fe* __restrict__ inv_dnm, uint64_t steps,
                                   fe* __restrict__ out) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= steps) return;
  fe_store(out + j, fe_mul(fe_load(nmr_m + j), fe_load(inv_dnm + j)));
}

// Zb2(x) = prod_k (x - x_k) (utils.rs:438-455) and Zb3(x) = x - x_last
// (utils.rs:466-474) for the batch inverse, each as Zb R^-1 (unit = R^-1, Mont::rinv): their
// inverses are then the Montgomery images of 1 / Zb, which the constraint kernel multiplies exactly.
// Local point i is the global evaluation point g_add + (i << log_g) (a residue
// class of the precision domain on a distributed prover; g_add = log_g = 0 on one GPU).
__global__ void r1cs_zb_kernel(const fe* __restrict__ lo, const fe* __restrict__ hi, uint32_t kb, uint64_t prec,
                               uint64_t g_add, uint32_t log_g,
                               const fe* __restrict__ xpub_m, uint32_t npub, fe xlast_m, fe unit, fe one_m,
                               fe* __restrict__ zb2, fe* __restrict__ zb3) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= prec) return;
  const fe x_m = pow_tab(lo, hi, kb, g_add + (i << log_g));
  if (zb2) {  // (null: Zb2 is the extension of its coefficients, the column route)
    fe acc = one_m;
    for (uint32_t k = 0; k < npub; ++k) acc = fe_mul(acc, fe_sub(x_m, xpub_m[k]));
    fe_store(zb2 + i, fe_mul(acc, unit));
  }
  if (zb3) fe_store(zb3 + i, fe_mul(fe_sub(x_m, xlast_m), unit));  // (null: 1 / Zb3 is the shared column)
}

struct ConstraintArgs {
  const fe* col[9];      // K F0 F1 F2 S P IDX PIDX A, precision (local points) each
  const fe* inv_zb;      // inv Zb2 (precision)
  const fe* inv_zb3;     // inv Zb3 (precision): inv_zb + precision, or the shared column
  // tinv != null: inv Zb2 by partial fractions instead of inv_zb, sum_k pf_coef[k] tinv[i - pf_shift[k]]
  // over the shared table tinv[m] = 1 / (x_m - 1) (kInvXm1; zb2_partial_fractions)
  const fe* tinv;
  uint32_t n_pf;
  uint64_t pf_shift[8];
  fe pf_coef[8];
  const fe* interp2;     // canonical coefficients, low degree first
  const fe* interp3;
  const fe* i2_col = nullptr;  // non-null: I2 at this host's points (the column route), read instead of Horner
  const fe* lo;          // g2 tables
  const fe* hi;
  fe* rows;              // precision x 8 elements: rows (plane = 0) or 8 columns of `plane` elements
  uint64_t plane;
  int* err;
  uint64_t prec;            // points on this GPU (a power of two)
  uint64_t shift1, shift2;  // original_steps/3*skips, original_steps/3*2*skips (mod precision), in local points
  uint64_t back;            // the -skips shift in local points
  uint64_t g_add;           // local point i is global point g_add + (i << log_g)
  uint32_t log_g;
  uint32_t log_prec, kb, n2, n3;
  const Transcript* tr;  // r0, r1, r2 (device transcript)
  // inv(Z) at the points t = i mod 8 (multi_inv of Z, prove.rs:203; 0 for t = 0) as the
  // Montgomery images of inv(Z) R^k, k = 0, 1, 2: the constraint kernel forms some Q's scaled by
  // R^-k (one product fewer per conversion it skips) and undoes the scale in D = Q inv(Z).
  fe invz_m[3][8];
  int mont_cols;         // K, F0-F2 are Montgomery images (prepared circuits); inv Zb2/Zb3 always are
  uint32_t* leaf = nullptr;  // non-null: each row's Blake2s (the main tree's level 0, merkle_level0), 8 words
};

// A batch's own arguments of the constraint kernel (BATCH): what a proof of the batch has of its own, each at a
// fixed stride from the previous proof's.  Everything else is read from ConstraintArgs as the single proof
// reads it: the circuit's columns, the inverses of Zb2 / Zb3, the tables of g2 and every scalar.
struct ConstraintBatch {
  const fe *sp, *a_col;  // S at sp + 2 b prec, P at sp + (2 b + 1) prec; A at a_col + b prec
  const fe* consts;      // boundary_consts of proof b at consts + b consts_stride (interp2 at + n2, interp3 at + 2 n2)
  uint64_t consts_stride;
  const fe* i2_col;      // null, or I2's column of proof b at i2_col + b prec
  fe* rows;              // proof b's 8 planes at rows + 8 b prec
  Transcript* tr;        // tr[b], whose err takes the proof's flags
  uint32_t* leaf;        // level 0 of tree b at leaf + b leaf_stride words
  uint64_t leaf_stride;
};
// Proof blockIdx.y's own (BATCH), or the single proof's arguments, read where the kernel reads them (the
// condition is a template constant: the single proof's instantiation is the kernel as it was, `g` unread).
#define CK_OWN(single, batched) (BATCH ? (batched) : (single))
#define CK_TR CK_OWN(a.tr, (const Transcript*)(g.tr + pb))
#define CK_ERR CK_OWN(a.err, &g.tr[pb].err)
#define CK_INTERP2 CK_OWN(a.interp2, g.consts + pb * g.consts_stride + a.n2)
#define CK_INTERP3 CK_OWN(a.interp3, g.consts + pb * g.consts_stride + 2 * (uint64_t)a.n2)
#define CK_I2COL CK_OWN(a.i2_col, g.i2_col ? g.i2_col + pb * a.prec : (const fe*)nullptr)
#define CK_ROWS CK_OWN(a.rows, g.rows + 8 * pb * a.prec)
#define CK_LEAF CK_OWN(a.leaf, g.leaf + pb * g.leaf_stride)

// Q1/Q2/Q3 (utils.rs:181-248, 344-376) -> D1..D3 (utils.rs:379-418), I2/I3
// evaluations (prove.rs:216-220), B2/B3 (utils.rs:477-524); one main-tree row
// (prove.rs:235-258) per thread.
// (3 workgroups per CU: the digit-basis products need ~170 VGPRs; at 4 waves per SIMD they spill, at the
// compiler's free choice of 180-217 VGPRs two waves per SIMD leave the loads uncovered:
// 1.94 ms before the digit basis, 1.73 ms with it at this bound, 1.96-1.98 ms at the others,
// profiles/r05_constraint_db_ab.txt)
template <bool BATCH>
__global__ __launch_bounds__(256, 3) void r1cs_constraint_kernel(ConstraintArgs a, ConstraintBatch g) {
  const uint64_t pb = BATCH ? blockIdx.y : 0;  // the proof
  // The 24 inv(Z) R^k tables in LDS (a lane's t = i mod 8 picks its table): 76 words apart, so the 8
  // tables a wave reads at once start on distinct 4-bank groups.
  __shared__ __attribute__((aligned(16))) uint32_t izt[24 * 76];
  {
    const uint4* src = reinterpret_cast<const uint4*>(&CK_TR->c_db[9][0]);
    for (uint32_t k = threadIdx.x; k < 24 * 18; k += blockDim.x)
      reinterpret_cast<uint4*>(izt)[(k / 18) * 19 + k % 18] = src[k];
    __syncthreads();
  }
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.prec) return;
  const uint64_t n = a.prec, mask = n - 1;
  const fe* K = a.col[0];
  const fe* F0 = a.col[1];
  const fe* F1 = a.col[2];
  const fe* F2 = a.col[3];
  const fe* S = CK_OWN(a.col[4], g.sp + 2 * pb * a.prec);
  const fe* Pc = CK_OWN(a.col[5], g.sp + (2 * pb + 1) * a.prec);
  const fe* IDX = a.col[6];
  const fe* PIDX = a.col[7];
  const fe* A = CK_OWN(a.col[8], g.a_col + pb * a.prec);
  const uint64_t prev = (i + n - a.back) & mask;
  const uint64_t gi = a.g_add + (i << a.log_g);  // global evaluation point
  const fe r0 = CK_TR->r0;
  const fe p = fe_load(Pc + i), s = fe_load(S + i), av = fe_load(A + i);
  const fe p_prev = fe_load(Pc + prev), a_prev = fe_load(A + prev);
  const fe p2 = fe_load(Pc + ((i + a.shift1) & mask)), p3 = fe_load(Pc + ((i + a.shift2) & mask));
  // Data x data products: a Montgomery product of two canonical values is x y R^-1, so each Q is
  // formed at a scale R^-k and D = Q inv(Z) takes the inv(Z) R^k constant (zero tests are
  // scale-free).  Prepared circuits hold K, F0-F2 as Montgomery images: their products are exact.
  const bool mc = a.mont_cols != 0;
  // Products by the proof's constants (r1, r2, R^-1, the a_k below) by the digit basis from the
  // transcript's tables (wave-uniform: scalar loads), each reduced once to canonical: the same values
  // as the Montgomery products by their images, at about half the instructions.
  const uint32_t* __restrict__ db_r1 = CK_TR->r_db[0];
  const uint32_t* __restrict__ db_r2 = CK_TR->r_db[1];
  const uint32_t* __restrict__ db_rinv = CK_TR->c_db[0];
  auto cmul = [](const fe& x, const uint32_t* __restrict__ w) {  // x w mod p, canonical (x < 4p)
    fe y = fe_mul_db(x, w);
    fe_reduce_once(y);
    return y;
  };
  const fe k_s = fe_mul(fe_load(K + i), s), f1_p = fe_mul(fe_load(F1 + i), p_prev);
  const fe q1 = fe_mul(fe_load(F0 + i), fe_sub(fe_sub(mc ? p : cmul(p, db_rinv), f1_p), k_s));  // R^-(mc ? 0 : 2)
  const fe q2 = fe_mul(fe_load(F2 + i), fe_sub(cmul(p3, db_rinv), fe_mul(p, p2)));            // R^-(mc ? 1 : 2)
  const fe rs = cmul(s, db_r2);
  const fe nmr = fe_add(fe_add(r0, cmul(fe_load(IDX + i), db_r1)), rs);
  const fe dnm = fe_add(fe_add(r0, cmul(fe_load(PIDX + i), db_r1)), rs);
  const fe q3 = fe_sub(fe_mul(av, dnm), fe_mul(a_prev, nmr));                                // R^-1
  const uint32_t t = (uint32_t)(gi & 7);
  if (t == 0 && !(fe_is_zero(q1) && fe_is_zero(q2) && fe_is_zero(q3))) atomicOr(CK_ERR, 1);
  auto iz = [&](uint32_t k) {  // the table of inv(Z) R^k at this t
    return static_cast<const uint32_t*>(__builtin_assume_aligned(izt + 76 * (8 * k + t), 16));
  };
  const fe d1 = cmul(q1, iz(mc ? 0 : 2)), d2 = cmul(q2, iz(mc ? 1 : 2)), d3 = cmul(q3, iz(1));
  // I2 / I3 at x = g2^i (Horner; the interpolants are canonical).
  const fe x_m = pow_tab(a.lo, a.hi, a.kb, gi);
  // (Horner from the leading coefficient: the first step's 0 * x + c is c itself)
  fe i2;
  if (CK_I2COL) {  // (uniform)
    i2 = fe_load(CK_I2COL + i);
  } else {
    i2 = a.n2 ? CK_INTERP2[a.n2 - 1] : fe_zero();
    for (uint32_t k = a.n2 ? a.n2 - 1 : 0; k-- > 0;) i2 = fe_add(fe_mul(i2, x_m), CK_INTERP2[k]);
  }
  fe i3 = a.n3 ? CK_INTERP3[a.n3 - 1] : fe_zero();
  for (uint32_t k = a.n3 ? a.n3 - 1 : 0; k-- > 0;) i3 = fe_add(fe_mul(i3, x_m), CK_INTERP3[k]);
  fe izb2;
  if (a.tinv) {  // (uniform)
    izb2 = fe_zero();
    bool root = false;  // x = x_k: Zb2 = 0, whose batch inverse is 0
    for (uint32_t k = 0; k < a.n_pf; ++k) {
      const uint64_t m = (i + n - a.pf_shift[k]) & mask;
      root = root || (m == 0 && a.g_add == 0);
      // a_k tinv (a Montgomery image times a canonical a_k: the image of the product), sum in [0, 2p)
      izb2 = fe_add_raw(izb2, fe_mul_db(fe_load(a.tinv + m), CK_TR->c_db[1 + k]));
      fe_csub2p(izb2);
    }
    fe_reduce_once(izb2);
    if (root) izb2 = fe_zero();
  } else {
    izb2 = fe_load(a.inv_zb + i);
  }
  const fe izb3 = fe_load(a.inv_zb3 + i);
  const fe e2 = fe_sub(s, i2), e3 = fe_sub(av, i3);
  if (fe_is_zero(izb2) && !fe_is_zero(e2)) atomicOr(CK_ERR, 2);
  if (fe_is_zero(izb3) && !fe_is_zero(e3)) atomicOr(CK_ERR, 4);
  const fe b2 = fe_mul(e2, izb2), b3 = fe_mul(e3, izb3);  // (Montgomery images of the inverses: exact)
  // Row i = P|A|S|D1|D2|D3|B2|B3: contiguous (256 B), or column c at rows + c * plane + i
  const uint64_t cs = a.plane ? a.plane : 1;
  fe* row = a.plane ? CK_ROWS + i : CK_ROWS + 8 * i;
  fe_store(row + 0 * cs, p);
  fe_store(row + 1 * cs, av);
  fe_store(row + 2 * cs, s);
  fe_store(row + 3 * cs, d1);
  fe_store(row + 4 * cs, d2);
  fe_store(row + 5 * cs, d3);
  fe_store(row + 6 * cs, b2);
  fe_store(row + 7 * cs, b3);
  if (CK_LEAF) {  // (uniform) the main tree's leaf: Blake2s of the 256-B row, 4 blocks of two values each
    uint32_t h[8], m[16];
    b2s_init(h);
    auto block = [&](const fe& x, const fe& y, uint32_t t_bytes, bool last) {
#pragma unroll
      for (int w = 0; w < 8; ++w) {
        m[w] = x.w[w];
        m[8 + w] = y.w[w];
      }
      b2s_compress(h, m, t_bytes, 0, last);
    };
    block(p, av, 64, false);
    block(s, d1, 128, false);
    block(d2, d3, 192, false);
    block(b2, b3, 256, true);
    uint4* q = reinterpret_cast<uint4*>(CK_LEAF + 8 * i);
    q[0] = make_uint4(h[0], h[1], h[2], h[3]);
    q[1] = make_uint4(h[4], h[5], h[6], h[7]);
  }
}
#undef CK_OWN
#undef CK_TR
#undef CK_ERR
#undef CK_INTERP2
#undef CK_INTERP3
#undef CK_I2COL
#undef CK_ROWS
#undef CK_LEAF

struct LincombArgs {
  const fe* rows;        // the constraint kernel's rows (plane = 0) or columns (plane elements apart)
  uint64_t plane;
  fe* out;
  uint64_t prec;
  uint64_t g_add;        // local point i is global point g_add + (i << log_g)
  uint32_t log_g;
  const Transcript* tr;  // k and kx (device transcript)
  uint32_t* leaf = nullptr;  // non-null: each value's Blake2s (the L tree's level 0, merkle_level0), 8 words
};

// L = k0 D1 + k1 D2 + k2 D3 + k3 P + k4 P x^steps + k5 B2 + k6 B2 x^steps +
//     k7 B3 + k8 B3 x^steps + k9 A + k10 S (prove.rs:293-322).
__device__ __forceinline__ void r1cs_lincomb_row(const LincombArgs& a, const fe* __restrict__ rows,
                                                 fe* __restrict__ out, const Transcript* __restrict__ tr,
                                                 uint32_t* __restrict__ leaf) {
  // Every product is data x a constant of the proof: the digit-basis product (fe_db.h) from the
  // transcript's tables, staged in LDS; the sum stays in [0, 2p) and is reduced once at the end.
  __shared__ __attribute__((aligned(16))) uint32_t tab[kLincombConsts * 72];
  for (uint32_t k = threadIdx.x; k < kLincombConsts * 18; k += blockDim.x)
    reinterpret_cast<uint4*>(tab)[k] = reinterpret_cast<const uint4*>(&tr->k_db[0][0])[k];
  __syncthreads();
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.prec) return;
  const uint64_t cs = a.plane ? a.plane : 1;
  const fe* row = a.plane ? rows + i : rows + 8 * i;
  const uint64_t gi = a.g_add + (i << a.log_g);
  const fe p = fe_load(row + 0 * cs), av = fe_load(row + 1 * cs), s = fe_load(row + 2 * cs),
           d1 = fe_load(row + 3 * cs), d2 = fe_load(row + 4 * cs), d3 = fe_load(row + 5 * cs),
           b2 = fe_load(row + 6 * cs), b3 = fe_load(row + 7 * cs);
  const uint32_t t = (uint32_t)(gi & 7);
  auto T = [&](uint32_t c) { return static_cast<const uint32_t*>(__builtin_assume_aligned(tab + 72 * c, 16)); };
  auto add = [](fe& acc, const fe& x) {  // acc, x in [0, 2p): acc + x < 4p < 2^256, back to [0, 2p)
    acc = fe_add_raw(acc, x);
    fe_csub2p(acc);
  };
  fe acc = fe_mul_db(d1, T(0));           // k0 D1
  add(acc, fe_mul_db(d2, T(1)));          // k1 D2
  add(acc, fe_mul_db(d3, T(2)));          // k2 D3
  add(acc, fe_mul_db(p, T(5 + 3 * t)));   // (k3 + k4 x^steps) P
  add(acc, fe_mul_db(b2, T(6 + 3 * t)));  // (k5 + k6 x^steps) B2
  add(acc, fe_mul_db(b3, T(7 + 3 * t)));  // (k7 + k8 x^steps) B3
  add(acc, fe_mul_db(av, T(3)));          // k9 A
  add(acc, fe_mul_db(s, T(4)));           // k10 S
  fe_reduce_once(acc);
  fe_store(out + i, acc);
  if (leaf) {  // (uniform) the L tree's leaf: Blake2s of the 32-B value
    uint32_t h[8], m[16];
    b2s_init(h);
#pragma unroll
    for (int w = 0; w < 8; ++w) {
      m[w] = acc.w[w];
      m[8 + w] = 0;
    }
    b2s_compress(h, m, 32, 0, true);
    uint4* q = reinterpret_cast<uint4*>(leaf + 8 * i);
    q[0] = make_uint4(h[0], h[1], h[2], h[3]);
    q[1] = make_uint4(h[4], h[5], h[6], h[7]);
  }
}
__global__ __launch_bounds__(256) void r1cs_lincomb_kernel(LincombArgs a) {
  r1cs_lincomb_row(a, a.rows, a.out, a.tr, a.leaf);
}
// L of proof blockIdx.y of a batch: its rows (8 planes) at a.rows + 8 y prec, its values at a.out + y prec, its
// transcript a.tr[y] and its tree's level 0 at a.leaf + y leaf_stride words.
__global__ __launch_bounds__(256) void r1cs_lincomb_batch_kernel(LincombArgs a, uint64_t leaf_stride) {
  const uint64_t b = blockIdx.y;
  r1cs_lincomb_row(a, a.rows + 8 * b * a.prec, a.out + b * a.prec, a.tr + b, a.leaf + b * leaf_stride);
}

// ---- host helpers -----------------------------------------------------------

// Z(g2^i) = (g2^steps)^(i mod 8) - 1; its inverse with 0 -> 0 (prove.rs:128-129, 203), times
// R^k for the kernel's R^-k-scaled Q's.
static void set_inv_z(ConstraintArgs& ca, const HostFp& g2, uint64_t steps) {
  const FieldHost& F = FieldHost::get();
  const HostFp rv = F.from_canonical(F.one().v);  // the field element R = 2^256 mod p
  const HostFp w8 = F.pow_u64(g2, steps);
  HostFp wt = F.one();
  for (int t = 0; t < 8; ++t) {
    const HostFp z = F.sub(wt, F.one());
    HostFp iz = FieldHost::eq(z, F.zero()) ? F.zero() : F.inv(z);
    for (int k = 0; k < 3; ++k) {
      ca.invz_m[k][t] = to_dev(iz);
      iz = F.mul(iz, rv);
    }
    wt = F.mul(wt, w8);
  }
}

// log2_ceil, utils.rs:14-23.
static uint32_t log2_ceil_ref(size_t v) {
  uint32_t l = 1;
  while (v > 1) {
    v /= 2;
    ++l;
  }
  return l;
}

static HostFp host_fe(const uint64_t* c) { return FieldHost::get().from_canonical(c); }

// c = a * b (coefficient lists, low degree first); the output coefficients are split over the
// host workers when the product is large.
static std::vector<HostFp> poly_mul(const std::vector<HostFp>& a, const std::vector<HostFp>& b) {
  const FieldHost& F = FieldHost::get();
  std::vector<HostFp> c(a.size() + b.size() - 1, F.zero());
  const size_t nc = c.size();
  const unsigned T = a.size() * b.size() > 20000 ? host_threads() : 1;
  host_parallel(T, [&](unsigned t) {
    for (size_t k = t; k < nc; k += T) {
      const size_t lo = k >= b.size() ? k - (b.size() - 1) : 0, hi = k < a.size() ? k : a.size() - 1;
      HostFp acc = F.zero();
      for (size_t i = lo; i <= hi; ++i) acc = F.add(acc, F.mul(a[i], b[k - i]));
      c[k] = acc;
    }
  });
  return c;
}

// lagrange_interp (fri/src/poly_utils.rs:409-439): the unique interpolant, n coefficients, Montgomery on
// the host.  The same polynomial as the reference's, by another O(n^2) route that parallelises:
//   root = prod (X - x_i) by a product tree (leaves on the host workers),
//   den_i = root'(x_i) = prod_{j != i} (x_i - x_j), one batch inverse (0 -> 0, as F.inv),
//   b = sum_i (y_i / den_i) root / (X - x_i), each worker summing its share of the i.
// (A public-input list of 1,062 wires, bits.r1cs, took 70 ms serially.)
std::vector<HostFp> lagrange_interp(const std::vector<HostFp>& xs, const std::vector<HostFp>& ys) {
  const FieldHost& F = FieldHost::get();
  const size_t n = xs.size();
  if (n == 0) return {};
  const unsigned T = n >= 64 ? host_threads() : 1;
  // Product tree: T leaf products, then pairwise merges.
  std::vector<std::vector<HostFp>> parts(T);
  host_parallel(T, [&](unsigned t) {
    const size_t i0 = n * t / T, i1 = n * (t + 1) / T;
    std::vector<HostFp> r(1, F.one());
    for (size_t i = i0; i < i1; ++i) {
      std::vector<HostFp> nxt(r.size() + 1, F.zero());
      for (size_t j = 0; j < r.size(); ++j) {
        nxt[j + 1] = F.add(nxt[j + 1], r[j]);
        nxt[j] = F.sub(nxt[j], F.mul(r[j], xs[i]));
      }
      r.swap(nxt);
    }
    parts[t] = std::move(r);
  });
  while (parts.size() > 1) {
    std::vector<std::vector<HostFp>> next;
    for (size_t i = 0; i + 1 < parts.size(); i += 2) next.push_back(poly_mul(parts[i], parts[i + 1]));
    if (parts.size() & 1) next.push_back(std::move(parts.back()));
    parts.swap(next);
  }
  const std::vector<HostFp>& root = parts[0];  // n + 1 coefficients, root[n] = 1
  std::vector<HostFp> droot(n);
  for (size_t d = 1; d <= n; ++d) droot[d - 1] = F.mul(root[d], F.from_u64(d));
  std::vector<HostFp> den(n);
  host_parallel(T, [&](unsigned t) {
    for (size_t i = t; i < n; i += T) {
      HostFp y = F.zero();
      for (size_t d = n; d-- > 0;) y = F.add(F.mul(y, xs[i]), droot[d]);
      den[i] = y;
    }
  });
  // Batch inverse with zeros kept (F.inv(0) = 0).
  std::vector<HostFp> pre(n);
  HostFp acc = F.one();
  for (size_t i = 0; i < n; ++i) {
    pre[i] = acc;
    if (!FieldHost::eq(den[i], F.zero())) acc = F.mul(acc, den[i]);
  }
  HostFp inv_acc = F.inv(acc);
  std::vector<HostFp> s(n);
  for (size_t i = n; i-- > 0;) {
    if (FieldHost::eq(den[i], F.zero())) {
      s[i] = F.zero();
      continue;
    }
    s[i] = F.mul(ys[i], F.mul(inv_acc, pre[i]));
    inv_acc = F.mul(inv_acc, den[i]);
  }
  std::vector<std::vector<HostFp>> partial(T, std::vector<HostFp>(n, F.zero()));
  host_parallel(T, [&](unsigned t) {
    std::vector<HostFp>& b = partial[t];
    std::vector<HostFp> num(n);
    for (size_t i = t; i < n; i += T) {
      HostFp carry = root[n];
      num[n - 1] = carry;
      for (size_t d = n - 1; d >= 1; --d) {  // root / (X - x_i), synthetic division
        carry = F.add(root[d], F.mul(carry, xs[i]));
        num[d - 1] = carry;
      }
      for (size_t j = 0; j < n; ++j) b[j] = F.add(b[j], F.mul(num[j], s[i]));
    }
  });
  std::vector<HostFp> b = std::move(partial[0]);
  for (unsigned t = 1; t < T; ++t)
    for (size_t j = 0; j < n; ++j) b[j] = F.add(b[j], partial[t][j]);
  return b;
}

// Carves the proof's buffers out of the context's grow-only arena (no
// hipMalloc/hipFree per proof).
struct Carve {
  size_t off = 0;
  std::vector<std::pair<void**, size_t>> req;
  template <class T>
  void add(T** p, size_t count) {
    req.push_back({(void**)p, off});
    off += ((count ? count : 1) * sizeof(T) + 255) & ~(size_t)255;
  }
  stark_status commit(stark_ctx* ctx, DevBuf& arena) {
    stark_status st = ensure_buf(ctx, arena, off);
    if (st != STARK_OK) return st;
    for (auto& r : req) *r.first = (uint8_t*)arena.ptr + r.second;
    return STARK_OK;
  }
};


static unsigned blocks_for(uint64_t n, unsigned t = 256) { return (unsigned)((n + t - 1) / t); }

// In-place inclusive product scan of n Montgomery values; canonical copy to `canon` if non-null.
// Inclusive product scans of the arrays a.v[0 .. count) (n elements each, in place, Montgomery images), their
// canonical values into a.canon[k] where given; a.tot[k] holds ceil(n / kScanBlock) block products.
static stark_status product_scan(stark_ctx* ctx, const ScanArrays& a, uint32_t count, uint64_t n, const Mont& mc,
                                 hipStream_t s) {
  const uint32_t nb = (uint32_t)((n + kScanBlock - 1) / kScanBlock);
  hipLaunchKernelGGL(scan_block_kernel<false>, dim3(nb, count), dim3(256), 0, s, a, n, mc.one, 0u);
  hipLaunchKernelGGL(scan_tot_kernel, dim3(1, count), dim3(256), 0, s, a, nb, mc.one);
  hipLaunchKernelGGL(scan_apply_kernel, dim3(blocks_for(n), count), dim3(256), 0, s, a, n, mc.unit);
  STARK_HIP(ctx, hipGetLastError());
  return STARK_OK;
}

// LDE of `batch` step columns (in place in `coef`, destroyed) into `out`
// (batch x precision): inv_best_fft(., g1) then best_fft(., g2) (prove.rs:100-101).
// coef[c][k] *= g2^(r k) for the batch of step columns (coset shift of the LDE).
__global__ void coset_scale_kernel(fe* __restrict__ coef, uint32_t log_steps, uint64_t total, const fe* __restrict__ lo,
                                   const fe* __restrict__ hi, uint32_t kb, uint64_t r, uint64_t prec_mask) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  const uint64_t k = g & (((uint64_t)1 << log_steps) - 1);
  fe_store(coef + g, fe_mul(fe_load(coef + g), pow_tab(lo, hi, kb, (r * k) & prec_mask)));
}

// The values of the step columns' polynomials at the points r + 2^log_g j of the precision
// domain (j < P = precision >> log_g): iNTT(steps, g1), coefficients scaled by g2^(r k), then a
// P-point NTT with root h = g2^(2^log_g) over the zero-padded coefficients (degree < steps <= P).
// log_g = r = 0 is the plain LDE of prove.rs:100-101.  coef is destroyed.  coset_forward is the half from
// the coefficients on (columns that are made as coefficients: Zb2 and I2 on the column route).
static stark_status coset_forward(stark_ctx* ctx, fe* coef, uint32_t batch, fe* out, uint32_t log_steps,
                                  uint32_t log_prec, uint32_t log_g, uint32_t r, const Twiddles& tw_g2,
                                  const Twiddles& tw_h, hipStream_t s) {
  if (r) {
    const uint64_t total = (uint64_t)batch << log_steps;
    hipLaunchKernelGGL(coset_scale_kernel, dim3(blocks_for(total)), dim3(256), 0, s, coef, log_steps, total,
                       tw_g2.d_lo, tw_g2.d_hi, tw_g2.kb, (uint64_t)r, ((uint64_t)1 << log_prec) - 1);
    STARK_HIP(ctx, hipGetLastError());
  }
  // best_fft's zero padding (fft.rs:327-357) is implicit: the first pass reads the steps coefficients only.
  const uint32_t log_p = log_prec - log_g;
  return ntt_device_from(ctx, coef, log_p - log_steps, out, log_p, batch, tw_h, false, s);
}
static stark_status coset_lde(stark_ctx* ctx, fe* coef, uint32_t batch, fe* out, uint32_t log_steps,
                              uint32_t log_prec, uint32_t log_g, uint32_t r, const Twiddles& tw_g1_inv,
                              const Twiddles& tw_g2, const Twiddles& tw_h, hipStream_t s) {
  STARK_TRY(ntt_device(ctx, coef, log_steps, batch, tw_g1_inv, true, s));
  return coset_forward(ctx, coef, batch, out, log_steps, log_prec, log_g, r, tw_g2, tw_h, s);
}

// ---- the public points' columns -----------------------------------------------------------------------
//
// With many public wires (stark_ctx_set_public_column_min) Zb2 = prod_k (X - x_k) and the interpolant I2 are
// what every other polynomial of the proof is: coefficients (from the subproduct tree, poly.hip) extended to
// the host's points by the forward half of the extension.  The points are x_k = g1^(w_k), w_k the wires'
// first uses (utils.rs:421-455), so the interpolation's denominators are one steps-point transform.

// Fewer than `steps` points (Zb2 has n + 1 coefficients), at least the context's threshold.
static bool public_columns(const stark_ctx* ctx, size_t n_pfi, uint64_t steps) {
  const size_t m = ctx->public_column_min ? ctx->public_column_min : kDefaultPublicColumnMin;
  return n_pfi > 0 && n_pfi >= m && n_pfi < steps;
}

// out[k] = in[k] R^-1 (the scale r1cs_zb_kernel stores Zb at: the batch inverse then gives Montgomery images).
__global__ void scale_rinv_kernel(const fe* __restrict__ in, uint64_t n, fe* __restrict__ out) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  fe unit = fe_zero();
  unit.w[0] = 1;
  fe_store(out + k, fe_mul(fe_load(in + k), unit));
}

// The public points on the device: d_exps[i] = w_i, d_xy = the points g1^(w_i) (n), then, with public_wires,
// the wires' values (n).  hint names the points for the interpolation.  h is the uploads' host staging: the
// caller keeps it until its next synchronisation of s.
static stark_status public_points(stark_ctx* ctx, const HostFp& g2, uint64_t skips, uint32_t log_steps,
                                  const uint64_t* public_wires, const size_t* pfi, size_t n, uint64_t* d_exps,
                                  fe* d_xy, DomainHint& hint, std::vector<uint64_t>& h, hipStream_t s) {
  const FieldHost& F = FieldHost::get();
  uint64_t g1c[4];
  F.to_canonical(F.pow_u64(g2, skips), g1c);
  STARK_TRY(get_twiddles(ctx, g1c, log_steps, &hint.tw));
  hint.log_order = log_steps;
  hint.d_exps = d_exps;
  h.assign(n * (public_wires ? 5 : 1), 0);
  for (size_t i = 0; i < n; ++i) {
    h[i] = pfi[2 * i + 1];  // (below steps: stage_dims / circuit_lde)
    if (public_wires) memcpy(&h[n + 4 * i], public_wires + 4 * pfi[2 * i], 32);
  }
  STARK_HIP(ctx, hipMemcpyAsync(d_exps, h.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice, s));
  if (public_wires)
    STARK_HIP(ctx, hipMemcpyAsync(d_xy + n, h.data() + n, n * sizeof(fe), hipMemcpyHostToDevice, s));
  return poly_domain_points(ctx, *hint.tw, d_exps, n, d_xy, s);
}

stark_status circuit_public_plan(stark_ctx* ctx, const PreparedCircuit& c, const HostFp& g2, uint64_t skips,
                                 uint32_t log_steps, hipStream_t s, const InterpPlan** out) {
  if (!c.pub_plan.mem) {
    const FieldHost& F = FieldHost::get();
    const size_t n = c.pfi.size() / 2;
    uint64_t g1c[4];
    F.to_canonical(F.pow_u64(g2, skips), g1c);
    std::vector<uint64_t> exps(n);
    for (size_t i = 0; i < n; ++i) exps[i] = c.pfi[2 * i + 1];
    STARK_TRY(interp_plan_build_domain(ctx, g1c, log_steps, exps.data(), n, c.pub_plan, s));
  }
  *out = &c.pub_plan;
  return STARK_OK;
}

// Zb2's coefficients from the tree alone (a prepared circuit: no witness, no interpolation), scaled by R^-1
// and zero-padded to steps, into coef.  staging: as public_points' h.
static stark_status public_zb2_coefficients(stark_ctx* ctx, const HostFp& g2, uint64_t skips, uint32_t log_steps,
                                            const size_t* pfi, size_t n, fe* coef, std::vector<uint64_t>& staging,
                                            hipStream_t s) {
  const uint64_t steps = (uint64_t)1 << log_steps;
  PolyTree t;
  poly_tree_plan(n, t);
  // the tree, Z's n + 1 coefficients, the points and their exponents
  const size_t tree = poly_tree_elems(t);
  STARK_TRY(buf_acquire(ctx, ctx->poly, s));
  STARK_TRY(ensure_buf(ctx, ctx->poly, (tree + 2 * n + 1) * sizeof(fe) + n * sizeof(uint64_t)));
  fe* mem = (fe*)ctx->poly.ptr;
  fe* z = mem + tree;
  fe* xs = z + n + 1;
  DomainHint hint;
  STARK_TRY(public_points(ctx, g2, skips, log_steps, nullptr, pfi, n, (uint64_t*)(xs + n), xs, hint, staging, s));
  STARK_TRY(poly_tree_build(ctx, xs, t, mem, s));
  STARK_TRY(poly_tree_zpoly(ctx, t, z, s));
  STARK_HIP(ctx, hipMemsetAsync(coef, 0, steps * sizeof(fe), s));
  hipLaunchKernelGGL(scale_rinv_kernel, dim3(blocks_for(n + 1)), dim3(256), 0, s, (const fe*)z, (uint64_t)(n + 1), coef);
  STARK_HIP(ctx, hipGetLastError());
  return buf_release(ctx, ctx->poly, s);
}

// tag 0: IDX[i] = i; tag > 0: F0[i] = 1 for i < tag (calc_flags' flag0, run.rs:283-308), 0 after.
__global__ void const_column_kernel(fe* __restrict__ out, uint64_t n, uint64_t tag) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) fe_store(out + i, fe_from_u64(tag ? (i < tag ? 1 : 0) : i));
}

// Columns of a proof that depend on its size only, over the rank's points r + 2^log_g j (the whole
// domain for log_g = r = 0); each is computed on a context's first proof of that size and shared by
// every later one:
//   kExtIdx: ext_indices (prove.rs:160-163), the extension of IDX[i] = i (coset_lde with log_g, r);
//   kExtF0:  the extension of F0, which calc_flags (run.rs:283-308) sets to 1 on each of the os trace
//            rows (zero-padded to steps);
//   kInvZb3: 1 / Zb3 = 1 / (x - x_last) (utils.rs:466-474; x_last = g2^((steps - 1) skips) depends on
//            the size alone), 0 at x_last as multi_inv gives it, as Montgomery images (r1cs_zb_kernel);
//   kInvXm1: 1 / (x - 1), the same way (0 at x = 1): the table of 1 / Zb2's partial fractions.
// Call before the proof enqueues work on `s`: a first call synchronises s.  An IDX extension larger
// than the cache cap lives in a per-context buffer for this proof only; the others are not built
// when they cannot be cached (*out = nullptr: the caller computes them as part of the proof).
//   kSpotF0 / kSpotIdx: F0's / IDX's first forward pass, transposed (ntt_first_pass_tmajor: the verifier's
//            cold build, circuit_spot_values; world 1), not built when it cannot be cached.
enum : uint32_t { kExtIdx = 0, kExtF0 = 1, kInvZb3 = 2, kInvXm1 = 3, kSpotF0 = 4, kSpotIdx = 5 };
static stark_status ext_const_column(stark_ctx* ctx, uint32_t kind, uint64_t os, uint32_t log_steps,
                                     uint32_t log_prec, uint32_t log_g, uint32_t r, const Twiddles& tw_g1_inv,
                                     const Twiddles& tw_g2, const Twiddles& tw_h, hipStream_t s, const fe** out) {
  const bool spot = kind == kSpotF0 || kind == kSpotIdx;
  if (spot && (log_g || r)) return STARK_ERR_BAD_ARG;
  const uint64_t tag = (kind == kExtF0 || kind == kSpotF0) ? os : 0;
  const auto key = std::make_tuple(kind, log_steps, log_prec, log_g, r, tag);
  auto it = ctx->ext_idx.find(key);
  if (it != ctx->ext_idx.end()) {
    it->second.used = ++ctx->cache_clock;
    *out = (const fe*)it->second.ptr;
    return STARK_OK;
  }
  const uint64_t steps = (uint64_t)1 << log_steps, P = (uint64_t)1 << (log_prec - log_g);
  // Counted in the context's capped cache (stark_ctx_set_cache_limit).
  const bool cached = cache_reserve(ctx, P * sizeof(fe), true);
  void *col = nullptr, *coef = nullptr;
  if (cached) {
    if (hipMalloc(&col, P * sizeof(fe)) != hipSuccess) {
      hipGetLastError();
      if (kind != kExtIdx) {
        *out = nullptr;
        return STARK_OK;
      }
      return STARK_ERR_OOM;
    }
    poison_dev(col, P * sizeof(fe));
    ctx->ext_idx[key] = CacheBuf{col, P * sizeof(fe), ++ctx->cache_clock};  // counted while it is built
  } else if (kind != kExtIdx) {
    *out = nullptr;
    return STARK_OK;
  } else {
    STARK_TRY(ensure_buf(ctx, ctx->ext_idx_tmp, P * sizeof(fe)));
    col = ctx->ext_idx_tmp.ptr;
  }
  auto drop = [&] {
    if (cached) {
      ctx->ext_idx.erase(key);
      hipFree(col);
    }
  };
  const bool inv = kind == kInvZb3 || kind == kInvXm1;
  const uint64_t tmp_n = inv ? 2 * P : steps;
  if (hipMalloc(&coef, tmp_n * sizeof(fe)) != hipSuccess) {
    hipGetLastError();
    drop();
    return STARK_ERR_OOM;
  }
  poison_dev(coef, tmp_n * sizeof(fe));
  stark_status st = STARK_OK;
  if (inv) {  // r1cs_zb_kernel with no public points: Zb2 = 1 (unused), x - c in the second half
    const FieldHost& F = FieldHost::get();
    const Mont mc = mont();
    const uint64_t prec = (uint64_t)1 << log_prec, skips = prec >> log_steps;
    const fe c = kind == kInvZb3 ? to_dev(F.pow_u64(tw_g2.root, prec - skips)) : mc.one;
    fe* z = (fe*)coef;
    hipLaunchKernelGGL(r1cs_zb_kernel, dim3(blocks_for(P)), dim3(256), 0, s, tw_g2.d_lo, tw_g2.d_hi, tw_g2.kb, P,
                       (uint64_t)r, log_g, (const fe*)nullptr, 0u, c, mc.rinv, mc.one, z, z + P);
    st = hipGetLastError() == hipSuccess ? STARK_OK : STARK_ERR_HIP;
    if (st == STARK_OK) st = multi_inv_device(ctx, z + P, (fe*)col, P, s);
  } else {
    hipLaunchKernelGGL(const_column_kernel, dim3(blocks_for(steps)), dim3(256), 0, s, (fe*)coef, steps, tag);
    st = hipGetLastError() == hipSuccess ? STARK_OK : STARK_ERR_HIP;
    if (st == STARK_OK && spot) {
      uint32_t log_t = 0;
      st = ntt_device(ctx, (fe*)coef, log_steps, 1, tw_g1_inv, true, s);
      if (st == STARK_OK)
        st = ntt_first_pass_tmajor(ctx, (fe*)coef, log_prec - log_steps, (fe*)col, log_prec, 1, tw_g2, s, &log_t);
    } else if (st == STARK_OK) {
      st = coset_lde(ctx, (fe*)coef, 1, (fe*)col, log_steps, log_prec, log_g, r, tw_g1_inv, tw_g2, tw_h, s);
    }
  }
  if (hipStreamSynchronize(s) != hipSuccess && st == STARK_OK) st = STARK_ERR_HIP;
  hipFree(coef);
  if (st != STARK_OK) {
    drop();
    return st;
  }
  *out = (const fe*)col;
  return STARK_OK;
}

// The size-only columns of one proof (ext_const_column), taken in one place: every later reservation
// may evict an earlier column, so each is looked up again once all are taken (IDX last: its pointer is
// always valid).  want_f0: the flags are a trace builder's (F0 = 1 on the os rows).
struct SharedCols {
  const fe *idx = nullptr, *f0 = nullptr, *izb3 = nullptr, *tinv = nullptr;
};
static stark_status shared_columns(stark_ctx* ctx, bool want_f0, uint64_t os, uint32_t log_steps, uint32_t log_prec,
                                   uint32_t log_g, uint32_t r, const Twiddles& tw_g1_inv, const Twiddles& tw_g2,
                                   const Twiddles& tw_h, hipStream_t s, SharedCols& o) {
  STARK_TRY(ext_const_column(ctx, kInvZb3, 0, log_steps, log_prec, log_g, r, tw_g1_inv, tw_g2, tw_h, s, &o.izb3));
  STARK_TRY(ext_const_column(ctx, kInvXm1, 0, log_steps, log_prec, log_g, r, tw_g1_inv, tw_g2, tw_h, s, &o.tinv));
  if (want_f0)
    STARK_TRY(ext_const_column(ctx, kExtF0, os, log_steps, log_prec, log_g, r, tw_g1_inv, tw_g2, tw_h, s, &o.f0));
  STARK_TRY(ext_const_column(ctx, kExtIdx, 0, log_steps, log_prec, log_g, r, tw_g1_inv, tw_g2, tw_h, s, &o.idx));
  auto live = [&](uint32_t kind, uint64_t tag) {
    return ctx->ext_idx.count(std::make_tuple(kind, log_steps, log_prec, log_g, r, tag)) != 0;
  };
  if (o.izb3 && !live(kInvZb3, 0)) o.izb3 = nullptr;
  if (o.tinv && !live(kInvXm1, 0)) o.tinv = nullptr;
  if (o.f0 && !live(kExtF0, os)) o.f0 = nullptr;
  return STARK_OK;
}

// 1 / Zb2 = 1 / prod_k (x - x_k) (utils.rs:438-455) by partial fractions: sum_k c_k / (x - x_k) with
// c_k = 1 / prod_(j != k) (x_k - x_j), and 1 / (x - x_k) = x_k^-1 / (x / x_k - 1), where x / x_k is the
// domain point e_k = skips j_k places back, so the term is a_k tinv[i - e_k / 2^log_g] with
// a_k = c_k / x_k (Montgomery, like the table).  The same field value as the batch inverse, bit for
// bit (both canonical); at x = x_k the kernel gives 0 as the batch inverse does.  Up to 8 distinct
// points (false otherwise: the proof takes the batch inverse).
static bool zb2_partial_fractions(const HostFp& g2, uint64_t prec, uint64_t skips, uint32_t log_g,
                                  const size_t* public_first_indices, size_t n_pfi, ConstraintArgs& ca) {
  const FieldHost& F = FieldHost::get();
  constexpr size_t kMaxPf = sizeof(ca.pf_shift) / sizeof(ca.pf_shift[0]);
  if (n_pfi == 0 || n_pfi > kMaxPf) return false;
  std::vector<HostFp> xs(n_pfi);
  for (size_t k = 0; k < n_pfi; ++k) {
    const uint64_t e = (skips * (uint64_t)public_first_indices[2 * k + 1]) % prec;  // a multiple of skips
    xs[k] = F.pow_u64(g2, e);
    ca.pf_shift[k] = e >> log_g;
  }
  for (size_t k = 0; k < n_pfi; ++k) {
    HostFp c = xs[k];
    for (size_t j = 0; j < n_pfi; ++j) {
      if (j == k) continue;
      const HostFp d = F.sub(xs[k], xs[j]);
      if (FieldHost::eq(d, F.zero())) return false;  // a repeated point
      c = F.mul(c, d);
    }
    ca.pf_coef[k] = to_dev(F.inv(c));
  }
  ca.n_pf = (uint32_t)n_pfi;
  return true;
}

// The host part of the transcript's c_db: R^-1, the partial-fraction coefficients a_k and the 24 inv(Z) R^k
// constants (ca.pf_coef and ca.invz_m hold Montgomery images, which are the HostFp representation itself:
// the tables are of the values the Montgomery products multiply by).  A pageable copy: the
// runtime stages it before returning, so the table may live on this stack.
static Pow32 pow32() {
  const FieldHost& F = FieldHost::get();
  Pow32 p;
  HostFp x = F.one();
  const HostFp t = F.from_u64((uint64_t)1 << 32);
  for (int i = 0; i < 8; ++i) {
    p.m[i] = to_dev(x);
    x = F.mul(x, t);
  }
  return p;
}

static stark_status upload_constraint_tables(stark_ctx* ctx, Transcript* d_tr, const ConstraintArgs& ca,
                                             hipStream_t s) {
  const FieldHost& F = FieldHost::get();
  // built in pinned slot 4 (its first kPinned4ConstsOff bytes), so the copy is asynchronous
  static_assert(sizeof(uint32_t) * 33 * 72 <= kPinned4ConstsOff, "pinned slot 4 layout");
  void* pin = nullptr;
  STARK_TRY(ctx_pinned(ctx, 4, kPinned4ConstsOff, &pin));
  uint32_t(&t)[33][72] = *reinterpret_cast<uint32_t(*)[33][72]>(pin);
  db_table(F.inv(F.pow_u64(F.from_u64(2), 256)), t[0]);  // R^-1
  const uint32_t n = ca.tinv ? ca.n_pf : 0;
  for (uint32_t k = 0; k < 8; ++k) {
    HostFp c;
    if (k < n) memcpy(c.v, &ca.pf_coef[k], 32);
    else c = F.zero();
    db_table(c, t[1 + k]);
  }
  for (int k = 0; k < 3; ++k)
    for (int u = 0; u < 8; ++u) {
      HostFp c;
      memcpy(c.v, &ca.invz_m[k][u], 32);
      db_table(c, t[9 + 8 * k + u]);
    }
  STARK_HIP(ctx, hipMemcpyAsync(&d_tr->c_db[0][0], &t[0][0], sizeof t, hipMemcpyHostToDevice, s));
  return STARK_OK;
}

static stark_status ext_index_column(stark_ctx* ctx, uint32_t log_steps, uint32_t log_prec, uint32_t log_g,
                                     uint32_t r, const Twiddles& tw_g1_inv, const Twiddles& tw_g2,
                                     const Twiddles& tw_h, hipStream_t s, const fe** out) {
  return ext_const_column(ctx, kExtIdx, 0, log_steps, log_prec, log_g, r, tw_g1_inv, tw_g2, tw_h, s, out);
}

// The proof's roots (prove.rs:71-94): g2 = 7^((p-1)/precision), g1 = g2^skips = xs[skips], and
// h = g2^world (the generator of one rank's residue class of the domain), with the twiddle
// tables of g2, g1^-1 (the LDE's iNTT) and h.
struct ProofRoots {
  HostFp g2;
  uint64_t g2c[4];
  const Twiddles *tw2 = nullptr, *tw1i = nullptr, *twh = nullptr;
};

static stark_status proof_roots(stark_ctx* ctx, uint32_t log_steps, uint32_t log_prec, uint32_t world,
                                ProofRoots& R) {
  const FieldHost& F = FieldHost::get();
  uint64_t pm1[4];  // (p - 1) / precision
  memcpy(pm1, FieldHost::kP, 32);
  pm1[0] -= 1;
  for (uint32_t k = 0; k < log_prec; ++k)
    for (int l = 0; l < 4; ++l) pm1[l] = (pm1[l] >> 1) | (l < 3 ? pm1[l + 1] << 63 : 0);
  R.g2 = F.pow(F.from_u64(7), pm1, 4);
  uint32_t log_g = 0;
  while ((1u << log_g) < world) ++log_g;
  uint64_t g1ic[4], hc[4];
  F.to_canonical(R.g2, R.g2c);
  F.to_canonical(F.inv(F.pow_u64(R.g2, (uint64_t)1 << (log_prec - log_steps))), g1ic);
  F.to_canonical(F.pow_u64(R.g2, world), hc);
  STARK_TRY(get_twiddles(ctx, R.g2c, log_prec, &R.tw2));
  STARK_TRY(get_twiddles(ctx, g1ic, log_steps, &R.tw1i));
  STARK_TRY(get_twiddles(ctx, hc, log_prec - log_g, &R.twh));
  return STARK_OK;
}

// The proof's host-side constants (utils.rs:421-474): the boundary points x_k = g2^(skips w_k) of
// the public wires' first uses (Montgomery, for Zb2), the coefficients of the interpolant I2
// through (x_k, public value) and of I3 through (x_last, 1) (canonical): 2 n_pfi + 1 elements.
// with_i2 = false (the column route: the device interpolates, public_coefficients): the 2 n_pfi elements
// stay zero, unread.
static std::vector<fe> boundary_consts(const HostFp& g2, uint64_t prec, uint64_t skips, const uint64_t* public_wires,
                                       const size_t* public_first_indices, size_t n_pfi, bool with_i2,
                                       HostFp* x_last_out) {
  const FieldHost& F = FieldHost::get();
  const HostFp x_last = F.pow_u64(g2, prec - skips);
  std::vector<HostFp> xv(n_pfi, F.zero()), yv(n_pfi, F.zero());
  for (size_t i = 0; with_i2 && i < n_pfi; ++i) {
    xv[i] = F.pow_u64(g2, skips * public_first_indices[2 * i + 1]);
    yv[i] = host_fe(public_wires + 4 * public_first_indices[2 * i]);
  }
  const std::vector<HostFp> interp2 = with_i2 ? lagrange_interp(xv, yv) : xv;
  const std::vector<HostFp> interp3 = lagrange_interp({x_last}, {F.one()});
  auto canon_fe = [&](const HostFp& x) {
    uint64_t c[4];
    F.to_canonical(x, c);
    fe v;
    for (int k = 0; k < 4; ++k) {
      v.w[2 * k] = (uint32_t)c[k];
      v.w[2 * k + 1] = (uint32_t)(c[k] >> 32);
    }
    return v;
  };
  std::vector<fe> h(2 * n_pfi + 2);
  for (size_t i = 0; i < n_pfi; ++i) {
    h[i] = to_dev(xv[i]);
    h[n_pfi + i] = canon_fe(interp2[i]);
  }
  h[2 * n_pfi] = canon_fe(interp3[0]);
  *x_last_out = x_last;
  return h;
}

// ---- the constraint stage ---------------------------------------------------------------------------
//
// What a proof runs up to its constraint rows, on one GPU (prove_r1cs: the whole domain, log_g = rank = 0)
// or as one rank of a world (dprove_begin: the points rank + 2^log_g j).  Both hosts call the steps below
// in the same order; where they differ on purpose (streams, trees, arenas, how Zb is inverted) the
// difference is an argument of a step or stays in the host.

struct StageDims {
  uint32_t log_steps = 0, log_prec = 0, log_g = 0, rank = 0;
  uint64_t os = 0, steps = 0, prec = 0, skips = 0;
  uint64_t P = 0;  // this host's points: prec >> log_g
};

// prove.rs:30-53's argument checks and the sizes they give.
static stark_status stage_dims(const TraceView& v, uint32_t world, uint32_t rank, StageDims& d) {
  if (world == 0 || world > (uint32_t)kExtensionFactor || (world & (world - 1)) || rank >= world)
    return STARK_ERR_BAD_ARG;
  if (v.os > 3 * v.n_constraints * v.n_wires || v.os % 3 != 0) return STARK_ERR_BAD_ARG;
  if (v.os < 5) return STARK_ERR_BAD_LENGTH;  // the reference's steps/log_steps disagree below 8 steps
  d.log_steps = log2_ceil_ref(v.os - 1);
  d.log_prec = d.log_steps + kLogExtensionFactor;
  // get_pseudorandom_indices(_, precision, ...) asserts precision < 2^24 (fri/src/utils.rs:88), first reached
  // when r is derived (utils.rs:279); the reference cannot prove larger traces.
  if (d.log_prec >= 24) return STARK_ERR_BAD_LENGTH;
  d.log_g = 0;
  while ((1u << d.log_g) < world) ++d.log_g;
  d.rank = rank;
  d.os = v.os;
  d.steps = (uint64_t)1 << d.log_steps;
  d.prec = (uint64_t)1 << d.log_prec;
  d.skips = d.prec / d.steps;
  d.P = d.prec >> d.log_g;
  for (size_t i = 0; i < v.n_pfi; ++i)
    if (v.pfi[2 * i] >= v.n_public || v.pfi[2 * i + 1] >= d.steps) return STARK_ERR_BAD_ARG;
  return STARK_OK;
}

// One proof's working set up to the constraint rows.
struct Stage {
  StageDims d;
  ProofRoots roots;  // twh = tw2 on one GPU (h = g2)
  Mont mc;
  // The shared size-only columns (prepared circuits carry their own): IDX's extension; F0's whenever the
  // flags are a trace builder's (flag bytes, calc_flags run.rs:283-308: 1 on the os rows), so only
  // K F1 F2 S P PIDX are extended; 1 / Zb3; and the table that gives 1 / Zb2 by partial fractions
  // (ca.tinv), so the proof has no batch inverse over the domain at all (zb2_partial_fractions).
  SharedCols sc;
  ConstraintArgs ca;
  HostFp x_last;
  std::vector<fe> consts_h;  // boundary_consts: alive until the host's synchronisation behind their upload
  fe *raw, *wcopy, *cols, *nmr, *dnm, *tot, *dnm_c, *inv_dnm, *zb, *inv_zb, *consts, *rows, *lvals;
  uint64_t *perm, *acc_leaves;
  Transcript* d_tr;
  uint32_t nb;     // the scans' blocks
  InvPlan inv_d;   // the batch inverse of A's denominators
  // The column route (public_columns): Zb2's (times R^-1) and I2's coefficients, steps each, zero-padded,
  // and I2's extension.
  bool pub_cols = false;
  fe *pubc = nullptr, *i2col = nullptr;
};

static stark_status stage_begin(stark_ctx* ctx, const TraceView& v, const fe* pre, uint32_t world, uint32_t rank,
                                hipStream_t s, Stage& st) {
  STARK_TRY(stage_dims(v, world, rank, st.d));
  const StageDims& d = st.d;
  // Roots (prove.rs:71-94): g2 = 7^((p-1)/precision), g1 = g2^8; h = g2^world generates a rank's coset.
  STARK_TRY(proof_roots(ctx, d.log_steps, d.log_prec, world, st.roots));
  st.mc = mont();
  if (!pre)
    STARK_TRY(shared_columns(ctx, v.flag_bytes != nullptr, d.os, d.log_steps, d.log_prec, d.log_g, d.rank,
                             *st.roots.tw1i, *st.roots.tw2, *st.roots.twh, s, st.sc));
  st.ca.tinv = nullptr;
  if (st.sc.tinv && st.sc.izb3 &&
      zb2_partial_fractions(st.roots.g2, d.prec, d.skips, d.log_g, v.pfi, v.n_pfi, st.ca))
    st.ca.tinv = st.sc.tinv;
  st.pub_cols = public_columns(ctx, v.n_pfi, d.steps);
  return STARK_OK;
}

// The working set carved out of the host's arena (zb also stages the flag bytes: zb_count elements), and
// the interpolants and boundary points (utils.rs:421-474), host side (#pub points).
static stark_status stage_buffers(stark_ctx* ctx, const TraceView& v, Stage& st, size_t zb_count, DevBuf& arena) {
  const uint64_t steps = st.d.steps, P = st.d.P;
  st.nb = (uint32_t)((steps + kScanBlock - 1) / kScanBlock);
  Carve cv;
  cv.add(&st.raw, 7 * steps);  // K F0 F1 F2 S P PIDX (then A's coefficients reuse K's slot)
  cv.add(&st.wcopy, steps);
  cv.add(&st.perm, steps);
  cv.add(&st.acc_leaves, 5 * steps);
  cv.add(&st.cols, 8 * P);  // the extensions of K F0 F1 F2 S P PIDX A (IDX's is shared: sc.idx)
  cv.add(&st.nmr, steps);
  cv.add(&st.dnm, steps);
  cv.add(&st.tot, 2 * (size_t)st.nb);
  cv.add(&st.dnm_c, steps);
  cv.add(&st.inv_dnm, steps);
  cv.add(&st.zb, zb_count);
  cv.add(&st.inv_zb, 2 * P);
  cv.add(&st.consts, 2 * v.n_pfi + 2);
  cv.add(&st.rows, 8 * P);
  cv.add(&st.lvals, P);
  cv.add(&st.d_tr, 1);
  if (st.pub_cols) {
    cv.add(&st.pubc, 2 * steps);
    cv.add(&st.i2col, P);
  }
  STARK_TRY(cv.commit(ctx, arena));
  st.consts_h = boundary_consts(st.roots.g2, st.d.prec, st.d.skips, v.public_wires, v.pfi, v.n_pfi, !st.pub_cols,
                                &st.x_last);
  return STARK_OK;
}

// The column route's coefficients, before anything of the proof is enqueued on s (the interpolation's batch
// inverse takes a host round trip): I2's into pubc + steps and, with_zb2 (no table gives 1 / Zb2), Zb2's
// times R^-1 into pubc.  (A batch's I2 coefficients come from the circuit's interpolation plan instead,
// prove_r1cs_batch.)
static stark_status public_coefficients(stark_ctx* ctx, const TraceView& v, const Stage& st, bool with_zb2,
                                        hipStream_t s) {
  const uint64_t steps = st.d.steps;
  const size_t n = v.n_pfi;
  STARK_HIP(ctx, hipMemsetAsync(st.pubc, 0, 2 * steps * sizeof(fe), s));
  DomainHint hint;
  std::vector<uint64_t> staging;
  hint.log_order = st.d.log_steps;
  const size_t scratch = lagrange_scratch_elems(n, &hint);  // (n < steps: Z' fits the domain)
  STARK_TRY(buf_acquire(ctx, ctx->poly, s));
  STARK_TRY(ensure_buf(ctx, ctx->poly, (scratch + 2 * n) * sizeof(fe) + n * sizeof(uint64_t)));
  fe* mem = (fe*)ctx->poly.ptr;
  fe* xy = mem + scratch;
  STARK_TRY(public_points(ctx, st.roots.g2, st.d.skips, st.d.log_steps, v.public_wires, v.pfi, n,
                          (uint64_t*)(xy + 2 * n), xy, hint, staging, s));
  fe* z = nullptr;  // (the interpolation synchronises s for its batch inverse: staging is free after it)
  STARK_TRY(lagrange_interp_device(ctx, xy, xy + n, n, st.pubc + steps, mem, s, &hint, &z));
  if (with_zb2) {
    hipLaunchKernelGGL(scale_rinv_kernel, dim3(blocks_for(n + 1)), dim3(256), 0, s, (const fe*)z, (uint64_t)(n + 1),
                       st.pubc);
    STARK_HIP(ctx, hipGetLastError());
  }
  return buf_release(ctx, ctx->poly, s);
}

// Column c of pubc (0: Zb2 R^-1, 1: I2) at this host's points.
static stark_status public_extend(stark_ctx* ctx, const Stage& st, int c, fe* out, hipStream_t s) {
  return coset_forward(ctx, st.pubc + c * st.d.steps, 1, out, st.d.log_steps, st.d.log_prec, st.d.log_g, st.d.rank,
                       *st.roots.tw2, *st.roots.twh, s);
}

// The step columns with zero tails (prove.rs:59-69; inv_best_fft pads the flags), host or device sources
// (hipMemcpyDefault), 0/1 flag bytes widened on the GPU; K moved into F0's slot when F0's extension is
// shared (the six extended columns are then contiguous from slot 1); the permutation, the witness copy
// and the transcript's zero fill.
static stark_status stage_uploads(stark_ctx* ctx, const TraceView& v, const fe* pre, const Stage& st, hipStream_t s) {
  const uint64_t steps = st.d.steps, os = st.d.os;
  fe* const raw = st.raw;
  for (int c = pre ? 4 : 0; c < 6; ++c) {
    if (!(v.flag_bytes && c >= 1 && c <= 3))
      STARK_HIP(ctx, hipMemcpyAsync(raw + c * steps, v.col[c], os * sizeof(fe), hipMemcpyDefault, s));
    if (steps > os) STARK_HIP(ctx, hipMemsetAsync(raw + c * steps + os, 0, (steps - os) * sizeof(fe), s));
  }
  if (v.flag_bytes && !pre) {
    uint8_t* d_fb = (uint8_t*)st.zb;  // zb is free until the Zb kernel
    STARK_HIP(ctx, hipMemcpyAsync(d_fb, v.flag_bytes, 3 * os, hipMemcpyDefault, s));
    hipLaunchKernelGGL(r1cs_flags_kernel, dim3(blocks_for(3 * os)), dim3(256), 0, s, (const uint8_t*)d_fb, os, steps,
                       raw + steps);
    STARK_HIP(ctx, hipGetLastError());
  }
  static_assert(sizeof(size_t) == sizeof(uint64_t), "size_t is 64-bit");
  if (st.sc.f0) STARK_HIP(ctx, hipMemcpyAsync(raw + steps, raw, steps * sizeof(fe), hipMemcpyDeviceToDevice, s));
  STARK_HIP(ctx, hipMemcpyAsync(st.perm, v.perm, os * sizeof(uint64_t), hipMemcpyDefault, s));
  STARK_HIP(ctx, hipMemcpyAsync(st.wcopy, raw + 4 * steps, steps * sizeof(fe), hipMemcpyDeviceToDevice, s));
  STARK_HIP(ctx, hipMemsetAsync(st.d_tr, 0, sizeof(Transcript), s));
  return STARK_OK;
}

// The same as one launch, when every source is a device pointer (TraceView::dev_pack, one GPU only).
static stark_status stage_pack(stark_ctx* ctx, const TraceView& v, const Stage& st, hipStream_t s) {
  if (!v.flag_bytes && (!v.col[1] || !v.col[2] || !v.col[3])) return STARK_ERR_BAD_ARG;
  PackArgs pa;
  for (int c = 0; c < 6; ++c) pa.col[c] = (const fe*)v.col[c];
  pa.fb = v.flag_bytes;
  pa.perm_in = (const uint64_t*)v.perm;
  pa.os = st.d.os;
  pa.steps = st.d.steps;
  pa.raw = st.raw;
  pa.wcopy = st.wcopy;
  pa.perm = st.perm;
  static_assert(sizeof(Transcript) % 4 == 0, "transcript words");
  pa.tr = (uint32_t*)st.d_tr;
  pa.tr_words = (uint32_t)(sizeof(Transcript) / 4);
  pa.k_slot = st.sc.f0 ? 1 : 0;
  hipLaunchKernelGGL(r1cs_pack_kernel, dim3(blocks_for(std::max<uint64_t>(st.d.steps, pa.tr_words))), dim3(256), 0, s,
                     pa);
  STARK_HIP(ctx, hipGetLastError());
  return STARK_OK;
}

// PIDX's step column (slot 6; IDX is not materialised: sc.idx is its shared extension) and the accumulator
// tree -> a_root (utils.rs:250-270).  acc_dig non-null (merkle_level0): the index kernel hashes each 40-B
// leaf as it writes it, and the tree is built from those digests.
static stark_status stage_accumulator(stark_ctx* ctx, const Stage& st, stark_merkle_tree* acc_tree, uint32_t* acc_dig,
                                      hipStream_t s) {
  const uint64_t steps = st.d.steps;
  hipLaunchKernelGGL(r1cs_index_kernel, dim3(blocks_for(steps)), dim3(256), 0, s, (const uint64_t*)st.perm, st.d.os,
                     steps, (const fe*)st.wcopy, st.raw + 6 * steps, st.acc_leaves, acc_dig);
  STARK_HIP(ctx, hipGetLastError());
  return merkle_build(ctx, acc_tree, (const uint8_t*)st.acc_leaves, steps, 40, s, 0, acc_dig != nullptr);
}

// The context's second stream and its event, created on first use.
static stark_status aux_stream(stark_ctx* ctx) {
  if (!ctx->ev_aux) STARK_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_aux, hipEventDisableTiming));
  if (!ctx->aux) STARK_HIP(ctx, hipStreamCreateWithFlags(&ctx->aux, hipStreamNonBlocking));
  return STARK_OK;
}

// A (utils.rs:293-339, prove.rs:183-184): r from a_root (utils.rs:272-290), the running products of the
// numerators and denominators over the steps, their batch inverse (whose top level is the proof's one
// mid-pipeline host round trip) and A = nmr / dnm.  It reads the trace and a_root only (IDX and PIDX at
// the step points are i and the permutation), so on sa = the aux stream it runs beside the main LDE,
// which the host enqueues between the two halves; on sa = s it runs in line.
// The enqueue half: up to the scans, and io2's guard taken for sa (it covers the pinned top arrays too:
// multi_inv_device on another stream uses both).  The host then enqueues the denominators' multi_inv_up
// on sa with the scratch of its choice.
static stark_status a_chain_enqueue(stark_ctx* ctx, Stage& st, stark_merkle_tree* acc_tree, hipStream_t s,
                                    hipStream_t sa) {
  const uint64_t steps = st.d.steps;
  if (sa != s) {
    STARK_HIP(ctx, hipEventRecord(ctx->ev_aux, s));  // the trace columns, the transcript's zero fill, a_root
    STARK_HIP(ctx, hipStreamWaitEvent(sa, ctx->ev_aux, 0));
  }
  hipLaunchKernelGGL(r1cs_r_kernel<false>, dim3(1), dim3(64), 0, sa, (const uint32_t*)merkle_root_dev(acc_tree),
                     (uint32_t)(st.d.prec - 1), st.mc.r2, pow32(), st.d_tr, ForestRoots{});
  STARK_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(r1cs_a_vals_kernel, dim3(blocks_for(steps)), dim3(256), 0, sa, (const fe*)nullptr,
                     (const fe*)nullptr, (const uint64_t*)st.perm, st.d.os, (const fe*)st.wcopy, steps,
                     (const Transcript*)st.d_tr, st.mc.r2, st.nmr, st.dnm);
  STARK_HIP(ctx, hipGetLastError());
  STARK_TRY(product_scan(ctx, ScanArrays{{st.nmr, st.dnm}, {st.tot, st.tot + st.nb}, {nullptr, st.dnm_c}}, 2, steps,
                         st.mc, sa));
  return buf_acquire(ctx, ctx->io2, sa);
}

static stark_status a_denominators_up(stark_ctx* ctx, Stage& st, hipStream_t sa, DevBuf& scratch) {
  fe* const top_d = multi_inv_h_top(ctx, 0);
  if (!top_d) return STARK_ERR_OOM;
  return multi_inv_up(ctx, st.dnm_c, st.inv_dnm, st.d.steps, sa, scratch, top_d, st.inv_d);
}

// Which step columns are extended here, into their slots of cols.
static stark_status extend_columns(stark_ctx* ctx, const Stage& st, fe* coef, uint32_t batch, fe* out, hipStream_t s) {
  return coset_lde(ctx, coef, batch, out, st.d.log_steps, st.d.log_prec, st.d.log_g, st.d.rank, *st.roots.tw1i,
                   *st.roots.tw2, *st.roots.twh, s);
}
static stark_status extend_trace(stark_ctx* ctx, const Stage& st, const fe* pre, hipStream_t s) {
  const uint64_t steps = st.d.steps, P = st.d.P;
  if (pre)  // S and P only: K, the flags, IDX and PIDX are the circuit's
    return extend_columns(ctx, st, st.raw + 4 * steps, 2, st.cols + 4 * P, s);
  if (st.sc.f0)  // K (in F0's slot) F1 F2 S P PIDX
    return extend_columns(ctx, st, st.raw + steps, 6, st.cols + P, s);
  return extend_columns(ctx, st, st.raw, 7, st.cols, s);  // K F0 F1 F2 S P PIDX
}

// The finish half: the host round trip (shared_top: a second batch inverse whose up pass the host enqueued,
// so that both top levels are inverted behind this one synchronisation), the denominators' down pass,
// A = nmr / dnm into dnm (free after its scan's canonical copy; raw may still be read by the LDE), s
// joined behind sa, and A's extension in slot 7.
static stark_status a_chain_finish(stark_ctx* ctx, Stage& st, hipStream_t s, hipStream_t sa,
                                   const InvPlan* shared_top = nullptr) {
  const uint64_t steps = st.d.steps;
  STARK_HIP(ctx, hipStreamSynchronize(sa));
  multi_inv_top(st.inv_d);
  if (shared_top) multi_inv_top(*shared_top);
  STARK_TRY(multi_inv_down(ctx, st.inv_d, sa));
  hipLaunchKernelGGL(r1cs_a_mini_kernel, dim3(blocks_for(steps)), dim3(256), 0, sa, (const fe*)st.nmr,
                     (const fe*)st.inv_dnm, steps, st.dnm);
  STARK_HIP(ctx, hipGetLastError());
  STARK_TRY(buf_release(ctx, ctx->io2, sa));
  if (sa != s) {
    STARK_HIP(ctx, hipEventRecord(ctx->ev_aux, sa));
    STARK_HIP(ctx, hipStreamWaitEvent(s, ctx->ev_aux, 0));
  }
  return extend_columns(ctx, st, st.dnm, 1, st.cols + 7 * st.d.P, s);
}

// Zb2 = prod_k (x - x_k), Zb3 = x - x_last at this host's points (utils.rs:438-474) into zb, for a proof
// that has no table of their inverses; *count = how many values the host then inverts (Zb2's, and Zb3's
// unless 1 / Zb3 is the shared column).
static stark_status zb_enqueue(stark_ctx* ctx, const Stage& st, size_t n_pfi, hipStream_t s, uint64_t* count) {
  const Twiddles* tw2 = st.roots.tw2;
  const uint64_t P = st.d.P;
  if (st.pub_cols) STARK_TRY(public_extend(ctx, st, 0, st.zb, s));  // Zb2 from its coefficients
  if (!st.pub_cols || !st.sc.izb3) {
    hipLaunchKernelGGL(r1cs_zb_kernel, dim3(blocks_for(P)), dim3(256), 0, s, tw2->d_lo, tw2->d_hi, tw2->kb, P,
                       (uint64_t)st.d.rank, st.d.log_g, (const fe*)st.consts, (uint32_t)n_pfi, to_dev(st.x_last),
                       st.mc.rinv, st.mc.one, st.pub_cols ? nullptr : st.zb, st.sc.izb3 ? nullptr : st.zb + P);
    STARK_HIP(ctx, hipGetLastError());
  }
  *count = st.sc.izb3 ? P : 2 * P;
  return STARK_OK;
}

// The constraint kernel's arguments and their tables (upload_constraint_tables).  plane: the rows'
// layout (ConstraintArgs::rows).  The shifts are multiples of 8, hence of 2^log_g.
static stark_status constraint_args(stark_ctx* ctx, const TraceView& v, const fe* pre, Stage& st, uint64_t plane,
                                    hipStream_t s) {
  const StageDims& d = st.d;
  const uint64_t P = d.P;
  const Twiddles* tw2 = st.roots.tw2;
  ConstraintArgs& ca = st.ca;
  for (int c = 0; c < 6; ++c) ca.col[c] = st.cols + (size_t)c * P;
  ca.col[6] = pre ? pre + 4 * P : st.sc.idx;
  ca.col[7] = pre ? pre + 5 * P : st.cols + 6 * P;
  ca.col[8] = st.cols + 7 * P;  // A
  if (st.sc.f0) {
    ca.col[0] = st.cols + P;  // K
    ca.col[1] = st.sc.f0;
  }
  if (pre)
    for (int c = 0; c < 4; ++c) ca.col[c] = pre + (size_t)c * P;
  ca.inv_zb = pre ? pre + 6 * P : st.inv_zb;
  ca.inv_zb3 = st.sc.izb3 ? st.sc.izb3 : ca.inv_zb + P;
  ca.interp2 = st.consts + v.n_pfi;
  ca.interp3 = st.consts + 2 * v.n_pfi;
  ca.i2_col = nullptr;
  if (st.pub_cols) {  // I2 from its coefficients
    STARK_TRY(public_extend(ctx, st, 1, st.i2col, s));
    ca.i2_col = st.i2col;
  }
  ca.lo = tw2->d_lo;
  ca.hi = tw2->d_hi;
  ca.rows = st.rows;
  ca.plane = plane;
  ca.err = &st.d_tr->err;
  ca.prec = P;
  ca.shift1 = ((d.os / 3 * d.skips) % d.prec) >> d.log_g;
  ca.shift2 = ((d.os / 3 * 2 * d.skips) % d.prec) >> d.log_g;
  ca.back = d.skips >> d.log_g;
  ca.g_add = d.rank;
  ca.log_g = d.log_g;
  ca.log_prec = d.log_prec;
  ca.kb = tw2->kb;
  ca.n2 = (uint32_t)v.n_pfi;
  ca.n3 = 1;
  ca.tr = st.d_tr;
  set_inv_z(ca, st.roots.g2, d.steps);
  ca.mont_cols = pre ? 1 : 0;
  return upload_constraint_tables(ctx, st.d_tr, ca, s);
}

static stark_status constraint_launch(stark_ctx* ctx, const Stage& st, hipStream_t s) {
  hipLaunchKernelGGL(r1cs_constraint_kernel<false>, dim3(blocks_for(st.d.P)), dim3(256), 0, s, st.ca,
                     ConstraintBatch{});
  STARK_HIP(ctx, hipGetLastError());
  return STARK_OK;
}

// The eight powers of g2^steps (the k kernel's xs table).
static XsPowers xs_powers(const HostFp& g2, uint64_t steps) {
  const FieldHost& F = FieldHost::get();
  XsPowers xs;
  const HostFp w8 = F.pow_u64(g2, steps);
  HostFp wt = F.one();
  for (int t = 0; t < 8; ++t) {
    xs.v[t] = to_dev(wt);
    wt = F.mul(wt, w8);
  }
  return xs;
}

// Transcript::err (the constraint kernel's flags) as a call's status and message.
static stark_status transcript_status(stark_ctx* ctx, int err) {
  if (!err) return STARK_OK;
  ctx->last_error = (err & 1) ? "invalid D: Q does not vanish where Z does (utils.rs:379-418)"
                              : "invalid B: boundary value mismatch (utils.rs:477-524)";
  return STARK_ERR_CHECK;
}

// pre != nullptr: the circuit's LDE columns K F0 F1 F2 IDX PIDX (precision each) and the inverses of
// Zb2, Zb3 (2 x precision), prepared once per circuit (stark_r1cs_circuit_new); only S, P and A are
// extended here.
static stark_status prove_r1cs(stark_ctx* ctx, const TraceView& v, const fe* pre, stark_r1cs_proof** out) {
  PhaseClock clk("mk_r1cs_proof");
  hipStream_t s = ctx->stream;
  Stage st;
  STARK_TRY(stage_begin(ctx, v, pre, 1, 0, s, st));
  const uint32_t log_prec = st.d.log_prec;
  const uint64_t os = st.d.os, prec = st.d.prec, skips = st.d.skips;
  const Mont& mc = st.mc;
  STARK_TRY(stage_buffers(ctx, v, st, 2 * prec, ctx->r1cs_arena));
  fe* const rows = st.rows;
  fe* const lvals = st.lvals;
  Transcript* const d_tr = st.d_tr;
  {  // the boundary constants through pinned slot 4 (an asynchronous copy; a pageable one blocks the host)
    const std::vector<fe>& h = st.consts_h;
    uint8_t* pin = nullptr;
    STARK_TRY(ctx_pinned(ctx, 4, kPinned4ConstsOff + h.size() * sizeof(fe), (void**)&pin));
    memcpy(pin + kPinned4ConstsOff, h.data(), h.size() * sizeof(fe));
    STARK_HIP(ctx, hipMemcpyAsync(st.consts, pin + kPinned4ConstsOff, h.size() * sizeof(fe), hipMemcpyHostToDevice, s));
  }
  if (st.pub_cols) STARK_TRY(public_coefficients(ctx, v, st, !pre && !st.ca.tinv, s));
  if (v.dev_pack && !pre) STARK_TRY(stage_pack(ctx, v, st, s));
  else STARK_TRY(stage_uploads(ctx, v, pre, st, s));
  clk.mark("setup + uploads enqueued");
  auto proof = std::make_unique<stark_r1cs_proof>();
  // The trees are the context's; the index, constraint and linear-combination kernels hash level 0.
  stark_merkle_tree *acc_tree, *m_tree, *l_tree;
  STARK_TRY(ctx_tree(ctx, 2, &acc_tree));
  STARK_TRY(ctx_tree(ctx, 3, &m_tree));
  STARK_TRY(ctx_tree(ctx, 4, &l_tree));
  uint32_t* acc_dig = nullptr;
  STARK_TRY(merkle_level0(ctx, acc_tree, st.d.steps, s, &acc_dig));
  STARK_TRY(stage_accumulator(ctx, st, acc_tree, acc_dig, s));
  // The A chain runs on the aux stream when no Zb inverse shares its round trip.  Otherwise (the cold proof
  // without the partial-fraction table) it runs in line, and the two batch inverses (the A denominators over
  // the steps; Zb2, Zb3 over the precision domain) share one host round trip: both up passes, one
  // synchronisation, both top levels on the host, then the down passes.
  const bool a_aside = pre || st.ca.tinv;
  STARK_TRY(aux_stream(ctx));
  const hipStream_t sa = a_aside ? ctx->aux : s;
  STARK_TRY(a_chain_enqueue(ctx, st, acc_tree, s, sa));
  InvPlan inv_z;
  if (!a_aside) {
    fe* const top_z = multi_inv_h_top(ctx, 1);
    if (!top_z) return STARK_ERR_OOM;
    uint64_t n_zb = 0;
    STARK_TRY(zb_enqueue(ctx, st, v.n_pfi, s, &n_zb));
    STARK_TRY(multi_inv_up(ctx, st.zb, st.inv_zb, n_zb, s, ctx->io2, top_z, inv_z));
  }
  STARK_TRY(a_denominators_up(ctx, st, sa, ctx->inv_tmp));
  STARK_TRY(extend_trace(ctx, st, pre, s));
  STARK_TRY(a_chain_finish(ctx, st, s, sa, &inv_z));
  STARK_TRY(multi_inv_down(ctx, inv_z, s));  // (empty plan when the A chain ran aside)
  // plane = prec, column-major rows: coalesced stores here and loads in the L kernel and the main tree
  STARK_TRY(constraint_args(ctx, v, pre, st, prec, s));
  // Main tree over the 256-B rows (prove.rs:261-264): the constraint kernel hashes each row as it makes it
  // (level 0), the tree's levels above are built from those digests; the proofs open the rows as 8 planes.
  STARK_TRY(merkle_level0(ctx, m_tree, prec, s, &st.ca.leaf));
  STARK_TRY(constraint_launch(ctx, st, s));
  STARK_TRY(merkle_build(ctx, m_tree, (const uint8_t*)rows, prec, 256, s, prec * sizeof(fe), true));
  hipLaunchKernelGGL(r1cs_k_kernel, dim3(1), dim3(kKThreads), 0, s, (const uint32_t*)merkle_root_dev(m_tree), mc.r2,
                     mc.one, xs_powers(st.roots.g2, st.d.steps), pow32(), d_tr);
  STARK_HIP(ctx, hipGetLastError());
  LincombArgs la;
  la.rows = rows;
  la.plane = prec;
  la.out = lvals;
  la.prec = prec;
  la.g_add = 0;
  la.log_g = 0;
  la.tr = d_tr;
  // L tree (prove.rs:329-332): the linear-combination kernel hashes each value as it makes it (level 0).
  STARK_TRY(merkle_level0(ctx, l_tree, prec, s, &la.leaf));
  hipLaunchKernelGGL(r1cs_lincomb_kernel, dim3(blocks_for(prec)), dim3(256), 0, s, la);
  STARK_HIP(ctx, hipGetLastError());
  // Its root launch also copies the root into the transcript (l_root) and writes FRI layer 0's special_x
  // (fri.rs:135) into the FRI's slot 0 of fri_misc; where no tail launch makes the root, kernels do.
  STARK_TRY(ensure_buf(ctx, ctx->fri_misc, kFriMiscBytes));
  STARK_TRY(buf_acquire(ctx, ctx->fri_misc, s));
  RootFe l_rf{(fe*)ctx->fri_misc.ptr, mc.r2, &d_tr->roots[2][0], false};
  STARK_TRY(merkle_build(ctx, l_tree, (const uint8_t*)lvals, prec, 32, s, 0, true, &l_rf));
  if (!l_rf.made) {
    hipLaunchKernelGGL(r1cs_l_root_kernel, dim3(1), dim3(64), 0, s, (const uint32_t*)merkle_root_dev(l_tree), d_tr);
    STARK_HIP(ctx, hipGetLastError());
  }
  // The roots and the constraint flags come down behind the L tree; an event marks them.
  Transcript* h_tr = nullptr;
  // (slot 1 layout: internal.h kPinned1Bytes)
  // (only the head: the constants' digit-basis tables stay on the device)
  constexpr size_t kTrHead = offsetof(Transcript, k_db);
  static_assert(kTrHead <= 2048, "pinned slot 1 layout");
  STARK_TRY(ctx_pinned(ctx, 1, kPinned1Bytes, (void**)&h_tr));
  uint32_t* h_trace_err = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(h_tr) + kPinned1TraceErrOff);
  STARK_HIP(ctx, hipMemcpyAsync(h_tr, d_tr, kTrHead, hipMemcpyDeviceToHost, s));
  if (ctx->trace_err) STARK_HIP(ctx, hipMemcpyAsync(h_trace_err, ctx->trace_err, 4, hipMemcpyDeviceToHost, s));
  STARK_HIP(ctx, hipEventRecord(ctx->ev_aux, s));

  // prove_low_degree(L, g2, precision / 4, skips) on the resident L (prove.rs:367), enqueued behind the rest.
  FriPendingPtr fri_pending;
  clk.mark("prover kernels enqueued");
  STARK_TRY(fri_enqueue(ctx, (const fe*)lvals, prec, st.roots.g2c, prec / 4, (uint32_t)skips, &fri_pending, l_tree,
                        l_rf.made));
  clk.mark("FRI kernels enqueued");
  // While the FRI layers run: the roots, the spot checks (prove.rs:337-362), their openings (gathered on
  // the second stream) and the StarkProof JSON up to fri_proof.
  STARK_HIP(ctx, hipEventSynchronize(ctx->ev_aux));
  clk.mark("wait for the L root");
  if (ctx->trace_err && *h_trace_err) {  // a wire id >= n_wires (reader.rs:4-89 bounds), found by the trace builder
    hipStreamSynchronize(s);
    ctx->last_error = "constraint record with a wire id >= n_wires";
    return STARK_ERR_BAD_ARG;
  }
  if (h_tr->err) {
    hipStreamSynchronize(s);  // (the enqueued FRI work finishes before the proof is dropped)
    return transcript_status(ctx, h_tr->err);
  }
  memcpy(proof->a_root, h_tr->roots[0], 32);
  memcpy(proof->m_root, h_tr->roots[1], 32);
  memcpy(proof->l_root, h_tr->roots[2], 32);
  uint32_t pos32[kSpotChecks];
  STARK_TRY(stark_get_pseudorandom_indices(proof->l_root, 32, (uint32_t)prec, kSpotChecks, (uint32_t)skips, pos32));
  std::vector<size_t> positions(kSpotChecks), aug(4 * kSpotChecks);
  for (int i = 0; i < kSpotChecks; ++i) {
    positions[i] = pos32[i];
    spot_rows(pos32[i], os, skips, prec, &aug[4 * i]);
  }
  std::vector<uint8_t> l_leaves(32 * kSpotChecks), l_nodes(32 * kSpotChecks * log_prec);
  std::vector<uint8_t> m_leaves(256 * 4 * kSpotChecks), m_nodes(32 * 4 * kSpotChecks * log_prec);
  {
    // the trees are complete (behind the event); the gather runs beside the FRI kernels
    std::vector<GatherReq> spot = {{l_tree, positions.data(), (size_t)kSpotChecks, l_leaves.data(), l_nodes.data()},
                                   {m_tree, aug.data(), (size_t)4 * kSpotChecks, m_leaves.data(), m_nodes.data()}};
    STARK_TRY(merkle_gather_batch(ctx, spot, ctx->aux));
  }
  // StarkProof JSON (utils.rs:122-130; run.rs:549 serde_json::to_string), its head rendered now.
  JsonPieces j;
  stark_proof_json_head(proof->m_root, proof->l_root, proof->a_root,
                        {m_leaves, 256, m_nodes, (size_t)4 * kSpotChecks, log_prec},
                        {l_leaves, 32, l_nodes, (size_t)kSpotChecks, log_prec}, j);
  clk.mark("spot-check openings");
  std::vector<GatherReq> extra;
  stark_fri_proof* fri = nullptr;
  {
    // The head renders on the side thread while this one waits for the FRI layers and gathers their
    // openings (for a small proof the FRI kernels finish before the head would be rendered).
    HostTask head([&] { j.prerender(16); });
    const stark_status fst = fri_finish(ctx, fri_pending.get(), extra, &fri);
    clk.mark("FRI wait + indices + gather");
    head.wait();
    clk.mark("proof head JSON (beside them)");
    if (fst != STARK_OK) return fst;
  }
  proof->fri = fri;  // owned by the proof from here on
  fri_proof_json_pieces(fri, j);
  j.text("}");
  j.render(proof->json);
  clk.mark("proof JSON");
  proof->depth = log_prec;
  proof->m_leaves = std::move(m_leaves);
  proof->m_nodes = std::move(m_nodes);
  proof->l_leaves = std::move(l_leaves);
  proof->l_nodes = std::move(l_nodes);
  *out = proof.release();
  return STARK_OK;
}

// ---- batched proofs of one prepared circuit (stark_prove_r1cs_circuit_batch) --------------------------
//
// prove_r1cs with pre != nullptr for B witnesses through one chain of launches: every kernel of the chain takes
// the proof as a grid coordinate (or runs over the proofs' arrays laid back to back where it is elementwise),
// every per-proof array is batch-major (proof b at base + b * len), and the three trees of a proof are tree b of
// three forests.  What stays per witness: the boundary constants and interpolants (host).  On the column route
// I2's coefficients of every proof come from one application of the circuit's interpolation plan (poly.hip
// interp_plan_apply; the plan's one host round trip is the first call's), enqueued with the chain.
// The chain itself keeps the single proof's one mid-pipeline round trip (the batch inverse's top level).

// One chunk's working set, carved out of ctx->prove_batch.
struct BatchBufs {
  WitnessBatchBufs wb;
  fe *wcopy, *pidx, *cols_sp, *cols_a, *nmr, *dnm, *tot, *dnm_c, *inv_dnm, *consts, *rows, *lvals;
  fe *i2coef = nullptr, *i2col = nullptr, *pubv = nullptr;  // the column route (pubv: the boundary points' values)
  uint64_t* acc_leaves;
  Transcript* d_tr;
};

static void batch_carve(Carve& cv, BatchBufs& bb, const PreparedCircuit& c, const StageDims& d, size_t n_pfi,
                        bool pub_cols, size_t B) {
  const uint64_t steps = d.steps, P = d.prec;
  const size_t nb = (size_t)((steps + kScanBlock - 1) / kScanBlock);
  cv.add(&bb.wb.raw, B * c.n_wires * 32);
  cv.add(&bb.wb.wcan, B * c.n_wires);
  cv.add(&bb.wb.wmont, B * c.n_wires);
  cv.add(&bb.wb.list, B * c.n_c);
  cv.add(&bb.wb.count, B);
  cv.add(&bb.wb.sp, 2 * B * steps);  // S P per proof (then destroyed by their extension)
  cv.add(&bb.wcopy, B * steps);
  cv.add(&bb.pidx, B * steps);       // (the index kernel's PIDX column: the circuit's extension is read instead)
  cv.add(&bb.acc_leaves, 5 * B * steps);
  cv.add(&bb.cols_sp, 2 * B * P);
  cv.add(&bb.cols_a, B * P);
  cv.add(&bb.nmr, B * steps);
  cv.add(&bb.dnm, B * steps);
  cv.add(&bb.tot, 2 * B * nb);
  cv.add(&bb.dnm_c, B * steps);
  cv.add(&bb.inv_dnm, B * steps);
  cv.add(&bb.consts, B * (2 * n_pfi + 2));
  cv.add(&bb.rows, 8 * B * P);
  cv.add(&bb.lvals, B * P);
  cv.add(&bb.d_tr, B);
  if (pub_cols) {
    cv.add(&bb.i2coef, B * steps);
    cv.add(&bb.i2col, B * P);
    cv.add(&bb.pubv, B * n_pfi);
  }
}

// The device bytes a chunk of B proofs takes: the arena, the accumulator, main and L forests, the batched FRI's
// forests and columns, and the NTT's ping-pong partner of the 2 B extended columns.
static size_t batch_bytes(const PreparedCircuit& c, const StageDims& d, size_t n_pfi, bool pub_cols, uint32_t B) {
  Carve cv;
  BatchBufs bb;
  batch_carve(cv, bb, c, d, n_pfi, pub_cols, B);
  return cv.off + forest_node_bytes(d.steps, B) + 2 * forest_node_bytes(d.prec, B) +
         fri_batch_bytes(d.prec, B, d.prec / 4) + 2 * (size_t)B * d.prec * sizeof(fe);
}

static ForestRoots forest_roots(const stark_merkle_forest* f) {
  ForestRoots r;
  r.nodes = forest_nodes_dev(f, &r.stride, &r.root_at);
  return r;
}

// The circuit's trace view with one witness' public wires (the sizes and the first uses are every witness').
static TraceView batch_view(const PreparedCircuit& c, const BatchWitness& w) {
  TraceView v = c.view(DevTrace());
  v.public_wires = w.public_wires.data();
  v.n_public = w.public_wires.size() / 4;
  return v;
}

static stark_status prove_r1cs_batch(stark_ctx* ctx, const PreparedCircuit& c, const BatchWitness* const* w,
                                     uint32_t B, stark_r1cs_proof** out, stark_status* statuses) {
  PhaseClock clk("mk_r1cs_proof batch");
  hipStream_t s = ctx->stream;
  const fe* const pre = (const fe*)c.lde.ptr;
  const TraceView v = batch_view(c, *w[0]);
  Stage st;
  STARK_TRY(stage_begin(ctx, v, pre, 1, 0, s, st));
  const StageDims& d = st.d;
  const uint32_t log_prec = d.log_prec;
  const uint64_t os = d.os, steps = d.steps, prec = d.prec, skips = d.skips;
  const size_t n_pfi = v.n_pfi, n_consts = 2 * n_pfi + 2;
  const uint32_t nb = (uint32_t)((steps + kScanBlock - 1) / kScanBlock);
  const Mont& mc = st.mc;
  BatchBufs bb;
  {
    Carve cv;
    batch_carve(cv, bb, c, d, n_pfi, st.pub_cols, B);
    STARK_TRY(cv.commit(ctx, ctx->prove_batch));
  }
  bb.wb.steps = steps;
  for (stark_merkle_forest*& f : ctx->r1cs_forests)
    if (!f) STARK_TRY(stark_merkle_forest_new(ctx, &f));
  stark_merkle_forest *const f_acc = ctx->r1cs_forests[0], *const f_m = ctx->r1cs_forests[1],
                      *const f_l = ctx->r1cs_forests[2];
  // Pinned slot 6: the transcript heads, the boundary constants, on the column route the boundary points' values,
  // the witnesses' staging.
  constexpr size_t kTrHead = offsetof(Transcript, k_db);
  static_assert(kTrHead <= kBatchHeadBytes, "pinned slot 6 layout");
  const size_t heads_bytes = (size_t)B * kBatchHeadBytes, consts_bytes = (size_t)B * n_consts * sizeof(fe);
  const size_t pubv_bytes = st.pub_cols ? (size_t)B * n_pfi * sizeof(fe) : 0;
  uint8_t* pin = nullptr;
  STARK_TRY(ctx_pinned(ctx, 6, heads_bytes + consts_bytes + pubv_bytes + (size_t)B * c.n_wires * 32, (void**)&pin));
  const uint8_t* const h_heads = pin;
  bb.wb.h_stage = pin + heads_bytes + consts_bytes + pubv_bytes;
  {  // per witness: the interpolants through its public wires' values (utils.rs:421-474)
    fe* const h_consts = (fe*)(pin + heads_bytes);
    HostFp x_last;
    for (uint32_t b = 0; b < B; ++b) {
      const std::vector<fe> h = boundary_consts(st.roots.g2, prec, skips, w[b]->public_wires.data(), v.pfi, n_pfi,
                                                !st.pub_cols, &x_last);
      memcpy(h_consts + (size_t)b * n_consts, h.data(), n_consts * sizeof(fe));
    }
    STARK_HIP(ctx, hipMemcpyAsync(bb.consts, h_consts, consts_bytes, hipMemcpyHostToDevice, s));
  }
  if (st.pub_cols) {  // I2's coefficients of every proof, zero-padded to steps: one upload, one plan application
    const InterpPlan* plan = nullptr;
    STARK_TRY(circuit_public_plan(ctx, c, st.roots.g2, skips, d.log_steps, s, &plan));
    uint64_t* const h_pubv = (uint64_t*)(pin + heads_bytes + consts_bytes);
    for (uint32_t b = 0; b < B; ++b)
      for (size_t i = 0; i < n_pfi; ++i)
        memcpy(h_pubv + 4 * ((size_t)b * n_pfi + i), w[b]->public_wires.data() + 4 * v.pfi[2 * i], 32);
    STARK_HIP(ctx, hipMemcpyAsync(bb.pubv, h_pubv, pubv_bytes, hipMemcpyHostToDevice, s));
    const InterpValues ys{(const uint8_t*)bb.pubv, n_pfi * sizeof(fe), nullptr};
    const InterpOut o{(uint8_t*)bb.i2coef, steps * sizeof(fe), false, steps};
    STARK_TRY(interp_plan_apply(ctx, *plan, ys, B, o, s));
  }
  // The constraint kernel's shared arguments and the host-built constants (into tr[0], then every transcript's).
  st.cols = bb.cols_sp;
  st.consts = bb.consts;
  st.rows = bb.rows;
  st.d_tr = bb.d_tr;
  {
    const bool pub = st.pub_cols;
    st.pub_cols = false;  // (I2's columns are extended below, every proof's by one transform)
    const stark_status cst = constraint_args(ctx, v, pre, st, prec, s);
    st.pub_cols = pub;
    STARK_TRY(cst);
  }
  hipLaunchKernelGGL(r1cs_tr_init_batch_kernel, dim3(B), dim3(256), 0, s, bb.d_tr);
  STARK_HIP(ctx, hipGetLastError());
  // 1. The witness columns, S and P of proof b side by side (their tails beyond os zero).
  STARK_HIP(ctx, hipMemsetAsync(bb.wb.sp, 0, 2 * (size_t)B * steps * sizeof(fe), s));
  STARK_TRY(circuit_witness_batch(ctx, c, w, B, bb.wb, s));
  STARK_HIP(ctx, hipMemcpy2DAsync(bb.wcopy, steps * sizeof(fe), bb.wb.sp, 2 * steps * sizeof(fe), steps * sizeof(fe), B,
                                  hipMemcpyDeviceToDevice, s));
  clk.mark("setup + witnesses enqueued");
  // 2. The accumulator forest -> a_root -> r, per proof.
  uint32_t* lvl0 = nullptr;
  size_t lstride = 0;
  STARK_TRY(forest_level0(ctx, f_acc, steps, B, &lvl0, &lstride));
  hipLaunchKernelGGL(r1cs_index_batch_kernel, dim3(blocks_for(steps), B), dim3(256), 0, s, c.perm, os, steps,
                     (const fe*)bb.wcopy, bb.pidx, bb.acc_leaves, lvl0, (uint64_t)lstride);
  STARK_HIP(ctx, hipGetLastError());
  STARK_TRY(forest_build(ctx, f_acc, (const uint8_t*)bb.acc_leaves, steps, 40, B, s, true));
  // 3. The A chain on the aux stream beside the extension of S and P, as the single proof's; the denominators
  // of all proofs through one batch inverse (elementwise, 0 -> 0: the concatenation changes no value).
  STARK_TRY(aux_stream(ctx));
  const hipStream_t sa = ctx->aux;
  STARK_HIP(ctx, hipEventRecord(ctx->ev_aux, s));
  STARK_HIP(ctx, hipStreamWaitEvent(sa, ctx->ev_aux, 0));
  hipLaunchKernelGGL(r1cs_r_kernel<true>, dim3(B), dim3(64), 0, sa, (const uint32_t*)nullptr, (uint32_t)(prec - 1),
                     mc.r2, pow32(), bb.d_tr, forest_roots(f_acc));
  hipLaunchKernelGGL(r1cs_a_vals_batch_kernel, dim3(blocks_for(steps), B), dim3(256), 0, sa, c.perm, os,
                     (const fe*)bb.wcopy, steps, (const Transcript*)bb.d_tr, mc.r2, bb.nmr, bb.dnm);
  {
    const ScanArrays a{{bb.nmr, bb.dnm}, {bb.tot, bb.tot + (size_t)B * nb}, {nullptr, bb.dnm_c}};
    hipLaunchKernelGGL(scan_block_kernel<true>, dim3(nb, 2, B), dim3(256), 0, sa, a, steps, mc.one, nb);
    hipLaunchKernelGGL(scan_tot_batch_kernel, dim3(1, 2, B), dim3(256), 0, sa, a, nb, mc.one);
    hipLaunchKernelGGL(scan_apply_batch_kernel, dim3(blocks_for(steps), 2, B), dim3(256), 0, sa, a, steps, nb, mc.unit);
  }
  STARK_HIP(ctx, hipGetLastError());
  STARK_TRY(buf_acquire(ctx, ctx->io2, sa));
  fe* const top_d = multi_inv_h_top(ctx, 0);
  if (!top_d) return STARK_ERR_OOM;
  InvPlan inv_d;
  STARK_TRY(multi_inv_up(ctx, bb.dnm_c, bb.inv_dnm, (uint64_t)B * steps, sa, ctx->inv_tmp, top_d, inv_d));
  // 4. S and P of every proof as one batch of 2 B columns.
  STARK_TRY(extend_columns(ctx, st, bb.wb.sp, 2 * B, bb.cols_sp, s));
  STARK_HIP(ctx, hipStreamSynchronize(sa));
  multi_inv_top(inv_d);
  STARK_TRY(multi_inv_down(ctx, inv_d, sa));
  hipLaunchKernelGGL(r1cs_a_mini_kernel, dim3(blocks_for((uint64_t)B * steps)), dim3(256), 0, sa, (const fe*)bb.nmr,
                     (const fe*)bb.inv_dnm, (uint64_t)B * steps, bb.dnm);
  STARK_HIP(ctx, hipGetLastError());
  STARK_TRY(buf_release(ctx, ctx->io2, sa));
  STARK_HIP(ctx, hipEventRecord(ctx->ev_aux, sa));
  STARK_HIP(ctx, hipStreamWaitEvent(s, ctx->ev_aux, 0));
  STARK_TRY(extend_columns(ctx, st, bb.dnm, B, bb.cols_a, s));
  // 5. The column route: I2 of every proof from its coefficients.
  if (st.pub_cols)
    STARK_TRY(coset_forward(ctx, bb.i2coef, B, bb.i2col, d.log_steps, d.log_prec, 0, 0, *st.roots.tw2, *st.roots.twh,
                            s));
  // 6. The constraint rows, hashed into level 0 of the main forest (8 planes per proof, as the single tree's).
  ConstraintBatch g{bb.cols_sp, bb.cols_a, bb.consts,  n_consts, st.pub_cols ? bb.i2col : nullptr,
                    bb.rows,    bb.d_tr,   nullptr,    0};
  STARK_TRY(forest_level0(ctx, f_m, prec, B, &g.leaf, &lstride));
  g.leaf_stride = lstride;
  hipLaunchKernelGGL(r1cs_constraint_kernel<true>, dim3(blocks_for(prec), B), dim3(256), 0, s, st.ca, g);
  STARK_HIP(ctx, hipGetLastError());
  STARK_TRY(forest_build(ctx, f_m, (const uint8_t*)bb.rows, prec, 256, B, s, true, nullptr, nullptr, nullptr,
                         prec * sizeof(fe)));
  // 7. k per proof, L hashed into level 0 of the L forest, whose root launch writes FRI layer 0's special_x.
  hipLaunchKernelGGL(r1cs_k_batch_kernel, dim3(B), dim3(kKThreads), 0, s, forest_roots(f_m), mc.r2, mc.one,
                     xs_powers(st.roots.g2, steps), pow32(), bb.d_tr);
  STARK_HIP(ctx, hipGetLastError());
  LincombArgs la;
  la.rows = bb.rows;
  la.plane = prec;
  la.out = bb.lvals;
  la.prec = prec;
  la.g_add = 0;
  la.log_g = 0;
  la.tr = bb.d_tr;
  STARK_TRY(forest_level0(ctx, f_l, prec, B, &la.leaf, &lstride));
  hipLaunchKernelGGL(r1cs_lincomb_batch_kernel, dim3(blocks_for(prec), B), dim3(256), 0, s, la, (uint64_t)lstride);
  STARK_HIP(ctx, hipGetLastError());
  fe* sx0 = nullptr;
  STARK_TRY(fri_batch_sx0(ctx, prec, B, st.roots.g2c, prec / 4, (uint32_t)skips, &sx0));
  bool sx_made = false;
  STARK_TRY(forest_build(ctx, f_l, (const uint8_t*)bb.lvals, prec, 32, B, s, true, sx0, &mc.r2, &sx_made));
  if (!sx_made) {
    ctx->last_error = "prove_r1cs_batch: the L forest did not make its roots' field elements";
    return STARK_ERR_STATE;
  }
  hipLaunchKernelGGL(r1cs_l_root_batch_kernel, dim3(B), dim3(64), 0, s, forest_roots(f_l), bb.d_tr);
  STARK_HIP(ctx, hipGetLastError());
  // 9. Every proof's transcript head in one copy; an event marks them.
  STARK_HIP(ctx, hipMemcpy2DAsync(pin, kBatchHeadBytes, bb.d_tr, sizeof(Transcript), kTrHead, B,
                                  hipMemcpyDeviceToHost, s));
  STARK_HIP(ctx, hipEventRecord(ctx->ev_aux, s));
  clk.mark("prover kernels enqueued");
  // While the FRI layers run: the positions of every proof (prove.rs:337-362) and all their openings as one
  // gather batch on the second stream.
  std::vector<std::unique_ptr<stark_r1cs_proof>> proofs(B);
  std::vector<int> errs(B, 0);
  std::vector<std::vector<size_t>> positions(B), aug(B);
  auto spot_checks = [&]() -> stark_status {
    STARK_HIP(ctx, hipEventSynchronize(ctx->ev_aux));
    clk.mark("wait for the L roots");
    std::vector<GatherReq> spot;
    spot.reserve(2 * (size_t)B);
    for (uint32_t b = 0; b < B; ++b) {
      const Transcript* h_tr = reinterpret_cast<const Transcript*>(h_heads + (size_t)b * kBatchHeadBytes);
      proofs[b] = std::make_unique<stark_r1cs_proof>();
      stark_r1cs_proof& p = *proofs[b];
      errs[b] = h_tr->err;
      memcpy(p.a_root, h_tr->roots[0], 32);
      memcpy(p.m_root, h_tr->roots[1], 32);
      memcpy(p.l_root, h_tr->roots[2], 32);
      uint32_t pos32[kSpotChecks];
      STARK_TRY(stark_get_pseudorandom_indices(p.l_root, 32, (uint32_t)prec, kSpotChecks, (uint32_t)skips, pos32));
      positions[b].resize(kSpotChecks);
      aug[b].resize(4 * kSpotChecks);
      for (int i = 0; i < kSpotChecks; ++i) {
        positions[b][i] = pos32[i];
        spot_rows(pos32[i], os, skips, prec, &aug[b][4 * i]);
      }
      p.depth = log_prec;
      p.l_leaves.resize(32 * kSpotChecks);
      p.l_nodes.resize((size_t)32 * kSpotChecks * log_prec);
      p.m_leaves.resize(256 * 4 * kSpotChecks);
      p.m_nodes.resize((size_t)32 * 4 * kSpotChecks * log_prec);
      spot.push_back({forest_tree(f_l, b), positions[b].data(), (size_t)kSpotChecks, p.l_leaves.data(),
                      p.l_nodes.data()});
      spot.push_back({forest_tree(f_m, b), aug[b].data(), (size_t)4 * kSpotChecks, p.m_leaves.data(),
                      p.m_nodes.data()});
    }
    STARK_TRY(merkle_gather_batch(ctx, spot, ctx->aux));
    clk.mark("spot-check openings");
    return STARK_OK;
  };
  // 8. prove_low_degree of the B linear combinations on the L forest (prove.rs:367).
  std::vector<stark_fri_proof*> fri(B, nullptr);
  STARK_TRY(fri_prove_batch_device(ctx, (const fe*)bb.lvals, prec, B, st.roots.g2c, prec / 4, (uint32_t)skips,
                                   fri.data(), f_l, spot_checks));
  clk.mark("FRI wait + indices + gather (last download)");
  // A witness that failed the constraint kernel's flags ran to the end of the chain and is dropped here.
  for (uint32_t b = 0; b < B; ++b) {
    stark_r1cs_proof& p = *proofs[b];
    p.fri = fri[b];  // owned by the proof from here on
    if (errs[b]) {
      statuses[b] = transcript_status(ctx, errs[b]);
      out[b] = nullptr;
      continue;
    }
    JsonPieces j;
    stark_proof_json_head(p.m_root, p.l_root, p.a_root, {p.m_leaves, 256, p.m_nodes, (size_t)4 * kSpotChecks, log_prec},
                          {p.l_leaves, 32, p.l_nodes, (size_t)kSpotChecks, log_prec}, j);
    fri_proof_json_pieces(p.fri, j);
    j.text("}");
    j.render(p.json);
    statuses[b] = STARK_OK;
    out[b] = proofs[b].release();
  }
  clk.mark("proof JSON");
  return STARK_OK;
}

stark_status mk_r1cs_proof_batch(stark_ctx* ctx, const PreparedCircuit& c, const BatchWitness* const* w,
                                 uint32_t batch, stark_r1cs_proof** out, stark_status* statuses) {
  if (!ctx || !w || !out || !statuses || !c.lde.ptr || c.world != 1) return STARK_ERR_BAD_ARG;
  for (uint32_t b = 0; b < batch; ++b) out[b] = nullptr;
  if (batch == 0) return STARK_OK;
  // The chunk: as many proofs as stay under the limit by the size of one proof's working set (at least one).
  const TraceView v = batch_view(c, *w[0]);
  StageDims d;
  STARK_TRY(stage_dims(v, 1, 0, d));
  const size_t one = batch_bytes(c, d, v.n_pfi, public_columns(ctx, v.n_pfi, d.steps), 1);
  const size_t limit = ctx->prove_batch_limit ? ctx->prove_batch_limit : kDefaultProveBatchLimit;
  const uint32_t chunk = (uint32_t)std::min<size_t>(batch, std::max<size_t>(1, limit / one));
  stark_status st = STARK_OK;
  for (uint32_t b0 = 0; b0 < batch && st == STARK_OK; b0 += chunk) {
    st = prove_r1cs_batch(ctx, c, w + b0, std::min(chunk, batch - b0), out + b0, statuses + b0);
    // the chunk's buffers, pinned regions and the witnesses' staging are free for the next one
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && st == STARK_OK) st = STARK_ERR_HIP;
    if (ctx->aux && hipStreamSynchronize(ctx->aux) != hipSuccess && st == STARK_OK) st = STARK_ERR_HIP;
  }
  if (st != STARK_OK)
    for (uint32_t b = 0; b < batch; ++b) {
      stark_r1cs_proof_free(out[b]);
      out[b] = nullptr;
    }
  return st;
}

// v[i] <- Montgomery image of v[i] (canonical in).
__global__ void to_mont_kernel(fe* __restrict__ v, uint64_t n, fe r2) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) fe_store(v + i, fe_mul(fe_load(v + i), r2));
}

// IDX / PIDX step columns only (the circuit's part of r1cs_index_kernel).
__global__ void r1cs_idx_kernel(const uint64_t* __restrict__ perm, uint64_t os, uint64_t steps, fe* __restrict__ idx,
                                fe* __restrict__ pidx) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= steps) return;
  fe_store(idx + i, fe_from_u64(i));
  fe_store(pidx + i, fe_from_u64(i < os ? perm[i] : i));
}

// The LDE columns of a circuit that no witness changes: K, F0, F1, F2, IDX, PIDX
// (prove.rs:100-124, 160-167), 6 x precision into `out`.  coef / flag bytes / perm
// are the device trace builder's circuit columns (os slots).
stark_status circuit_lde(stark_ctx* ctx, const fe* coef, const uint8_t* flag_bytes, const uint64_t* perm, size_t os,
                         const size_t* public_first_indices, size_t n_pfi, uint32_t world, uint32_t rank, DevBuf& out,
                         hipStream_t s, bool with_zb, const fe** colp, uint32_t* spot_log_t) {
  const FieldHost& F = FieldHost::get();
  // with_zb = false (the verifier's cold build, which needs six values per spot position): the columns
  // stay where they are made -- K's extension in slot 1, F0's and IDX's in their shared entries -- with
  // no slot copies and no Montgomery images (colp tells the caller where each one is).  With spot_log_t
  // no extension is made at all: out holds the six columns' first forward passes (circuit_spot_values).
  const bool verify_only = !with_zb;
  if (spot_log_t && (with_zb || world != 1)) return STARK_ERR_BAD_ARG;
  const fe* col[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  if (world == 0 || world > (uint32_t)kExtensionFactor || (world & (world - 1)) || rank >= world)
    return STARK_ERR_BAD_ARG;
  uint32_t log_g = 0;
  while ((1u << log_g) < world) ++log_g;
  if (os < 5 || os % 3 != 0) return STARK_ERR_BAD_LENGTH;
  const uint32_t log_steps = log2_ceil_ref(os - 1);
  const uint32_t log_prec = log_steps + kLogExtensionFactor;
  if (log_prec >= 24) return STARK_ERR_BAD_LENGTH;
  const uint64_t steps = (uint64_t)1 << log_steps, prec = (uint64_t)1 << log_prec;
  const uint64_t P = prec >> log_g;  // this rank's points r + world j
  ProofRoots roots;
  STARK_TRY(proof_roots(ctx, log_steps, log_prec, world, roots));
  const HostFp g2 = roots.g2;
  const Twiddles *tw2 = roots.tw2, *tw1i = roots.tw1i, *twh = roots.twh;
  for (size_t i = 0; i < n_pfi; ++i)
    if (public_first_indices[2 * i + 1] >= steps) return STARK_ERR_BAD_ARG;
  // The column route: Zb2 from its coefficients (public_zb2_coefficients), as the proofs take I2.
  const bool zb2_col = with_zb && public_columns(ctx, n_pfi, steps);
  DevBuf& tmp = ctx->lde_tmp;  // 6 step columns, then Zb2 / Zb3, the x_k (2 P + n_pfi) and Zb2's coefficients
  STARK_TRY(ensure_buf(ctx, tmp, (6 * steps + 2 * P + n_pfi + 1 + (zb2_col ? steps : 0)) * sizeof(fe)));
  stark_status st = ensure_buf(ctx, out, (with_zb ? 8 : 6) * P * sizeof(fe));
  if (st == STARK_OK) {
    fe* raw = (fe*)tmp.ptr;
    hipMemsetAsync(raw, 0, 6 * steps * sizeof(fe), s);
    hipMemcpyAsync(raw, coef, os * sizeof(fe), hipMemcpyDeviceToDevice, s);
    hipLaunchKernelGGL(r1cs_flags_kernel, dim3(blocks_for(3 * os)), dim3(256), 0, s, flag_bytes, (uint64_t)os, steps,
                       raw + steps);
    hipLaunchKernelGGL(r1cs_idx_kernel, dim3(blocks_for(steps)), dim3(256), 0, s, perm, (uint64_t)os, steps,
                       raw + 4 * steps, raw + 5 * steps);
    if (spot_log_t) {
      // The step columns' coefficients (inv_best_fft, one batch), then only the first pass of their
      // forward transforms over the precision domain, transposed (ntt_first_pass_tmajor).  F0's and
      // IDX's depend on the size alone: from the context's cache when it holds them (K moved over F0's
      // step column and PIDX over IDX's, K F1 F2 PIDX are then one batch of four), else in the batch.
      fe* const o = (fe*)out.ptr;
      const fe *yf0 = nullptr, *yidx = nullptr;
      st = ext_const_column(ctx, kSpotF0, os, log_steps, log_prec, 0, 0, *tw1i, *tw2, *twh, s, &yf0);
      if (st == STARK_OK) st = ext_const_column(ctx, kSpotIdx, 0, log_steps, log_prec, 0, 0, *tw1i, *tw2, *twh, s, &yidx);
      auto live = [&](uint32_t kind, uint64_t tag) {  // (a later reservation may evict an earlier column)
        return ctx->ext_idx.count(std::make_tuple(kind, log_steps, log_prec, 0u, 0u, tag)) != 0;
      };
      if (yf0 && !live(kSpotF0, os)) yf0 = nullptr;
      if (yidx && !live(kSpotIdx, 0)) yidx = nullptr;
      const bool shared = yf0 && yidx;
      if (st == STARK_OK && shared &&
          (hipMemcpyAsync(raw + steps, raw, steps * sizeof(fe), hipMemcpyDeviceToDevice, s) != hipSuccess ||
           hipMemcpyAsync(raw + 4 * steps, raw + 5 * steps, steps * sizeof(fe), hipMemcpyDeviceToDevice, s) !=
               hipSuccess))
        st = STARK_ERR_HIP;
      fe* const first = shared ? raw + steps : raw;
      const uint32_t batch = shared ? 4 : 6;
      if (st == STARK_OK) st = ntt_device(ctx, first, log_steps, batch, *tw1i, true, s);
      if (st == STARK_OK)
        st = ntt_first_pass_tmajor(ctx, first, log_prec - log_steps, o, log_prec, batch, *tw2, s, spot_log_t);
      if (shared) {
        const fe* c6[6] = {o, yf0, o + P, o + 2 * P, yidx, o + 3 * P};
        for (int k = 0; k < 6; ++k) col[k] = c6[k];
      } else {
        for (int k = 0; k < 6; ++k) col[k] = o + (uint64_t)k * P;
      }
      if (hipStreamSynchronize(s) != hipSuccess && st == STARK_OK) st = STARK_ERR_HIP;
      if (colp)
        for (int k = 0; k < 6; ++k) colp[k] = col[k];
      return st;
    }
    // K F0 F1 F2, then PIDX; IDX and F0 (1 on the os rows: the flags are circuit_build's calc_flags)
    // are the shared extensions (ext_const_column), copied into their slots.  With F0's: K is moved
    // over F0's step column, K F1 F2 are extended into slots 1-3, and K then copied to slot 0.
    const fe *idx_ext = nullptr, *f0_ext = nullptr;
    st = ext_const_column(ctx, kExtF0, os, log_steps, log_prec, log_g, rank, *tw1i, *tw2, *twh, s, &f0_ext);
    if (st == STARK_OK)
      st = ext_index_column(ctx, log_steps, log_prec, log_g, rank, *tw1i, *tw2, *twh, s, &idx_ext);
    if (f0_ext && !ctx->ext_idx.count(std::make_tuple(kExtF0, log_steps, log_prec, log_g, rank, (uint64_t)os)))
      f0_ext = nullptr;  // evicted by IDX's reservation
    fe* const o = (fe*)out.ptr;
    if (st == STARK_OK && f0_ext) {
      if (hipMemcpyAsync(raw + steps, raw, steps * sizeof(fe), hipMemcpyDeviceToDevice, s) != hipSuccess)
        st = STARK_ERR_HIP;
      if (st == STARK_OK)
        st = coset_lde(ctx, raw + steps, 3, o + P, log_steps, log_prec, log_g, rank, *tw1i, *tw2, *twh, s);
      if (st == STARK_OK && !verify_only &&
          (hipMemcpyAsync(o, o + P, P * sizeof(fe), hipMemcpyDeviceToDevice, s) != hipSuccess ||
           hipMemcpyAsync(o + P, f0_ext, P * sizeof(fe), hipMemcpyDeviceToDevice, s) != hipSuccess))
        st = STARK_ERR_HIP;
      col[0] = verify_only ? o + P : o;
      col[1] = verify_only ? f0_ext : o + P;
    } else if (st == STARK_OK) {
      st = coset_lde(ctx, raw, 4, o, log_steps, log_prec, log_g, rank, *tw1i, *tw2, *twh, s);
      col[0] = o;
      col[1] = o + P;
    }
    col[2] = o + 2 * P;
    col[3] = o + 3 * P;
    col[4] = verify_only ? idx_ext : o + 4 * P;
    col[5] = o + 5 * P;
    if (st == STARK_OK)
      st = coset_lde(ctx, raw + 5 * steps, 1, (fe*)out.ptr + 5 * P, log_steps, log_prec, log_g, rank, *tw1i, *tw2,
                     *twh, s);
    if (st == STARK_OK && !verify_only &&
        hipMemcpyAsync((fe*)out.ptr + 4 * P, idx_ext, P * sizeof(fe), hipMemcpyDeviceToDevice, s) != hipSuccess)
      st = STARK_ERR_HIP;
    // Zb2 = prod_k (x - x_k), Zb3 = x - x_last (utils.rs:438-474) and their inverses (0 -> 0).
    const uint64_t skips = prec / steps;
    std::vector<fe> xk(n_pfi + 1);
    std::vector<uint64_t> staging;  // (alive until the synchronisation below)
    for (size_t i = 0; !zb2_col && i < n_pfi; ++i)
      xk[i] = to_dev(F.pow_u64(g2, skips * public_first_indices[2 * i + 1]));
    fe* zb = raw + 6 * steps;
    fe* d_xk = zb + 2 * P;
    const Mont mc = mont();
    if (st == STARK_OK && with_zb && !zb2_col && n_pfi &&
        hipMemcpyAsync(d_xk, xk.data(), n_pfi * sizeof(fe), hipMemcpyHostToDevice, s) != hipSuccess)
      st = STARK_ERR_HIP;
    if (st == STARK_OK && zb2_col) {
      fe* zc = d_xk + n_pfi + 1;
      st = public_zb2_coefficients(ctx, g2, skips, log_steps, public_first_indices, n_pfi, zc, staging, s);
      if (st == STARK_OK) st = coset_forward(ctx, zc, 1, zb, log_steps, log_prec, log_g, rank, *tw2, *twh, s);
    }
    if (st == STARK_OK && with_zb) {
      hipLaunchKernelGGL(r1cs_zb_kernel, dim3(blocks_for(P)), dim3(256), 0, s, tw2->d_lo, tw2->d_hi, tw2->kb, P,
                         (uint64_t)rank, log_g, (const fe*)d_xk, (uint32_t)n_pfi,
                         to_dev(F.pow_u64(g2, prec - skips)), mc.rinv, mc.one, zb2_col ? nullptr : zb, zb + P);
      st = multi_inv_device(ctx, zb, (fe*)out.ptr + 6 * P, 2 * P, s);
    }
    if (st == STARK_OK && !verify_only) {  // K, F0-F2 as Montgomery images (ConstraintArgs::mont_cols; the Zb inverses are)
      hipLaunchKernelGGL(to_mont_kernel, dim3(blocks_for(4 * P)), dim3(256), 0, s, o, 4 * P, mc.r2);
      if (hipGetLastError() != hipSuccess) st = STARK_ERR_HIP;
    }
    if (st == STARK_OK && hipStreamSynchronize(s) != hipSuccess) st = STARK_ERR_HIP;
  }
  hipStreamSynchronize(s);  // tmp (a context buffer) is free for the next call
  if (colp)
    for (int k = 0; k < 6; ++k) colp[k] = col[k];
  return st;
}

// ---- the verifier's spot values (circuit_lde's spot mode) -------------------------------------------
//
// Y = the six step columns' first forward passes, T-major (column k at c.col[k], Y[t A + j], T = 2^log_t,
// A = P / T): column k at x = g2^e is sum_{j < A} x^j Y_k[(e mod T) A + j] (ntt_first_pass_tmajor), a
// contiguous run of A values per column and position instead of the two further passes of its extension.
// Workgroup (b, i) takes position i's j = g + S l (g = 256 b + thread < S, l < A / S): Horner over l with
// the constant x^S (its digit-basis table, spot_setup_kernel), then one product by x^g (the two-level
// table of g2), summed over the workgroup; spot_sum_kernel adds position i's workgroups.
constexpr uint32_t kSpotMax = 128;
struct SpotPos {
  uint64_t e[kSpotMax];
};

__global__ void spot_setup_kernel(SpotPos pos, uint32_t n, uint32_t log_s, uint64_t P, const fe* __restrict__ lo,
                                  const fe* __restrict__ hi, uint32_t kb, Pow32 p32, uint32_t* __restrict__ tabs) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, i = t >> 3, r = t & 7;  // row r of position i's table
  if (i >= n) return;
  fe unit = fe_zero();
  unit.w[0] = 1;
  const fe xs = fe_mul(pow_tab(lo, hi, kb, (pos.e[i] << log_s) & (P - 1)), unit);  // x^S, canonical
  db_limbs(fe_mul(xs, p32.m[r]), tabs + 72 * i + 9 * r);
}

struct SpotCols {
  const fe* c[6];
};

__global__ __launch_bounds__(256) void spot_eval_kernel(SpotCols y, uint64_t P, uint32_t log_t,
                                                        uint32_t log_s, SpotPos pos, const uint32_t* __restrict__ tabs,
                                                        const fe* __restrict__ lo, const fe* __restrict__ hi,
                                                        uint32_t kb, fe* __restrict__ partial) {
  __shared__ fe red[256];
  const uint32_t i = blockIdx.y;
  const uint64_t e = pos.e[i];
  const uint64_t T = (uint64_t)1 << log_t, A = P >> log_t, S = (uint64_t)1 << log_s, nl = A >> log_s;
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool on = g < S;
  const uint32_t* W = tabs + 72 * i;  // (uniform: scalar loads)
  const fe xg = on ? pow_tab(lo, hi, kb, (e * g) & (P - 1)) : fe_zero();  // Montgomery image of x^g
  const uint64_t off = (e & (T - 1)) * A + g;
  fe sum[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    fe acc = fe_zero();
    if (on) {
      const fe* c = y.c[k] + off;
      acc = fe_load(c + (nl - 1) * S);
#pragma unroll 4
      for (uint64_t l = nl - 1; l-- > 0;) {
        const fe v = fe_load(c + l * S);
        acc = fe_add_raw(fe_mul_db(acc, W), v);  // [0, 2p) + [0, p): below 3p, a digit-basis input
      }
      acc = fe_mul(acc, xg);  // canonical
    }
    sum[k] = acc;
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    red[threadIdx.x] = sum[k];
    __syncthreads();
    for (uint32_t w = blockDim.x / 2; w > 0; w >>= 1) {
      if (threadIdx.x < w) red[threadIdx.x] = fe_add(red[threadIdx.x], red[threadIdx.x + w]);
      __syncthreads();
    }
    if (threadIdx.x == 0) fe_store(partial + ((uint64_t)i * gridDim.x + blockIdx.x) * 6 + k, red[0]);
    __syncthreads();
  }
}

__global__ void spot_sum_kernel(const fe* __restrict__ partial, uint32_t bp, uint32_t n, fe* __restrict__ out) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;  // position q / 6, column q % 6
  if (q >= 6 * n) return;
  const uint32_t i = q / 6, k = q % 6;
  fe s = fe_zero();
  for (uint32_t b = 0; b < bp; ++b) s = fe_add(s, fe_load(partial + ((uint64_t)i * bp + b) * 6 + k));
  fe_store(out + (uint64_t)k * n + i, s);
}

stark_status circuit_spot_values(stark_ctx* ctx, const PreparedCircuit& c, const size_t* positions, size_t n,
                                 uint8_t* out, hipStream_t s) {
  if (!c.spot || !c.col[0] || n == 0 || n > kSpotMax || !positions || !out) return STARK_ERR_BAD_ARG;
  STARK_HIP(ctx, hipSetDevice(ctx->device));  // (the verifier calls this from its side thread)
  const FieldHost& F = FieldHost::get();
  const uint32_t log_steps = log2_ceil_ref(c.os - 1), log_prec = log_steps + kLogExtensionFactor;
  const uint64_t P = (uint64_t)1 << log_prec;
  if (c.spot_log_t == 0 || c.spot_log_t > log_prec) return STARK_ERR_BAD_ARG;
  ProofRoots roots;
  STARK_TRY(proof_roots(ctx, log_steps, log_prec, 1, roots));
  const Twiddles& tw = *roots.tw2;
  // j's per thread: 16 where the positions' threads fill the chip (A = 2^16 at 2^20 steps: 80 x 16
  // workgroups), 4 below (a few hundred workgroups, each short)
  const uint32_t log_a = log_prec - c.spot_log_t;
  const uint32_t log_nl = std::min<uint32_t>(log_a, log_a >= 16 ? 4 : log_a >= 14 ? log_a - 12 : 2);
  const uint32_t log_s = log_a - log_nl;
  const uint32_t bp = log_s > 8 ? 1u << (log_s - 8) : 1u;
  SpotPos sp;
  for (size_t i = 0; i < n; ++i) {
    if (positions[i] >= P) return STARK_ERR_BAD_ARG;
    sp.e[i] = positions[i];
  }
  const size_t tab_bytes = (n * 72 * 4 + 255) & ~(size_t)255, part_bytes = n * bp * 6 * sizeof(fe);
  STARK_TRY(ensure_buf(ctx, ctx->spot, tab_bytes + part_bytes + 6 * n * sizeof(fe)));
  uint8_t* d = (uint8_t*)ctx->spot.ptr;
  uint32_t* tabs = (uint32_t*)d;
  fe* partial = (fe*)(d + tab_bytes);
  fe* vals = (fe*)(d + tab_bytes + part_bytes);
  uint8_t* host = nullptr;
  STARK_TRY(ctx_pinned(ctx, 0, 6 * n * sizeof(fe), (void**)&host));
  hipLaunchKernelGGL(spot_setup_kernel, dim3((unsigned)((8 * n + 255) / 256)), dim3(256), 0, s, sp, (uint32_t)n, log_s,
                     P, tw.d_lo, tw.d_hi, tw.kb, pow32(), tabs);
  SpotCols cols;
  for (int k = 0; k < 6; ++k) {
    if (!c.col[k]) return STARK_ERR_BAD_ARG;
    cols.c[k] = c.col[k];
  }
  hipLaunchKernelGGL(spot_eval_kernel, dim3(bp, (unsigned)n), dim3(256), 0, s, cols, P, c.spot_log_t,
                     log_s, sp, (const uint32_t*)tabs, tw.d_lo, tw.d_hi, tw.kb, partial);
  hipLaunchKernelGGL(spot_sum_kernel, dim3((unsigned)((6 * n + 255) / 256)), dim3(256), 0, s, (const fe*)partial, bp,
                     (uint32_t)n, vals);
  STARK_HIP(ctx, hipGetLastError());
  STARK_HIP(ctx, hipMemcpyAsync(host, vals, 6 * n * sizeof(fe), hipMemcpyDeviceToHost, s));
  STARK_HIP(ctx, hipStreamSynchronize(s));
  memcpy(out, host, 6 * n * sizeof(fe));
  return STARK_OK;
}

stark_status mk_r1cs_proof_view(stark_ctx* ctx, const TraceView& v, const fe* pre, stark_r1cs_proof** out) {
  if (!ctx || !out) return STARK_ERR_BAD_ARG;
  *out = nullptr;
  STARK_HIP(ctx, hipSetDevice(ctx->device));
  const stark_status st = prove_r1cs(ctx, v, pre, out);
  hipStreamSynchronize(ctx->stream);
  return st;
}

// ---- distributed prover (one rank of `world` GPUs) -------------------------
//
// The precision domain is split by residue class: rank r owns the evaluation
// points i = r + G j (j < P = precision / G), G | 8.  Then
//  * the LDE of every column is a coset evaluation with no exchange: the
//    polynomial has degree < steps <= P, so f(g2^(r + G j)) =
//    sum_k (c_k g2^(r k)) (g2^G)^(j k) is a P-point NTT of the scaled
//    coefficients;
//  * every shifted read of the constraints (-skips, +k skips, +2k skips) is a
//    multiple of 8, hence of G, and stays inside the residue class;
//  * the FRI fold's four points i + t n/4 are in the same class while
//    n/4 >= G, so each layer's column is again residue-class distributed.
// Only the Merkle trees need other ranks' data; the caller exchanges leaf
// digests (stark_amd/dprove.py).  The small step-domain work (accumulator
// tree, transcript r, A's running products) is repeated on every rank.
struct DProveState {
  stark_ctx* ctx = nullptr;
  hipStream_t s = nullptr;
  StageDims dim;
  uint64_t g2c[4];
  DevBuf arena;
  stark_merkle_tree* acc_tree = nullptr;
  fe *rows = nullptr, *lvals = nullptr;
  Transcript* d_tr = nullptr;
  XsPowers xs;
};

}  // namespace stark

struct stark_dprove {
  stark::DProveState st;
  ~stark_dprove() {
    if (st.acc_tree) stark_merkle_free(st.acc_tree);
    if (st.arena.ptr) hipFree(st.arena.ptr);
  }
};

namespace stark {

// pre != nullptr: this rank's prepared circuit columns (circuit_lde with world, rank): the coset LDEs of
// K F0 F1 F2 IDX PIDX and the Zb inverses; only S, P and A are extended here.
static stark_status dprove_begin(stark_ctx* ctx, uint32_t world, uint32_t rank, const TraceView& v, const fe* pre,
                                 hipStream_t s, stark_dprove* h) {
  DProveState& d = h->st;
  Stage st;
  STARK_TRY(stage_begin(ctx, v, pre, world, rank, s, st));
  d.ctx = ctx;
  d.s = s;
  d.dim = st.d;
  memcpy(d.g2c, st.roots.g2c, 32);
  d.xs = xs_powers(st.roots.g2, st.d.steps);
  // The handle owns its arena (zb is sized for the 3 os flag bytes too) and its accumulator tree.
  STARK_TRY(stage_buffers(ctx, v, st, std::max<uint64_t>(2 * st.d.P, 3 * st.d.os / 32 + 1), d.arena));
  d.rows = st.rows;
  d.lvals = st.lvals;
  d.d_tr = st.d_tr;
  STARK_HIP(ctx, hipMemcpyAsync(st.consts, st.consts_h.data(), st.consts_h.size() * sizeof(fe), hipMemcpyHostToDevice,
                                s));
  if (st.pub_cols) STARK_TRY(public_coefficients(ctx, v, st, !pre && !st.ca.tinv, s));
  STARK_TRY(stage_uploads(ctx, v, pre, st, s));
  STARK_TRY(stark_merkle_new(ctx, &d.acc_tree));
  STARK_TRY(stage_accumulator(ctx, st, d.acc_tree, nullptr, s));  // on every rank
  // The step-domain A chain is repeated on every rank, on the context's aux stream beside the coset LDE.
  STARK_TRY(aux_stream(ctx));
  const hipStream_t sa = ctx->aux;
  STARK_TRY(a_chain_enqueue(ctx, st, d.acc_tree, s, sa));
  STARK_TRY(a_denominators_up(ctx, st, sa, ctx->io2));
  STARK_TRY(extend_trace(ctx, st, pre, s));
  STARK_TRY(a_chain_finish(ctx, st, s, sa));
  if (!pre && !st.ca.tinv) {  // Zb2 / Zb3 at this rank's points and their inverses
    uint64_t n_zb = 0;
    STARK_TRY(zb_enqueue(ctx, st, v.n_pfi, s, &n_zb));
    STARK_TRY(multi_inv_device(ctx, st.zb, st.inv_zb, n_zb, s));
  }
  STARK_TRY(constraint_args(ctx, v, pre, st, 0, s));  // plane = 0: the rank exports its rows (stark_dprove_rows)
  STARK_TRY(constraint_launch(ctx, st, s));
  // consts_h and the uploads above must outlive the copies: wait here (the caller
  // reads a_root and the constraint flags next anyway).
  STARK_HIP(ctx, hipStreamSynchronize(s));
  return STARK_OK;
}

}  // namespace stark

using namespace stark;

extern "C" {

// The host-array entry points' check (the flags as field elements): an array is null while its length is not 0.
static bool host_trace_null(const TraceView& v) {
  if (v.os && (!v.col[0] || !v.col[1] || !v.col[2] || !v.col[3] || !v.col[4] || !v.col[5] || !v.perm)) return true;
  return (v.n_public && !v.public_wires) || (v.n_pfi && !v.pfi);
}

stark_status stark_mk_r1cs_proof(stark_ctx* ctx, const uint64_t* witness_trace, const uint64_t* computational_trace,
                                 size_t original_steps, const uint64_t* public_wires, size_t n_public,
                                 const size_t* public_first_indices, size_t n_public_first,
                                 const size_t* permuted_indices, const uint64_t* coefficients, const uint64_t* flag0,
                                 const uint64_t* flag1, const uint64_t* flag2, size_t n_constraints, size_t n_wires,
                                 stark_r1cs_proof** out) {
  if (!ctx || !out) return STARK_ERR_BAD_ARG;
  *out = nullptr;
  const TraceView v{{coefficients, flag0, flag1, flag2, witness_trace, computational_trace}, nullptr,
                    permuted_indices, original_steps, public_wires, n_public, public_first_indices, n_public_first,
                    n_constraints, n_wires, false};
  if (host_trace_null(v)) return STARK_ERR_BAD_ARG;
  return mk_r1cs_proof_view(ctx, v, nullptr, out);
}

stark_status stark_r1cs_proof_json(const stark_r1cs_proof* proof, char* buf, size_t cap, size_t* len) {
  if (!proof || !len) return STARK_ERR_BAD_ARG;
  const JsonText& text = r1cs_proof_text(proof);
  *len = text.size();
  if (buf && cap) {
    const size_t k = text.size() < cap ? text.size() : cap;
    host_memcpy(buf, text.data(), k);
    if (k < cap) buf[k] = 0;
  }
  return STARK_OK;
}

stark_status stark_r1cs_proof_json_view(const stark_r1cs_proof* proof, const char** data, size_t* len) {
  if (!proof || !data || !len) return STARK_ERR_BAD_ARG;
  const JsonText& text = r1cs_proof_text(proof);
  *data = text.data();
  *len = text.size();
  return STARK_OK;
}

stark_status stark_r1cs_proof_roots(const stark_r1cs_proof* proof, uint8_t m_root[32], uint8_t l_root[32],
                                    uint8_t a_root[32]) {
  if (!proof) return STARK_ERR_BAD_ARG;
  if (m_root) memcpy(m_root, proof->m_root, 32);
  if (l_root) memcpy(l_root, proof->l_root, 32);
  if (a_root) memcpy(a_root, proof->a_root, 32);
  return STARK_OK;
}

stark_status stark_r1cs_proof_branches(const stark_r1cs_proof* proof, int which, size_t* k, size_t* leaf_len,
                                       size_t* depth, uint8_t* leaves, size_t leaves_cap, uint8_t* nodes,
                                       size_t nodes_cap) {
  if (!proof || (which != 0 && which != 1)) return STARK_ERR_BAD_ARG;
  const size_t ll = which == 0 ? proof->m_leaf_len : proof->l_leaf_len;
  const std::vector<uint8_t>& lv = which == 0 ? proof->m_leaves : proof->l_leaves;
  const std::vector<uint8_t>& nd = which == 0 ? proof->m_nodes : proof->l_nodes;
  if (k) *k = lv.size() / ll;
  if (leaf_len) *leaf_len = ll;
  if (depth) *depth = proof->depth_of(which);
  // capacities checked before either buffer is written
  if ((leaves && leaves_cap < lv.size()) || (nodes && nodes_cap < nd.size())) return STARK_ERR_BAD_LENGTH;
  if (leaves) memcpy(leaves, lv.data(), lv.size());
  if (nodes) memcpy(nodes, nd.data(), nd.size());
  return STARK_OK;
}

const stark_fri_proof* stark_r1cs_proof_fri(const stark_r1cs_proof* proof) { return proof ? proof->fri : nullptr; }

void stark_r1cs_proof_free(stark_r1cs_proof* proof) { delete proof; }

stark_status stark_dprove_begin(stark_ctx* ctx, uint32_t world, uint32_t rank, const uint64_t* witness_trace,
                                const uint64_t* computational_trace, size_t original_steps,
                                const uint64_t* public_wires, size_t n_public, const size_t* public_first_indices,
                                size_t n_public_first, const size_t* permuted_indices, const uint64_t* coefficients,
                                const uint64_t* flag0, const uint64_t* flag1, const uint64_t* flag2,
                                size_t n_constraints, size_t n_wires, void* stream, stark_dprove** out) {
  if (!ctx || !out) return STARK_ERR_BAD_ARG;
  *out = nullptr;
  const TraceView v{{coefficients, flag0, flag1, flag2, witness_trace, computational_trace}, nullptr,
                    permuted_indices, original_steps, public_wires, n_public, public_first_indices, n_public_first,
                    n_constraints, n_wires, false};
  if (host_trace_null(v)) return STARK_ERR_BAD_ARG;
  return dprove_open(ctx, world, rank, v, nullptr, stream, out);
}

stark_status stark_dprove_begin_bytes(stark_ctx* ctx, uint32_t world, uint32_t rank, const uint8_t* r1cs,
                                      size_t r1cs_len, const uint8_t* wtns, size_t wtns_len, void* stream,
                                      stark_dprove** out) {
  if (!ctx || !r1cs || !wtns || !out) return STARK_ERR_BAD_ARG;
  *out = nullptr;
  STARK_HIP(ctx, hipSetDevice(ctx->device));
  DevTrace dt;
  stark_status st = r1cs_trace_device(ctx, r1cs, r1cs_len, wtns, wtns_len, &dt);
  if (st != STARK_OK) return st;
  STARK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the trace builder runs on the context stream
  return dprove_open(ctx, world, rank, dt.view(false), nullptr, stream, out);
}

}  // extern "C"

stark_status stark::dprove_open(stark_ctx* ctx, uint32_t world, uint32_t rank, const TraceView& v, const fe* pre,
                                void* stream, stark_dprove** out) {
  if (!ctx || !out) return STARK_ERR_BAD_ARG;
  *out = nullptr;
  STARK_HIP(ctx, hipSetDevice(ctx->device));
  auto h = std::make_unique<stark_dprove>();
  hipStream_t s = pick_stream(ctx, stream);
  const stark_status st = dprove_begin(ctx, world, rank, v, pre, s, h.get());
  if (st != STARK_OK) {
    hipStreamSynchronize(s);
    return st;
  }
  *out = h.release();
  return STARK_OK;
}

extern "C" {

stark_status stark_dprove_info(stark_dprove* h, size_t* precision, size_t* n_local, size_t* original_steps,
                               uint64_t g2[4], uint8_t a_root[32]) {
  if (!h) return STARK_ERR_BAD_ARG;
  DProveState& d = h->st;
  if (precision) *precision = d.dim.prec;
  if (n_local) *n_local = d.dim.P;
  if (original_steps) *original_steps = d.dim.os;
  if (g2) memcpy(g2, d.g2c, 32);
  Transcript t;
  STARK_HIP(d.ctx, hipMemcpyAsync(&t, d.d_tr, sizeof(Transcript), hipMemcpyDeviceToHost, d.s));
  STARK_HIP(d.ctx, hipStreamSynchronize(d.s));
  if (a_root) memcpy(a_root, t.roots[0], 32);
  return transcript_status(d.ctx, t.err);
}

stark_status stark_dprove_rows(stark_dprove* h, uint8_t** rows_dev) {
  if (!h || !rows_dev) return STARK_ERR_BAD_ARG;
  *rows_dev = (uint8_t*)h->st.rows;
  return STARK_OK;
}

// k from the main tree's root (prove.rs:274-283) on the device, then L at this rank's points; the root
// is host memory (m_root) or device memory (d_m_root, no host round trip).
static stark_status dprove_lincomb(stark_dprove* h, const uint8_t* m_root, const uint8_t* d_m_root, uint64_t** l_dev) {
  DProveState& d = h->st;
  const Mont mc = mont();
  STARK_HIP(d.ctx, hipSetDevice(d.ctx->device));
  const uint32_t* d_root = (const uint32_t*)d_m_root;
  if (m_root) {
    STARK_HIP(d.ctx, hipMemcpyAsync(d.d_tr->roots[1], m_root, 32, hipMemcpyHostToDevice, d.s));
    d_root = d.d_tr->roots[1];
  }
  hipLaunchKernelGGL(r1cs_k_kernel, dim3(1), dim3(kKThreads), 0, d.s, (const uint32_t*)d_root, mc.r2, mc.one, d.xs,
                     pow32(), d.d_tr);
  STARK_HIP(d.ctx, hipGetLastError());
  LincombArgs la;
  la.rows = d.rows;
  la.plane = 0;
  la.out = d.lvals;
  la.prec = d.dim.P;
  la.g_add = d.dim.rank;
  la.log_g = d.dim.log_g;
  la.tr = d.d_tr;
  hipLaunchKernelGGL(r1cs_lincomb_kernel, dim3(blocks_for(d.dim.P)), dim3(256), 0, d.s, la);
  STARK_HIP(d.ctx, hipGetLastError());
  if (m_root) STARK_HIP(d.ctx, hipStreamSynchronize(d.s));  // m_root is the caller's (pageable) buffer
  *l_dev = (uint64_t*)d.lvals;
  return STARK_OK;
}

stark_status stark_dprove_lincomb(stark_dprove* h, const uint8_t m_root[32], uint64_t** l_dev) {
  if (!h || !m_root || !l_dev) return STARK_ERR_BAD_ARG;
  return dprove_lincomb(h, m_root, nullptr, l_dev);
}

stark_status stark_dprove_lincomb_dev(stark_dprove* h, const uint8_t* d_m_root, uint64_t** l_dev) {
  if (!h || !d_m_root || !l_dev || (((uintptr_t)d_m_root) & 3)) return STARK_ERR_BAD_ARG;
  return dprove_lincomb(h, nullptr, d_m_root, l_dev);
}

void stark_dprove_free(stark_dprove* h) { delete h; }

}  // extern "C"
