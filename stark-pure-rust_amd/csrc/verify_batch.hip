// Batched verifier: verify_with_witness (packages/r1cs-stark/src/run.rs:454-526, verify.rs:13-258,
// packages/fri/src/fri.rs:226-404) for many proofs of one prepared circuit.
//
// One proof's verification is a few thousand hashes and products, best done on the host (verify.hip).  B proofs
// of one circuit hold B x (400 + 200 per FRI layer) Merkle paths of a handful of shapes, B x 40 x layers
// independent cubics and B x 80 independent spot checks: wide, regular work.  The host parses the proofs,
// derives every index from their roots (the sampler) and packs the openings of a chunk of proofs into one
// staging image; one upload, three launches -- paths, FRI rows, spot checks, one lane per check, one ok byte
// per check -- and one download follow on the context stream, while the host workers check the Last layers.
// The circuit's six columns are read in place at the spot positions.
//
// Only a proof whose structure is exactly what the circuit implies enters that chain (in_shape below); every
// other proof goes through the single-proof verifier, so each status is stark_verify_r1cs_circuit's.  Nothing
// a proof's text supplies is used as a length or an offset on the device: the records hold offsets the host
// computed from the circuit's shape, and indices the sampler produced below the trees' sizes.
//
// A proof comes as serde_json text or as a stark_r1cs_proof handle (views over its vectors, no text: view_proof).
// Two more launches may precede the three: verify_transcript_batch_kernel derives a chain proof's indices,
// challenges and records from the roots in its block, one workgroup per proof, where the context asks for the
// device's transcript (the host then uploads openings only); verify_interp2_batch_kernel forms every chain proof's
// I2 from the Lagrange basis of the circuit's boundary points where that matrix is small enough; from the
// verification threshold on, one application of the circuit's interpolation plan (poly.hip) forms them instead.
//
// The file's second part is the same chain for standalone FRI proofs (stark_verify_low_degree_batch): the path and
// row kernels above on stark_fri_proof handles, and the Last element's kernels.
#include <string.h>

#include <algorithm>
#include <atomic>
#include <vector>

#include "internal.h"
#include "merkle_dev.h"
#include "transcript_dev.h"
#include "verify_in.h"

namespace stark {
namespace {

constexpr uint32_t kSpots = 80, kMainPer = 4, kRows = 40, kPolyPer = 4;  // verify.rs:86-118, fri.rs:288-316
constexpr uint32_t kMainLeaf = 256, kMaxLayers = 16;
constexpr uint32_t kThreads = 64;  // one wave per workgroup: a chunk's few thousand lanes spread over the CUs

// The roots come first in a block: m_root, l_root, then each Middle layer's root2 (a_root follows them, Shape).
constexpr size_t kRootM = 0, kRootL = 32, kRoot2 = 64;

// One Merkle path (Proof::validate, merkle_tree.rs:25-43): byte offsets into the chunk's image.
struct PathRec {
  uint32_t root, leaf, nodes, index, leaf_len, depth, pad0, pad1;
};
// One row of one FRI layer of one proof (fri.rs:318-345): the layer's tree root (special_x), the column leaf,
// the row's four polynomial leaves (contiguous) and the row's index y.
struct RowRec {
  uint32_t root, col_leaf, poly_leaf, y, layer, pad0, pad1, pad2;
};
// One spot check (verify.rs:185-254): the position's four main leaves (contiguous) and L leaf, the proof's
// constants (r[3], k[11]) and I2's coefficients.
struct SpotRec {
  uint32_t main_leaf, l_leaf, consts, interp2, pos, pad0, pad1, pad2;
};
static_assert(sizeof(PathRec) == 32 && sizeof(RowRec) == 32 && sizeof(SpotRec) == 32, "records are 32 B");

// Constants of the launches, all Montgomery images.
struct RowConsts {
  fe r2m, one, inv4, quartic[4];  // r2m: R^2 (x -> its Montgomery image), 1, 1/4, zeta^j
};
struct SpotConsts {
  fe r2m, one, g2, x_last;
  const fe* col[6];  // K F0 F1 F2 IDX PIDX over the precision domain (PreparedCircuit::col)
  uint32_t bx, n_b;  // Zb2's roots: offset and count
  uint32_t i3, n_i3; // I3's coefficients
  uint32_t log_steps;
  uint32_t k_mont;   // K, F0-F2 are Montgomery images (a prover's circuit)
};

template <class T>
__device__ __forceinline__ T load_rec(const T* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 a = q[0], b = q[1];
  T r;
  uint32_t* w = reinterpret_cast<uint32_t*>(&r);
  w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
  w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
  return r;
}

__device__ __forceinline__ fe arena_fe(const uint8_t* __restrict__ arena, uint32_t off) {
  return fe_load(reinterpret_cast<const fe*>(arena + off));
}
// from_bytes_le (ff_utils/src/fp.rs:70-77) of 32 bytes as a Montgomery image: any x < 2^256 times R^2 < p
// is within the product's bounds (fe_mul_asm.inc), and the product is x R mod p, reduced.
__device__ __forceinline__ fe arena_mont(const uint8_t* __restrict__ arena, uint32_t off, const fe& r2m) {
  return fe_mul(arena_fe(arena, off), r2m);
}
__device__ __forceinline__ bool fe_eq(const fe& a, const fe& b) {
  uint32_t x = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) x |= a.w[i] ^ b.w[i];
  return x == 0;
}
// b^e by square-and-multiply, low bit first (Montgomery images).
__device__ __forceinline__ fe fe_pow(fe b, uint64_t e, const fe& one) {
  fe r = one;
  while (e) {
    const fe t = fe_mul(r, b);
    if (e & 1) r = t;
    b = fe_mul(b, b);
    e >>= 1;
  }
  return r;
}

// Every Merkle path of the chunk, one per lane: the leaf's digest, `depth` pair hashes ordered by the index
// bits (the current node on the left where bit d is 0), and the compare with the root.  The records come in
// runs of one (leaf_len, depth), so a wave's trip count is uniform but at a run's end.
__global__ __launch_bounds__(kThreads) void verify_paths_batch_kernel(const uint8_t* __restrict__ arena,
                                                                       const PathRec* __restrict__ recs, uint32_t n,
                                                                       uint8_t* __restrict__ ok) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const PathRec r = load_rec(recs + i);
  Digest d = r.leaf_len == 32 ? hash_leaf32(arena + r.leaf) : hash_leaf(arena + r.leaf, r.leaf_len);
  const Digest* nodes = reinterpret_cast<const Digest*>(arena + r.nodes);
  for (uint32_t k = 0; k < r.depth; ++k) {
    const Digest sib = load_digest(nodes + k);
    const bool right = (r.index >> k) & 1;
    Digest left, rgt;
#pragma unroll
    for (int w = 0; w < 8; ++w) {
      left.h[w] = right ? sib.h[w] : d.h[w];
      rgt.h[w] = right ? d.h[w] : sib.h[w];
    }
    d = hash_pair(left, rgt);
  }
  const Digest root = load_digest(reinterpret_cast<const Digest*>(arena + r.root));
  uint32_t diff = 0;
#pragma unroll
  for (int w = 0; w < 8; ++w) diff |= d.h[w] ^ root.h[w];
  ok[i] = diff == 0;
}

// verify_low_degree_proof_rec's row loop (fri.rs:318-345; verify.hip verify_fri), one (proof, layer, row) per
// lane: the cubic through (x1 zeta^j, row_j) at special_x against the column value.  x1 = root_l^y and
// 1 / x1^3 = root_l^(-3 y mod deg_l) by square-and-multiply from the layer's root of unity.
__global__ __launch_bounds__(kThreads) void verify_fri_rows_batch_kernel(const uint8_t* __restrict__ arena,
                                                                          const RowRec* __restrict__ recs, uint32_t n,
                                                                          const fe* __restrict__ layer_root,
                                                                          const uint64_t* __restrict__ layer_deg,
                                                                          RowConsts K, uint8_t* __restrict__ ok) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const RowRec r = load_rec(recs + i);
  const fe root = fe_load(layer_root + r.layer);
  const uint64_t dl = layer_deg[r.layer], y = r.y;
  const fe x1 = fe_pow(root, y, K.one);
  const fe inv_x13 = fe_pow(root, (dl - (3 * y) % dl) % dl, K.one);
  const fe sx = arena_mont(arena, r.root, K.r2m);  // special_x = from_bytes_le(the layer's tree root)
  // Lagrange weights prod_{t != j}(sx - x_t) / (4 x1^3 zeta^(3j)), zeta^(-3j) = zeta^j (multi_interp_4 +
  // eval_quartic, poly_utils.rs:442-511).
  fe dx[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) dx[j] = fe_sub(sx, fe_mul(K.quartic[j], x1));
  const fe inv_den = fe_mul(K.inv4, inv_x13);
  fe val = fe_zero();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    fe num = K.one;
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (t != j) num = fe_mul(num, dx[t]);
    const fe row = arena_mont(arena, r.poly_leaf + 32 * j, K.r2m);
    val = fe_add(val, fe_mul(fe_mul(row, num), fe_mul(inv_den, K.quartic[j])));
  }
  ok[i] = fe_eq(val, arena_mont(arena, r.col_leaf, K.r2m));  // assert_eq (fri.rs:337)
}

// A circuit column's value at a position as a Montgomery image: the extensions hold K, F0-F2 as Montgomery
// images (in a prover's circuit) and IDX, PIDX canonical, each as the transform left it (any value below 2^256
// of the right class).
__device__ __forceinline__ fe column_mont(const fe* __restrict__ col, uint32_t pos, bool is_mont, const fe& r2m) {
  fe v = fe_load(col + pos);
  if (!is_mont) return fe_mul(v, r2m);
  fe_csub2p(v);  // 2^256 < 5p: two conditional 2p, one conditional p
  fe_csub2p(v);
  fe_reduce_once(v);
  return v;
}

// verify_r1cs_proof's six equalities at one position (verify.rs:185-254; verify.hip's spot), one (proof,
// position) per lane, on Montgomery images throughout.
__global__ __launch_bounds__(kThreads) void verify_spot_batch_kernel(const uint8_t* __restrict__ arena,
                                                                      const SpotRec* __restrict__ recs, uint32_t n,
                                                                      SpotConsts K, uint8_t* __restrict__ ok) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const SpotRec rec = load_rec(recs + i);
  const fe* pc = reinterpret_cast<const fe*>(arena + rec.consts);  // r[0..3), k[0..11)
  auto leaf = [&](uint32_t b, uint32_t chunk) {
    return arena_mont(arena, rec.main_leaf + kMainLeaf * b + 32 * chunk, K.r2m);
  };
  const fe x = fe_pow(K.g2, rec.pos, K.one);
  fe xs = x;  // x^steps
  for (uint32_t s = 0; s < K.log_steps; ++s) xs = fe_mul(xs, xs);
  const fe z = fe_sub(xs, K.one);  // best_fft of X^steps - 1 at x
  const bool km = K.k_mont != 0;
  const fe p_x = leaf(0, 0), s_x = leaf(0, 2), a_x = leaf(0, 1);
  const fe d1 = leaf(0, 3), d2 = leaf(0, 4), d3 = leaf(0, 5), b2 = leaf(0, 6), b3 = leaf(0, 7);
  bool good = true;
  {  // Q1 = Z D1 (verify.rs:208-219)
    const fe p_prev = leaf(1, 0);
    const fe k_x = column_mont(K.col[0], rec.pos, km, K.r2m), f0 = column_mont(K.col[1], rec.pos, km, K.r2m),
             f1 = column_mont(K.col[2], rec.pos, km, K.r2m);
    const fe q1 = fe_mul(f0, fe_sub(fe_sub(p_x, fe_mul(f1, p_prev)), fe_mul(k_x, s_x)));
    good &= fe_eq(q1, fe_mul(z, d1));
  }
  {  // Q2 = Z D2
    const fe p_w = leaf(2, 0), p_2w = leaf(3, 0);
    const fe f2 = column_mont(K.col[3], rec.pos, km, K.r2m);
    good &= fe_eq(fe_mul(f2, fe_sub(p_2w, fe_mul(p_x, p_w))), fe_mul(z, d2));
  }
  {  // Q3 = Z D3 (verify.rs:221-225)
    const fe a_prev = leaf(1, 1);
    const fe ext_idx = column_mont(K.col[4], rec.pos, false, K.r2m),
             ext_pidx = column_mont(K.col[5], rec.pos, false, K.r2m);
    const fe r0 = fe_load(pc), r1 = fe_load(pc + 1), r2 = fe_load(pc + 2);
    const fe rs = fe_mul(r2, s_x);
    const fe nmr = fe_add(fe_add(r0, fe_mul(r1, ext_idx)), rs);
    const fe dnm = fe_add(fe_add(r0, fe_mul(r1, ext_pidx)), rs);
    good &= fe_eq(fe_sub(fe_mul(a_x, dnm), fe_mul(a_prev, nmr)), fe_mul(z, d3));
  }
  {  // Boundary constraints (verify.rs:227-238): Zb2(x) over the circuit's boundary points, I2(x) and I3(x) by Horner
    const fe* bx = reinterpret_cast<const fe*>(arena + K.bx);
    fe zb2 = K.one;
    for (uint32_t k = 0; k < K.n_b; ++k) zb2 = fe_mul(zb2, fe_sub(x, fe_load(bx + k)));
    const fe* c2 = reinterpret_cast<const fe*>(arena + rec.interp2);
    fe i2 = fe_zero();
    for (uint32_t k = K.n_b; k-- > 0;) i2 = fe_add(fe_mul(i2, x), fe_load(c2 + k));
    good &= fe_eq(fe_sub(s_x, i2), fe_mul(zb2, b2));
    const fe* c3 = reinterpret_cast<const fe*>(arena + K.i3);
    fe i3 = fe_zero();
    for (uint32_t k = K.n_i3; k-- > 0;) i3 = fe_add(fe_mul(i3, x), fe_load(c3 + k));
    good &= fe_eq(fe_sub(a_x, i3), fe_mul(fe_sub(x, K.x_last), b3));
  }
  {  // The linear combination (verify.rs:240-254)
    const fe* kk = pc + 3;
    fe l = fe_mul(fe_load(kk), d1);
    l = fe_add(l, fe_mul(fe_load(kk + 1), d2));
    l = fe_add(l, fe_mul(fe_load(kk + 2), d3));
    l = fe_add(l, fe_mul(fe_load(kk + 3), p_x));
    l = fe_add(l, fe_mul(fe_mul(fe_load(kk + 4), p_x), xs));
    l = fe_add(l, fe_mul(fe_load(kk + 5), b2));
    l = fe_add(l, fe_mul(fe_mul(fe_load(kk + 6), b2), xs));
    l = fe_add(l, fe_mul(fe_load(kk + 7), b3));
    l = fe_add(l, fe_mul(fe_mul(fe_load(kk + 8), b3), xs));
    l = fe_add(l, fe_mul(fe_load(kk + 9), a_x));
    l = fe_add(l, fe_mul(fe_load(kk + 10), s_x));
    good &= fe_eq(arena_mont(arena, rec.l_leaf, K.r2m), l);
  }
  ok[i] = good;
}

// ---- the transcript and I2 on the device ----

// Where a chunk's parts are, as the transcript kernel takes them: the Shape and ChunkPlan below, in 32 bits (a
// chunk's image stays under 4 GiB).  Everything here is a function of the circuit and of the number of chain
// proofs in the chunk; nothing comes from a proof.
struct TranscriptArgs {
  uint32_t nb, layers, depth, prec, os, skips;
  uint32_t o_paths, o_rows, o_spots, o_blocks, block;
  uint32_t o_aroot, o_consts, o_i2, o_main_leaf, o_main_nodes, o_l_leaf, o_l_nodes;
  uint32_t o_col_leaf[kMaxLayers], o_col_nodes[kMaxLayers], o_poly_leaf[kMaxLayers], o_poly_nodes[kMaxLayers];
  fe r2m, one;
};

template <class T>
__device__ __forceinline__ void store_rec(T* p, const T& r) {
  const uint32_t* w = reinterpret_cast<const uint32_t*>(&r);
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(w[0], w[1], w[2], w[3]);
  q[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// get_pseudorandom_indices' map of one big-endian word (fri/src/utils.rs:101-109; fri.hip fri_indices_block): below
// `modulus`, never a multiple of `excl`.  (plan_shape checked modulus (excl - 1) / excl > 0 for every tree.)
__device__ __forceinline__ uint32_t sampled_index(uint32_t le_word, uint32_t modulus, uint32_t excl) {
  const uint32_t real_mod = (uint32_t)((uint64_t)modulus * (excl - 1) / excl);
  const uint32_t v = __builtin_bswap32(le_word) % real_mod;
  return v + 1 + v / (excl - 1);
}

constexpr uint32_t kChainWords = 80;                // the longest chain: the 80 positions' words
constexpr uint32_t kMaxChains = kMaxLayers + 12;    // l_root, the layers, a_root, k_1..k_10

// Everything the host's pack derives from a chain proof's roots, one workgroup (one wave) per proof, from the
// roots in the proof's block: the 80 positions (l_root), each Middle layer's 40 rows (its root2), r (a_root)
// and k (m_root) into the block's constant slots, and every PathRec, RowRec and SpotRec of the proof in pack's
// order.  The Blake2s chains are independent -- l_root's 9 dependent hashes, 4 per layer, 2 for r, one each for
// k_1..k_10 -- so each runs on a lane of its own, all through the same loop (a lane past its chain's end idles);
// then every lane derives indices and writes records.  No workgroup reads what another writes.
__global__ __launch_bounds__(kThreads) void verify_transcript_batch_kernel(uint8_t* arena, TranscriptArgs A) {
  __shared__ uint32_t chain[kMaxChains][kChainWords];  // a chain's seed, then its digests, as LE words
  __shared__ uint32_t pos[kSpots];
  __shared__ uint32_t ys[kMaxLayers][kRows];
  const uint32_t t = threadIdx.x, k = blockIdx.x;
  const uint32_t blk = A.o_blocks + k * A.block;
  const uint32_t n_chains = A.layers + 12;
  {
    // Lane t's chain: its seed's place in the block, its count of dependent hashes, and the byte that follows
    // the seed in its first message (k_i hashes m_root || i, 33 bytes).
    uint32_t seed = blk + kRootL, hashes = 9, extra = 0;
    if (t >= 1 && t <= A.layers) {
      seed = blk + kRoot2 + 32 * (t - 1);
      hashes = 4;
    } else if (t == A.layers + 1) {
      seed = blk + A.o_aroot;
      hashes = 2;
    } else if (t > A.layers + 1) {
      seed = blk + kRootM;
      hashes = 1;
      extra = t - A.layers - 1;
    }
    if (t >= n_chains) hashes = 0;
    uint32_t w[8];
    if (t < n_chains) {
      const Digest d = load_digest(reinterpret_cast<const Digest*>(arena + seed));
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        w[i] = d.h[i];
        chain[t][i] = w[i];
      }
    }
#pragma unroll 1
    for (uint32_t b = 0; b < 9; ++b) {
      if (b < hashes) {
        uint32_t h[8];
        b2s_short(w, extra, extra ? 33 : 32, h);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          w[i] = h[i];
          chain[t][8 * (b + 1) + i] = h[i];
        }
      }
    }
  }
  __syncthreads();
  // Indices and challenges.
  for (uint32_t i = t; i < kSpots; i += kThreads) pos[i] = sampled_index(chain[0][i], A.prec, A.skips);
  for (uint32_t i = t; i < A.layers * kRows; i += kThreads) {
    const uint32_t l = i / kRows, y = i % kRows;
    ys[l][y] = sampled_index(chain[1 + l][y], A.prec >> (2 * l + 2), A.skips);
  }
  fe* const consts = reinterpret_cast<fe*>(arena + blk + A.o_consts);
  if (t < 3) {
    fe_store(consts + t, fe_mul(challenge_r(&chain[A.layers + 1][8 * t], A.prec - 1), A.r2m));
  } else if (t == 3) {
    fe_store(consts + 3, A.one);  // k_0 = 1
  } else if (t < 14) {
    fe_store(consts + t, fe_mul(challenge_k(&chain[A.layers + 1 + (t - 3)][8]), A.r2m));  // k_(t-3) at slot 3 + (t-3)
  }
  __syncthreads();
  // The records, in pack's order: paths class-major (main, L, then each layer's polynomial and column openings),
  // rows layer-major, spots.
  PathRec* const paths = reinterpret_cast<PathRec*>(arena + A.o_paths);
  RowRec* const rows = reinterpret_cast<RowRec*>(arena + A.o_rows);
  SpotRec* const spots = reinterpret_cast<SpotRec*>(arena + A.o_spots);
  uint32_t cls = 0;
  for (uint32_t q = t; q < kSpots * kMainPer; q += kThreads) {
    size_t rows4[4];
    spot_rows(pos[q / kMainPer], A.os, A.skips, A.prec, rows4);
    store_rec(paths + cls + k * kSpots * kMainPer + q,
              PathRec{blk + (uint32_t)kRootM, blk + A.o_main_leaf + kMainLeaf * q, blk + A.o_main_nodes + 32 * A.depth * q,
                      (uint32_t)rows4[q % kMainPer], kMainLeaf, A.depth, 0, 0});
  }
  cls += A.nb * kSpots * kMainPer;
  for (uint32_t i = t; i < kSpots; i += kThreads) {
    store_rec(paths + cls + k * kSpots + i, PathRec{blk + (uint32_t)kRootL, blk + A.o_l_leaf + 32 * i,
                                                     blk + A.o_l_nodes + 32 * A.depth * i, pos[i], 32, A.depth, 0, 0});
    store_rec(spots + k * kSpots + i, SpotRec{blk + A.o_main_leaf + kMainLeaf * kMainPer * i, blk + A.o_l_leaf + 32 * i,
                                               blk + A.o_consts, blk + A.o_i2, pos[i], 0, 0, 0});
  }
  cls += A.nb * kSpots;
  for (uint32_t l = 0; l < A.layers; ++l) {
    const uint32_t root_l = blk + (uint32_t)(l == 0 ? kRootL : kRoot2 + 32 * (l - 1)), root2 = blk + (uint32_t)kRoot2 + 32 * l;
    const uint32_t pd = A.depth - 2 * l, cd = A.depth - 2 * l - 2, quarter = A.prec >> (2 * l + 2);
    for (uint32_t q = t; q < kRows * kPolyPer; q += kThreads)
      store_rec(paths + cls + k * kRows * kPolyPer + q,
                PathRec{root_l, blk + A.o_poly_leaf[l] + 32 * q, blk + A.o_poly_nodes[l] + 32 * pd * q,
                        (q % kPolyPer) * quarter + ys[l][q / kPolyPer], 32, pd, 0, 0});
    cls += A.nb * kRows * kPolyPer;
    for (uint32_t i = t; i < kRows; i += kThreads) {
      store_rec(paths + cls + k * kRows + i, PathRec{root2, blk + A.o_col_leaf[l] + 32 * i,
                                                      blk + A.o_col_nodes[l] + 32 * cd * i, ys[l][i], 32, cd, 0, 0});
      store_rec(rows + (l * A.nb + k) * kRows + i, RowRec{root_l, blk + A.o_col_leaf[l] + 32 * i,
                                                           blk + A.o_poly_leaf[l] + 32 * kPolyPer * i, ys[l][i], l, 0, 0, 0});
    }
    cls += A.nb * kRows;
  }
}

// I2 of every chain proof at once.  The boundary points are the circuit's, so I2_b = sum_k pub_b[wire_k] L_k
// with L_k the k-th Lagrange basis polynomial over them: one lane per (proof, coefficient j) forms the n_b-term
// sum over column j of the basis matrix and writes the block's I2 slot j as a Montgomery image.  mat[k n_b + j]
// holds coefficient j of L_k times R^2, so its product with the wire's 32 bytes as they are (any value below
// 2^256, as from_bytes_le takes them) is the term's Montgomery image; wire[k] < n_public (checked by the host).
__global__ __launch_bounds__(kThreads) void verify_interp2_batch_kernel(uint8_t* arena, const fe* __restrict__ mat,
                                                                         const uint32_t* __restrict__ wire, uint32_t n_b,
                                                                         uint32_t o_blocks, uint32_t block,
                                                                         uint32_t o_pub, uint32_t o_i2) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= n_b) return;
  const uint32_t blk = o_blocks + blockIdx.y * block;
  fe acc = fe_zero();
  for (uint32_t k = 0; k < n_b; ++k)
    acc = fe_add(acc, fe_mul(arena_fe(arena, blk + o_pub + 32 * wire[k]), fe_load(mat + (size_t)k * n_b + j)));
  fe_store(reinterpret_cast<fe*>(arena + blk + o_i2) + j, acc);
}

// ---- host ----

// What the circuit implies of a proof's structure, and where a proof's parts are in its block of the image.
struct Shape {
  uint32_t depth = 0, layers = 0;  // log2 precision; FriProof::Middle layers
  size_t n_b = 0;                  // boundary points
  size_t n_public = 0;             // public wires
  // offsets in a proof's block (bytes; everything is a multiple of 32)
  size_t o_aroot = 0, o_pub = 0;   // a_root and the public wires as given (what the device forms derive from)
  size_t o_consts = 0, o_i2 = 0, o_main_leaf = 0, o_main_nodes = 0, o_l_leaf = 0, o_l_nodes = 0;
  size_t o_col_leaf[kMaxLayers], o_col_nodes[kMaxLayers], o_poly_leaf[kMaxLayers], o_poly_nodes[kMaxLayers];
  size_t block = 0;  // bytes per proof
  uint32_t col_depth(uint32_t l) const { return depth - 2 * l - 2; }
  uint32_t poly_depth(uint32_t l) const { return depth - 2 * l; }
  size_t paths() const { return kSpots * kMainPer + kSpots + (size_t)layers * (kRows + kRows * kPolyPer); }
  size_t rows() const { return (size_t)layers * kRows; }
  size_t checks() const { return paths() + rows() + kSpots; }
  size_t staged() const { return block + 32 * checks(); }  // a proof's block and records
};

// False where the chain cannot take the circuit at all (every proof then goes to the single-proof verifier).
bool plan_shape(const PreparedCircuit& c, const VerifyDomain& d, Shape& s) {
  // (The sampler's bounds on the precision, utils.rs:88 and :101, for the 80 positions and for r: they depend on
  // the circuit alone, so a precision the sampler refuses sends every proof to the single-proof verifier.)
  if (c.spot || !c.col[0] || d.prec >= ((uint64_t)1 << 24) || d.skips < 2 || d.prec * (d.skips - 1) / d.skips == 0)
    return false;
  while (((uint64_t)1 << s.depth) < d.prec) ++s.depth;
  // The layers prove_low_degree makes of precision values below degree precision / 4 (fri.rs:64-66; fri.hip
  // fri_check), each with the sampler's bounds on its column (utils.rs:88).
  uint64_t m = d.prec, deg = d.prec / 4;
  while (deg > 16) {
    if (m < 8 || m / 4 >= (1u << 24) || m / 4 * (d.skips - 1) / d.skips == 0) return false;
    m /= 4;
    deg /= 4;
    ++s.layers;
  }
  if (s.layers + 1 > kMaxLayers) return false;
  s.n_b = c.pfi.size() / 2;
  s.n_public = c.n_public;
  size_t at = 32 * (2 + (size_t)s.layers);
  auto take = [&](size_t bytes) {
    const size_t o = at;
    at += bytes;
    return o;
  };
  s.o_aroot = take(32);
  s.o_pub = take(32 * s.n_public);
  s.o_consts = take(32 * 14);
  s.o_i2 = take(32 * s.n_b);
  s.o_main_leaf = take((size_t)kSpots * kMainPer * kMainLeaf);
  s.o_main_nodes = take((size_t)kSpots * kMainPer * 32 * s.depth);
  s.o_l_leaf = take((size_t)kSpots * 32);
  s.o_l_nodes = take((size_t)kSpots * 32 * s.depth);
  for (uint32_t l = 0; l < s.layers; ++l) {
    s.o_col_leaf[l] = take((size_t)kRows * 32);
    s.o_col_nodes[l] = take((size_t)kRows * 32 * s.col_depth(l));
    s.o_poly_leaf[l] = take((size_t)kRows * kPolyPer * 32);
    s.o_poly_nodes[l] = take((size_t)kRows * kPolyPer * 32 * s.poly_depth(l));
  }
  s.block = at;
  return true;
}

bool branches_are(const std::vector<Branch>& v, size_t count, size_t leaf_len, size_t depth) {
  if (v.size() != count) return false;
  for (const Branch& b : v)
    if (b.leaf.size() != leaf_len || b.nodes.size() != 32 * depth) return false;
  return true;
}

// The proof's structure is exactly what the circuit implies: every length the packing and the kernels assume.
bool in_shape(const ProofIn& pr, const Shape& s) {
  if (pr.fri.size() != (size_t)s.layers + 1) return false;
  for (uint32_t l = 0; l < s.layers; ++l) {
    const FriIn& f = pr.fri[l];
    if (f.last || !branches_are(f.col, kRows, 32, s.col_depth(l)) ||
        !branches_are(f.poly, kRows * kPolyPer, 32, s.poly_depth(l)))
      return false;
  }
  const FriIn& last = pr.fri.back();
  const size_t n = last.last_vals.size();
  if (!last.last || n == 0 || (n & (n - 1))) return false;
  for (const std::vector<uint8_t>& v : last.last_vals)
    if (v.size() != 32) return false;
  return branches_are(pr.main, kSpots * kMainPer, kMainLeaf, s.depth) && branches_are(pr.lcomb, kSpots, 32, s.depth);
}

// A handle's parts as the parsed proof the verifier reads: views over the handle's vectors (nothing is copied
// but the Last layer's values, nothing allocated per opening).  A handle is untrusted input -- anything can be
// made into one (stark_r1cs_proof_from_parts) -- so only sizes the vectors really have become views, the
// prover's own index vectors are never read, and the views pass the same screen as a parsed text.
bool view_branches(const std::vector<uint8_t>& leaves, size_t leaf_len, const std::vector<uint8_t>& nodes, size_t depth,
                   std::vector<Branch>& out) {
  if (leaf_len == 0 || leaves.size() % leaf_len) return false;
  const size_t k = leaves.size() / leaf_len;
  if (k == 0) return nodes.empty();
  if (nodes.size() % (32 * k) || nodes.size() / (32 * k) != depth) return false;
  out.resize(k);
  for (size_t i = 0; i < k; ++i) {
    out[i].leaf = Bytes{leaves.data() + i * leaf_len, leaf_len};
    out[i].nodes = Bytes{nodes.data() + i * depth * 32, depth * 32};
  }
  return true;
}
// A Vec<FriProof> handle's layers (the FRI part of a StarkProof handle, or a standalone proof's handle).
bool view_fri(const stark_fri_proof& h, std::vector<FriIn>& out) {
  out.resize(h.layers.size());
  for (size_t l = 0; l < out.size(); ++l) {
    const stark_fri_layer& L = h.layers[l];
    FriIn& f = out[l];
    f.last = L.last;
    if (L.last) {
      for (size_t i = 0; i + 32 <= L.last_values.size(); i += 32)
        f.last_vals.emplace_back(L.last_values.data() + i, L.last_values.data() + i + 32);
      continue;
    }
    memcpy(f.root2, L.root2, 32);
    if (!view_branches(L.col_leaves, L.col_leaf_len, L.col_nodes, L.col_depth, f.col) ||
        !view_branches(L.poly_leaves, L.poly_leaf_len, L.poly_nodes, L.poly_depth, f.poly))
      return false;
  }
  return true;
}
bool view_proof(const stark_r1cs_proof& h, ProofIn& pr) {
  if (!h.fri) return false;
  memcpy(pr.m_root, h.m_root, 32);
  memcpy(pr.l_root, h.l_root, 32);
  memcpy(pr.a_root, h.a_root, 32);
  if (!view_branches(h.m_leaves, h.m_leaf_len, h.m_nodes, h.depth_of(0), pr.main) ||
      !view_branches(h.l_leaves, h.l_leaf_len, h.l_nodes, h.depth_of(1), pr.lcomb))
    return false;
  return view_fri(*h.fri, pr.fri);
}

// One entry's proof as the caller gave it: serde_json text, or a handle.
struct ProofSrc {
  const char* json = nullptr;
  size_t json_len = 0;
  const stark_r1cs_proof* handle = nullptr;
  bool is_handle = false;
};

// One entry of the batch on its way through a chunk.
struct Item {
  ProofIn pr;
  const uint8_t* pub_bytes = nullptr;
  std::vector<HostFp> pub;
  bool chain = false;      // enters the device chain
  bool fallback = false;   // goes to verify_r1cs
  stark_status st = STARK_OK;
  uint32_t reasons = 0;
  std::vector<size_t> positions;
  std::vector<std::vector<size_t>> ys;  // per Middle layer
  HostFp r[3], kk[11];
  std::vector<HostFp> interp2;
  bool last_ok = false;
};

// Everything of entry b that needs neither the device nor the worker pool: the parse, the reference's first
// checks, the shape screen and, with the host's transcript, the indices and challenges (with the device's, the
// transcript kernel derives them from the roots in the proof's block and the host calls no sampler).
void screen(const PreparedCircuit& c, const VerifyDomain& d, const Shape& s, bool chain_ok, bool device_tr,
            const uint8_t* pub_bytes, size_t n_public, const ProofSrc& src, bool serial_parse, Item& it) {
  const FieldHost& F = FieldHost::get();
  const bool read = src.is_handle ? src.handle && view_proof(*src.handle, it.pr)
                                  : src.json && read_proof(src.json, src.json_len, it.pr, serial_parse);
  if (!pub_bytes || !read) {
    it.st = STARK_ERR_BAD_ARG;  // (stark_verify_r1cs_circuit's null checks; serde_json::from_reader fails, run.rs:579)
    return;
  }
  it.pub_bytes = pub_bytes;
  if (n_public != c.n_public) {
    it.st = STARK_ERR_BAD_ARG;
    return;
  }
  it.pub.resize(c.n_public);
  for (size_t i = 0; i < c.n_public; ++i) it.pub[i] = F.from_bytes_le(pub_bytes + 32 * i, 32);
  if (!FieldHost::eq(it.pub[0], F.one())) {  // run.rs:480
    it.st = STARK_ERR_CHECK;
    it.reasons = STARK_VERIFY_FAIL_PUBLIC_ONE;
    return;
  }
  it.fallback = true;
  if (!chain_ok || !in_shape(it.pr, s)) return;
  if (!device_tr) {
    if (!sampler(it.pr.l_root, d.prec, kSpots, (uint32_t)d.skips, it.positions)) return;
    it.ys.resize(s.layers);
    uint64_t deg = d.prec;
    for (uint32_t l = 0; l < s.layers; ++l, deg /= 4)
      if (!sampler(it.pr.fri[l].root2, deg / 4, kRows, (uint32_t)d.skips, it.ys[l])) return;
    if (!verify_challenges(it.pr, d.prec, it.r, it.kk)) return;
  }
  it.fallback = false;
  it.chain = true;
}

// Where a chunk of nb chain proofs puts its parts in the image (after the call's constants at [0, base)).
struct ChunkPlan {
  size_t o_paths, o_rows, o_spots, o_blocks, o_ok, total;
  size_t n_paths, n_rows, n_spots;
};
size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
ChunkPlan plan_chunk(const Shape& s, size_t base, size_t nb) {
  ChunkPlan p;
  p.n_paths = nb * s.paths();
  p.n_rows = nb * s.rows();
  p.n_spots = nb * kSpots;
  p.o_paths = base;
  p.o_rows = p.o_paths + 32 * p.n_paths;
  p.o_spots = p.o_rows + 32 * p.n_rows;
  p.o_blocks = p.o_spots + 32 * p.n_spots;
  p.o_ok = align256(p.o_blocks + nb * s.block);
  p.total = p.o_ok + align256(p.n_paths + p.n_rows + p.n_spots);
  return p;
}

void put_branches(uint8_t* leaves, uint8_t* nodes, const std::vector<Branch>& v) {
  for (const Branch& b : v) {
    memcpy(leaves, b.leaf.data(), b.leaf.size());
    leaves += b.leaf.size();
    memcpy(nodes, b.nodes.data(), b.nodes.size());
    nodes += b.nodes.size();
  }
}

// Chain proof k of nb: its block and its records.  The path records are class-major -- main, L, then each
// layer's polynomial and column openings -- so that equal shapes are side by side; rows are layer-major.
// host_tr: the host writes the constants and the records (else verify_transcript_batch_kernel does, and nothing
// of them is written or uploaded); host_i2: the host writes I2's coefficients (else verify_interp2_batch_kernel
// or the circuit's interpolation plan does).
void pack(const Shape& s, const VerifyDomain& d, size_t os, const ChunkPlan& p, size_t nb, size_t k, const Item& it,
          bool host_tr, bool host_i2, uint8_t* img) {
  const size_t blk = p.o_blocks + k * s.block;
  uint8_t* const b = img + blk;
  memcpy(b + kRootM, it.pr.m_root, 32);
  memcpy(b + kRootL, it.pr.l_root, 32);
  for (uint32_t l = 0; l < s.layers; ++l) memcpy(b + kRoot2 + 32 * l, it.pr.fri[l].root2, 32);
  memcpy(b + s.o_aroot, it.pr.a_root, 32);
  memcpy(b + s.o_pub, it.pub_bytes, 32 * s.n_public);
  if (host_tr) {
    for (int j = 0; j < 3; ++j) memcpy(b + s.o_consts + 32 * j, it.r[j].v, 32);
    for (int j = 0; j < 11; ++j) memcpy(b + s.o_consts + 32 * (3 + j), it.kk[j].v, 32);
  }
  for (size_t j = 0; host_i2 && j < s.n_b; ++j) {
    if (j < it.interp2.size()) memcpy(b + s.o_i2 + 32 * j, it.interp2[j].v, 32);
    else memset(b + s.o_i2 + 32 * j, 0, 32);
  }
  put_branches(b + s.o_main_leaf, b + s.o_main_nodes, it.pr.main);
  put_branches(b + s.o_l_leaf, b + s.o_l_nodes, it.pr.lcomb);
  for (uint32_t l = 0; l < s.layers; ++l) {
    put_branches(b + s.o_col_leaf[l], b + s.o_col_nodes[l], it.pr.fri[l].col);
    put_branches(b + s.o_poly_leaf[l], b + s.o_poly_nodes[l], it.pr.fri[l].poly);
  }
  if (!host_tr) return;
  PathRec* paths = reinterpret_cast<PathRec*>(img + p.o_paths);
  auto u = [](size_t x) { return (uint32_t)x; };
  size_t cls = 0;  // the class's first record
  for (uint32_t i = 0; i < kSpots; ++i) {
    size_t rows4[4];
    spot_rows(it.positions[i], os, d.skips, d.prec, rows4);
    for (uint32_t j = 0; j < kMainPer; ++j) {
      const size_t q = kMainPer * i + j;
      paths[cls + k * kSpots * kMainPer + q] = PathRec{u(blk + kRootM), u(blk + s.o_main_leaf + kMainLeaf * q),
                                                       u(blk + s.o_main_nodes + 32 * s.depth * q), u(rows4[j]), kMainLeaf,
                                                       s.depth, 0, 0};
    }
  }
  cls += nb * kSpots * kMainPer;
  for (uint32_t i = 0; i < kSpots; ++i)
    paths[cls + k * kSpots + i] = PathRec{u(blk + kRootL), u(blk + s.o_l_leaf + 32 * i),
                                          u(blk + s.o_l_nodes + 32 * s.depth * i), u(it.positions[i]), 32, s.depth, 0, 0};
  cls += nb * kSpots;
  RowRec* rows = reinterpret_cast<RowRec*>(img + p.o_rows);
  uint64_t deg = d.prec;
  for (uint32_t l = 0; l < s.layers; ++l, deg /= 4) {
    const size_t root_l = blk + (l == 0 ? kRootL : kRoot2 + 32 * (l - 1)), root2 = blk + kRoot2 + 32 * l;
    const uint32_t pd = s.poly_depth(l), cd = s.col_depth(l);
    for (uint32_t i = 0; i < kRows; ++i) {
      const size_t y = it.ys[l][i];
      for (uint32_t j = 0; j < kPolyPer; ++j) {
        const size_t q = kPolyPer * i + j;
        paths[cls + k * kRows * kPolyPer + q] = PathRec{u(root_l), u(blk + s.o_poly_leaf[l] + 32 * q),
                                                        u(blk + s.o_poly_nodes[l] + 32 * pd * q), u(j * (deg / 4) + y), 32,
                                                        pd, 0, 0};
      }
    }
    cls += nb * kRows * kPolyPer;
    for (uint32_t i = 0; i < kRows; ++i) {
      paths[cls + k * kRows + i] = PathRec{u(root2), u(blk + s.o_col_leaf[l] + 32 * i),
                                           u(blk + s.o_col_nodes[l] + 32 * cd * i), u(it.ys[l][i]), 32, cd, 0, 0};
      rows[((size_t)l * nb + k) * kRows + i] = RowRec{u(root_l), u(blk + s.o_col_leaf[l] + 32 * i),
                                                      u(blk + s.o_poly_leaf[l] + 32 * kPolyPer * i), u(it.ys[l][i]), l, 0, 0, 0};
    }
    cls += nb * kRows;
  }
  SpotRec* spots = reinterpret_cast<SpotRec*>(img + p.o_spots);
  for (uint32_t i = 0; i < kSpots; ++i)
    spots[k * kSpots + i] = SpotRec{u(blk + s.o_main_leaf + kMainLeaf * kMainPer * i), u(blk + s.o_l_leaf + 32 * i),
                                    u(blk + s.o_consts), u(blk + s.o_i2), u(it.positions[i]), 0, 0, 0};
}

// The failed classes of chain proof k from the chunk's ok bytes (the records' order, pack above).
uint32_t reasons_of(const Shape& s, const ChunkPlan& p, size_t nb, size_t k, const uint8_t* ok) {
  uint32_t why = 0;
  auto any_bad = [&](size_t first, size_t count) {
    for (size_t i = 0; i < count; ++i)
      if (!ok[first + i]) return true;
    return false;
  };
  size_t cls = 0;
  if (any_bad(cls + k * kSpots * kMainPer, kSpots * kMainPer)) why |= STARK_VERIFY_FAIL_OPENING_PATHS;
  cls += nb * kSpots * kMainPer;
  if (any_bad(cls + k * kSpots, kSpots)) why |= STARK_VERIFY_FAIL_OPENING_PATHS;
  cls += nb * kSpots;
  for (uint32_t l = 0; l < s.layers; ++l) {
    if (any_bad(cls + k * kRows * kPolyPer, kRows * kPolyPer)) why |= STARK_VERIFY_FAIL_FRI_PATHS;
    cls += nb * kRows * kPolyPer;
    if (any_bad(cls + k * kRows, kRows)) why |= STARK_VERIFY_FAIL_FRI_PATHS;
    cls += nb * kRows;
    if (any_bad(p.n_paths + ((size_t)l * nb + k) * kRows, kRows)) why |= STARK_VERIFY_FAIL_FRI_ROWS;
  }
  if (any_bad(p.n_paths + p.n_rows + k * kSpots, kSpots)) why |= STARK_VERIFY_FAIL_SPOT;
  return why;
}

// The n x n Lagrange basis over the points xs (distinct), in O(n^2): Z = prod (X - x_k) once, then
// L_k = Z / (X - x_k) / Z'(x_k) by synthetic division, Z'(x_k) being that quotient at x_k.  Row k of `out` holds
// L_k's coefficients, low degree first, each times R^2 as verify_interp2_batch_kernel takes them.
void lagrange_basis(const std::vector<HostFp>& xs, uint8_t* out) {
  const FieldHost& F = FieldHost::get();
  const size_t n = xs.size();
  std::vector<HostFp> z(n + 1, F.zero());
  z[0] = F.one();
  for (size_t k = 0; k < n; ++k)  // z <- z (X - x_k)
    for (size_t i = k + 1; i-- > 0;) {
      z[i + 1] = F.add(z[i + 1], z[i]);
      z[i] = F.sub(F.zero(), F.mul(z[i], xs[k]));
    }
  std::atomic<size_t> next{0};
  host_parallel((unsigned)std::min<size_t>(host_threads(), (n + 15) / 16), [&](unsigned) {
    std::vector<HostFp> q(n);
    for (size_t k; (k = next.fetch_add(1)) < n;) {
      q[n - 1] = z[n];
      for (size_t i = n - 1; i > 0; --i) q[i - 1] = F.add(z[i], F.mul(xs[k], q[i]));
      HostFp den = q[n - 1];
      for (size_t i = n - 1; i-- > 0;) den = F.add(F.mul(den, xs[k]), q[i]);
      const HostFp inv = F.inv(den);
      for (size_t j = 0; j < n; ++j) {
        const HostFp v = F.from_canonical(F.mul(q[j], inv).v);  // (the Montgomery image's limbs as a value: x R^2)
        memcpy(out + 32 * (k * n + j), v.v, 32);
      }
    }
  });
}

}  // namespace

// statuses / reasons of entries [0, batch) (both non-null here).  The proofs are texts (proof_json, json_lens) or,
// with `handles` non-null, handles.
static stark_status verify_r1cs_batch(stark_ctx* ctx, const PreparedCircuit& c, const uint8_t* const* public_wires,
                                      size_t n_public, const char* const* proof_json, const size_t* json_lens,
                                      const stark_r1cs_proof* const* handles, uint32_t batch, stark_status* statuses,
                                      uint32_t* reasons) {
  const FieldHost& F = FieldHost::get();
  PhaseClock clk("verify_r1cs_batch");
  const VerifyDomain d = verify_domain(c.os);
  Shape s;
  const bool chain_ok = plan_shape(c, d, s);
  const bool device_tr =
      (ctx->verify_batch_transcript ? ctx->verify_batch_transcript : kDefaultVerifyTranscript) == 2;
  auto source = [&](size_t b) {
    ProofSrc src;
    if (handles) {
      src.is_handle = true;
      src.handle = handles[b];
    } else {
      src.json = proof_json[b];
      src.json_len = json_lens[b];
    }
    return src;
  };
  hipStream_t stream = ctx->stream;
  // The call's constants at the image's start: Zb2's roots, I3's coefficients, the layers' roots of unity and
  // sizes.  Uploaded with the first chunk that has a chain proof.
  std::vector<HostFp> bx, interp3;
  size_t o_i3 = 0, o_lroot = 0, o_ldeg = 0, o_wire = 0, o_mat = 0, base = 0;
  HostFp x_last = F.zero();
  uint32_t log_steps = 0;
  // Chain proofs per chunk under the context's limit, and under the records' 32-bit offsets.
  const size_t limit = std::min<size_t>(ctx->verify_batch_limit ? ctx->verify_batch_limit : kDefaultVerifyBatchLimit,
                                        (size_t)3 << 30);
  // I2 of a chunk's proofs by one launch over the Lagrange basis of the circuit's boundary points
  // (verify_interp2_batch_kernel): below the threshold from which verify_interp2 interpolates on the GPU, and
  // where the n_b x n_b matrix stays under a quarter of the cap.  From that threshold on, where verify_interp2
  // would interpolate on the GPU (fewer points than steps), by one application of the circuit's interpolation
  // plan per chunk (poly.hip interp_plan_apply), which reads the wires' values out of the blocks and writes every
  // I2 slot.  Else per proof, by verify_interp2 (the host's lagrange_interp).
  bool mat_i2 = false, plan_i2 = false;
  const InterpPlan* i2_plan = nullptr;
  if (chain_ok) {
    bx = verify_boundary_points(c, d);
    x_last = F.pow_u64(d.g2, (d.steps - 1) * d.skips);
    interp3 = lagrange_interp({x_last}, {F.one()});
    while (((uint64_t)1 << log_steps) < d.steps) ++log_steps;
    o_i3 = 32 * bx.size();
    o_lroot = o_i3 + 32 * interp3.size();
    o_ldeg = o_lroot + 32 * kMaxLayers;
    o_wire = o_ldeg + 8 * kMaxLayers;
    const size_t n_b = bx.size(), col_min = ctx->public_column_min ? ctx->public_column_min : kDefaultVerifyColumnMin;
    mat_i2 = n_b > 0 && n_b < col_min && 32 * n_b * n_b <= limit / 4;  // (n_b < 2^21: the product fits)
    for (size_t i = 0; mat_i2 && i < n_b; ++i) mat_i2 = c.pfi[2 * i] < c.n_public;
    plan_i2 = n_b > 0 && n_b >= col_min && n_b < d.steps;
    for (size_t i = 0; plan_i2 && i < n_b; ++i) plan_i2 = c.pfi[2 * i] < c.n_public && c.pfi[2 * i + 1] < d.steps;
    o_mat = (o_wire + (mat_i2 || plan_i2 ? 4 * n_b : 0) + 31) & ~(size_t)31;
    base = align256(o_mat + (mat_i2 ? 32 * n_b * n_b : 0));
  }
  const size_t per_chunk = chain_ok ? std::max<size_t>(1, limit / s.staged()) : batch;
  bool consts_up = false;
  const size_t parse_threads = host_threads();
  for (uint32_t b0 = 0; b0 < batch;) {
    const uint32_t b1 = (uint32_t)std::min<size_t>(batch, (size_t)b0 + per_chunk);
    const size_t n = b1 - b0;
    std::vector<Item> items(n);
    // Two ways to read a chunk's proofs, never nested in one another (the pool runs one call at a time): one
    // proof per host worker, each read serially, or one proof after another, each through the reader's own
    // parallel passes.  Measured (profiles/verify_batch_ab.txt; per proof against the sequential calls): with 16
    // and 64 proofs on 16 workers the first form gives 2.4 / 3.9 x against 1.8 / 2.0 x, with 8 the two tie
    // (1.6 / 1.7 x); with 2 proofs the first leaves 14 workers idle behind two serial parses and loses to the
    // sequential calls (0.6-0.8 x) where the second ties or wins (1.0-1.1 x).  So a chunk of at least half as
    // many proofs as workers is read one per worker, a smaller one through the reader's passes.
    // STARK_VERIFY_BATCH_PARSE=worker|inner forces a form (the A/B's switch).
    static const int forced = [] {
      const char* v = getenv("STARK_VERIFY_BATCH_PARSE");
      return !v ? 0 : strcmp(v, "inner") == 0 ? 1 : strcmp(v, "worker") == 0 ? 2 : 0;
    }();
    // (A handle has no text to read, but the host's transcript of a large chunk is still worth the workers.)
    const bool inner = forced ? forced == 1 : 2 * n < parse_threads;
    if (inner) {
      for (size_t i = 0; i < n; ++i)
        screen(c, d, s, chain_ok, device_tr, public_wires[b0 + i], n_public, source(b0 + i), false, items[i]);
    } else {
      std::atomic<size_t> next{0};
      host_parallel((unsigned)std::min(parse_threads, n), [&](unsigned) {
        for (size_t i; (i = next.fetch_add(1)) < n;)
          screen(c, d, s, chain_ok, device_tr, public_wires[b0 + i], n_public, source(b0 + i), true, items[i]);
      });
    }
    clk.mark("proofs read and screened");
    // I2 per chain proof, as the single call forms it (it may take the device and the pool), unless the matrix
    // launch below forms the chunk's at once.
    std::vector<size_t> chain;
    for (size_t i = 0; i < n; ++i) {
      if (!items[i].chain) continue;
      if (!mat_i2 && !plan_i2) {
        const stark_status st = verify_interp2(ctx, c, items[i].pub, d, bx, items[i].interp2);
        if (st != STARK_OK) return st;
      }
      chain.push_back(i);
    }
    clk.mark("boundary interpolants");
    const size_t nb = chain.size();
    if (nb > 0) {
      const ChunkPlan p = plan_chunk(s, base, nb);
      const ChunkPlan widest = plan_chunk(s, base, std::min<size_t>(per_chunk, batch));
      STARK_TRY(ensure_buf(ctx, ctx->verify_batch, widest.total));
      uint8_t* img = nullptr;
      STARK_TRY(ctx_pinned(ctx, 7, widest.total, (void**)&img));
      uint8_t* const d_img = (uint8_t*)ctx->verify_batch.ptr;
      if (!consts_up) {
        for (size_t j = 0; j < bx.size(); ++j) memcpy(img + 32 * j, bx[j].v, 32);
        for (size_t j = 0; j < interp3.size(); ++j) memcpy(img + o_i3 + 32 * j, interp3[j].v, 32);
        HostFp rt = d.g2;
        uint64_t dg = d.prec;
        for (uint32_t l = 0; l < kMaxLayers; ++l) {
          memcpy(img + o_lroot + 32 * l, rt.v, 32);
          memcpy(img + o_ldeg + 8 * l, &dg, 8);
          rt = F.pow_u64(rt, 4);
          dg = std::max<uint64_t>(dg / 4, 1);
        }
        if (mat_i2 || plan_i2)
          for (size_t j = 0; j < bx.size(); ++j) {
            const uint32_t w = (uint32_t)c.pfi[2 * j];
            memcpy(img + o_wire + 4 * j, &w, 4);
          }
        if (mat_i2) lagrange_basis(bx, img + o_mat);
        if (plan_i2) STARK_TRY(circuit_public_plan(ctx, c, d.g2, d.skips, log_steps, stream, &i2_plan));
      }
      {
        std::atomic<size_t> next{0};
        host_parallel((unsigned)std::min(parse_threads, nb), [&](unsigned) {
          for (size_t k; (k = next.fetch_add(1)) < nb;)
            pack(s, d, c.os, p, nb, k, items[chain[k]], !device_tr, !mat_i2 && !plan_i2, img);
        });
      }
      clk.mark("openings packed");
      if (device_tr) {  // the call's constants once, then the blocks alone: the records are made on the device
        if (!consts_up) STARK_HIP(ctx, hipMemcpyAsync(d_img, img, base, hipMemcpyHostToDevice, stream));
        STARK_HIP(ctx, hipMemcpyAsync(d_img + p.o_blocks, img + p.o_blocks, nb * s.block, hipMemcpyHostToDevice, stream));
      } else {
        const size_t from = consts_up ? base : 0;
        STARK_HIP(ctx, hipMemcpyAsync(d_img + from, img + from, p.o_blocks + nb * s.block - from, hipMemcpyHostToDevice,
                                      stream));
      }
      consts_up = true;
      uint8_t* const d_ok = d_img + p.o_ok;
      auto blocks = [](size_t lanes) { return dim3((unsigned)((lanes + kThreads - 1) / kThreads)); };
      auto u = [](size_t x) { return (uint32_t)x; };
      if (device_tr) {
        TranscriptArgs A;
        A.nb = u(nb);
        A.layers = s.layers;
        A.depth = s.depth;
        A.prec = u(d.prec);
        A.os = u(c.os);
        A.skips = u(d.skips);
        A.o_paths = u(p.o_paths);
        A.o_rows = u(p.o_rows);
        A.o_spots = u(p.o_spots);
        A.o_blocks = u(p.o_blocks);
        A.block = u(s.block);
        A.o_aroot = u(s.o_aroot);
        A.o_consts = u(s.o_consts);
        A.o_i2 = u(s.o_i2);
        A.o_main_leaf = u(s.o_main_leaf);
        A.o_main_nodes = u(s.o_main_nodes);
        A.o_l_leaf = u(s.o_l_leaf);
        A.o_l_nodes = u(s.o_l_nodes);
        for (uint32_t l = 0; l < kMaxLayers; ++l) {
          const bool in = l < s.layers;
          A.o_col_leaf[l] = in ? u(s.o_col_leaf[l]) : 0;
          A.o_col_nodes[l] = in ? u(s.o_col_nodes[l]) : 0;
          A.o_poly_leaf[l] = in ? u(s.o_poly_leaf[l]) : 0;
          A.o_poly_nodes[l] = in ? u(s.o_poly_nodes[l]) : 0;
        }
        A.r2m = to_dev(F.from_canonical(F.one().v));
        A.one = to_dev(F.one());
        hipLaunchKernelGGL(verify_transcript_batch_kernel, dim3((unsigned)nb), dim3(kThreads), 0, stream, d_img, A);
      }
      if (mat_i2)
        hipLaunchKernelGGL(verify_interp2_batch_kernel, dim3((unsigned)((bx.size() + kThreads - 1) / kThreads), (unsigned)nb),
                           dim3(kThreads), 0, stream, d_img, (const fe*)(d_img + o_mat), (const uint32_t*)(d_img + o_wire),
                           u(bx.size()), u(p.o_blocks), u(s.block), u(s.o_pub), u(s.o_i2));
      if (plan_i2) {  // the wires' bytes as they are, gathered through the wire indices; Montgomery images out
        STARK_HIP(ctx, hipGetLastError());
        const InterpValues ys{d_img + p.o_blocks + s.o_pub, s.block, (const uint32_t*)(d_img + o_wire)};
        const InterpOut o{d_img + p.o_blocks + s.o_i2, s.block, true, 0};
        STARK_TRY(interp_plan_apply(ctx, *i2_plan, ys, (uint32_t)nb, o, stream));
      }
      hipLaunchKernelGGL(verify_paths_batch_kernel, blocks(p.n_paths), dim3(kThreads), 0, stream, d_img,
                         (const PathRec*)(d_img + p.o_paths), (uint32_t)p.n_paths, d_ok);
      if (p.n_rows > 0) {
        RowConsts K;
        K.r2m = to_dev(F.from_canonical(F.one().v));  // (R mod p) R = R^2
        K.one = to_dev(F.one());
        K.inv4 = to_dev(F.inv(F.from_u64(4)));
        for (int j = 0; j < 4; ++j) K.quartic[j] = to_dev(F.pow_u64(d.g2, d.prec / 4 * (uint64_t)j));
        hipLaunchKernelGGL(verify_fri_rows_batch_kernel, blocks(p.n_rows), dim3(kThreads), 0, stream, d_img,
                           (const RowRec*)(d_img + p.o_rows), (uint32_t)p.n_rows, (const fe*)(d_img + o_lroot),
                           (const uint64_t*)(d_img + o_ldeg), K, d_ok + p.n_paths);
      }
      {
        SpotConsts K;
        K.r2m = to_dev(F.from_canonical(F.one().v));
        K.one = to_dev(F.one());
        K.g2 = to_dev(d.g2);
        K.x_last = to_dev(x_last);
        for (int j = 0; j < 6; ++j) K.col[j] = c.col[j];
        K.bx = 0;
        K.n_b = (uint32_t)bx.size();
        K.i3 = (uint32_t)o_i3;
        K.n_i3 = (uint32_t)interp3.size();
        K.log_steps = log_steps;
        K.k_mont = c.with_zb;
        hipLaunchKernelGGL(verify_spot_batch_kernel, blocks(p.n_spots), dim3(kThreads), 0, stream, d_img,
                           (const SpotRec*)(d_img + p.o_spots), (uint32_t)p.n_spots, K, d_ok + p.n_paths + p.n_rows);
      }
      STARK_HIP(ctx, hipGetLastError());
      const size_t n_ok = p.n_paths + p.n_rows + p.n_spots;
      STARK_HIP(ctx, hipMemcpyAsync(img + p.o_ok, d_ok, n_ok, hipMemcpyDeviceToHost, stream));
      clk.mark("upload, three launches, download enqueued");
      // The Last layers beside the device work, one proof per task (fri.rs:346-403 with what the Middle layers
      // leave: the last root2, root^(4^layers), the degree bound over 4^layers).
      {
        HostFp rt = d.g2;
        size_t max_deg = d.prec / 4;
        for (uint32_t l = 0; l < s.layers; ++l) {
          rt = F.pow_u64(rt, 4);
          max_deg /= 4;
        }
        std::atomic<size_t> next{0};
        host_parallel((unsigned)std::min(parse_threads, nb), [&](unsigned) {
          for (size_t k; (k = next.fetch_add(1)) < nb;) {
            Item& it = items[chain[k]];
            const uint8_t* m_root = s.layers ? it.pr.fri[s.layers - 1].root2 : it.pr.l_root;
            it.last_ok = fri_last_check(it.pr.fri.back(), m_root, rt, max_deg, (uint32_t)d.skips) == STARK_OK;
          }
        });
      }
      clk.mark("Last layers (host)");
      STARK_HIP(ctx, hipStreamSynchronize(stream));
      clk.mark("device joined");
      // A chain proof passed stark_verify_r1cs_circuit's argument checks, parsed, has public_wires[0] = 1 and
      // the exact structure the circuit implies, and the sampler took each of its roots.  For such a proof the
      // single-proof verifier has no STARK_ERR_BAD_ARG left to return (every one of verify_fri's and
      // verify_r1cs's is a shape or sampler condition screened above), so in the reference's order it returns
      // STARK_ERR_CHECK at its first failed check and STARK_OK when none fails: the status is STARK_OK iff every
      // path, row and spot byte and the Last layer's check hold, whatever order they were evaluated in.
      const uint8_t* ok = img + p.o_ok;
      for (size_t k = 0; k < nb; ++k) {
        Item& it = items[chain[k]];
        it.reasons = reasons_of(s, p, nb, k, ok) | (it.last_ok ? 0 : STARK_VERIFY_FAIL_FRI_LAST);
        it.st = it.reasons ? STARK_ERR_CHECK : STARK_OK;
      }
    }
    // Everything else that parsed: the single-proof verifier's status.
    for (size_t i = 0; i < n; ++i) {
      Item& it = items[i];
      if (it.fallback) {
        it.st = verify_r1cs(ctx, c, public_wires[b0 + i], n_public, it.pr);
        it.reasons = it.st == STARK_OK ? 0 : STARK_VERIFY_FAIL_SINGLE;
      }
      statuses[b0 + i] = it.st;
      reasons[b0 + i] = it.reasons;
    }
    clk.mark("statuses composed");
    b0 = b1;
  }
  return STARK_OK;
}

// ---- standalone FRI proofs: stark_verify_low_degree_batch ----
//
// verify_low_degree_proof (fri.rs:226-404) for many stark_fri_proof handles of one (root of unity, degree bound,
// exclusion).  The chain is the one above without a circuit: the host views each handle's vectors (view_fri),
// screens its structure against what prove_low_degree makes of the parameters (fri_in_shape), samples each
// layer's rows from the roots as given and packs the openings with the same PathRec / RowRec records; one upload,
// verify_paths_batch_kernel, verify_fri_rows_batch_kernel, the Last element's kernels below, one download of the
// ok bytes.  Every other proof goes to verify_fri_single, so each status is stark_verify_low_degree_proof's.
//
// A handle is untrusted input (stark_fri_proof_from_parts makes one of anything).  As above, nothing a handle
// supplies is used as a length or an offset on the device: every offset in a record comes from the parameters'
// shape (FriShape), every index from the sampler below its tree's size, and the Last kernels take the count of
// values, the interpolation positions and the rest positions from the parameters alone.  A handle's bytes are only
// ever hashed or multiplied.
//
// The Last element (fri.rs:346-403; fri_last_check): all proofs of a call share w = root^(4^L), n_last, the degree
// bound m and the exclusion, hence the admissible positions: the first m are the interpolation points x_i, the
// others the rest points x_r.  "The values at the rest points lie on the polynomial through the first m" is
//   y_r = sum_i M[r][i] y_i,   M[r][i] = L_i(x_r) = w_i prod_(j != i) (x_r - x_j),   w_i = 1 / prod_(j != i) (x_i - x_j),
// with one matrix for the whole call: verify_last_matrix_kernel forms it once (the m weights and points come from
// the host: m <= 16 for a proof of the chain), verify_last_degree_batch_kernel applies it, one lane per (proof,
// rest point).  The field arithmetic is exact, so the outcome is eval_poly(lagrange_interp(..)) == y_r's.

namespace {

// The k-th position that is no multiple of excl (excl >= 2), or k itself without an exclusion (fri.rs:377-385).
__host__ __device__ inline uint64_t admissible_pos(uint64_t k, uint32_t excl) {
  return excl ? k + 1 + k / (excl - 1) : k;
}

// What every proof of the call shares of its Last element.
struct LastArgs {
  uint32_t n_last, m, n_rest, excl;
  uint32_t o_xi, o_mat;  // the m interpolation points (Montgomery images), the matrix [i][r] (m x n_rest)
  fe w, r2m, one;        // the Last element's root of unity, R^2, 1
};

// The check matrix, one lane per (i, r): Mt[i n_rest + r] = w_i prod_(j != i) (x_r - x_j), x_r = w^pos(m + r)
// (pos < n_last: the host counted the admissible positions).  A lane's i is uniform over a wave but at a row's end.
__global__ __launch_bounds__(kThreads) void verify_last_matrix_kernel(uint8_t* arena, const fe* __restrict__ wi,
                                                                       LastArgs A) {
  const uint32_t g = blockIdx.x * kThreads + threadIdx.x;
  if (g >= A.m * A.n_rest) return;
  const uint32_t i = g / A.n_rest, r = g % A.n_rest;
  const fe* xi = reinterpret_cast<const fe*>(arena + A.o_xi);
  const fe x = fe_pow(A.w, admissible_pos((uint64_t)A.m + r, A.excl), A.one);
  fe acc = fe_load(wi + i);
  for (uint32_t j = 0; j < A.m; ++j) {
    const fe t = fe_mul(acc, fe_sub(x, fe_load(xi + j)));
    if (j != i) acc = t;
  }
  fe_store(reinterpret_cast<fe*>(arena + A.o_mat) + g, acc);
}

// One lane per (proof, rest point): sum_i Mt[i][r] y_i against y_r on Montgomery images, the y's being
// from_bytes_le of the raw 32 bytes (any value below 2^256: arena_mont).  Proof k's values are the n_last x 32 B
// at o_last + 32 k n_last; a wave's lanes share the proof (but at a proof's end) and read the matrix side by side.
__global__ __launch_bounds__(kThreads) void verify_last_degree_batch_kernel(const uint8_t* __restrict__ arena,
                                                                             uint64_t o_last, uint32_t nb, LastArgs A,
                                                                             uint8_t* __restrict__ ok) {
  const uint64_t g = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (g >= (uint64_t)nb * A.n_rest) return;
  const uint32_t k = (uint32_t)(g / A.n_rest), r = (uint32_t)(g % A.n_rest);
  const uint8_t* vals = arena + o_last + (uint64_t)32 * k * A.n_last;
  const fe* mt = reinterpret_cast<const fe*>(arena + A.o_mat);
  auto y_at = [&](uint64_t pos) { return fe_mul(fe_load(reinterpret_cast<const fe*>(vals + 32 * pos)), A.r2m); };
  fe acc = fe_zero();
  for (uint32_t i = 0; i < A.m; ++i)
    acc = fe_add(acc, fe_mul(fe_load(mt + (size_t)i * A.n_rest + r), y_at(admissible_pos(i, A.excl))));
  ok[g] = fe_eq(acc, y_at(admissible_pos((uint64_t)A.m + r, A.excl)));
}

// The tree over a proof's raw Last values (fri.rs:367-372) against the root the layers before it leave, one
// workgroup per proof through LDS: leaf digests, then one level per step, two pair hashes per lane at the widest.
// Taken up to kLastLdsMax = 1,024 values (the common Lasts hold 32 or 64): that many digests are 32 KB of LDS, and
// a wider Last in one workgroup would leave its 4 waves hashing a thousand leaves each while the other CUs idle --
// from there on the Merkle forest build (merkle.hip), which spreads every level over the grid, makes the trees and
// verify_last_root_cmp_kernel compares the roots.
constexpr uint32_t kLastLdsMax = 1024, kLastThreads = 256;
__global__ __launch_bounds__(kLastThreads) void verify_last_root_batch_kernel(const uint8_t* __restrict__ arena,
                                                                              uint64_t o_last, uint32_t n_last,
                                                                              uint32_t o_blocks, uint32_t block,
                                                                              uint32_t o_root, uint8_t* __restrict__ ok) {
  __shared__ __attribute__((aligned(16))) Digest lds[kLastLdsMax];
  const uint32_t k = blockIdx.x, t = threadIdx.x;
  const uint8_t* vals = arena + o_last + (uint64_t)32 * k * n_last;
  for (uint32_t i = t; i < n_last; i += kLastThreads) lds[i] = hash_leaf32(vals + 32 * i);
  __syncthreads();
  for (uint32_t width = n_last / 2; width >= 1; width /= 2) {  // (width <= kLastLdsMax / 2 = 2 kLastThreads)
    const uint32_t i0 = t, i1 = t + kLastThreads;
    Digest r0, r1;
    if (i0 < width) r0 = hash_pair(lds[2 * i0], lds[2 * i0 + 1]);
    if (i1 < width) r1 = hash_pair(lds[2 * i1], lds[2 * i1 + 1]);
    __syncthreads();
    if (i0 < width) lds[i0] = r0;
    if (i1 < width) lds[i1] = r1;
    __syncthreads();
  }
  if (t == 0) {
    const Digest want = load_digest(reinterpret_cast<const Digest*>(arena + o_blocks + (size_t)k * block + o_root));
    uint32_t diff = 0;
#pragma unroll
    for (int w = 0; w < 8; ++w) diff |= lds[0].h[w] ^ want.h[w];
    ok[k] = diff == 0;
  }
}

// The wide route's compare: tree k's root in the forest against the root in proof k's block, one lane per proof.
__global__ __launch_bounds__(kThreads) void verify_last_root_cmp_kernel(const uint8_t* __restrict__ arena,
                                                                         const uint32_t* __restrict__ nodes,
                                                                         uint64_t stride_words, uint64_t root_word,
                                                                         uint32_t nb, uint32_t o_blocks, uint32_t block,
                                                                         uint32_t o_root, uint8_t* __restrict__ ok) {
  const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= nb) return;
  const Digest got = load_digest(reinterpret_cast<const Digest*>(nodes + k * stride_words + root_word));
  const Digest want = load_digest(reinterpret_cast<const Digest*>(arena + o_blocks + (size_t)k * block + o_root));
  uint32_t diff = 0;
#pragma unroll
  for (int w = 0; w < 8; ++w) diff |= got.h[w] ^ want.h[w];
  ok[k] = diff == 0;
}

// What prove_low_degree makes of (n, max_deg_plus_1, excl) (fri.rs:46-224; fri.hip fri_check), and where a
// proof's parts are in its block: the roots first -- the caller's merkle_roots[b], then each layer's root2 --
// then each layer's openings.  The Last values of a chunk are side by side after the blocks (the forest build
// takes contiguous trees).
struct FriShape {
  uint32_t depth = 0, layers = 0;  // log2 n; Middle layers
  uint64_t n = 0, n_last = 0, m = 0, n_adm = 0, n_rest = 0;  // m: the bound the Last element is checked against
  bool last_refused = false;  // the parameters alone refuse every Last (fri.rs:348-351, :359, split_off)
  bool wide = false;          // n_last > kLastLdsMax
  size_t o_col_leaf[kMaxLayers], o_col_nodes[kMaxLayers], o_poly_leaf[kMaxLayers], o_poly_nodes[kMaxLayers];
  size_t block = 0;
  uint32_t col_depth(uint32_t l) const { return depth - 2 * l - 2; }
  uint32_t poly_depth(uint32_t l) const { return depth - 2 * l; }
  size_t o_root(uint32_t slot) const { return 32 * (size_t)slot; }  // slot 0: merkle_roots[b]; 1 + l: root2 of layer l
  size_t paths() const { return (size_t)layers * (kRows + kRows * kPolyPer); }
  size_t rows() const { return (size_t)layers * kRows; }
  size_t last_lanes() const { return last_refused ? 0 : 1 + n_rest; }  // ok bytes: the root, then each rest point
  // a proof's block, Last values (with the wide route's tree nodes), records and ok bytes
  size_t staged() const { return block + 32 * n_last * (wide ? 3 : 1) + 32 * (paths() + rows()) + paths() + rows() + last_lanes(); }
  size_t matrix_bytes() const { return last_refused ? 0 : 32 * m * n_rest; }
};

// get_pseudorandom_indices takes this modulus and exclusion (fri/src/utils.rs:88, :101; api.hip).
bool sampler_takes(uint64_t modulus, uint32_t excl) {
  if (modulus >= ((uint64_t)1 << 24) || excl == 1) return false;
  if (excl == 0) return modulus > 0;
  return modulus * (excl - 1) <= 0xFFFFFFFFull && modulus * (excl - 1) / excl > 0;
}

// False where the chain cannot take the parameters at all (every proof then goes to the single-proof verifier):
// n = the root's order (a power of two, at most 2^28).
bool plan_fri_shape(uint64_t n, size_t max_deg_plus_1, uint32_t excl, size_t limit, FriShape& s) {
  if (excl == 1 || n == 0) return false;
  s.n = n;
  while (((uint64_t)1 << s.depth) < n) ++s.depth;
  uint64_t m = n;
  size_t deg = max_deg_plus_1;
  while (deg > 16) {
    if (m < 8 || !sampler_takes(m / 4, excl)) return false;
    m /= 4;
    deg /= 4;
    if (++s.layers + 1 > kMaxLayers) return false;
  }
  s.n_last = m;
  s.m = deg;
  s.n_adm = excl ? m - (m + excl - 1) / excl : m;
  s.last_refused = s.m < 16 / 2 || s.n_last <= s.m || s.n_adm < s.m;
  s.n_rest = s.last_refused ? 0 : s.n_adm - s.m;
  s.wide = s.n_last > kLastLdsMax;
  if (s.matrix_bytes() > limit / 4) return false;
  size_t at = 32 * (1 + (size_t)s.layers);
  auto take = [&](size_t bytes) {
    const size_t o = at;
    at += bytes;
    return o;
  };
  for (uint32_t l = 0; l < s.layers; ++l) {
    s.o_col_leaf[l] = take((size_t)kRows * 32);
    s.o_col_nodes[l] = take((size_t)kRows * 32 * s.col_depth(l));
    s.o_poly_leaf[l] = take((size_t)kRows * kPolyPer * 32);
    s.o_poly_nodes[l] = take((size_t)kRows * kPolyPer * 32 * s.poly_depth(l));
  }
  s.block = at;
  // (the records hold 32-bit offsets: a chunk of one proof must stay under them with the call's constants)
  return s.matrix_bytes() + s.staged() < ((size_t)3 << 30);
}

// The handle's structure is exactly what the parameters imply: every length the packing and the kernels assume.
bool fri_in_shape(const std::vector<FriIn>& fri, const FriShape& s) {
  if (fri.size() != (size_t)s.layers + 1) return false;
  for (uint32_t l = 0; l < s.layers; ++l) {
    const FriIn& f = fri[l];
    if (f.last || !branches_are(f.col, kRows, 32, s.col_depth(l)) ||
        !branches_are(f.poly, kRows * kPolyPer, 32, s.poly_depth(l)))
      return false;
  }
  const FriIn& last = fri.back();
  if (!last.last || last.last_vals.size() != s.n_last) return false;
  for (const std::vector<uint8_t>& v : last.last_vals)
    if (v.size() != 32) return false;
  return true;
}

struct FriItem {
  std::vector<FriIn> fri;
  bool chain = false, fallback = false, last_ok = false;
  stark_status st = STARK_OK;
  uint32_t reasons = 0;
  std::vector<std::vector<size_t>> ys;  // per Middle layer
};

struct FriChunkPlan {
  size_t o_paths, o_rows, o_blocks, o_last, o_ok, total;
  size_t n_paths, n_rows, n_last_ok;
};
FriChunkPlan plan_fri_chunk(const FriShape& s, size_t base, size_t nb, bool device_last) {
  FriChunkPlan p;
  p.n_paths = nb * s.paths();
  p.n_rows = nb * s.rows();
  p.n_last_ok = device_last ? nb * s.last_lanes() : 0;
  p.o_paths = base;
  p.o_rows = p.o_paths + 32 * p.n_paths;
  p.o_blocks = p.o_rows + 32 * p.n_rows;
  p.o_last = p.o_blocks + nb * s.block;
  p.o_ok = align256(p.o_last + (device_last && !s.last_refused ? nb * 32 * s.n_last : 0));
  p.total = p.o_ok + align256(p.n_paths + p.n_rows + p.n_last_ok);
  return p;
}

// Chain proof k of nb: its block (roots first), its records (class-major per layer: the polynomial openings,
// then the column openings; rows layer-major) and, for the device's Last check, its Last values.
void pack_fri(const FriShape& s, const FriChunkPlan& p, size_t nb, size_t k, const uint8_t* merkle_root,
              const FriItem& it, bool with_last, uint8_t* img) {
  const size_t blk = p.o_blocks + k * s.block;
  uint8_t* const b = img + blk;
  memcpy(b, merkle_root, 32);
  for (uint32_t l = 0; l < s.layers; ++l) {
    memcpy(b + s.o_root(1 + l), it.fri[l].root2, 32);
    put_branches(b + s.o_col_leaf[l], b + s.o_col_nodes[l], it.fri[l].col);
    put_branches(b + s.o_poly_leaf[l], b + s.o_poly_nodes[l], it.fri[l].poly);
  }
  if (with_last) {
    uint8_t* v = img + p.o_last + k * 32 * s.n_last;
    for (const std::vector<uint8_t>& x : it.fri.back().last_vals) {
      memcpy(v, x.data(), 32);
      v += 32;
    }
  }
  PathRec* paths = reinterpret_cast<PathRec*>(img + p.o_paths);
  RowRec* rows = reinterpret_cast<RowRec*>(img + p.o_rows);
  auto u = [](size_t x) { return (uint32_t)x; };
  size_t cls = 0;
  uint64_t deg = s.n;
  for (uint32_t l = 0; l < s.layers; ++l, deg /= 4) {
    const size_t root_l = blk + s.o_root(l), root2 = blk + s.o_root(1 + l);
    const uint32_t pd = s.poly_depth(l), cd = s.col_depth(l);
    for (uint32_t i = 0; i < kRows; ++i)
      for (uint32_t j = 0; j < kPolyPer; ++j) {
        const size_t q = kPolyPer * i + j;
        paths[cls + k * kRows * kPolyPer + q] = PathRec{u(root_l), u(blk + s.o_poly_leaf[l] + 32 * q),
                                                        u(blk + s.o_poly_nodes[l] + 32 * pd * q),
                                                        u(j * (deg / 4) + it.ys[l][i]), 32, pd, 0, 0};
      }
    cls += nb * kRows * kPolyPer;
    for (uint32_t i = 0; i < kRows; ++i) {
      paths[cls + k * kRows + i] = PathRec{u(root2), u(blk + s.o_col_leaf[l] + 32 * i),
                                           u(blk + s.o_col_nodes[l] + 32 * cd * i), u(it.ys[l][i]), 32, cd, 0, 0};
      rows[((size_t)l * nb + k) * kRows + i] = RowRec{u(root_l), u(blk + s.o_col_leaf[l] + 32 * i),
                                                      u(blk + s.o_poly_leaf[l] + 32 * kPolyPer * i), u(it.ys[l][i]), l, 0, 0, 0};
    }
    cls += nb * kRows;
  }
}

}  // namespace

// statuses / reasons of entries [0, batch) (both non-null here).
static stark_status verify_fri_batch(stark_ctx* ctx, const uint8_t* merkle_roots, const uint64_t root_of_unity[4],
                                     const stark_fri_proof* const* proofs, uint32_t batch, size_t max_deg_plus_1,
                                     uint32_t excl, stark_status* statuses, uint32_t* reasons) {
  const FieldHost& F = FieldHost::get();
  PhaseClock clk("verify_low_degree_batch");
  const HostFp root = F.from_canonical(root_of_unity);
  // The root's order as verify_fri finds it: a power of two up to 2^28, else no proof of the call has a chain.
  uint64_t n = 1;
  for (HostFp t = root; n <= ((uint64_t)1 << 28) && !FieldHost::eq(t, F.one()); t = F.mul(t, t)) n *= 2;
  const size_t limit = std::min<size_t>(ctx->verify_batch_limit ? ctx->verify_batch_limit : kDefaultVerifyBatchLimit,
                                        (size_t)3 << 30);
  FriShape s;
  const bool chain_ok = n <= ((uint64_t)1 << 28) && plan_fri_shape(n, max_deg_plus_1, excl, limit, s);
  const bool device_last = (ctx->verify_batch_last ? ctx->verify_batch_last : kDefaultVerifyLast) == 2;
  const bool last_dev = device_last && chain_ok && !s.last_refused;  // the Last kernels run
  hipStream_t stream = ctx->stream;
  // The call's constants at the image's start: the layers' roots of unity and sizes, the Last element's m
  // interpolation points and weights, then the check matrix (made on the device, never uploaded).
  const size_t o_lroot = 0, o_ldeg = o_lroot + 32 * kMaxLayers, o_xi = o_ldeg + 8 * kMaxLayers, o_wi = o_xi + 32 * 16,
               o_mat = o_wi + 32 * 16;
  const size_t base = chain_ok ? align256(o_mat + (last_dev ? s.matrix_bytes() : 0)) : 0;
  HostFp w_last = root;  // root^(4^layers): the Last element's root of unity
  if (chain_ok)
    for (uint32_t l = 0; l < s.layers; ++l) w_last = F.pow_u64(w_last, 4);
  const size_t per_chunk = chain_ok ? std::max<size_t>(1, (limit > base ? limit - base : 0) / s.staged()) : batch;
  bool consts_up = false;
  const size_t workers = host_threads();
  for (uint32_t b0 = 0; b0 < batch;) {
    const uint32_t b1 = (uint32_t)std::min<size_t>(batch, (size_t)b0 + per_chunk);
    const size_t cn = b1 - b0;
    std::vector<FriItem> items(cn);
    // View, screen and sample each entry (the indices come from the roots as given, per proof on the workers).
    auto screen_one = [&](size_t i) {
      FriItem& it = items[i];
      const stark_fri_proof* h = proofs[b0 + i];
      if (!h || !view_fri(*h, it.fri)) {
        it.st = STARK_ERR_BAD_ARG;
        it.reasons = STARK_VERIFY_FAIL_SINGLE;
        return;
      }
      it.fallback = true;
      if (!chain_ok || !fri_in_shape(it.fri, s)) return;
      it.ys.resize(s.layers);
      uint64_t deg = s.n;
      for (uint32_t l = 0; l < s.layers; ++l, deg /= 4)
        if (!sampler(it.fri[l].root2, deg / 4, kRows, excl, it.ys[l])) return;
      it.fallback = false;
      it.chain = true;
    };
    if (2 * cn < workers) {
      for (size_t i = 0; i < cn; ++i) screen_one(i);
    } else {
      std::atomic<size_t> next{0};
      host_parallel((unsigned)std::min(workers, cn), [&](unsigned) {
        for (size_t i; (i = next.fetch_add(1)) < cn;) screen_one(i);
      });
    }
    clk.mark("handles viewed and screened");
    std::vector<size_t> chain;
    for (size_t i = 0; i < cn; ++i)
      if (items[i].chain) chain.push_back(i);
    const size_t nb = chain.size();
    if (nb > 0) {
      const FriChunkPlan p = plan_fri_chunk(s, base, nb, device_last);
      const FriChunkPlan widest = plan_fri_chunk(s, base, std::min<size_t>(per_chunk, batch), device_last);
      STARK_TRY(ensure_buf(ctx, ctx->verify_batch, widest.total));
      uint8_t* img = nullptr;
      STARK_TRY(ctx_pinned(ctx, 7, widest.total, (void**)&img));
      uint8_t* const d_img = (uint8_t*)ctx->verify_batch.ptr;
      std::vector<HostFp> xi, wi;
      if (!consts_up) {
        HostFp rt = root;
        uint64_t dg = s.n;
        for (uint32_t l = 0; l < kMaxLayers; ++l) {
          memcpy(img + o_lroot + 32 * l, rt.v, 32);
          memcpy(img + o_ldeg + 8 * l, &dg, 8);
          rt = F.pow_u64(rt, 4);
          dg = std::max<uint64_t>(dg / 4, 1);
        }
        memset(img + o_xi, 0, 2 * 32 * 16);
        if (last_dev) {  // x_i = w^pos(i), w_i = 1 / prod_(j != i) (x_i - x_j), i < m <= 16
          for (uint64_t i = 0; i < s.m; ++i) xi.push_back(F.pow_u64(w_last, admissible_pos(i, excl)));
          // (one field inversion for all m denominators: the products before each, the inverse of the whole, then
          // back down -- an inversion is some 380 products, sixteen of them were most of the call's fixed cost)
          std::vector<HostFp> den(s.m, F.one()), before(s.m + 1, F.one());
          for (uint64_t i = 0; i < s.m; ++i) {
            for (uint64_t j = 0; j < s.m; ++j)
              if (j != i) den[i] = F.mul(den[i], F.sub(xi[i], xi[j]));  // (distinct powers below the order: not 0)
            before[i + 1] = F.mul(before[i], den[i]);
          }
          HostFp inv_rest = F.inv(before[s.m]);
          wi.assign(s.m, F.one());
          for (uint64_t i = s.m; i-- > 0;) {
            wi[i] = F.mul(inv_rest, before[i]);
            inv_rest = F.mul(inv_rest, den[i]);
          }
          for (uint64_t i = 0; i < s.m; ++i) {
            memcpy(img + o_xi + 32 * i, xi[i].v, 32);
            memcpy(img + o_wi + 32 * i, wi[i].v, 32);
          }
        }
      }
      {
        std::atomic<size_t> next{0};
        host_parallel((unsigned)std::min(workers, nb), [&](unsigned) {
          for (size_t k; (k = next.fetch_add(1)) < nb;)
            pack_fri(s, p, nb, k, merkle_roots + 32 * (size_t)(b0 + chain[k]), items[chain[k]], last_dev, img);
        });
      }
      clk.mark("openings packed");
      {
        // (the matrix region [o_mat, base) is the device's own: the upload goes around it)
        if (!consts_up) STARK_HIP(ctx, hipMemcpyAsync(d_img, img, o_mat, hipMemcpyHostToDevice, stream));
        const size_t end = last_dev ? p.o_last + nb * 32 * s.n_last : p.o_blocks + nb * s.block;
        STARK_HIP(ctx, hipMemcpyAsync(d_img + base, img + base, end - base, hipMemcpyHostToDevice, stream));
      }
      auto blocks = [](size_t lanes) { return dim3((unsigned)((lanes + kThreads - 1) / kThreads)); };
      auto u = [](size_t x) { return (uint32_t)x; };
      LastArgs A{};
      if (last_dev) {
        A.n_last = u(s.n_last);
        A.m = u(s.m);
        A.n_rest = u(s.n_rest);
        A.excl = excl;
        A.o_xi = u(o_xi);
        A.o_mat = u(o_mat);
        A.w = to_dev(w_last);
        A.r2m = to_dev(F.from_canonical(F.one().v));
        A.one = to_dev(F.one());
        if (!consts_up && s.n_rest > 0)
          hipLaunchKernelGGL(verify_last_matrix_kernel, blocks(s.m * s.n_rest), dim3(kThreads), 0, stream, d_img,
                             (const fe*)(d_img + o_wi), A);
      }
      consts_up = true;
      uint8_t* const d_ok = d_img + p.o_ok;
      if (p.n_paths > 0)
        hipLaunchKernelGGL(verify_paths_batch_kernel, blocks(p.n_paths), dim3(kThreads), 0, stream, d_img,
                           (const PathRec*)(d_img + p.o_paths), (uint32_t)p.n_paths, d_ok);
      if (p.n_rows > 0) {
        RowConsts K;
        K.r2m = to_dev(F.from_canonical(F.one().v));  // (R mod p) R = R^2
        K.one = to_dev(F.one());
        K.inv4 = to_dev(F.inv(F.from_u64(4)));
        for (int j = 0; j < 4; ++j) K.quartic[j] = to_dev(F.pow_u64(root, s.n / 4 * (uint64_t)j));
        hipLaunchKernelGGL(verify_fri_rows_batch_kernel, blocks(p.n_rows), dim3(kThreads), 0, stream, d_img,
                           (const RowRec*)(d_img + p.o_rows), (uint32_t)p.n_rows, (const fe*)(d_img + o_lroot),
                           (const uint64_t*)(d_img + o_ldeg), K, d_ok + p.n_paths);
      }
      STARK_HIP(ctx, hipGetLastError());
      if (last_dev) {
        // ok bytes of the Last elements: nb roots, then nb x n_rest rest points.
        uint8_t* const d_root_ok = d_ok + p.n_paths + p.n_rows;
        if (!s.wide) {
          hipLaunchKernelGGL(verify_last_root_batch_kernel, dim3((unsigned)nb), dim3(kLastThreads), 0, stream, d_img,
                             (uint64_t)p.o_last, u(s.n_last), u(p.o_blocks), u(s.block), u(s.o_root(s.layers)),
                             d_root_ok);
        } else {
          if (!ctx->verify_forest) STARK_TRY(stark_merkle_forest_new(ctx, &ctx->verify_forest));
          STARK_TRY(forest_build(ctx, ctx->verify_forest, d_img + p.o_last, s.n_last, 32, (uint32_t)nb, stream));
          uint64_t stride_words = 0, root_word = 0;
          const uint32_t* nodes = forest_nodes_dev(ctx->verify_forest, &stride_words, &root_word);
          hipLaunchKernelGGL(verify_last_root_cmp_kernel, blocks(nb), dim3(kThreads), 0, stream, d_img, nodes,
                             stride_words, root_word, u(nb), u(p.o_blocks), u(s.block), u(s.o_root(s.layers)),
                             d_root_ok);
        }
        if (s.n_rest > 0)
          hipLaunchKernelGGL(verify_last_degree_batch_kernel, blocks(nb * s.n_rest), dim3(kThreads), 0, stream, d_img,
                             (uint64_t)p.o_last, u(nb), A, d_root_ok + nb);
        STARK_HIP(ctx, hipGetLastError());
      }
      const size_t n_ok = p.n_paths + p.n_rows + p.n_last_ok;
      if (n_ok > 0) STARK_HIP(ctx, hipMemcpyAsync(img + p.o_ok, d_ok, n_ok, hipMemcpyDeviceToHost, stream));
      clk.mark("upload, launches, download enqueued");
      if (!device_last && !s.last_refused) {
        // The Last elements beside the device work, one proof per task (fri_last_check with what the Middle layers
        // leave: the last root2 -- the caller's root without layers --, root^(4^layers), the bound over 4^layers).
        std::atomic<size_t> next{0};
        host_parallel((unsigned)std::min(workers, nb), [&](unsigned) {
          for (size_t k; (k = next.fetch_add(1)) < nb;) {
            FriItem& it = items[chain[k]];
            const uint8_t* m_root =
                s.layers ? it.fri[s.layers - 1].root2 : merkle_roots + 32 * (size_t)(b0 + chain[k]);
            it.last_ok = fri_last_check(it.fri.back(), m_root, w_last, s.m, excl) == STARK_OK;
          }
        });
        clk.mark("Last elements (host)");
      }
      STARK_HIP(ctx, hipStreamSynchronize(stream));
      clk.mark("device joined");
      // A chain proof has the exact structure the parameters imply and the sampler took each of its roots, so the
      // single-proof verifier has no STARK_ERR_BAD_ARG left for it (each of verify_fri's is a shape or order
      // condition screened above): it returns STARK_ERR_CHECK at its first failed check and STARK_OK when none
      // fails, so the status is STARK_OK iff every path and row byte and the Last element's check hold.
      const uint8_t* ok = img + p.o_ok;
      auto any_bad = [&](size_t first, size_t count) {
        for (size_t i = 0; i < count; ++i)
          if (!ok[first + i]) return true;
        return false;
      };
      for (size_t k = 0; k < nb; ++k) {
        FriItem& it = items[chain[k]];
        uint32_t why = 0;
        size_t cls = 0;
        for (uint32_t l = 0; l < s.layers; ++l) {
          if (any_bad(cls + k * kRows * kPolyPer, kRows * kPolyPer)) why |= STARK_VERIFY_FAIL_FRI_PATHS;
          cls += nb * kRows * kPolyPer;
          if (any_bad(cls + k * kRows, kRows)) why |= STARK_VERIFY_FAIL_FRI_PATHS;
          cls += nb * kRows;
          if (any_bad(p.n_paths + ((size_t)l * nb + k) * kRows, kRows)) why |= STARK_VERIFY_FAIL_FRI_ROWS;
        }
        bool last_ok = false;  // (the parameters alone may refuse every Last)
        if (!s.last_refused) {
          const size_t at = p.n_paths + p.n_rows;
          last_ok = device_last ? !any_bad(at + k, 1) && !any_bad(at + nb + k * s.n_rest, s.n_rest) : it.last_ok;
        }
        if (!last_ok) why |= STARK_VERIFY_FAIL_FRI_LAST;
        it.reasons = why;
        it.st = why ? STARK_ERR_CHECK : STARK_OK;
      }
    }
    // Everything else that has a handle: the single-proof verifier's status.
    for (size_t i = 0; i < cn; ++i) {
      FriItem& it = items[i];
      if (it.fallback) {
        it.st = verify_fri_single(merkle_roots + 32 * (size_t)(b0 + i), root, it.fri, max_deg_plus_1, excl);
        it.reasons = it.st == STARK_OK ? 0 : STARK_VERIFY_FAIL_SINGLE;
      }
      statuses[b0 + i] = it.st;
      reasons[b0 + i] = it.reasons;
    }
    clk.mark("statuses composed");
    b0 = b1;
  }
  return STARK_OK;
}

}  // namespace stark

using namespace stark;

extern "C" {

stark_status stark_verify_low_degree_batch(stark_ctx* ctx, const uint8_t* merkle_roots, const uint64_t root_of_unity[4],
                                           const stark_fri_proof* const* proofs, uint32_t batch, size_t max_deg_plus_1,
                                           uint32_t exclude_multiples_of, stark_status* statuses, uint32_t* reasons) {
  if (!ctx || !merkle_roots || !root_of_unity || !proofs || batch > 65535) return STARK_ERR_BAD_ARG;
  if (batch == 0) return STARK_OK;  // (nothing to read, the handles included)
  STARK_HIP(ctx, hipSetDevice(ctx->device));
  std::vector<stark_status> sts(batch, STARK_OK);
  std::vector<uint32_t> why(batch, 0);
  STARK_TRY(verify_fri_batch(ctx, merkle_roots, root_of_unity, proofs, batch, max_deg_plus_1, exclude_multiples_of,
                             sts.data(), why.data()));
  if (reasons) memcpy(reasons, why.data(), sizeof(uint32_t) * batch);
  if (statuses) {
    memcpy(statuses, sts.data(), sizeof(stark_status) * batch);
    return STARK_OK;
  }
  for (uint32_t b = 0; b < batch; ++b)
    if (sts[b] != STARK_OK) return sts[b];
  return STARK_OK;
}

stark_status stark_verify_r1cs_circuit_batch(stark_ctx* ctx, const stark_r1cs_circuit* circuit,
                                             const uint8_t* const* public_wires, size_t n_public,
                                             const char* const* proof_json, const size_t* json_lens, uint32_t batch,
                                             stark_status* statuses, uint32_t* reasons) {
  if (!ctx || !circuit || !public_wires || !proof_json || !json_lens || n_public == 0 || batch > 65535)
    return STARK_ERR_BAD_ARG;
  if (batch == 0) return STARK_OK;  // (nothing to read, the handles included)
  if (circuit->ctx != ctx || circuit->c.world != 1) return STARK_ERR_BAD_ARG;
  STARK_HIP(ctx, hipSetDevice(ctx->device));
  std::vector<stark_status> sts(batch, STARK_OK);
  std::vector<uint32_t> why(batch, 0);
  STARK_TRY(verify_r1cs_batch(ctx, circuit->c, public_wires, n_public, proof_json, json_lens, nullptr, batch,
                              sts.data(), why.data()));
  if (reasons) memcpy(reasons, why.data(), sizeof(uint32_t) * batch);
  if (statuses) {
    memcpy(statuses, sts.data(), sizeof(stark_status) * batch);
    return STARK_OK;
  }
  for (uint32_t b = 0; b < batch; ++b)
    if (sts[b] != STARK_OK) return sts[b];
  return STARK_OK;
}

stark_status stark_verify_r1cs_circuit_batch_proofs(stark_ctx* ctx, const stark_r1cs_circuit* circuit,
                                                    const uint8_t* const* public_wires, size_t n_public,
                                                    const stark_r1cs_proof* const* proofs, uint32_t batch,
                                                    stark_status* statuses, uint32_t* reasons) {
  if (!ctx || !circuit || !public_wires || !proofs || n_public == 0 || batch > 65535) return STARK_ERR_BAD_ARG;
  if (batch == 0) return STARK_OK;  // (nothing to read, the handles included)
  if (circuit->ctx != ctx || circuit->c.world != 1) return STARK_ERR_BAD_ARG;
  STARK_HIP(ctx, hipSetDevice(ctx->device));
  std::vector<stark_status> sts(batch, STARK_OK);
  std::vector<uint32_t> why(batch, 0);
  STARK_TRY(verify_r1cs_batch(ctx, circuit->c, public_wires, n_public, nullptr, nullptr, proofs, batch, sts.data(),
                              why.data()));
  if (reasons) memcpy(reasons, why.data(), sizeof(uint32_t) * batch);
  if (statuses) {
    memcpy(statuses, sts.data(), sizeof(stark_status) * batch);
    return STARK_OK;
  }
  for (uint32_t b = 0; b < batch; ++b)
    if (sts[b] != STARK_OK) return sts[b];
  return STARK_OK;
}

}  // extern "C"
