// Polynomial machinery on the GPU: zpoly and lagrange_interp (packages/fri/src/poly_utils.rs:362-439) by a
// subproduct tree, the DFT mul_polys / div_polys (packages/fri/src/fft.rs:381-432), multi-point evaluation
// (eval_poly_at, poly_utils.rs:93-102, over many points) down the same tree, and division with remainder
// (div_polys / mod_polys, poly_utils.rs:235-295) by a power-series reciprocal.
//
// The tree.  n points are padded with points x = 0 to N = max(kLeaf, the next power of two): every node of
// level l is then monic of degree exactly 2^l, stored as its 2^l low coefficients (the leading 1 is
// implicit), and the padded product is Z(X) X^(N - n): the coefficients of Z are the top's, N - n places up.
//   levels 0 .. kLeafLog   one launch: each group of kLeaf points is multiplied out factor by factor in LDS
//                          (poly_leaf_kernel; schoolbook, kLeaf products per coefficient);
//   level l -> l + 1       the batched forward NTT of size 2^(l+1) over all nodes (the first pass reads the
//                          2^l coefficients only), one pointwise launch over all pairs, the batched inverse NTT.
//                          A monic product of degree 2^(l+1) fits that cyclic transform: the leading 1 wraps
//                          onto coefficient 0.  Neither the implicit 1 nor the wrapped one is ever stored or
//                          removed: X^(2^l) transforms to (-1)^i and a constant 1 to 1, so the pointwise
//                          kernels add (+1, -1) to (even, odd) points of a leaf level's transform and
//                          (0, -2) to a wrapped level's (Adj), and the read-out subtracts the top's 1.
// The transforms of every level stay in the arena: the interpolation goes up the same tree with
// N_parent = N_L Z_R + N_R Z_L (degree < 2^(l+1): no wrap), from the leaves' sum_i c_i Z_leaf / (X - x_i),
// c_i = y_i / Z'(x_i) (the zero-preserving batch inverse: a repeated x has Z'(x) = 0 and drops out, as in
// the reference, whose numerator then evaluates to 0).  The padded points carry c = 0.
// An interpolation plan (InterpPlan) keeps what of this depends on the points alone -- the levels' transforms and
// 1 / Z'(x_i) -- and goes up the tree for many value vectors at once, with no host round trip.
//
// The cut-over kLeafLog = 5.  One more level in the leaf kernel costs 2^l more products per point on one
// dependent chain; one more NTT level costs about 3 (l + 1) products per point (three transforms of two
// elements per point) but five launches.  By products alone the two meet at l = 4 (16 against 15); the
// point counts this serves (public inputs: up to ~10^4) make a level's five launches dearer than the
// 2^18 extra products of l = 5, and at l = 6 the leaf's chain (64 steps of three dependent products) would
// be longer than those launches.  The choice is by this count, not by a measurement.
#include <algorithm>

#include "internal.h"

namespace stark {

constexpr uint32_t kLeafLog = 5, kLeaf = 1u << kLeafLog, kPolyThreads = 256;
static_assert(kPolyThreads % kLeaf == 0, "a leaf group lies in one workgroup");
// The descent's largest job: coefficients plus padded points (its product is a transform of up to 2^28 points,
// tree_twiddles' largest), and the longest dividend of stark_divrem_polys.
constexpr size_t kMultipointTreeLimit = (size_t)1 << 27;

struct PolyConsts {
  fe r2;    // R^2 mod p: montmul(x, r2) = Montgomery image of canonical x
  fe unit;  // canonical 1: montmul(x_m, unit) = canonical x
};

static PolyConsts poly_consts() {
  const FieldHost& F = FieldHost::get();
  PolyConsts c;
  c.r2 = to_dev(F.from_canonical(F.one().v));
  c.unit = to_dev(HostFp{{1, 0, 0, 0}});
  return c;
}

// What a stored level's transform lacks at even / odd points (canonical).
struct Adj {
  fe even, odd;
};
static Adj level_adj(bool wrapped) {
  const FieldHost& F = FieldHost::get();
  auto canon = [&](const HostFp& m) {
    HostFp c;
    F.to_canonical(m, c.v);
    return to_dev(c);
  };
  const HostFp one = F.one(), zero = F.zero();
  if (!wrapped) return {canon(one), canon(F.sub(zero, one))};
  return {canon(zero), canon(F.sub(zero, F.add(one, one)))};
}

// LDS images are limb-major (word w of thread t at w * 256 + t): every access is one dword per lane at
// consecutive addresses, conflict-free.
__device__ __forceinline__ void lds_put(uint32_t* a, uint32_t t, const fe& v) {
#pragma unroll
  for (int w = 0; w < 8; ++w) a[w * kPolyThreads + t] = v.w[w];
}
__device__ __forceinline__ fe lds_get(const uint32_t* a, uint32_t t) {
  fe v;
#pragma unroll
  for (int w = 0; w < 8; ++w) v.w[w] = a[w * kPolyThreads + t];
  return v;
}

// Level kLeafLog of the tree from the points: thread j of a group of kLeaf holds coefficient j of
// Z = prod (X - x_i) and, WITH_N, of N = sum_i c_i Z / (X - x_i), both grown one point at a time:
//   N <- N (X - x_i) + c_i Z,  Z <- Z (X - x_i)     (coefficient j - 1 comes from the neighbour through LDS).
// After kLeaf points Z's leading 1 has left the group's kLeaf coefficients.  Points from n on are x = 0, c = 0.
template <bool WITH_N>
__global__ __launch_bounds__(kPolyThreads) void poly_leaf_kernel(const fe* __restrict__ xs, const fe* __restrict__ ys,
                                                                 const fe* __restrict__ inv_den, uint64_t n,
                                                                 uint64_t N, fe r2, fe* __restrict__ z_out,
                                                                 fe* __restrict__ n_out) {
  __shared__ uint32_t xl[8 * kPolyThreads], zl[8 * kPolyThreads];
  __shared__ uint32_t cl[WITH_N ? 8 * kPolyThreads : 1], nl[WITH_N ? 8 * kPolyThreads : 1];
  const uint32_t t = threadIdx.x, j = t & (kLeaf - 1), base = t - j;
  const uint64_t g = (uint64_t)blockIdx.x * kPolyThreads + t;
  fe x = fe_zero(), c = fe_zero();
  if (g < n) {
    x = fe_mul(fe_load(xs + g), r2);
    if (WITH_N)  // y inv R^-1, then twice by R: the Montgomery image of c
      c = fe_mul(fe_mul(fe_mul(fe_load(ys + g), fe_load(inv_den + g)), r2), r2);
  }
  lds_put(xl, t, x);
  if (WITH_N) lds_put(cl, t, c);
  fe z = fe_zero(), nn = fe_zero();
  if (j == 0) z.w[0] = 1;
  for (uint32_t i = 0; i < kLeaf; ++i) {
    lds_put(zl, t, z);
    if (WITH_N) lds_put(nl, t, nn);
    __syncthreads();
    const fe xi = lds_get(xl, base + i);
    const fe zp = j ? lds_get(zl, t - 1) : fe_zero();
    if (WITH_N) {
      const fe np = j ? lds_get(nl, t - 1) : fe_zero();
      nn = fe_add(fe_sub(np, fe_mul(nn, xi)), fe_mul(z, lds_get(cl, base + i)));
    }
    z = fe_sub(zp, fe_mul(z, xi));
    __syncthreads();
  }
  if (g < N) {
    fe_store(z_out + g, z);
    if (WITH_N) fe_store(n_out + g, nn);
  }
}

// Pair k of a level: out[k][i] = Z_2k^[i] Z_(2k+1)^[i] over transforms of m = 2^log_m points (total = pairs m).
__global__ void poly_pair_mul_kernel(const fe* __restrict__ zt, uint32_t log_m, uint64_t total, Adj adj, fe r2,
                                     fe* __restrict__ out) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  const uint64_t k = g >> log_m, i = g & (((uint64_t)1 << log_m) - 1);
  const fe d = (i & 1) ? adj.odd : adj.even;
  const fe a = fe_add(fe_load(zt + ((2 * k) << log_m) + i), d);
  const fe b = fe_add(fe_load(zt + ((2 * k + 1) << log_m) + i), d);
  fe_store(out + g, fe_mul(fe_mul(a, b), r2));
}

// out[k][i] = N_2k^[i] Z_(2k+1)^[i] + N_(2k+1)^[i] Z_2k^[i].
__global__ void poly_pair_comb_kernel(const fe* __restrict__ zt, const fe* __restrict__ nt, uint32_t log_m,
                                      uint64_t total, Adj adj, fe r2, fe* __restrict__ out) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  const uint64_t k = g >> log_m, i = g & (((uint64_t)1 << log_m) - 1);
  const uint64_t l = ((2 * k) << log_m) + i, r = ((2 * k + 1) << log_m) + i;
  const fe d = (i & 1) ? adj.odd : adj.even;
  const fe zl = fe_add(fe_load(zt + l), d), zr = fe_add(fe_load(zt + r), d);
  const fe s = fe_add(fe_mul(fe_load(nt + l), zr), fe_mul(fe_load(nt + r), zl));
  fe_store(out + g, fe_mul(s, r2));
}

// out[i] = top[i + pad] for i < count (less top_fix at the top's coefficient 0); out[count] = 1 when lead.
__global__ void poly_readout_kernel(const fe* __restrict__ top, uint64_t pad, uint64_t count, int top_fix, int lead,
                                    fe* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > count || (i == count && !lead)) return;
  fe v = fe_zero();
  v.w[0] = 1;
  if (i < count) {
    const fe t = fe_load(top + i + pad);
    v = (top_fix && i + pad == 0) ? fe_sub(t, v) : t;
  }
  fe_store(out + i, v);
}

// ---- the interpolation plan's kernels: one interpolation's way up for `batch` value vectors ----
// Batched arrays are proof-major: proof b's N coefficients at nc + b N, its 2 N transform points at nt + 2 b N,
// so a level's nodes of all proofs are one contiguous run for the batched transforms.

// The plan's constants from the build's: xm[i] = x_i R (the Montgomery image) and inv2[i] = R^2 / Z'(x_i).
__global__ void poly_plan_consts_kernel(const fe* __restrict__ xs, const fe* __restrict__ inv, uint64_t n, fe r2,
                                        fe* __restrict__ xm, fe* __restrict__ inv2) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fe_store(xm + i, fe_mul(fe_load(xs + i), r2));
  fe_store(inv2 + i, fe_mul(fe_mul(fe_load(inv + i), r2), r2));
}

// poly_leaf_kernel<true>'s recurrence for proof blockIdx.y: N <- N (X - x_i) + c_i Z, Z <- Z (X - x_i) with
// c_(b,i) = y_(b,i) / Z'(x_i).  xm and inv2 are the plan's (poly_plan_consts_kernel): the value's 32 bytes as they
// are (any integer below 2^256; the product's bounds allow one such operand, fe_mul_asm.inc) times inv2 is c's
// Montgomery image, reduced.  Z is recomputed per proof and not stored: the levels above come from the plan's
// kept transforms.
__global__ __launch_bounds__(kPolyThreads) void poly_leaf_batch_kernel(const fe* __restrict__ xm,
                                                                       const fe* __restrict__ inv2, InterpValues ys,
                                                                       uint64_t n, uint64_t N, fe* __restrict__ n_out) {
  __shared__ uint32_t xl[8 * kPolyThreads], zl[8 * kPolyThreads], cl[8 * kPolyThreads], nl[8 * kPolyThreads];
  const uint32_t t = threadIdx.x, j = t & (kLeaf - 1), base = t - j;
  const uint64_t g = (uint64_t)blockIdx.x * kPolyThreads + t, b = blockIdx.y;
  fe x = fe_zero(), c = fe_zero();
  if (g < n) {
    x = fe_load(xm + g);
    const uint64_t at = ys.index ? ys.index[g] : g;
    c = fe_mul(fe_load(reinterpret_cast<const fe*>(ys.base + b * ys.stride) + at), fe_load(inv2 + g));
  }
  lds_put(xl, t, x);
  lds_put(cl, t, c);
  fe z = fe_zero(), nn = fe_zero();
  if (j == 0) z.w[0] = 1;
  for (uint32_t i = 0; i < kLeaf; ++i) {
    lds_put(zl, t, z);
    lds_put(nl, t, nn);
    __syncthreads();
    const fe xi = lds_get(xl, base + i);
    const fe zp = j ? lds_get(zl, t - 1) : fe_zero();
    const fe np = j ? lds_get(nl, t - 1) : fe_zero();
    nn = fe_add(fe_sub(np, fe_mul(nn, xi)), fe_mul(z, lds_get(cl, base + i)));
    z = fe_sub(zp, fe_mul(z, xi));
    __syncthreads();
  }
  if (g < N) fe_store(n_out + b * N + g, nn);
}

// out[b][k][i] = N_(b,2k)^[i] Z_(2k+1)^[i] + N_(b,2k+1)^[i] Z_2k^[i] over all proofs (total = batch N lanes):
// zt is the plan's level, shared by the proofs; nt and out are proof-major.  Adj as in poly_pair_comb_kernel.
__global__ void poly_pair_comb_batch_kernel(const fe* __restrict__ zt, const fe* __restrict__ nt, uint32_t log_m,
                                            uint32_t log_N, uint64_t total, Adj adj, fe r2, fe* __restrict__ out) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  const uint64_t b = g >> log_N, gi = g & (((uint64_t)1 << log_N) - 1);
  const uint64_t k = gi >> log_m, i = gi & (((uint64_t)1 << log_m) - 1);
  const uint64_t l = ((2 * k) << log_m) + i, r = ((2 * k + 1) << log_m) + i;
  const fe* ntb = nt + (b << (log_N + 1));
  const fe d = (i & 1) ? adj.odd : adj.even;
  const fe zl = fe_add(fe_load(zt + l), d), zr = fe_add(fe_load(zt + r), d);
  const fe s = fe_add(fe_mul(fe_load(ntb + l), zr), fe_mul(fe_load(ntb + r), zl));
  fe_store(out + g, fe_mul(s, r2));
}

// Proof blockIdx.y's coefficients out of the top: out_b[i] = nc_b[i + N - n] for i < n, canonical or (mont) as
// Montgomery images, then zeros for n <= i < fill; out_b is at out.base + b out.stride.
__global__ void poly_readout_batch_kernel(const fe* __restrict__ nc, uint64_t n, uint64_t N, InterpOut out, fe r2) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (i >= n && i >= out.fill) return;
  fe v = fe_zero();
  if (i < n) {
    v = fe_load(nc + b * N + i + (N - n));
    if (out.mont) v = fe_mul(v, r2);
  }
  fe_store(reinterpret_cast<fe*>(out.base + b * out.stride) + i, v);
}

// dz[k] = (k + 1) z[k + 1], k < n; dz[k] = 0 for n <= k < fill.
__global__ void poly_deriv_kernel(const fe* __restrict__ z, uint64_t n, uint64_t fill, fe r2, fe* __restrict__ dz) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= fill) return;
  fe v = fe_zero();
  if (k < n) {
    fe m = fe_zero();
    m.w[0] = (uint32_t)(k + 1);
    m.w[1] = (uint32_t)((k + 1) >> 32);
    v = fe_mul(fe_mul(fe_load(z + k + 1), m), r2);
  }
  fe_store(dz + k, v);
}

// xs[i] = root^exps[i] (canonical) from the root's two-level tables; exps are below the root's order.
__global__ void poly_domain_points_kernel(const fe* __restrict__ lo, const fe* __restrict__ hi, uint32_t kb,
                                          const uint64_t* __restrict__ exps, uint64_t n, fe unit,
                                          fe* __restrict__ xs) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t e = exps[i];
  fe_store(xs + i, fe_mul(fe_mul(lo[e & (((uint64_t)1 << kb) - 1)], hi[e >> kb]), unit));
}

__global__ void poly_gather_kernel(const fe* __restrict__ vals, const uint64_t* __restrict__ exps, uint64_t n,
                                   fe* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) fe_store(out + i, fe_load(vals + exps[i]));
}

// out[i] = a[i] b[i] (canonical in and out).
__global__ void poly_pointwise_kernel(const fe* __restrict__ a, const fe* __restrict__ b, uint64_t n, fe r2,
                                      fe* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) fe_store(out + i, fe_mul(fe_mul(fe_load(a + i), fe_load(b + i)), r2));
}

// The schoolbook phase of the reciprocal: g = 1 / h mod Y^kLeaf in one workgroup.  Lane t keeps
// acc_t = sum_(j >= 1) h_j g_(t - j) over the g known so far; once g_m is out, every later lane adds its
// h_(t - m) g_m and lane m + 1, whose sum is then complete, makes g_(m + 1) = -acc / h_0.
__global__ __launch_bounds__(kPolyThreads) void poly_recip_leaf_kernel(const fe* __restrict__ h, uint64_t hlen,
                                                                       fe h0_inv, PolyConsts pc, fe* __restrict__ g) {
  __shared__ uint32_t hl[8 * kPolyThreads], gl[8 * kPolyThreads];
  const uint32_t t = threadIdx.x;
  fe hm = fe_zero();
  if (t < kLeaf && t < hlen) hm = fe_mul(fe_load(h + t), pc.r2);
  lds_put(hl, t, hm);
  fe acc = fe_zero();
  fe gm = fe_mul(h0_inv, pc.unit);  // g_0 (lane 0's; the others overwrite theirs)
  __syncthreads();
  for (uint32_t m = 0; m < kLeaf; ++m) {
    if (t == m) {
      lds_put(gl, 0, gm);
      fe_store(g + m, gm);
    }
    __syncthreads();
    if (t > m && t < kLeaf) {
      acc = fe_add(acc, fe_mul(lds_get(hl, t - m), lds_get(gl, 0)));
      if (t == m + 1) gm = fe_mul(fe_sub(fe_zero(), acc), h0_inv);
    }
    __syncthreads();
  }
}

// dst[i] = -src[i], i < n.
__global__ void poly_neg_kernel(const fe* __restrict__ src, uint64_t n, fe* __restrict__ dst) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) fe_store(dst + i, fe_sub(fe_zero(), fe_load(src + i)));
}

// out[i] = f[len - 1 - i] for i < count (count <= len), 0 for count <= i < fill: a reversal, cut and padded.
__global__ void poly_rev_kernel(const fe* __restrict__ f, uint64_t len, uint64_t count, uint64_t fill,
                                fe* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < fill) fe_store(out + i, i < count ? fe_load(f + (len - 1 - i)) : fe_zero());
}

// out[i], i < fill: coefficient i of rev_N(Z_top) = Y^N Z_top(1 / Y): 1, then the top's stored coefficients
// N - 1 down to 0 (less the wrapped 1 at coefficient 0 when top_fix), then zeros.
__global__ void poly_rev_top_kernel(const fe* __restrict__ top, uint64_t N, int top_fix, uint64_t fill,
                                    fe* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= fill) return;
  fe v = fe_zero();
  if (i == 0) {
    v.w[0] = 1;
  } else if (i <= N) {
    v = fe_load(top + (N - i));
    if (top_fix && i == N) {
      fe one = fe_zero();
      one.w[0] = 1;
      v = fe_sub(v, one);
    }
  }
  fe_store(out + i, v);
}

// The root vector: out[i] = F[i + 1] = coefficient i + 1 - N + d of prod, 0 where that index is negative (i < N).
__global__ void poly_root_vec_kernel(const fe* __restrict__ prod, uint64_t N, uint64_t d, fe* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) fe_store(out + i, i + 1 + d >= N ? fe_load(prod + (i + 1 + d - N)) : fe_zero());
}

// One level down: child c of parent c / 2 (transforms of m = 2^log_m points, total = children m):
// out[c][i] = F^[c / 2][i] Z_sibling^[(-i) mod m], the sibling's kept transform completed by Adj (-i has i's parity).
__global__ void poly_down_mul_kernel(const fe* __restrict__ ft, const fe* __restrict__ zt, uint32_t log_m,
                                     uint64_t total, Adj adj, fe r2, fe* __restrict__ out) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  const uint64_t mask = ((uint64_t)1 << log_m) - 1, c = g >> log_m, i = g & mask;
  const fe z = fe_add(fe_load(zt + ((c ^ 1) << log_m) + ((0 - i) & mask)), (i & 1) ? adj.odd : adj.even);
  fe_store(out + g, fe_mul(fe_mul(fe_load(ft + ((c >> 1) << log_m) + i), z), r2));
}

// The kept halves into the next level's layout: out[c][k] = in[c][k], k < m / 2 (in: transforms of m = 2^log_m).
__global__ void poly_compact_kernel(const fe* __restrict__ in, uint32_t log_m, uint64_t total, fe* __restrict__ out) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  const uint64_t c = g >> (log_m - 1), k = g & (((uint64_t)1 << (log_m - 1)) - 1);
  fe_store(out + g, fe_load(in + (c << log_m) + k));
}

// The leaves of the descent: lane i of a group of kLeaf points, the group's Z_v (coefficients z, the leaf
// level) and vector F_v in LDS: f(x_i) = sum_j q_j F_v[j] over q = Z_v / (X - x_i) by synthetic division,
// q_(kLeaf - 1) = 1, q_(j - 1) = z_j + x_i q_j.  Values at the padded points (from n on) are dropped.
__global__ __launch_bounds__(kPolyThreads) void poly_leaf_eval_kernel(const fe* __restrict__ xs, uint64_t n, uint64_t N,
                                                                      const fe* __restrict__ z,
                                                                      const fe* __restrict__ fv, fe r2,
                                                                      fe* __restrict__ out) {
  __shared__ uint32_t zl[8 * kPolyThreads], fl[8 * kPolyThreads];
  const uint32_t t = threadIdx.x, base = t - (t & (kLeaf - 1));
  const uint64_t g = (uint64_t)blockIdx.x * kPolyThreads + t;
  lds_put(zl, t, g < N ? fe_load(z + g) : fe_zero());
  lds_put(fl, t, g < N ? fe_mul(fe_load(fv + g), r2) : fe_zero());  // Montgomery images
  __syncthreads();
  if (g >= n) return;
  const fe x = fe_mul(fe_load(xs + g), r2);
  fe q = fe_zero(), acc = fe_zero();
  q.w[0] = 1;
  for (uint32_t j = kLeaf; j-- > 0;) {
    if (j + 1 < kLeaf) q = fe_add(lds_get(zl, base + j + 1), fe_mul(q, x));
    acc = fe_add(acc, fe_mul(q, lds_get(fl, base + j)));
  }
  fe_store(out + g, acc);
}

// ---- the evaluation plan's kernels: one descent for `batch` polynomials ----
// Batched arrays are polynomial-major: polynomial b's K' reversed coefficients at b K', its 2 K' product points at
// 2 b K', its vector F at b N and its children's transforms at 2 b N, so a level's nodes of all polynomials are one
// contiguous run for the batched transforms.  The plan's alpha^, zt, z and xs are shared by the polynomials.
// (The compaction is poly_compact_kernel itself over batch N lanes: its child index is then the run's.)

// out[b][i] = f_b[len - 1 - i] for i < len, 0 for len <= i < K' = 2^log_k; f_b at f + b stride (total = batch K').
__global__ void poly_rev_batch_kernel(const fe* __restrict__ f, uint64_t stride, uint64_t len, uint32_t log_k,
                                      uint64_t total, fe* __restrict__ out) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  const uint64_t b = g >> log_k, i = g & (((uint64_t)1 << log_k) - 1);
  fe_store(out + g, i < len ? fe_load(f + b * stride + (len - 1 - i)) : fe_zero());
}

// t[b][i] <- t[b][i] at[i] over transforms of m = 2^log_m points (canonical in and out; total = batch m).
__global__ void poly_shared_mul_kernel(fe* __restrict__ t, const fe* __restrict__ at, uint32_t log_m, uint64_t total,
                                       fe r2) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  const fe a = fe_load(at + (g & (((uint64_t)1 << log_m) - 1)));
  fe_store(t + g, fe_mul(fe_mul(fe_load(t + g), a), r2));
}

// poly_root_vec_kernel for every polynomial: out[b][i] = prod_b[i + 1 + d - N], 0 where that index is negative;
// prod_b has 2^log_p coefficients (total = batch N, N = 2^log_N).
__global__ void poly_root_vec_batch_kernel(const fe* __restrict__ prod, uint32_t log_p, uint32_t log_N, uint64_t d,
                                           uint64_t total, fe* __restrict__ out) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  const uint64_t N = (uint64_t)1 << log_N, b = g >> log_N, i = g & (N - 1);
  fe_store(out + g, i + 1 + d >= N ? fe_load(prod + (b << log_p) + (i + 1 + d - N)) : fe_zero());
}

// poly_down_mul_kernel for every polynomial: c counts the children of the whole run (each polynomial has an even
// number of them, so c / 2 is the run's parent), c & cmask is the child within its polynomial, whose sibling's
// transform is the plan's.
__global__ void poly_down_mul_batch_kernel(const fe* __restrict__ ft, const fe* __restrict__ zt, uint32_t log_m,
                                           uint64_t cmask, uint64_t total, Adj adj, fe r2, fe* __restrict__ out) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  const uint64_t mask = ((uint64_t)1 << log_m) - 1, c = g >> log_m, i = g & mask;
  const fe z = fe_add(fe_load(zt + (((c & cmask) ^ 1) << log_m) + ((0 - i) & mask)), (i & 1) ? adj.odd : adj.even);
  fe_store(out + g, fe_mul(fe_mul(fe_load(ft + ((c >> 1) << log_m) + i), z), r2));
}

// poly_leaf_eval_kernel for polynomial blockIdx.y: its vector at fv + b N, its values to out + b out_stride.
__global__ __launch_bounds__(kPolyThreads) void poly_leaf_eval_batch_kernel(const fe* __restrict__ xs, uint64_t n,
                                                                            uint64_t N, const fe* __restrict__ z,
                                                                            const fe* __restrict__ fv, fe r2,
                                                                            fe* __restrict__ out, uint64_t out_stride) {
  __shared__ uint32_t zl[8 * kPolyThreads], fl[8 * kPolyThreads];
  const uint32_t t = threadIdx.x, base = t - (t & (kLeaf - 1));
  const uint64_t g = (uint64_t)blockIdx.x * kPolyThreads + t, b = blockIdx.y;
  lds_put(zl, t, g < N ? fe_load(z + g) : fe_zero());
  lds_put(fl, t, g < N ? fe_mul(fe_load(fv + b * N + g), r2) : fe_zero());  // Montgomery images
  __syncthreads();
  if (g >= n) return;
  const fe x = fe_mul(fe_load(xs + g), r2);
  fe q = fe_zero(), acc = fe_zero();
  q.w[0] = 1;
  for (uint32_t j = kLeaf; j-- > 0;) {
    if (j + 1 < kLeaf) q = fe_add(lds_get(zl, base + j + 1), fe_mul(q, x));
    acc = fe_add(acc, fe_mul(q, lds_get(fl, base + j)));
  }
  fe_store(out + b * out_stride + g, acc);
}

// r[i] = a[i] - prod[i] for i < m, 0 for m <= i < fill.
__global__ void poly_sub_kernel(const fe* __restrict__ a, const fe* __restrict__ prod, uint64_t m, uint64_t fill,
                                fe* __restrict__ r) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < fill) fe_store(r + i, i < m ? fe_sub(fe_load(a + i), fe_load(prod + i)) : fe_zero());
}

static unsigned grid_for(uint64_t n) { return (unsigned)((n + 255) / 256); }

// 7^((p - 1) / 2^k): the primitive 2^k-th root the tree's transforms use (the prover's g2, prove.rs:71-82),
// and its inverse.
static stark_status tree_twiddles(stark_ctx* ctx, uint32_t k, const Twiddles** fwd, const Twiddles** inv) {
  const FieldHost& F = FieldHost::get();
  static const HostFp w28 = [] {
    const FieldHost& G = FieldHost::get();
    uint64_t e[4];
    memcpy(e, FieldHost::kP, 32);
    e[0] -= 1;
    for (int s = 0; s < 28; ++s)
      for (int l = 0; l < 4; ++l) e[l] = (e[l] >> 1) | (l < 3 ? e[l + 1] << 63 : 0);
    return G.pow(G.from_u64(7), e, 4);
  }();
  if (k > 28) return STARK_ERR_BAD_LENGTH;
  const HostFp w = F.pow_u64(w28, (uint64_t)1 << (28 - k));
  uint64_t c[4];
  F.to_canonical(w, c);
  STARK_TRY(get_twiddles(ctx, c, k, fwd));
  F.to_canonical(F.inv(w), c);
  return get_twiddles(ctx, c, k, inv);
}

void poly_tree_plan(size_t n, PolyTree& t) {
  t.n = n;
  t.log_N = kLeafLog;
  while (((size_t)1 << t.log_N) < n) ++t.log_N;
  t.N = (size_t)1 << t.log_N;
  t.levels = t.log_N - kLeafLog;
}

size_t poly_tree_elems(const PolyTree& t) { return t.N + 2 * t.N * t.levels; }

// zpoly's tree over the device points xs (canonical): the top in t.z, each level's transforms in t.zt.
stark_status poly_tree_build(stark_ctx* ctx, const fe* d_xs, PolyTree& t, fe* mem, hipStream_t s) {
  const PolyConsts pc = poly_consts();
  t.z = mem;
  t.zt = mem + t.N;
  hipLaunchKernelGGL(poly_leaf_kernel<false>, dim3(grid_for(t.N)), dim3(kPolyThreads), 0, s, d_xs, (const fe*)nullptr,
                     (const fe*)nullptr, (uint64_t)t.n, (uint64_t)t.N, pc.r2, t.z, (fe*)nullptr);
  STARK_HIP(ctx, hipGetLastError());
  for (uint32_t lv = 0; lv < t.levels; ++lv) {
    const uint32_t log_m = kLeafLog + lv + 1;  // the transforms' size: twice the nodes'
    const uint32_t nodes = (uint32_t)(t.N >> (log_m - 1));
    const Twiddles *fwd, *inv;
    STARK_TRY(tree_twiddles(ctx, log_m, &fwd, &inv));
    fe* zt = t.zt + 2 * t.N * lv;
    STARK_TRY(ntt_device_from(ctx, t.z, 1, zt, log_m, nodes, *fwd, false, s));
    hipLaunchKernelGGL(poly_pair_mul_kernel, dim3(grid_for(t.N)), dim3(256), 0, s, (const fe*)zt, log_m,
                       (uint64_t)t.N, level_adj(lv > 0), pc.r2, t.z);
    STARK_HIP(ctx, hipGetLastError());
    STARK_TRY(ntt_device(ctx, t.z, log_m, nodes / 2, *inv, true, s));
  }
  return STARK_OK;
}

// The n + 1 coefficients of prod (X - x_i) out of a built tree (low degree first, out[n] = 1).
stark_status poly_tree_zpoly(stark_ctx* ctx, const PolyTree& t, fe* d_out, hipStream_t s) {
  hipLaunchKernelGGL(poly_readout_kernel, dim3(grid_for(t.n + 1)), dim3(256), 0, s, (const fe*)t.z,
                     (uint64_t)(t.N - t.n), (uint64_t)t.n, t.levels > 0 ? 1 : 0, 1, d_out);
  STARK_HIP(ctx, hipGetLastError());
  return STARK_OK;
}

size_t lagrange_scratch_elems(size_t n, const DomainHint* hint) {
  PolyTree t;
  poly_tree_plan(n, t);
  size_t dz = n;
  if (hint && n <= ((size_t)1 << hint->log_order)) dz = (size_t)1 << hint->log_order;
  // the tree, N's coefficients and transforms, Z (n + 1), Z', den, 1 / den; for arbitrary points the descent's
  // working set (whether it runs is the context's choice, stark_ctx_set_multipoint_tree_min)
  return poly_tree_elems(t) + 3 * t.N + (n + 1) + dz + 2 * n + (dz == n && n ? poly_descent_elems(t, n) : 0);
}

stark_status lagrange_interp_device(stark_ctx* ctx, const fe* d_xs, const fe* d_ys, size_t n, fe* d_out, fe* mem,
                                    hipStream_t s, const DomainHint* hint, fe** z_out) {
  if (n == 0) return STARK_OK;
  const PolyConsts pc = poly_consts();
  PolyTree t;
  poly_tree_plan(n, t);
  if (hint && n > ((size_t)1 << hint->log_order)) hint = nullptr;  // Z' does not fit the domain: Horner
  const size_t dz_n = hint ? (size_t)1 << hint->log_order : n;
  fe* at = mem + poly_tree_elems(t);
  fe* nc = at;         // N's coefficients, level by level
  fe* nt = nc + t.N;   // their transforms
  fe* z = nt + 2 * t.N;
  fe* dz = z + (n + 1);
  fe* den = dz + dz_n;
  fe* inv = den + n;
  STARK_TRY(poly_tree_build(ctx, d_xs, t, mem, s));
  STARK_TRY(poly_tree_zpoly(ctx, t, z, s));
  if (z_out) *z_out = z;
  hipLaunchKernelGGL(poly_deriv_kernel, dim3(grid_for(dz_n)), dim3(256), 0, s, (const fe*)z, (uint64_t)n,
                     (uint64_t)dz_n, pc.r2, dz);
  STARK_HIP(ctx, hipGetLastError());
  if (hint) {  // the points are root^e: Z' over the whole domain by one transform, then a gather
    STARK_TRY(ntt_device(ctx, dz, hint->log_order, 1, *hint->tw, false, s));
    hipLaunchKernelGGL(poly_gather_kernel, dim3(grid_for(n)), dim3(256), 0, s, (const fe*)dz, hint->d_exps,
                       (uint64_t)n, den);
    STARK_HIP(ctx, hipGetLastError());
  } else if (n >= (ctx->multipoint_tree_min ? ctx->multipoint_tree_min : kDefaultMultipointTreeMin) &&
             n + t.N <= kMultipointTreeLimit) {
    // arbitrary points, many: Z' down the tree just built (t.z becomes the leaf level, as it does below anyway)
    STARK_TRY(poly_tree_eval(ctx, t, d_xs, dz, n, den, inv + n, s));
  } else {
    STARK_TRY(eval_poly_device(ctx, dz, n, d_xs, n, den, s));
  }
  STARK_TRY(multi_inv_device(ctx, den, inv, n, s));
  hipLaunchKernelGGL(poly_leaf_kernel<true>, dim3(grid_for(t.N)), dim3(kPolyThreads), 0, s, d_xs, d_ys,
                     (const fe*)inv, (uint64_t)n, (uint64_t)t.N, pc.r2, t.z, nc);
  STARK_HIP(ctx, hipGetLastError());
  // (t.z is overwritten with the leaf level again: Z's coefficients were read out above, and the levels
  // above are taken from their kept transforms)
  for (uint32_t lv = 0; lv < t.levels; ++lv) {
    const uint32_t log_m = kLeafLog + lv + 1;
    const uint32_t nodes = (uint32_t)(t.N >> (log_m - 1));
    const Twiddles *fwd, *tinv;
    STARK_TRY(tree_twiddles(ctx, log_m, &fwd, &tinv));
    STARK_TRY(ntt_device_from(ctx, nc, 1, nt, log_m, nodes, *fwd, false, s));
    hipLaunchKernelGGL(poly_pair_comb_kernel, dim3(grid_for(t.N)), dim3(256), 0, s,
                       (const fe*)(t.zt + 2 * t.N * lv), (const fe*)nt, log_m, (uint64_t)t.N, level_adj(lv > 0), pc.r2,
                       nc);
    STARK_HIP(ctx, hipGetLastError());
    STARK_TRY(ntt_device(ctx, nc, log_m, nodes / 2, *tinv, true, s));
  }
  hipLaunchKernelGGL(poly_readout_kernel, dim3(grid_for(n)), dim3(256), 0, s, (const fe*)nc, (uint64_t)(t.N - n),
                     (uint64_t)n, 0, 0, d_out);
  STARK_HIP(ctx, hipGetLastError());
  return STARK_OK;
}

stark_status poly_domain_points(stark_ctx* ctx, const Twiddles& tw, const uint64_t* d_exps, size_t n, fe* d_xs,
                                hipStream_t s) {
  if (n == 0) return STARK_OK;
  hipLaunchKernelGGL(poly_domain_points_kernel, dim3(grid_for(n)), dim3(256), 0, s, tw.d_lo, tw.d_hi, tw.kb, d_exps,
                     (uint64_t)n, poly_consts().unit, d_xs);
  STARK_HIP(ctx, hipGetLastError());
  return STARK_OK;
}

// ---- interpolation plans ----

void interp_plan_release(stark_ctx* ctx, InterpPlan& plan) {
  if (plan.mem) {  // (then the plan is entered in its context, which is alive: its destruction empties the plans)
    hipFree(plan.mem);  // (waits for the device: a kernel of any stream may still read it)
    auto& live = ctx->interp_plans;
    live.erase(std::remove(live.begin(), live.end(), &plan), live.end());
  }
  plan = InterpPlan();
}

void interp_plans_release_all(stark_ctx* ctx) {
  for (InterpPlan* p : ctx->interp_plans) {
    hipFree(p->mem);
    *p = InterpPlan();
  }
  ctx->interp_plans.clear();
}

// lagrange_interp_device up to its batch inverse, in ctx->poly, then the plan's own buffer from it.
stark_status interp_plan_build(stark_ctx* ctx, const fe* d_xs, size_t n, const DomainHint* hint, InterpPlan& plan,
                               hipStream_t s) {
  plan = InterpPlan();
  if (n == 0) return STARK_OK;
  const PolyConsts pc = poly_consts();
  PolyTree t;
  poly_tree_plan(n, t);
  if (hint && n > ((size_t)1 << hint->log_order)) hint = nullptr;  // Z' does not fit the domain: as the single call
  const size_t dz_n = hint ? (size_t)1 << hint->log_order : n;
  const size_t zt_elems = 2 * t.N * t.levels;
  fe* own = nullptr;
  const size_t bytes = (2 * n + zt_elems) * sizeof(fe);
  if (hipMalloc((void**)&own, bytes) != hipSuccess) {
    (void)hipGetLastError();
    return STARK_ERR_OOM;
  }
  poison_dev(own, bytes);
  plan.mem = own;
  plan.bytes = bytes;
  ctx->interp_plans.push_back(&plan);
  plan.n = n;
  plan.N = t.N;
  plan.log_N = t.log_N;
  plan.levels = t.levels;
  plan.xs = own;
  plan.inv_den = own + n;
  plan.zt = own + 2 * n;
  auto build = [&]() -> stark_status {
    STARK_TRY(buf_acquire(ctx, ctx->poly, s));
    STARK_TRY(ensure_buf(ctx, ctx->poly, lagrange_scratch_elems(n, hint) * sizeof(fe)));
    fe* mem = (fe*)ctx->poly.ptr;
    fe* z = mem + poly_tree_elems(t) + 3 * t.N;  // lagrange_interp_device's layout
    fe* dz = z + (n + 1);
    fe* den = dz + dz_n;
    fe* inv = den + n;
    STARK_TRY(poly_tree_build(ctx, d_xs, t, mem, s));
    if (zt_elems)  // (before the descent below, which reads the tree's t.zt but writes t.z only)
      STARK_HIP(ctx, hipMemcpyAsync(plan.zt, t.zt, zt_elems * sizeof(fe), hipMemcpyDeviceToDevice, s));
    STARK_TRY(poly_tree_zpoly(ctx, t, z, s));
    hipLaunchKernelGGL(poly_deriv_kernel, dim3(grid_for(dz_n)), dim3(256), 0, s, (const fe*)z, (uint64_t)n,
                       (uint64_t)dz_n, pc.r2, dz);
    STARK_HIP(ctx, hipGetLastError());
    if (hint) {
      STARK_TRY(ntt_device(ctx, dz, hint->log_order, 1, *hint->tw, false, s));
      hipLaunchKernelGGL(poly_gather_kernel, dim3(grid_for(n)), dim3(256), 0, s, (const fe*)dz, hint->d_exps,
                         (uint64_t)n, den);
      STARK_HIP(ctx, hipGetLastError());
    } else if (n >= (ctx->multipoint_tree_min ? ctx->multipoint_tree_min : kDefaultMultipointTreeMin) &&
               n + t.N <= kMultipointTreeLimit) {
      STARK_TRY(poly_tree_eval(ctx, t, d_xs, dz, n, den, inv + n, s));
    } else {
      STARK_TRY(eval_poly_device(ctx, dz, n, d_xs, n, den, s));
    }
    STARK_TRY(multi_inv_device(ctx, den, inv, n, s));
    hipLaunchKernelGGL(poly_plan_consts_kernel, dim3(grid_for(n)), dim3(256), 0, s, d_xs, (const fe*)inv, (uint64_t)n,
                       pc.r2, plan.xs, plan.inv_den);
    STARK_HIP(ctx, hipGetLastError());
    STARK_TRY(buf_release(ctx, ctx->poly, s));
    // complete on return: the plan is applied on any stream, and d_xs is the caller's staging
    STARK_HIP(ctx, hipStreamSynchronize(s));
    return STARK_OK;
  };
  const stark_status st = build();
  if (st != STARK_OK) interp_plan_release(ctx, plan);
  return st;
}

stark_status interp_plan_build_domain(stark_ctx* ctx, const uint64_t root[4], uint32_t log_order, const uint64_t* exps,
                                      size_t n, InterpPlan& plan, hipStream_t s) {
  plan = InterpPlan();
  if (n == 0) return STARK_OK;
  if (log_order > 28) return STARK_ERR_BAD_LENGTH;
  for (size_t i = 0; i < n; ++i)
    if (exps[i] >> log_order) return STARK_ERR_BAD_ARG;
  DomainHint hint;
  STARK_TRY(get_twiddles(ctx, root, log_order, &hint.tw));
  hint.log_order = log_order;
  // staging: the points, then their exponents (the build returns synchronised: exps is read by then)
  STARK_TRY(ensure_buf(ctx, ctx->io, n * (sizeof(fe) + sizeof(uint64_t))));
  fe* d_xs = (fe*)ctx->io.ptr;
  uint64_t* d_exps = (uint64_t*)(d_xs + n);
  STARK_HIP(ctx, hipMemcpyAsync(d_exps, exps, n * sizeof(uint64_t), hipMemcpyHostToDevice, s));
  hint.d_exps = d_exps;
  STARK_TRY(poly_domain_points(ctx, *hint.tw, d_exps, n, d_xs, s));
  return interp_plan_build(ctx, d_xs, n, &hint, plan, s);
}

// Proofs per chunk of an application: their scratch (nc: N, nt: 2 N per proof) stays under the prove-batch limit,
// at least one proof; a grid's second coordinate and the transforms' 32-bit node count bound a chunk too.
static size_t interp_plan_chunk(const stark_ctx* ctx, const InterpPlan& plan, uint32_t batch) {
  const size_t limit = ctx->prove_batch_limit ? ctx->prove_batch_limit : kDefaultProveBatchLimit;
  const size_t chunk = std::max<size_t>(1, limit / (3 * plan.N * sizeof(fe)));
  return std::min<size_t>({chunk, batch, 65535, std::max<size_t>(1, ((size_t)1 << 31) / plan.N)});
}

stark_status interp_plan_apply(stark_ctx* ctx, const InterpPlan& plan, const InterpValues& ys, uint32_t batch,
                               const InterpOut& out, hipStream_t s) {
  if (batch == 0 || plan.n == 0) return STARK_OK;
  const PolyConsts pc = poly_consts();
  const size_t n = plan.n, N = plan.N;
  const size_t chunk = interp_plan_chunk(ctx, plan, batch);
  STARK_TRY(buf_acquire(ctx, ctx->poly, s));
  STARK_TRY(ensure_buf(ctx, ctx->poly, chunk * 3 * N * sizeof(fe)));
  fe* nc = (fe*)ctx->poly.ptr;
  fe* nt = nc + chunk * N;
  for (uint32_t b0 = 0; b0 < batch; b0 += (uint32_t)chunk) {
    const uint32_t B = (uint32_t)std::min<size_t>(chunk, batch - b0);
    InterpValues y = ys;
    y.base += (uint64_t)b0 * ys.stride;
    InterpOut o = out;
    o.base += (uint64_t)b0 * out.stride;
    hipLaunchKernelGGL(poly_leaf_batch_kernel, dim3(grid_for(N), B), dim3(kPolyThreads), 0, s, (const fe*)plan.xs,
                       (const fe*)plan.inv_den, y, (uint64_t)n, (uint64_t)N, nc);
    STARK_HIP(ctx, hipGetLastError());
    for (uint32_t lv = 0; lv < plan.levels; ++lv) {
      const uint32_t log_m = kLeafLog + lv + 1;
      const uint32_t nodes = (uint32_t)(N >> (log_m - 1));
      const Twiddles *fwd, *tinv;
      STARK_TRY(tree_twiddles(ctx, log_m, &fwd, &tinv));
      STARK_TRY(ntt_device_from(ctx, nc, 1, nt, log_m, B * nodes, *fwd, false, s));
      hipLaunchKernelGGL(poly_pair_comb_batch_kernel, dim3(grid_for((uint64_t)B * N)), dim3(256), 0, s,
                         (const fe*)(plan.zt + 2 * N * lv), (const fe*)nt, log_m, plan.log_N, (uint64_t)B * N,
                         level_adj(lv > 0), pc.r2, nc);
      STARK_HIP(ctx, hipGetLastError());
      STARK_TRY(ntt_device(ctx, nc, log_m, B * (nodes / 2), *tinv, true, s));
    }
    const uint64_t lanes = std::max<uint64_t>(n, out.fill);
    hipLaunchKernelGGL(poly_readout_batch_kernel, dim3(grid_for(lanes), B), dim3(256), 0, s, (const fe*)nc, (uint64_t)n,
                       (uint64_t)N, o, pc.r2);
    STARK_HIP(ctx, hipGetLastError());
  }
  return buf_release(ctx, ctx->poly, s);
}

// a <- the 2^(log_k + 1) coefficients of a b, for a and b of 2^log_k coefficients each (no wrap); ta and tb
// hold 2^(log_k + 1) elements each, the product lands in ta.
static stark_status poly_full_product(stark_ctx* ctx, const fe* a, const fe* b, uint32_t log_k, fe* ta, fe* tb,
                                      hipStream_t s) {
  const Twiddles *fwd, *inv;
  STARK_TRY(tree_twiddles(ctx, log_k + 1, &fwd, &inv));
  const uint64_t m = (uint64_t)2 << log_k;
  STARK_TRY(ntt_device_from(ctx, a, 1, ta, log_k + 1, 1, *fwd, false, s));
  STARK_TRY(ntt_device_from(ctx, b, 1, tb, log_k + 1, 1, *fwd, false, s));
  hipLaunchKernelGGL(poly_pointwise_kernel, dim3(grid_for(m)), dim3(256), 0, s, (const fe*)ta, (const fe*)tb, m,
                     poly_consts().r2, ta);
  STARK_HIP(ctx, hipGetLastError());
  return ntt_device(ctx, ta, log_k + 1, 1, *inv, true, s);
}

// Newton's iteration for the power-series reciprocal.  With g = 1 / h mod Y^j, e = h g mod Y^2j is 1 + Y^j e_hi,
// and g (2 - h g) = g - Y^j (g e_hi) mod Y^2j: the step appends -(g e_hi mod Y^j) to g.  Both products run as
// cyclic transforms of 2j points: h g has 3j coefficients, whose top j wrap onto the low j, which are known
// (1, 0, ..) and not read; g e_hi has 2j and does not wrap.  Five transforms of 2j points per step.
stark_status poly_recip_device(stark_ctx* ctx, const fe* d_h, size_t hlen, uint32_t log_k, const fe& h0_inv, fe* d_g,
                               fe* mem, hipStream_t s) {
  if (log_k < kLeafLog || log_k > 27) return STARK_ERR_BAD_LENGTH;
  const size_t K = (size_t)1 << log_k, hc = hlen < K ? hlen : K;
  const PolyConsts pc = poly_consts();
  fe *H = mem, *A = H + K, *B = A + K, *C = B + K;  // h padded; h^ then e; g^; e_hi^ then g e_hi
  STARK_HIP(ctx, hipMemcpyAsync(H, d_h, hc * sizeof(fe), hipMemcpyDeviceToDevice, s));
  if (hc < K) STARK_HIP(ctx, hipMemsetAsync(H + hc, 0, (K - hc) * sizeof(fe), s));
  hipLaunchKernelGGL(poly_recip_leaf_kernel, dim3(1), dim3(kPolyThreads), 0, s, (const fe*)H, (uint64_t)K, h0_inv, pc,
                     d_g);
  STARK_HIP(ctx, hipGetLastError());
  for (uint32_t log_j = kLeafLog; log_j < log_k; ++log_j) {
    const size_t j = (size_t)1 << log_j;
    const uint32_t log_m = log_j + 1;
    const Twiddles *fwd, *inv;
    STARK_TRY(tree_twiddles(ctx, log_m, &fwd, &inv));
    STARK_HIP(ctx, hipMemcpyAsync(A, H, 2 * j * sizeof(fe), hipMemcpyDeviceToDevice, s));
    STARK_TRY(ntt_device(ctx, A, log_m, 1, *fwd, false, s));
    STARK_TRY(ntt_device_from(ctx, d_g, 1, B, log_m, 1, *fwd, false, s));
    hipLaunchKernelGGL(poly_pointwise_kernel, dim3(grid_for(2 * j)), dim3(256), 0, s, (const fe*)A, (const fe*)B,
                       (uint64_t)(2 * j), pc.r2, A);
    STARK_HIP(ctx, hipGetLastError());
    STARK_TRY(ntt_device(ctx, A, log_m, 1, *inv, true, s));
    STARK_TRY(ntt_device_from(ctx, A + j, 1, C, log_m, 1, *fwd, false, s));
    hipLaunchKernelGGL(poly_pointwise_kernel, dim3(grid_for(2 * j)), dim3(256), 0, s, (const fe*)C, (const fe*)B,
                       (uint64_t)(2 * j), pc.r2, C);
    STARK_HIP(ctx, hipGetLastError());
    STARK_TRY(ntt_device(ctx, C, log_m, 1, *inv, true, s));
    hipLaunchKernelGGL(poly_neg_kernel, dim3(grid_for(j)), dim3(256), 0, s, (const fe*)C, (uint64_t)j, d_g + j);
    STARK_HIP(ctx, hipGetLastError());
  }
  return STARK_OK;
}

static uint32_t recip_log(size_t count) {  // log2 of the reciprocal's length for `count` coefficients
  uint32_t l = kLeafLog;
  while (((size_t)1 << l) < count) ++l;
  return l;
}

// The descent of the subproduct tree.  With Z_v the monic product over node v's 2m points, the
// vector F_v[k], k = 1..2m, holds the first 2m coefficients in 1 / X of the fractional part of f / Z_v.
//   root     f / Z_top = X^(d - N) rev_d(f)(1 / X) / rev_N(Z_top)(1 / X): F[k] is coefficient k - N + d of
//            rev_d(f) alpha, alpha = 1 / rev_N(Z_top) mod Y^(d + 1) (one reciprocal, one product; any d);
//   down     f / Z_L = (f / Z_v) Z_R, so child L's F[k] = sum_(j <= m) z^R_j F_v[k + j] for k <= m: a correlation,
//            as transforms of 2m points c^[i] = F^[i] z^[-i], whose first m entries no index wraps into;
//   leaves   (f mod Z_v) / (X - x_i) = (f mod Z_v) / Z_v times q, q = Z_v / (X - x_i), and its coefficient of
//            1 / X is f(x_i) = sum_j q_j F_v[j + 1] (poly_leaf_eval_kernel).
// No batch inverse, no host round trip.
size_t poly_descent_elems(const PolyTree& t, size_t deg_plus_1) {
  return 6 * ((size_t)1 << recip_log(deg_plus_1)) + 3 * t.N;  // alpha, the reciprocal's and product's 5 K, F, its 2 N
}

stark_status poly_tree_eval(stark_ctx* ctx, const PolyTree& t, const fe* d_xs, const fe* d_f, size_t deg_plus_1,
                            fe* d_out, fe* mem, hipStream_t s) {
  if (deg_plus_1 == 0) return STARK_ERR_BAD_ARG;
  const uint32_t log_k = recip_log(deg_plus_1);
  if (log_k > 27) return STARK_ERR_BAD_LENGTH;
  const size_t K = (size_t)1 << log_k, N = t.N;
  const PolyConsts pc = poly_consts();
  fe *alpha = mem, *W = alpha + K, *fv = W + 5 * K, *G = fv + N;
  hipLaunchKernelGGL(poly_rev_top_kernel, dim3(grid_for(K)), dim3(256), 0, s, (const fe*)t.z, (uint64_t)N,
                     t.levels > 0 ? 1 : 0, (uint64_t)K, W + 4 * K);
  STARK_HIP(ctx, hipGetLastError());
  STARK_TRY(poly_recip_device(ctx, W + 4 * K, K, log_k, to_dev(FieldHost::get().one()), alpha, W, s));
  hipLaunchKernelGGL(poly_rev_kernel, dim3(grid_for(K)), dim3(256), 0, s, d_f, (uint64_t)deg_plus_1,
                     (uint64_t)deg_plus_1, (uint64_t)K, W);
  STARK_HIP(ctx, hipGetLastError());
  STARK_TRY(poly_full_product(ctx, W, alpha, log_k, W + K, W + 3 * K, s));
  hipLaunchKernelGGL(poly_root_vec_kernel, dim3(grid_for(N)), dim3(256), 0, s, (const fe*)(W + K), (uint64_t)N,
                     (uint64_t)(deg_plus_1 - 1), fv);
  STARK_HIP(ctx, hipGetLastError());
  // the leaf level again (the levels above overwrote it; they are taken from their kept transforms)
  hipLaunchKernelGGL(poly_leaf_kernel<false>, dim3(grid_for(N)), dim3(kPolyThreads), 0, s, d_xs, (const fe*)nullptr,
                     (const fe*)nullptr, (uint64_t)t.n, (uint64_t)N, pc.r2, t.z, (fe*)nullptr);
  STARK_HIP(ctx, hipGetLastError());
  for (uint32_t lv = t.levels; lv-- > 0;) {
    const uint32_t log_m = kLeafLog + lv + 1;  // the transforms' size: the parents'
    const uint32_t parents = (uint32_t)(N >> log_m);
    const Twiddles *fwd, *inv;
    STARK_TRY(tree_twiddles(ctx, log_m, &fwd, &inv));
    STARK_TRY(ntt_device(ctx, fv, log_m, parents, *fwd, false, s));
    hipLaunchKernelGGL(poly_down_mul_kernel, dim3(grid_for(2 * N)), dim3(256), 0, s, (const fe*)fv,
                       (const fe*)(t.zt + 2 * N * lv), log_m, (uint64_t)(2 * N), level_adj(lv > 0), pc.r2, G);
    STARK_HIP(ctx, hipGetLastError());
    STARK_TRY(ntt_device(ctx, G, log_m, 2 * parents, *inv, true, s));
    hipLaunchKernelGGL(poly_compact_kernel, dim3(grid_for(N)), dim3(256), 0, s, (const fe*)G, log_m, (uint64_t)N, fv);
    STARK_HIP(ctx, hipGetLastError());
  }
  hipLaunchKernelGGL(poly_leaf_eval_kernel, dim3(grid_for(N)), dim3(kPolyThreads), 0, s, d_xs, (uint64_t)t.n,
                     (uint64_t)N, (const fe*)t.z, (const fe*)fv, pc.r2, d_out);
  STARK_HIP(ctx, hipGetLastError());
  return STARK_OK;
}

stark_status eval_multipoint_device(stark_ctx* ctx, const fe* d_poly, size_t deg_plus_1, const fe* d_xs, size_t n,
                                    fe* d_out, hipStream_t s) {
  if (n == 0) return STARK_OK;
  if (deg_plus_1 == 0) {
    STARK_HIP(ctx, hipMemsetAsync(d_out, 0, n * sizeof(fe), s));
    return STARK_OK;
  }
  const size_t tree_min = ctx->multipoint_tree_min ? ctx->multipoint_tree_min : kDefaultMultipointTreeMin;
  PolyTree t;
  poly_tree_plan(n, t);
  const bool tree = (n < deg_plus_1 ? n : deg_plus_1) >= tree_min && deg_plus_1 + t.N <= kMultipointTreeLimit;
  STARK_TRY(buf_acquire(ctx, ctx->poly, s));
  if (tree) {
    STARK_TRY(ensure_buf(ctx, ctx->poly, (poly_tree_elems(t) + poly_descent_elems(t, deg_plus_1)) * sizeof(fe)));
    fe* mem = (fe*)ctx->poly.ptr;
    STARK_TRY(poly_tree_build(ctx, d_xs, t, mem, s));
    STARK_TRY(poly_tree_eval(ctx, t, d_xs, d_poly, deg_plus_1, d_out, mem + poly_tree_elems(t), s));
  } else {
    STARK_TRY(ensure_buf(ctx, ctx->poly, eval_split_scratch_elems(deg_plus_1, n) * sizeof(fe)));
    STARK_TRY(eval_split_device(ctx, d_poly, deg_plus_1, d_xs, n, d_out, (fe*)ctx->poly.ptr, s));
  }
  return buf_release(ctx, ctx->poly, s);
}

// ---- evaluation plans ----

void eval_plan_release(stark_ctx* ctx, EvalPlan& plan) {
  if (plan.mem) {  // (then the plan is entered in its context, which is alive: its destruction empties the plans)
    hipFree(plan.mem);  // (waits for the device: a kernel of any stream may still read it)
    auto& live = ctx->eval_plans;
    live.erase(std::remove(live.begin(), live.end(), &plan), live.end());
  }
  plan = EvalPlan();
}

void eval_plans_release_all(stark_ctx* ctx) {
  for (EvalPlan* p : ctx->eval_plans) {
    hipFree(p->mem);
    *p = EvalPlan();
  }
  ctx->eval_plans.clear();
}

stark_status eval_plan_check(size_t n, size_t max_deg_plus_1) {
  if (n > kMultipointTreeLimit || max_deg_plus_1 > kMultipointTreeLimit) return STARK_ERR_BAD_LENGTH;
  PolyTree t;
  poly_tree_plan(n, t);
  return max_deg_plus_1 + t.N <= kMultipointTreeLimit ? STARK_OK : STARK_ERR_BAD_LENGTH;
}

// eval_multipoint_device's tree route up to its reciprocal, in ctx->poly, with what an application reads written to
// the plan's own buffer.  rev_N(Z_top) has constant term 1: the reciprocal needs no inverse from the host.
stark_status eval_plan_build(stark_ctx* ctx, const fe* d_xs, size_t n, size_t max_deg_plus_1, EvalPlan& plan,
                             hipStream_t s) {
  plan = EvalPlan();
  if (max_deg_plus_1 == 0) return STARK_ERR_BAD_ARG;
  STARK_TRY(eval_plan_check(n, max_deg_plus_1));
  plan.max_deg_plus_1 = max_deg_plus_1;
  if (n == 0) return STARK_OK;
  const PolyConsts pc = poly_consts();
  PolyTree t;
  poly_tree_plan(n, t);
  const uint32_t log_k = recip_log(max_deg_plus_1);
  const size_t K = (size_t)1 << log_k, N = t.N, zt_elems = 2 * N * t.levels;
  fe* own = nullptr;
  const size_t bytes = (n + N + zt_elems + 3 * K) * sizeof(fe);
  if (hipMalloc((void**)&own, bytes) != hipSuccess) {
    (void)hipGetLastError();
    return STARK_ERR_OOM;
  }
  poison_dev(own, bytes);
  plan.mem = own;
  plan.bytes = bytes;
  ctx->eval_plans.push_back(&plan);
  plan.n = n;
  plan.N = N;
  plan.K = K;
  plan.log_N = t.log_N;
  plan.levels = t.levels;
  plan.log_K = log_k;
  plan.xs = own;
  plan.z = plan.xs + n;
  plan.zt = plan.z + N;
  plan.alpha = plan.zt + zt_elems;
  plan.alpha_t = plan.alpha + K;
  auto build = [&]() -> stark_status {
    STARK_TRY(buf_acquire(ctx, ctx->poly, s));
    STARK_TRY(ensure_buf(ctx, ctx->poly, (poly_tree_elems(t) + 5 * K) * sizeof(fe)));
    fe* mem = (fe*)ctx->poly.ptr;
    fe* W = mem + poly_tree_elems(t);  // the reciprocal's 4 K, then rev_N(Z_top)
    STARK_TRY(poly_tree_build(ctx, d_xs, t, mem, s));
    STARK_HIP(ctx, hipMemcpyAsync(plan.xs, d_xs, n * sizeof(fe), hipMemcpyDeviceToDevice, s));
    if (zt_elems)
      STARK_HIP(ctx, hipMemcpyAsync(plan.zt, t.zt, zt_elems * sizeof(fe), hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(poly_rev_top_kernel, dim3(grid_for(K)), dim3(256), 0, s, (const fe*)t.z, (uint64_t)N,
                       t.levels > 0 ? 1 : 0, (uint64_t)K, W + 4 * K);
    STARK_HIP(ctx, hipGetLastError());
    STARK_TRY(poly_recip_device(ctx, W + 4 * K, K, log_k, to_dev(FieldHost::get().one()), plan.alpha, W, s));
    const Twiddles *fwd, *inv;
    STARK_TRY(tree_twiddles(ctx, log_k + 1, &fwd, &inv));
    STARK_TRY(ntt_device_from(ctx, plan.alpha, 1, plan.alpha_t, log_k + 1, 1, *fwd, false, s));
    // the leaf level (the tree's levels above overwrote theirs; they are taken from their kept transforms)
    hipLaunchKernelGGL(poly_leaf_kernel<false>, dim3(grid_for(N)), dim3(kPolyThreads), 0, s, d_xs, (const fe*)nullptr,
                       (const fe*)nullptr, (uint64_t)n, (uint64_t)N, pc.r2, plan.z, (fe*)nullptr);
    STARK_HIP(ctx, hipGetLastError());
    STARK_TRY(buf_release(ctx, ctx->poly, s));
    // complete on return: the plan is applied on any stream, and d_xs is the caller's staging
    STARK_HIP(ctx, hipStreamSynchronize(s));
    return STARK_OK;
  };
  const stark_status st = build();
  if (st != STARK_OK) eval_plan_release(ctx, plan);
  return st;
}

// Polynomials per chunk of an application: their scratch (eval_plan_poly_elems) stays under the prove-batch limit,
// at least one polynomial; a grid's second coordinate, the transforms' 32-bit node count (up to N / 32 per
// polynomial) and the flat launches' block count (2 K' or 2 N lanes per polynomial) bound a chunk too.
size_t eval_plan_chunk(const stark_ctx* ctx, const EvalPlan& plan, size_t deg_plus_1, uint32_t batch) {
  const size_t limit = ctx->prove_batch_limit ? ctx->prove_batch_limit : kDefaultProveBatchLimit;
  const size_t K1 = (size_t)1 << recip_log(deg_plus_1);
  const size_t chunk = std::max<size_t>(1, limit / (eval_plan_poly_elems(K1, plan.N) * sizeof(fe)));
  return std::min<size_t>({chunk, batch, 65535, std::max<size_t>(1, ((size_t)1 << 31) / std::max(plan.N, K1))});
}

stark_status eval_plan_apply(stark_ctx* ctx, const EvalPlan& plan, const fe* d_polys, size_t deg_plus_1,
                             size_t poly_stride, uint32_t batch, fe* d_out, size_t out_stride, hipStream_t s) {
  if (batch == 0 || plan.n == 0) return STARK_OK;
  if (deg_plus_1 > plan.max_deg_plus_1) return STARK_ERR_BAD_LENGTH;
  const size_t n = plan.n, N = plan.N;
  if (deg_plus_1 == 0) {
    STARK_HIP(ctx, hipMemset2DAsync(d_out, out_stride * sizeof(fe), 0, n * sizeof(fe), batch, s));
    return STARK_OK;
  }
  const PolyConsts pc = poly_consts();
  const uint32_t log_k = recip_log(deg_plus_1), log_p = log_k + 1;
  const size_t K1 = (size_t)1 << log_k;
  const bool prefix = log_k < plan.log_K;  // alpha mod Y^K' is alpha's first K' coefficients: their transform per call
  const size_t chunk = eval_plan_chunk(ctx, plan, deg_plus_1, batch);
  STARK_TRY(buf_acquire(ctx, ctx->poly, s));
  STARK_TRY(ensure_buf(ctx, ctx->poly, (chunk * eval_plan_poly_elems(K1, N) + (prefix ? 2 * K1 : 0)) * sizeof(fe)));
  fe* R = (fe*)ctx->poly.ptr;   // rev(f_b), K' each
  fe* T = R + chunk * K1;       // rev(f_b) alpha, 2 K' each
  fe* fv = T + chunk * 2 * K1;  // F_b, N each
  fe* G = fv + chunk * N;       // the children's transforms, 2 N each
  const fe* at = plan.alpha_t;
  const Twiddles *pf, *pi;
  STARK_TRY(tree_twiddles(ctx, log_p, &pf, &pi));
  if (prefix) {
    fe* At = G + chunk * 2 * N;
    STARK_TRY(ntt_device_from(ctx, plan.alpha, 1, At, log_p, 1, *pf, false, s));
    at = At;
  }
  for (size_t b0 = 0; b0 < batch; b0 += chunk) {
    const uint32_t B = (uint32_t)std::min<size_t>(chunk, batch - b0);
    hipLaunchKernelGGL(poly_rev_batch_kernel, dim3(grid_for((uint64_t)B * K1)), dim3(256), 0, s,
                       d_polys + (size_t)b0 * poly_stride, (uint64_t)poly_stride, (uint64_t)deg_plus_1, log_k,
                       (uint64_t)B * K1, R);
    STARK_HIP(ctx, hipGetLastError());
    STARK_TRY(ntt_device_from(ctx, R, 1, T, log_p, B, *pf, false, s));
    hipLaunchKernelGGL(poly_shared_mul_kernel, dim3(grid_for((uint64_t)B * 2 * K1)), dim3(256), 0, s, T, at, log_p,
                       (uint64_t)B * 2 * K1, pc.r2);
    STARK_HIP(ctx, hipGetLastError());
    STARK_TRY(ntt_device(ctx, T, log_p, B, *pi, true, s));
    hipLaunchKernelGGL(poly_root_vec_batch_kernel, dim3(grid_for((uint64_t)B * N)), dim3(256), 0, s, (const fe*)T, log_p,
                       plan.log_N, (uint64_t)(deg_plus_1 - 1), (uint64_t)B * N, fv);
    STARK_HIP(ctx, hipGetLastError());
    for (uint32_t lv = plan.levels; lv-- > 0;) {
      const uint32_t log_m = kLeafLog + lv + 1;  // the transforms' size: the parents'
      const uint32_t parents = (uint32_t)(N >> log_m);
      const Twiddles *fwd, *inv;
      STARK_TRY(tree_twiddles(ctx, log_m, &fwd, &inv));
      STARK_TRY(ntt_device(ctx, fv, log_m, B * parents, *fwd, false, s));
      hipLaunchKernelGGL(poly_down_mul_batch_kernel, dim3(grid_for((uint64_t)B * 2 * N)), dim3(256), 0, s, (const fe*)fv,
                         (const fe*)(plan.zt + 2 * N * lv), log_m, (uint64_t)(2 * parents - 1), (uint64_t)B * 2 * N,
                         level_adj(lv > 0), pc.r2, G);
      STARK_HIP(ctx, hipGetLastError());
      STARK_TRY(ntt_device(ctx, G, log_m, B * 2 * parents, *inv, true, s));
      hipLaunchKernelGGL(poly_compact_kernel, dim3(grid_for((uint64_t)B * N)), dim3(256), 0, s, (const fe*)G, log_m,
                         (uint64_t)B * N, fv);
      STARK_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(poly_leaf_eval_batch_kernel, dim3(grid_for(N), B), dim3(kPolyThreads), 0, s, (const fe*)plan.xs,
                       (uint64_t)n, (uint64_t)N, (const fe*)plan.z, (const fe*)fv, pc.r2,
                       d_out + (size_t)b0 * out_stride, (uint64_t)out_stride);
    STARK_HIP(ctx, hipGetLastError());
  }
  return buf_release(ctx, ctx->poly, s);
}

}  // namespace stark

using namespace stark;

// An interpolation plan handle (stark_interp_plan_new): the plan and the context it lives on.
struct stark_interp_plan {
  stark_ctx* ctx = nullptr;
  stark::InterpPlan p;
};

// An evaluation plan handle (stark_eval_plan_new): the plan and the context it lives on.
struct stark_eval_plan {
  stark_ctx* ctx = nullptr;
  stark::EvalPlan p;
};

namespace {

// mul_polys / div_polys (fft.rs:381-432): both inputs zero-padded to n = 2^log_n and transformed, the
// pointwise product (div: by multi_inv of b's transform, zeros kept), transformed back.
stark_status mul_div_polys(stark_ctx* ctx, const uint64_t* a, size_t la, const uint64_t* b, size_t lb,
                           const uint64_t root[4], uint32_t log_n, uint64_t* out, bool div) {
  if (!ctx || !root || !out || (la && !a) || (lb && !b)) return STARK_ERR_BAD_ARG;
  if (log_n > 28) return STARK_ERR_BAD_LENGTH;
  const size_t n = (size_t)1 << log_n;
  if (la > n || lb > n) return STARK_ERR_BAD_LENGTH;
  STARK_HIP(ctx, hipSetDevice(ctx->device));
  const FieldHost& F = FieldHost::get();
  const Twiddles *fwd = nullptr, *inv = nullptr;
  STARK_TRY(get_twiddles(ctx, root, log_n, &fwd));
  uint64_t rinv[4];
  F.to_canonical(F.inv(F.from_canonical(root)), rinv);
  STARK_TRY(get_twiddles(ctx, rinv, log_n, &inv));
  hipStream_t s = ctx->stream;
  STARK_TRY(ensure_buf(ctx, ctx->io, 3 * n * sizeof(fe)));
  fe* da = (fe*)ctx->io.ptr;
  fe* db = da + n;
  fe* dbi = db + n;
  if (la) STARK_HIP(ctx, hipMemcpyAsync(da, a, la * sizeof(fe), hipMemcpyHostToDevice, s));
  if (la < n) STARK_HIP(ctx, hipMemsetAsync(da + la, 0, (n - la) * sizeof(fe), s));
  if (lb) STARK_HIP(ctx, hipMemcpyAsync(db, b, lb * sizeof(fe), hipMemcpyHostToDevice, s));
  if (lb < n) STARK_HIP(ctx, hipMemsetAsync(db + lb, 0, (n - lb) * sizeof(fe), s));
  STARK_TRY(ntt_device(ctx, da, log_n, 2, *fwd, false, s));
  if (div) STARK_TRY(multi_inv_device(ctx, db, dbi, n, s));
  hipLaunchKernelGGL(poly_pointwise_kernel, dim3(grid_for(n)), dim3(256), 0, s, (const fe*)da,
                     (const fe*)(div ? dbi : db), (uint64_t)n, poly_consts().r2, da);
  STARK_HIP(ctx, hipGetLastError());
  STARK_TRY(ntt_device(ctx, da, log_n, 1, *inv, true, s));
  STARK_HIP(ctx, hipMemcpyAsync(out, da, n * sizeof(fe), hipMemcpyDeviceToHost, s));
  STARK_HIP(ctx, hipStreamSynchronize(s));
  return STARK_OK;
}

// lagrange_interp from host buffers; exps non-null: the points are root^exps[i] (xs is then not read).
stark_status interp_host(stark_ctx* ctx, const uint64_t* xs, const uint64_t* root, uint32_t log_order,
                         const uint64_t* exps, const uint64_t* ys, size_t n, uint64_t* out) {
  if (n == 0) return STARK_OK;
  STARK_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DomainHint hint;
  if (exps) {
    if (log_order > 28) return STARK_ERR_BAD_LENGTH;
    for (size_t i = 0; i < n; ++i)
      if (exps[i] >> log_order) return STARK_ERR_BAD_ARG;
    STARK_TRY(get_twiddles(ctx, root, log_order, &hint.tw));
    hint.log_order = log_order;
  }
  // staging: xs, ys, out, the exponents
  STARK_TRY(ensure_buf(ctx, ctx->io, 3 * n * sizeof(fe) + n * sizeof(uint64_t)));
  fe* d_xs = (fe*)ctx->io.ptr;
  fe* d_ys = d_xs + n;
  fe* d_out = d_ys + n;
  uint64_t* d_exps = (uint64_t*)(d_out + n);
  STARK_HIP(ctx, hipMemcpyAsync(d_ys, ys, n * sizeof(fe), hipMemcpyHostToDevice, s));
  if (exps) {
    STARK_HIP(ctx, hipMemcpyAsync(d_exps, exps, n * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    hint.d_exps = d_exps;
    STARK_TRY(poly_domain_points(ctx, *hint.tw, d_exps, n, d_xs, s));
  } else {
    STARK_HIP(ctx, hipMemcpyAsync(d_xs, xs, n * sizeof(fe), hipMemcpyHostToDevice, s));
  }
  STARK_TRY(buf_acquire(ctx, ctx->poly, s));
  STARK_TRY(ensure_buf(ctx, ctx->poly, lagrange_scratch_elems(n, exps ? &hint : nullptr) * sizeof(fe)));
  STARK_TRY(lagrange_interp_device(ctx, d_xs, d_ys, n, d_out, (fe*)ctx->poly.ptr, s, exps ? &hint : nullptr, nullptr));
  STARK_TRY(buf_release(ctx, ctx->poly, s));
  STARK_HIP(ctx, hipMemcpyAsync(out, d_out, n * sizeof(fe), hipMemcpyDeviceToHost, s));
  STARK_HIP(ctx, hipStreamSynchronize(s));
  return STARK_OK;
}

}  // namespace

extern "C" {

stark_status stark_zpoly(stark_ctx* ctx, const uint64_t* xs, size_t n, uint64_t* out) {
  if (!ctx || !out || (n && !xs)) return STARK_ERR_BAD_ARG;
  if (n == 0) {
    out[0] = 1;
    out[1] = out[2] = out[3] = 0;
    return STARK_OK;
  }
  STARK_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  PolyTree t;
  poly_tree_plan(n, t);
  STARK_TRY(ensure_buf(ctx, ctx->io, (2 * n + 1) * sizeof(fe)));
  fe* d_xs = (fe*)ctx->io.ptr;
  fe* d_out = d_xs + n;
  STARK_HIP(ctx, hipMemcpyAsync(d_xs, xs, n * sizeof(fe), hipMemcpyHostToDevice, s));
  STARK_TRY(buf_acquire(ctx, ctx->poly, s));
  STARK_TRY(ensure_buf(ctx, ctx->poly, poly_tree_elems(t) * sizeof(fe)));
  STARK_TRY(poly_tree_build(ctx, d_xs, t, (fe*)ctx->poly.ptr, s));
  STARK_TRY(poly_tree_zpoly(ctx, t, d_out, s));
  STARK_TRY(buf_release(ctx, ctx->poly, s));
  STARK_HIP(ctx, hipMemcpyAsync(out, d_out, (n + 1) * sizeof(fe), hipMemcpyDeviceToHost, s));
  STARK_HIP(ctx, hipStreamSynchronize(s));
  return STARK_OK;
}

stark_status stark_lagrange_interp(stark_ctx* ctx, const uint64_t* xs, const uint64_t* ys, size_t n, uint64_t* out) {
  if (!ctx || (n && (!xs || !ys || !out))) return STARK_ERR_BAD_ARG;
  return interp_host(ctx, xs, nullptr, 0, nullptr, ys, n, out);
}

stark_status stark_lagrange_interp_domain(stark_ctx* ctx, const uint64_t root[4], uint32_t log_order,
                                          const uint64_t* exps, const uint64_t* ys, size_t n, uint64_t* out) {
  if (!ctx || !root || (n && (!exps || !ys || !out))) return STARK_ERR_BAD_ARG;
  return interp_host(ctx, nullptr, root, log_order, exps, ys, n, out);
}

stark_status stark_interp_plan_new(stark_ctx* ctx, const uint64_t* xs, size_t n, stark_interp_plan** out) {
  if (!ctx || !out || (n && !xs)) return STARK_ERR_BAD_ARG;
  *out = nullptr;
  STARK_HIP(ctx, hipSetDevice(ctx->device));
  std::unique_ptr<stark_interp_plan> h(new stark_interp_plan);
  h->ctx = ctx;
  if (n) {
    hipStream_t s = ctx->stream;
    STARK_TRY(ensure_buf(ctx, ctx->io, n * sizeof(fe)));
    STARK_HIP(ctx, hipMemcpyAsync(ctx->io.ptr, xs, n * sizeof(fe), hipMemcpyHostToDevice, s));
    STARK_TRY(interp_plan_build(ctx, (const fe*)ctx->io.ptr, n, nullptr, h->p, s));
  }
  *out = h.release();
  return STARK_OK;
}

stark_status stark_interp_plan_new_domain(stark_ctx* ctx, const uint64_t root[4], uint32_t log_order,
                                          const uint64_t* exps, size_t n, stark_interp_plan** out) {
  if (!ctx || !root || !out || (n && !exps)) return STARK_ERR_BAD_ARG;
  *out = nullptr;
  STARK_HIP(ctx, hipSetDevice(ctx->device));
  std::unique_ptr<stark_interp_plan> h(new stark_interp_plan);
  h->ctx = ctx;
  STARK_TRY(interp_plan_build_domain(ctx, root, log_order, exps, n, h->p, ctx->stream));
  *out = h.release();
  return STARK_OK;
}

stark_status stark_interp_plan_free(stark_interp_plan* plan) {
  if (!plan) return STARK_OK;
  if (plan->p.mem) (void)hipSetDevice(plan->ctx->device);
  interp_plan_release(plan->ctx, plan->p);
  delete plan;
  return STARK_OK;
}

stark_status stark_interp_plan_apply_dev(stark_interp_plan* plan, const uint64_t* d_ys, uint32_t batch,
                                         uint64_t* d_out, void* stream) {
  if (!plan) return STARK_ERR_BAD_ARG;
  const size_t n = plan->p.n;
  if (batch == 0 || n == 0) return STARK_OK;
  if (!d_ys || !d_out) return STARK_ERR_BAD_ARG;
  stark_ctx* ctx = plan->ctx;
  STARK_HIP(ctx, hipSetDevice(ctx->device));
  const InterpValues ys{(const uint8_t*)d_ys, n * sizeof(fe), nullptr};
  const InterpOut o{(uint8_t*)d_out, n * sizeof(fe), false, 0};
  return interp_plan_apply(ctx, plan->p, ys, batch, o, pick_stream(ctx, stream));
}

stark_status stark_interp_plan_apply(stark_interp_plan* plan, const uint64_t* ys, uint32_t batch, uint64_t* out) {
  if (!plan) return STARK_ERR_BAD_ARG;
  const size_t n = plan->p.n;
  if (batch == 0 || n == 0) return STARK_OK;
  if (!ys || !out) return STARK_ERR_BAD_ARG;
  stark_ctx* ctx = plan->ctx;
  STARK_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  // staged a chunk of the application at a time (the values, the coefficients), each chunk behind the last on s
  const size_t chunk = interp_plan_chunk(ctx, plan->p, batch);
  STARK_TRY(ensure_buf(ctx, ctx->io, 2 * chunk * n * sizeof(fe)));
  fe* d_ys = (fe*)ctx->io.ptr;
  fe* d_out = d_ys + chunk * n;
  const InterpValues v{(const uint8_t*)d_ys, n * sizeof(fe), nullptr};
  const InterpOut o{(uint8_t*)d_out, n * sizeof(fe), false, 0};
  for (size_t b0 = 0; b0 < batch; b0 += chunk) {
    const size_t B = std::min<size_t>(chunk, batch - b0), at = 4 * b0 * n;
    STARK_HIP(ctx, hipMemcpyAsync(d_ys, ys + at, B * n * sizeof(fe), hipMemcpyHostToDevice, s));
    STARK_TRY(interp_plan_apply(ctx, plan->p, v, (uint32_t)B, o, s));
    STARK_HIP(ctx, hipMemcpyAsync(out + at, d_out, B * n * sizeof(fe), hipMemcpyDeviceToHost, s));
  }
  STARK_HIP(ctx, hipStreamSynchronize(s));
  return STARK_OK;
}

stark_status stark_lagrange_interp_batch(stark_ctx* ctx, const uint64_t* xs, const uint64_t* ys, size_t n,
                                         uint32_t batch, uint64_t* out) {
  if (!ctx) return STARK_ERR_BAD_ARG;
  if (n == 0 || batch == 0) return STARK_OK;
  if (!xs || !ys || !out) return STARK_ERR_BAD_ARG;
  stark_interp_plan* plan = nullptr;
  STARK_TRY(stark_interp_plan_new(ctx, xs, n, &plan));
  const stark_status st = stark_interp_plan_apply(plan, ys, batch, out);
  stark_interp_plan_free(plan);
  return st;
}

stark_status stark_eval_poly_multipoint(stark_ctx* ctx, const uint64_t* poly, size_t deg_plus_1, const uint64_t* xs,
                                        size_t n, uint64_t* out) {
  if (!ctx || (n && (!xs || !out)) || (deg_plus_1 && !poly)) return STARK_ERR_BAD_ARG;
  if (n == 0) return STARK_OK;
  STARK_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  STARK_TRY(ensure_buf(ctx, ctx->io, (deg_plus_1 + 2 * n) * sizeof(fe)));
  fe* d_poly = (fe*)ctx->io.ptr;
  fe* d_xs = d_poly + deg_plus_1;
  fe* d_out = d_xs + n;
  if (deg_plus_1) STARK_HIP(ctx, hipMemcpyAsync(d_poly, poly, deg_plus_1 * sizeof(fe), hipMemcpyHostToDevice, s));
  STARK_HIP(ctx, hipMemcpyAsync(d_xs, xs, n * sizeof(fe), hipMemcpyHostToDevice, s));
  STARK_TRY(eval_multipoint_device(ctx, d_poly, deg_plus_1, d_xs, n, d_out, s));
  STARK_HIP(ctx, hipMemcpyAsync(out, d_out, n * sizeof(fe), hipMemcpyDeviceToHost, s));
  STARK_HIP(ctx, hipStreamSynchronize(s));
  return STARK_OK;
}

stark_status stark_eval_poly_multipoint_dev(stark_ctx* ctx, const uint64_t* d_poly, size_t deg_plus_1,
                                            const uint64_t* d_xs, size_t n, uint64_t* d_out, void* stream) {
  if (!ctx || (n && (!d_xs || !d_out)) || (deg_plus_1 && !d_poly)) return STARK_ERR_BAD_ARG;
  if (n == 0) return STARK_OK;
  STARK_HIP(ctx, hipSetDevice(ctx->device));
  return eval_multipoint_device(ctx, (const fe*)d_poly, deg_plus_1, (const fe*)d_xs, n, (fe*)d_out,
                                pick_stream(ctx, stream));
}

stark_status stark_ctx_set_multipoint_tree_min(stark_ctx* ctx, size_t m) {
  if (!ctx) return STARK_ERR_BAD_ARG;
  ctx->multipoint_tree_min = m;
  return STARK_OK;
}

stark_status stark_eval_plan_new(stark_ctx* ctx, const uint64_t* xs, size_t n, size_t max_deg_plus_1,
                                 stark_eval_plan** out) {
  if (!ctx || !out || (n && !xs) || max_deg_plus_1 == 0) return STARK_ERR_BAD_ARG;
  *out = nullptr;
  STARK_TRY(eval_plan_check(n, max_deg_plus_1));
  STARK_HIP(ctx, hipSetDevice(ctx->device));
  std::unique_ptr<stark_eval_plan> h(new stark_eval_plan);
  h->ctx = ctx;
  hipStream_t s = ctx->stream;
  if (n) {
    STARK_TRY(ensure_buf(ctx, ctx->io, n * sizeof(fe)));
    STARK_HIP(ctx, hipMemcpyAsync(ctx->io.ptr, xs, n * sizeof(fe), hipMemcpyHostToDevice, s));
  }
  STARK_TRY(eval_plan_build(ctx, (const fe*)ctx->io.ptr, n, max_deg_plus_1, h->p, s));
  *out = h.release();
  return STARK_OK;
}

stark_status stark_eval_plan_new_domain(stark_ctx* ctx, const uint64_t root[4], uint32_t log_order,
                                        const uint64_t* exps, size_t n, size_t max_deg_plus_1, stark_eval_plan** out) {
  if (!ctx || !root || !out || (n && !exps) || max_deg_plus_1 == 0) return STARK_ERR_BAD_ARG;
  *out = nullptr;
  STARK_TRY(eval_plan_check(n, max_deg_plus_1));
  if (log_order > 28) return STARK_ERR_BAD_LENGTH;
  for (size_t i = 0; i < n; ++i)
    if (exps[i] >> log_order) return STARK_ERR_BAD_ARG;
  STARK_HIP(ctx, hipSetDevice(ctx->device));
  std::unique_ptr<stark_eval_plan> h(new stark_eval_plan);
  h->ctx = ctx;
  hipStream_t s = ctx->stream;
  const Twiddles* tw = nullptr;
  STARK_TRY(get_twiddles(ctx, root, log_order, &tw));
  fe* d_xs = nullptr;
  if (n) {  // staging: the points, then their exponents (the build returns synchronised: exps is read by then)
    STARK_TRY(ensure_buf(ctx, ctx->io, n * (sizeof(fe) + sizeof(uint64_t))));
    d_xs = (fe*)ctx->io.ptr;
    uint64_t* d_exps = (uint64_t*)(d_xs + n);
    STARK_HIP(ctx, hipMemcpyAsync(d_exps, exps, n * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    STARK_TRY(poly_domain_points(ctx, *tw, d_exps, n, d_xs, s));
  }
  STARK_TRY(eval_plan_build(ctx, d_xs, n, max_deg_plus_1, h->p, s));
  *out = h.release();
  return STARK_OK;
}

stark_status stark_eval_plan_free(stark_eval_plan* plan) {
  if (!plan) return STARK_OK;
  if (plan->p.mem) (void)hipSetDevice(plan->ctx->device);
  eval_plan_release(plan->ctx, plan->p);
  delete plan;
  return STARK_OK;
}

stark_status stark_eval_plan_apply_dev(stark_eval_plan* plan, const uint64_t* d_polys, size_t deg_plus_1,
                                       size_t poly_stride, uint32_t batch, uint64_t* d_out, size_t out_stride,
                                       void* stream) {
  if (!plan) return STARK_ERR_BAD_ARG;
  const size_t n = plan->p.n;
  if (batch == 0 || n == 0) return STARK_OK;
  if (!d_out || (deg_plus_1 && !d_polys) || poly_stride < deg_plus_1 || out_stride < n) return STARK_ERR_BAD_ARG;
  if (deg_plus_1 > plan->p.max_deg_plus_1) return STARK_ERR_BAD_LENGTH;
  stark_ctx* ctx = plan->ctx;
  STARK_HIP(ctx, hipSetDevice(ctx->device));
  return eval_plan_apply(ctx, plan->p, (const fe*)d_polys, deg_plus_1, poly_stride, batch, (fe*)d_out, out_stride,
                         pick_stream(ctx, stream));
}

stark_status stark_eval_plan_apply(stark_eval_plan* plan, const uint64_t* polys, size_t deg_plus_1, uint32_t batch,
                                   uint64_t* out) {
  if (!plan) return STARK_ERR_BAD_ARG;
  const size_t n = plan->p.n, d = deg_plus_1;
  if (batch == 0 || n == 0) return STARK_OK;
  if (!out || (d && !polys)) return STARK_ERR_BAD_ARG;
  if (d > plan->p.max_deg_plus_1) return STARK_ERR_BAD_LENGTH;
  stark_ctx* ctx = plan->ctx;
  STARK_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  // staged a chunk of the application at a time (the coefficients, the values), each chunk behind the last on s
  const size_t chunk = d ? eval_plan_chunk(ctx, plan->p, d, batch) : std::min<size_t>(batch, 65535);
  STARK_TRY(ensure_buf(ctx, ctx->io, chunk * (d + n) * sizeof(fe)));
  fe* d_polys = (fe*)ctx->io.ptr;
  fe* d_out = d_polys + chunk * d;
  for (size_t b0 = 0; b0 < batch; b0 += chunk) {
    const size_t B = std::min<size_t>(chunk, batch - b0);
    if (d) STARK_HIP(ctx, hipMemcpyAsync(d_polys, polys + 4 * b0 * d, B * d * sizeof(fe), hipMemcpyHostToDevice, s));
    STARK_TRY(eval_plan_apply(ctx, plan->p, d_polys, d, d, (uint32_t)B, d_out, n, s));
    STARK_HIP(ctx, hipMemcpyAsync(out + 4 * b0 * n, d_out, B * n * sizeof(fe), hipMemcpyDeviceToHost, s));
  }
  STARK_HIP(ctx, hipStreamSynchronize(s));
  return STARK_OK;
}

stark_status stark_eval_poly_multipoint_batch(stark_ctx* ctx, const uint64_t* polys, size_t deg_plus_1, uint32_t batch,
                                              const uint64_t* xs, size_t n, uint64_t* out) {
  if (!ctx) return STARK_ERR_BAD_ARG;
  if (n == 0 || batch == 0) return STARK_OK;
  if (!xs || !out || (deg_plus_1 && !polys)) return STARK_ERR_BAD_ARG;
  stark_eval_plan* plan = nullptr;
  STARK_TRY(stark_eval_plan_new(ctx, xs, n, deg_plus_1 ? deg_plus_1 : 1, &plan));
  const stark_status st = stark_eval_plan_apply(plan, polys, deg_plus_1, batch, out);
  stark_eval_plan_free(plan);
  return st;
}

// div_polys and mod_polys (poly_utils.rs:235-295) in one call.  With b' = b less its trailing zeros (lb'
// coefficients) and nq = la - lb' + 1: rev(q) = rev(a) / rev(b') mod Y^nq (the power-series reciprocal, whose
// 1 / b'_lead the host takes), then r = a - b q, of which only the coefficients below lb' - 1 can be non-zero
// and need b and q below that only: one more transform-size product.  Every size takes this route (the
// reciprocal's schoolbook phase covers the first 32 coefficients); there is no separate small-size kernel.
stark_status stark_divrem_polys(stark_ctx* ctx, const uint64_t* a, size_t la, const uint64_t* b, size_t lb,
                                uint64_t* q, size_t* q_len, uint64_t* r) {
  if (!ctx || !q || !q_len || (la && !a) || (lb && !b)) return STARK_ERR_BAD_ARG;
  size_t lbp = lb;
  while (lbp && !(b[4 * lbp - 4] | b[4 * lbp - 3] | b[4 * lbp - 2] | b[4 * lbp - 1])) --lbp;
  if (lbp == 0) return STARK_ERR_BAD_ARG;                                // (the reference underflows here)
  if (la < lbp || la > kMultipointTreeLimit) return STARK_ERR_BAD_LENGTH;  // assert!(a.len() >= b.len())
  STARK_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const FieldHost& F = FieldHost::get();
  const size_t nq = la - lbp + 1, m = lbp - 1, lr = lb - 1;
  const uint32_t log_k = recip_log(nq), log_r = recip_log(m);
  const size_t K = (size_t)1 << log_k, Kr = (size_t)1 << log_r;
  // staging: a, b', q, r
  STARK_TRY(ensure_buf(ctx, ctx->io, (la + lbp + nq + lr + 1) * sizeof(fe)));
  fe* d_a = (fe*)ctx->io.ptr;
  fe* d_b = d_a + la;
  fe* d_q = d_b + lbp;
  fe* d_r = d_q + nq;
  STARK_HIP(ctx, hipMemcpyAsync(d_a, a, la * sizeof(fe), hipMemcpyHostToDevice, s));
  STARK_HIP(ctx, hipMemcpyAsync(d_b, b, lbp * sizeof(fe), hipMemcpyHostToDevice, s));
  STARK_TRY(buf_acquire(ctx, ctx->poly, s));
  STARK_TRY(ensure_buf(ctx, ctx->poly, 6 * (K > Kr ? K : Kr) * sizeof(fe)));
  fe* g = (fe*)ctx->poly.ptr;  // 1 / rev(b'), then 5 K of work: the reciprocal's 4 K with rev(b') behind them
  fe* W = g + K;
  hipLaunchKernelGGL(poly_rev_kernel, dim3(grid_for(K)), dim3(256), 0, s, (const fe*)d_b, (uint64_t)lbp,
                     (uint64_t)(lbp < K ? lbp : K), (uint64_t)K, W + 4 * K);
  STARK_HIP(ctx, hipGetLastError());
  STARK_TRY(poly_recip_device(ctx, W + 4 * K, K, log_k, to_dev(F.inv(F.from_canonical(b + 4 * (lbp - 1)))), g, W, s));
  hipLaunchKernelGGL(poly_rev_kernel, dim3(grid_for(K)), dim3(256), 0, s, (const fe*)d_a, (uint64_t)la, (uint64_t)nq,
                     (uint64_t)K, W);
  STARK_HIP(ctx, hipGetLastError());
  STARK_TRY(poly_full_product(ctx, W, g, log_k, W + K, W + 3 * K, s));
  hipLaunchKernelGGL(poly_rev_kernel, dim3(grid_for(nq)), dim3(256), 0, s, (const fe*)(W + K), (uint64_t)nq,
                     (uint64_t)nq, (uint64_t)nq, d_q);
  STARK_HIP(ctx, hipGetLastError());
  if (r && lr) {
    fe* R = (fe*)ctx->poly.ptr;  // b and q below X^m, padded to Kr each, then their transforms
    const size_t qc = nq < m ? nq : m;
    if (m) STARK_HIP(ctx, hipMemcpyAsync(R, d_b, m * sizeof(fe), hipMemcpyDeviceToDevice, s));
    if (m < Kr) STARK_HIP(ctx, hipMemsetAsync(R + m, 0, (Kr - m) * sizeof(fe), s));
    if (qc) STARK_HIP(ctx, hipMemcpyAsync(R + Kr, d_q, qc * sizeof(fe), hipMemcpyDeviceToDevice, s));
    if (qc < Kr) STARK_HIP(ctx, hipMemsetAsync(R + Kr + qc, 0, (Kr - qc) * sizeof(fe), s));
    STARK_TRY(poly_full_product(ctx, R, R + Kr, log_r, R + 2 * Kr, R + 4 * Kr, s));
    hipLaunchKernelGGL(poly_sub_kernel, dim3(grid_for(lr)), dim3(256), 0, s, (const fe*)d_a, (const fe*)(R + 2 * Kr),
                       (uint64_t)m, (uint64_t)lr, d_r);
    STARK_HIP(ctx, hipGetLastError());
  }
  STARK_TRY(buf_release(ctx, ctx->poly, s));
  STARK_HIP(ctx, hipMemcpyAsync(q, d_q, nq * sizeof(fe), hipMemcpyDeviceToHost, s));
  if (r && lr) STARK_HIP(ctx, hipMemcpyAsync(r, d_r, lr * sizeof(fe), hipMemcpyDeviceToHost, s));
  STARK_HIP(ctx, hipStreamSynchronize(s));
  *q_len = nq;
  return STARK_OK;
}

stark_status stark_mul_polys(stark_ctx* ctx, const uint64_t* a, size_t la, const uint64_t* b, size_t lb,
                             const uint64_t root[4], uint32_t log_n, uint64_t* out) {
  return mul_div_polys(ctx, a, la, b, lb, root, log_n, out, false);
}

stark_status stark_div_polys(stark_ctx* ctx, const uint64_t* a, size_t la, const uint64_t* b, size_t lb,
                             const uint64_t root[4], uint32_t log_n, uint64_t* out) {
  return mul_div_polys(ctx, a, la, b, lb, root, log_n, out, true);
}

}  // extern "C"
