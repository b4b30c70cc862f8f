// Witness check: the failing R1CS constraints of a batch of witnesses of one prepared circuit
// (stark_check_r1cs_circuit_batch; no reference counterpart: the reference learns of a bad witness from a
// divisibility assert at the end of its prover, r1cs-stark/src/utils.rs:379-418).
//
// The check reads the circuit's base, coef and slot_wire in place and the decoded witnesses; it builds no
// witness column, no extension and no tree.  One chunk of B witnesses is one upload, these launches and one
// download, with no host round trip in between:
//
//   decode    from_bytes_le of every witness value, its Montgomery image alone (run.rs:354-357)
//   short     one lane per (constraint, witness) for constraints of up to kLongFactor slots: the three sums
//             of coef[slot] x wmont[slot_wire[slot]] (the fill kernels' canonical x Montgomery product),
//             then a b against c; a wave's 64 verdicts are one ballot, written as one word of the
//             witness's failure bitmap
//   long      one wave per (long constraint, witness): lanes stride over the slots, a shuffle tree of
//             fe_add reduces each sum; the verdict is OR-ed into the bitmap word the short kernel wrote.
//             The long constraints depend on the circuit alone: their list is built by the circuit's first
//             check and kept with it (PreparedCircuit::long_list)
//   compact   one workgroup per witness: word popcounts, a prefix sum, n_failed and the first
//             min(cap, n_c) failing indices in ascending order
//   values    one wave per listed failure recomputes its A.w, B.w and C.w (the listed ones are few; keeping
//             the sums of every constraint would cost 96 B per constraint and witness)
#include <string.h>

#include <algorithm>
#include <vector>

#include "host_pool.h"
#include "internal.h"

namespace stark {

namespace {

constexpr uint32_t kLongFactor = 32;  // as running_sum_kernel's (r1cs_trace_dev.hip)

// A stark_r1cs_failure as the device writes it (include/stark_hip.h).
struct FailureRec {
  uint32_t constraint, reserved;
  uint32_t a[8], b[8], c[8];
};
static_assert(sizeof(FailureRec) == sizeof(stark_r1cs_failure), "FailureRec is the ABI's record");

struct CheckArgs {
  const uint32_t* base;       // n_c + 1 slot bases
  const fe* coef;             // 3 a_len canonical coefficients
  const uint32_t* slot_wire;  // 3 a_len wires
  uint64_t a_len;
  uint32_t n_c;
  uint64_t n_wires;
  const fe* wmont;   // batch x n_wires Montgomery witness values
  uint32_t* bitmap;  // batch x words failure bits (words even: one 64-bit word per wave)
  uint32_t words;
  fe r2;             // R^2 mod p
};

__device__ __forceinline__ fe reduce_any(fe v) {  // any 256-bit value < 5.3 p -> canonical
#pragma unroll
  for (int t = 0; t < 5; ++t) fe_reduce_once(v);
  return v;
}

__device__ __forceinline__ bool fe_eq(const fe& x, const fe& y) {
  uint32_t d = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) d |= x.w[k] ^ y.w[k];
  return d == 0;
}

// a b != c for canonical sums: (a R^2 / R) b / R = a b, canonical.
__device__ __forceinline__ bool fails(const fe& a, const fe& b, const fe& c, const fe& r2) {
  return !fe_eq(fe_mul(fe_mul(a, r2), b), c);
}

__global__ void check_decode_kernel(const uint32_t* __restrict__ raw, uint64_t n, fe r2, fe* __restrict__ wmont) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fe v;
#pragma unroll
  for (int k = 0; k < 8; ++k) v.w[k] = raw[8 * i + k];
  fe_store(wmont + i, fe_mul(reduce_any(v), r2));
}

// One factor's sum over the slots b0 .. b0 + n - 1 of third f, slot i0 first and `step` apart.
__device__ __forceinline__ fe factor_sum(const CheckArgs& a, const fe* __restrict__ w, uint32_t f, uint32_t b0,
                                         uint32_t n, uint32_t i0, uint32_t step) {
  const uint64_t s0 = (uint64_t)f * a.a_len + b0;
  fe acc = fe_zero();
  for (uint32_t i = i0; i < n; i += step)
    acc = fe_add(acc, fe_mul(fe_load(a.coef + s0 + i), fe_load(w + a.slot_wire[s0 + i])));
  return acc;
}

__global__ __launch_bounds__(256) void check_short_kernel(CheckArgs a) {
  const uint32_t ci = blockIdx.x * 256 + threadIdx.x;
  if ((ci & ~63u) >= a.n_c) return;  // a whole wave past the last constraint: no word of the bitmap is its
  bool bad = false;
  if (ci < a.n_c) {
    const uint32_t b0 = a.base[ci], n = a.base[ci + 1] - b0;
    if (n <= kLongFactor) {  // (a constraint without terms: 0 x 0 = 0 holds)
      const fe* w = a.wmont + (uint64_t)blockIdx.y * a.n_wires;
      const fe sa = factor_sum(a, w, 0, b0, n, 0, 1);
      const fe sb = factor_sum(a, w, 1, b0, n, 0, 1);
      const fe sc = factor_sum(a, w, 2, b0, n, 0, 1);
      bad = fails(sa, sb, sc, a.r2);
    }
  }
  const unsigned long long m = __ballot(bad);
  if ((threadIdx.x & 63) == 0) {
    uint32_t* dst = a.bitmap + (uint64_t)blockIdx.y * a.words + 2 * (ci >> 6);
    *reinterpret_cast<uint2*>(dst) = make_uint2((uint32_t)m, (uint32_t)(m >> 32));
  }
}

// One factor's sum of a constraint by one wave; every lane ends with the total.
__device__ __forceinline__ fe wave_sum(const CheckArgs& a, const fe* __restrict__ w, uint32_t f, uint32_t b0,
                                       uint32_t n) {
  fe x = factor_sum(a, w, f, b0, n, threadIdx.x & 63, 64);
#pragma unroll
  for (uint32_t d = 32; d >= 1; d >>= 1) {
    fe y;
#pragma unroll
    for (int k = 0; k < 8; ++k) y.w[k] = (uint32_t)__shfl_xor((int)x.w[k], (int)d, 64);
    x = fe_add(x, y);
  }
  return x;
}

__global__ __launch_bounds__(256) void check_long_kernel(CheckArgs a, const uint32_t* __restrict__ list,
                                                         uint32_t n_long) {
  const uint32_t it = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (it >= n_long) return;
  const uint32_t ci = list[it];
  const fe* w = a.wmont + (uint64_t)blockIdx.y * a.n_wires;
  const uint32_t b0 = a.base[ci], n = a.base[ci + 1] - b0;
  const fe sa = wave_sum(a, w, 0, b0, n), sb = wave_sum(a, w, 1, b0, n), sc = wave_sum(a, w, 2, b0, n);
  if ((threadIdx.x & 63) == 0 && fails(sa, sb, sc, a.r2))
    atomicOr(a.bitmap + (uint64_t)blockIdx.y * a.words + (ci >> 5), 1u << (ci & 31));
}

// n_failed[b] and the first capc failing indices of witness b = blockIdx.x, ascending.
__global__ __launch_bounds__(256) void check_compact_kernel(const uint32_t* __restrict__ bitmap, uint32_t words,
                                                            uint32_t capc, uint32_t* __restrict__ n_failed,
                                                            FailureRec* __restrict__ recs) {
  __shared__ uint32_t sh[256];
  const uint32_t t = threadIdx.x;
  const uint32_t* bm = bitmap + (uint64_t)blockIdx.x * words;
  FailureRec* out = recs + (uint64_t)blockIdx.x * capc;
  uint32_t before = 0;
  for (uint32_t w0 = 0; w0 < words; w0 += 256) {
    uint32_t v = w0 + t < words ? bm[w0 + t] : 0;
    const uint32_t cnt = __popc(v);
    sh[t] = cnt;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
      const uint32_t add = t >= d ? sh[t - d] : 0;
      __syncthreads();
      sh[t] += add;
      __syncthreads();
    }
    uint32_t pos = before + sh[t] - cnt;
    before += sh[255];
    while (v && pos < capc) {
      const uint32_t bit = __ffs(v) - 1;
      out[pos].constraint = 32 * (w0 + t) + bit;
      out[pos].reserved = 0;
      v &= v - 1;
      ++pos;
    }
    __syncthreads();
  }
  if (t == 0) n_failed[blockIdx.x] = before;
}

__global__ __launch_bounds__(256) void check_values_kernel(CheckArgs a, const uint32_t* __restrict__ n_failed,
                                                           uint32_t capc, FailureRec* __restrict__ recs) {
  const uint32_t k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= capc || k >= n_failed[blockIdx.y]) return;
  FailureRec* r = recs + (uint64_t)blockIdx.y * capc + k;
  const fe* w = a.wmont + (uint64_t)blockIdx.y * a.n_wires;
  const uint32_t ci = r->constraint;
  const uint32_t b0 = a.base[ci], n = a.base[ci + 1] - b0;
  const fe sa = wave_sum(a, w, 0, b0, n), sb = wave_sum(a, w, 1, b0, n), sc = wave_sum(a, w, 2, b0, n);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      r->a[j] = sa.w[j];
      r->b[j] = sb.w[j];
      r->c[j] = sc.w[j];
    }
  }
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

void long_list_release(stark_ctx* ctx, LongList& l) {
  if (l.d) {  // (then the list is entered in its context, which is alive: its destruction empties the lists)
    hipFree(l.d);
    auto& live = ctx->long_lists;
    live.erase(std::remove(live.begin(), live.end(), &l), live.end());
  }
  l = LongList();
}

void long_lists_release_all(stark_ctx* ctx) {
  for (LongList* l : ctx->long_lists) {
    hipFree(l->d);
    *l = LongList();
  }
  ctx->long_lists.clear();
}

// The circuit's constraints of more than kLongFactor slots, from its slot bases: one download, once.
static stark_status long_list_build(stark_ctx* ctx, const PreparedCircuit& c, hipStream_t s) {
  LongList& l = c.long_list;
  if (l.built) return STARK_OK;
  std::vector<uint32_t> base((size_t)c.n_c + 1), list;
  STARK_HIP(ctx, hipMemcpyAsync(base.data(), c.base, base.size() * 4, hipMemcpyDeviceToHost, s));
  STARK_HIP(ctx, hipStreamSynchronize(s));
  for (uint32_t ci = 0; ci < c.n_c; ++ci)
    if (base[ci + 1] - base[ci] > kLongFactor) list.push_back(ci);
  if (!list.empty()) {
    uint32_t* d = nullptr;
    if (hipMalloc((void**)&d, list.size() * 4) != hipSuccess) {
      (void)hipGetLastError();
      return STARK_ERR_OOM;
    }
    const hipError_t e = hipMemcpyAsync(d, list.data(), list.size() * 4, hipMemcpyHostToDevice, s);
    if (e != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {  // (list is this frame's: read by then)
      hipFree(d);
      return hip_fail(ctx, e != hipSuccess ? e : hipGetLastError(), "long constraint list upload");
    }
    l.d = d;
    l.n = (uint32_t)list.size();
    l.bytes = list.size() * 4;
    ctx->long_lists.push_back(&l);
  }
  l.built = true;
  return STARK_OK;
}

size_t witness_check_bytes(const PreparedCircuit& c, uint32_t cap) {
  const size_t words = 2 * (((size_t)c.n_c + 63) / 64), capc = std::min<size_t>(cap, c.n_c);
  return c.n_wires * 64 + words * 4 + capc * sizeof(FailureRec) + 4;
}

// One chunk: w[0 .. B) through the chain, n_failed[b] and the records of witness b into h_out
// (B counts, then at align256(4 B) the B x capc records).
static stark_status check_chunk(stark_ctx* ctx, const PreparedCircuit& c, const BatchWitness* const* w, uint32_t B,
                                uint32_t capc, uint8_t* h_stage, uint8_t* h_out, hipStream_t s) {
  PhaseClock clk("witness check chunk");
  const FieldHost& F = FieldHost::get();
  const size_t n_wires = c.n_wires, per = n_wires * 32;
  const uint32_t words = 2 * ((c.n_c + 63) / 64);
  const size_t o_raw = 0, o_mont = align256((size_t)B * per), o_bits = o_mont + align256((size_t)B * per),
               o_out = o_bits + align256((size_t)B * words * 4), o_recs = o_out + align256((size_t)B * 4),
               total = o_recs + align256((size_t)B * capc * sizeof(FailureRec));
  STARK_TRY(ensure_buf(ctx, ctx->witness_check, total));
  uint8_t* A = (uint8_t*)ctx->witness_check.ptr;
  // Only the circuit's n_wires values of a witness are read (surplus values stay behind), widened to 32 B.
  const unsigned T = (size_t)B * per > ((size_t)1 << 20) ? std::min<unsigned>(host_threads(), B) : 1;
  host_parallel(T, [&](unsigned t) {
    for (uint32_t b = t; b < B; b += T) {
      uint8_t* dst = h_stage + (size_t)b * per;
      const uint32_t fs = w[b]->field_size;
      if (fs == 32) {
        memcpy(dst, w[b]->values, per);
      } else {
        memset(dst, 0, per);
        for (size_t i = 0; i < n_wires; ++i) memcpy(dst + 32 * i, w[b]->values + i * fs, fs);
      }
    }
  });
  clk.mark("witnesses staged (host)");
  STARK_HIP(ctx, hipMemcpyAsync(A + o_raw, h_stage, (size_t)B * per, hipMemcpyHostToDevice, s));
  uint64_t one_r[4];  // Montgomery image of R = R^2 mod p
  memcpy(one_r, F.one().v, 32);
  CheckArgs a;
  a.base = c.base;
  a.coef = c.coef;
  a.slot_wire = c.slot_wire;
  a.a_len = c.a_len;
  a.n_c = c.n_c;
  a.n_wires = n_wires;
  a.wmont = (const fe*)(A + o_mont);
  a.bitmap = (uint32_t*)(A + o_bits);
  a.words = words;
  a.r2 = to_dev(F.from_canonical(one_r));
  uint32_t* d_nf = (uint32_t*)(A + o_out);
  FailureRec* d_recs = (FailureRec*)(A + o_recs);
  const uint64_t n_all = (uint64_t)B * n_wires;
  hipLaunchKernelGGL(check_decode_kernel, dim3((unsigned)((n_all + 255) / 256)), dim3(256), 0, s,
                     (const uint32_t*)(A + o_raw), n_all, a.r2, (fe*)(A + o_mont));
  hipLaunchKernelGGL(check_short_kernel, dim3((c.n_c + 255) / 256, B), dim3(256), 0, s, a);
  if (c.long_list.n)
    hipLaunchKernelGGL(check_long_kernel, dim3((c.long_list.n + 3) / 4, B), dim3(256), 0, s, a,
                       (const uint32_t*)c.long_list.d, c.long_list.n);
  hipLaunchKernelGGL(check_compact_kernel, dim3(B), dim3(256), 0, s, (const uint32_t*)a.bitmap, words, capc, d_nf,
                     d_recs);
  if (capc)
    hipLaunchKernelGGL(check_values_kernel, dim3((capc + 3) / 4, B), dim3(256), 0, s, a, (const uint32_t*)d_nf, capc,
                       d_recs);
  STARK_HIP(ctx, hipGetLastError());
  // n_failed and the records are one region of the arena: one download
  const size_t down = (o_recs - o_out) + (size_t)B * capc * sizeof(FailureRec);
  STARK_HIP(ctx, hipMemcpyAsync(h_out, A + o_out, down, hipMemcpyDeviceToHost, s));
  clk.mark("upload + launches enqueued");
  STARK_HIP(ctx, hipStreamSynchronize(s));
  clk.mark("chain + download (synced)");
  return STARK_OK;
}

stark_status check_r1cs_batch(stark_ctx* ctx, const PreparedCircuit& c, const BatchWitness* const* w,
                              const uint32_t* at, uint32_t batch, uint32_t* n_failed, stark_r1cs_failure* failures,
                              uint32_t cap) {
  hipStream_t s = ctx->stream;
  STARK_TRY(long_list_build(ctx, c, s));
  const uint32_t capc = (uint32_t)std::min<size_t>(cap, c.n_c);
  const size_t limit = ctx->prove_batch_limit ? ctx->prove_batch_limit : kDefaultProveBatchLimit;
  const size_t per = witness_check_bytes(c, cap);
  // (the arena's parts are 256-B aligned: six parts' slack stays out of the count of a chunk of one)
  const uint32_t chunk =
      (uint32_t)std::min<size_t>(std::max<size_t>(limit > 6 * 256 ? (limit - 6 * 256) / per : 0, 1), batch);
  const size_t out_recs = align256((size_t)chunk * 4), out_bytes = out_recs + (size_t)chunk * capc * sizeof(FailureRec),
               o_stage = align256(out_bytes);
  // Pinned slot 6, the batched prover's staging (both users synchronise before they return): the chunk's counts and
  // records, then its witnesses' 32-B values.  The slot only grows and is host memory outside resident_bytes:
  // about half the chunk's device bytes, so the prove-batch limit bounds it too (include/stark_hip.h says so).
  uint8_t* pin = nullptr;
  STARK_TRY(ctx_pinned(ctx, 6, o_stage + (size_t)chunk * c.n_wires * 32, (void**)&pin));
  for (uint32_t b0 = 0; b0 < batch; b0 += chunk) {
    const uint32_t B = std::min(chunk, batch - b0);
    // (the offsets of a shorter last chunk are its own: check_chunk's layout follows B)
    const size_t recs_off = align256((size_t)B * 4);
    STARK_TRY(check_chunk(ctx, c, w + b0, B, capc, pin + o_stage, pin, s));
    const uint32_t* nf = (const uint32_t*)pin;
    const stark_r1cs_failure* recs = (const stark_r1cs_failure*)(pin + recs_off);
    for (uint32_t b = 0; b < B; ++b) {
      n_failed[at[b0 + b]] = nf[b];
      const size_t k = std::min<size_t>(nf[b], capc);
      if (k) memcpy(failures + (size_t)at[b0 + b] * cap, recs + (size_t)b * capc, k * sizeof(stark_r1cs_failure));
    }
  }
  return STARK_OK;
}

}  // namespace stark

using namespace stark;

extern "C" {

stark_status stark_check_r1cs_circuit_batch(stark_ctx* ctx, const stark_r1cs_circuit* circuit,
                                            const uint8_t* const* wtns, const size_t* wtns_lens, uint32_t batch,
                                            stark_status* statuses, uint32_t* n_failed, stark_r1cs_failure* failures,
                                            uint32_t cap) {
  if (!ctx || !circuit || !wtns || !wtns_lens) return STARK_ERR_BAD_ARG;
  if (batch > 65535) return STARK_ERR_BAD_ARG;  // (the witness coordinate is grid.y; nothing is read or written)
  if (cap > 0 && !failures) return STARK_ERR_BAD_ARG;
  if (circuit->ctx != ctx || circuit->c.world != 1) return STARK_ERR_BAD_ARG;
  if (batch == 0) return STARK_OK;
  STARK_HIP(ctx, hipSetDevice(ctx->device));
  const PreparedCircuit& c = circuit->c;
  std::vector<BatchWitness> ws(batch);
  std::vector<stark_status> sts(batch, STARK_OK);
  std::vector<uint32_t> nf(batch, 0);
  std::vector<const BatchWitness*> live;
  std::vector<uint32_t> at;
  for (uint32_t b = 0; b < batch; ++b) {
    sts[b] = wtns[b] ? witness_host_checks(c, wtns[b], wtns_lens[b], &ws[b]) : STARK_ERR_BAD_ARG;
    if (sts[b] == STARK_OK) {
      live.push_back(&ws[b]);
      at.push_back(b);
    }
  }
  if (!live.empty()) {
    const stark_status st = check_r1cs_batch(ctx, c, live.data(), at.data(), (uint32_t)live.size(), nf.data(), failures, cap);
    if (st != STARK_OK) return st;
    for (uint32_t b : at)
      if (nf[b]) sts[b] = STARK_ERR_CHECK;
  }
  if (n_failed)
    for (uint32_t b = 0; b < batch; ++b) n_failed[b] = nf[b];
  if (statuses) {
    for (uint32_t b = 0; b < batch; ++b) statuses[b] = sts[b];
    return STARK_OK;
  }
  for (uint32_t b = 0; b < batch; ++b)
    if (sts[b] != STARK_OK) return sts[b];
  return STARK_OK;
}

stark_status stark_check_r1cs_circuit(stark_ctx* ctx, const stark_r1cs_circuit* circuit, const uint8_t* wtns,
                                      size_t wtns_len, uint32_t* n_failed, stark_r1cs_failure* failures,
                                      uint32_t cap) {
  // (a null wtns is the witness's error, as in the batch: n_failed 0, nothing written)
  return stark_check_r1cs_circuit_batch(ctx, circuit, &wtns, &wtns_len, 1, nullptr, n_failed, failures, cap);
}

}  // extern "C"
