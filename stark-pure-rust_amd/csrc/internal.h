// Internal declarations shared by the HIP translation units of libstark_hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <chrono>

#include <functional>
#include <future>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "stark_hip.h"
#include "fp_dev.h"
#include "fp_host.h"
#include "host_pool.h"

namespace stark {

// STARK_PROFILE=1: host-side phase timings of a call on stderr (what the
// host waits on between the device phases; the kernels themselves are timed
// with rocprofv3).
struct PhaseClock {
  bool on;
  std::chrono::steady_clock::time_point t0, last;
  explicit PhaseClock(const char* what) : on(enabled()) {
    if (on) {
      t0 = last = std::chrono::steady_clock::now();
      fprintf(stderr, "[stark] %s\n", what);
    }
  }
  static bool enabled() {
    static const bool e = [] {
      const char* v = getenv("STARK_PROFILE");
      return v && v[0] && v[0] != '0';
    }();
    return e;
  }
  void mark(const char* phase) {
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "[stark]   %-28s %8.1f us (at %8.1f)\n", phase,
            std::chrono::duration<double, std::micro>(now - last).count(),
            std::chrono::duration<double, std::micro>(now - t0).count());
    last = now;
  }
};

// Device buffer owned by a context.  A context buffer that calls on different streams share (the NTT
// ping-pong, the batch inverse's scratch, the fold's special_x slot, ...) also carries the stream of
// its last enqueued use: buf_acquire makes a call on another stream wait for everything enqueued on
// that one (an event recorded there at that moment), buf_release notes the stream (api.hip).
struct DevBuf {
  void* ptr = nullptr;
  size_t bytes = 0;
  hipEvent_t ev = nullptr;
  hipStream_t last = nullptr;
};

// Twiddle set for one (root, log_n): everything in Montgomery form.
//   lo[i] = w^i                   i < 2^kb
//   hi[i] = w^(i * 2^kb)          i < 2^(log_n - kb)
//   small_off[l] = offset (in fe) into `small` of the Shoup pairs of w_R^k = w^(k * n / R), k < R/2, R = 2^l
//     (k < R for R = 2^8)
struct Twiddles {
  uint32_t log_n = 0, kb = 0;
  fe* d_lo = nullptr;
  fe* d_hi = nullptr;
  fe* d_small = nullptr; // Shoup pairs (shoup_pair), 2 fe per root
  fe* d_t16 = nullptr;   // Shoup pairs of t16[i] = w^(i n / 2^l16), l16 = min(16, log_n) (18 from 2^25 on)
  fe* d_hi_s = nullptr;  // hi[i] * n^-1   (last pass of an inverse transform)
  fe* d_t16_s = nullptr; // Shoup pairs of t16[i] * n^-1
  uint32_t l16 = 0;
  uint32_t small_off[16] = {0};
  // Full column-twiddle table of the last pass (built on first use when that
  // pass's twiddles do not fit t16): full[c R + r] = w^(c r), c < n/R, r < R;
  // full[1] holds the same times n^-1 for the inverse.  One product per element instead of
  // the two of lo * hi, for one 32-B coalesced read.
  static constexpr uint32_t kFullFused = 0x100;
  struct FullSlot {
    fe* ptr = nullptr;
    // What the slot holds: the last pass's log2 radix for the table above, or kFullFused for the fused
    // producer's per-element table (ntt.hip fused_tw_kernel), which takes its place in a plan whose last
    // boundary is fused-streamed.  A call that needs the other kind rebuilds the slot.
    uint32_t kind = 0;
    uint64_t used = 0;  // cache clock of its last use (LRU eviction, cache_reserve)
    // The fill is enqueued on the stream of the call that first needs the table; a call on another
    // stream waits for this event until the fill is known to be complete (fill = null).
    hipEvent_t ev = nullptr;
    hipStream_t fill = nullptr;
  } full[2];                     // [1]: the table scaled by n^-1
  size_t base_bytes = 0;         // device bytes of the tables above `full` (one allocation at d_lo) and of d_res
  size_t n_small_pairs = 0;      // Shoup pairs in d_small
  // Digit-basis tables (fe_db.h) of w_R^k, k < R/2, for every radix R = 2^l >= 16: the constants of the
  // radix-4 steps (ntt.hip DbPlan).  db_off[l] = offset in u32 into d_db (72 u32 per root).
  uint32_t* d_db = nullptr;
  uint32_t db_off[16] = {0};
  // Residual digit-basis tables of the fused passes (ntt.hip): d_res[m] holds w_{2^m}^e, e < 2^m (72 u32
  // each), m = 4 + log2 of the consumer's radix; built for the boundaries a size's plan fuses.
  uint32_t* d_res[13] = {nullptr};
  HostFp root;      // the root these tables were built for (Montgomery)
  HostFp inv_n;     // n^-1 (Montgomery)

  Twiddles() = default;
  Twiddles(const Twiddles&) = delete;
  Twiddles& operator=(const Twiddles&) = delete;
  // Owns its device memory: the base allocation, the full slots with their events, the residual tables.
  // (The owner makes sure no kernel still reads them: stark_ctx_destroy synchronises the device first.)
  ~Twiddles() {
    if (d_lo) hipFree(d_lo);
    for (FullSlot& f : full) {
      if (f.ptr) hipFree(f.ptr);
      if (f.ev) hipEventDestroy(f.ev);
    }
    for (uint32_t* r : d_res)
      if (r) hipFree(r);
  }
};

// A cached device buffer with the cache clock of its last use.
struct CacheBuf {
  void* ptr = nullptr;
  size_t bytes = 0;
  uint64_t used = 0;
  bool in_use = false;          // held by a call in progress: never evicted (cache_reserve)
  hipEvent_t ev = nullptr;      // the fill's event while it may still run (stream `fill`), as Twiddles::FullSlot::ev
  hipStream_t fill = nullptr;
};

// Default cap on a context's cached tables (the last-pass full twiddle tables, 2^log_n x 32 B per
// direction, and the shared IDX extensions): both directions of a 2^26 transform.
constexpr size_t kDefaultCacheLimit = (size_t)4 << 30;
// Public points from which I2 and Zb2 are columns by default (stark_ctx_set_public_column_min): the smallest
// measured count at which that route wins at 2^13 and at 2^17 steps, for the prover and, with its fixed cost
// of a device round trip against a host interpolation that is small below it, for the verifier
// (profiles/public_column_ab.txt).
constexpr size_t kDefaultPublicColumnMin = 128;
constexpr size_t kDefaultVerifyColumnMin = 1024;
// min(points, coefficients) from which stark_eval_poly_multipoint and the unhinted lagrange_interp descend the
// subproduct tree instead of running the split Horner (stark_ctx_set_multipoint_tree_min): the smallest
// measured min(n, deg_plus_1) from which the tree beats the split Horner by more than three spreads at every
// measured shape (at 8,192 x 8,192 the split Horner still wins, 0.78 ms against 1.86;
// profiles/multipoint_eval_ab.txt).
constexpr size_t kDefaultMultipointTreeMin = 65536;
// Default cap on the device bytes of one chunk of stark_prove_r1cs_circuit_batch (its arena, its three forests
// and the batched FRI's forests and columns; stark_ctx_set_prove_batch_limit): a larger batch runs as consecutive
// chunks.  About 20 x precision x 32 B per proof: some 300 proofs at precision 2^15.
constexpr size_t kDefaultProveBatchLimit = (size_t)6 << 30;
// Default cap on the bytes one chunk of stark_verify_r1cs_circuit_batch stages (the packed openings with their
// records, in pinned host memory and again on the device; stark_ctx_set_verify_batch_limit): a larger batch runs
// as consecutive chunks.  A proof stages its leaves, a 32-B node per tree level of each path and 32 B per record
// (DESIGN.md 5.6.1): 0.9 MB at precision 2^18, some 280 proofs per chunk.
constexpr size_t kDefaultVerifyBatchLimit = (size_t)256 << 20;
// Who derives the batched verifier's transcript by default: 1 the host, 2 the device
// (stark_ctx_set_verify_batch_transcript).
constexpr uint32_t kDefaultVerifyTranscript = 1;
// Who checks the Last elements of stark_verify_low_degree_batch's chain proofs by default: 1 the host workers,
// 2 the device (stark_ctx_set_verify_batch_last).  Measured (profiles/fri_verify_batch_ab.txt): the
// device form costs some 0.075 ms more per call -- three more launches behind the chain, where the host workers
// check the Last elements beside it -- which at 64 proofs is beyond three of the host form's spreads, and the two
// tie from 256 proofs on: the host.
constexpr uint32_t kDefaultVerifyLast = 1;

}  // namespace stark

namespace stark {
struct InterpPlan;
struct EvalPlan;
struct LongList;
}

struct stark_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string last_error;
  stark::DevBuf scratch;   // NTT ping-pong partner
  stark::DevBuf io;        // staging for host-buffer entry points
  stark::DevBuf io2;
  stark::DevBuf fri_cols;    // folded FRI columns (prove_low_degree)
  stark::DevBuf r1cs_arena;  // mk_r1cs_proof working set
  stark::DevBuf trace_arena;  // device trace builder working set (r1cs_trace_dev.hip)
  stark::DevBuf trace_raw;    // the raw constraint section and witness bytes it reads
  stark::DevBuf lde_tmp;      // circuit_lde's step columns and Zb values
  // stark_verify_r1cs_bytes' circuit: built anew by every call, kept for the allocations only (scratch contents)
  stark::DevBuf verify_arena, verify_lde;
  stark::DevBuf ext_idx_tmp;  // an IDX extension too large for the cache cap (this proof only)
  stark::DevBuf inv_tmp;      // the scratch of a second batch inverse sharing a host round trip (r1cs.hip)
  stark::DevBuf spot;         // circuit_spot_values' tables and sums (r1cs.hip)
  stark::DevBuf poly;         // the subproduct tree and the interpolation's working set (poly.hip)
  // Merkle trees reused across calls: [0, 1] FRI layer ping-pong, [2..4] the
  // accumulator, main and linear-combination trees of mk_r1cs_proof.
  stark_merkle_tree* trees[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  std::vector<stark_merkle_tree*> fri_trees;  // one per FRI layer (+ the input's), reused across proofs
  stark::DevBuf fri_misc;                     // per-layer special_x (device transcript)
  // prove_low_degree_batch: one forest per FRI layer (+ the inputs'), special_x per (layer, proof); reused and
  // grown across calls, as pinned slot 5 (the batch's roots and Last values).
  std::vector<stark_merkle_forest*> fri_forests;
  stark::DevBuf fri_batch;
  // stark_prove_r1cs_circuit_batch (r1cs.hip prove_r1cs_batch): one chunk's working set, its accumulator, main
  // and linear-combination forests, and the cap on a chunk's device bytes (0: stark::kDefaultProveBatchLimit);
  // reused across calls, freed when the cap is lowered below what they hold.
  stark::DevBuf prove_batch;
  stark_merkle_forest* r1cs_forests[3] = {nullptr, nullptr, nullptr};
  size_t prove_batch_limit = 0;
  // stark_verify_r1cs_circuit_batch (verify_batch.hip): one chunk's device image (boundary points, records, packed
  // openings, ok bytes), staged in pinned slot 7, and the cap on a chunk's staged bytes (0:
  // stark::kDefaultVerifyBatchLimit); reused across calls, freed when the cap is lowered below what they hold.
  stark::DevBuf verify_batch;
  size_t verify_batch_limit = 0;
  // Who derives a chain proof's indices, challenges and records (stark_ctx_set_verify_batch_transcript): 0 the
  // default (stark::kDefaultVerifyTranscript), 1 the host, 2 the device.
  uint32_t verify_batch_transcript = 0;
  // stark_verify_low_degree_batch (verify_batch.hip) stages its chunks in verify_batch and pinned slot 7 too.  Who
  // checks its Last elements (stark_ctx_set_verify_batch_last): 0 the default (stark::kDefaultVerifyLast), 1 the
  // host, 2 the device; verify_forest: the trees over Last elements too wide for one workgroup (created on first
  // use, reused across calls, released with the staging when the cap is lowered below what they hold).
  uint32_t verify_batch_last = 0;
  stark_merkle_forest* verify_forest = nullptr;
  // pinned host scratch (ctx_pinned)
  void* pinned[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  size_t pinned_bytes[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  hipEvent_t staged = nullptr;  // the last DMA out of pinned slot 3 (r1cs_trace_dev.hip staged_upload)
  // A second stream and an event for work the host overlaps with the main stream (the prover's spot-check
  // openings gathered while its FRI layers still run, r1cs.hip); created on first use.
  hipStream_t aux = nullptr;
  hipEvent_t ev_aux = nullptr;
  // The device trace builder's deferred wire-id flag for the proof being built (stark_prove_r1cs_bytes).
  const uint32_t* trace_err = nullptr;
  // (root canonical limbs, log_n) -> tables
  std::map<std::tuple<uint64_t, uint64_t, uint64_t, uint64_t, uint32_t>, std::unique_ptr<stark::Twiddles>> tw;
  // (log_steps, log_prec, log_world, rank) -> the extension of the index column IDX[i] = i
  // (prove.rs:160-163) at that rank's points: it depends on the trace length only, so every
  // proof of that size shares it (r1cs.hip ext_index_column).
  // Size-only columns of the r1cs prover (r1cs.hip ext_const_column), key (kind, log_steps, log_prec,
  // log_g, rank, os): kind 0 = IDX's extension, 1 = F0's (1 on the first os rows), 2 = 1 / Zb3.
  std::map<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint64_t>, stark::CacheBuf> ext_idx;
  // (root canonical limbs, log_n, rank) -> post[k] = root^(rank k), k < n / world: the one-exchange
  // distributed NTT's twiddle, applied in the rank's last local pass (dist.hip).
  std::map<std::tuple<uint64_t, uint64_t, uint64_t, uint64_t, uint32_t, uint32_t>, stark::CacheBuf> post_tw;
  // Cached tables (full twiddle tables + ext_idx) stay under cache_limit bytes: least recently used
  // ones are freed first (stark::cache_reserve).  stark_ctx_set_cache_limit changes it.
  size_t cache_limit = stark::kDefaultCacheLimit;
  uint64_t cache_clock = 0;
  // Public points from which proofs and verifications take the column route (stark_ctx_set_public_column_min);
  // 0: stark::kDefaultPublicColumnMin.
  size_t public_column_min = 0;
  // min(points, coefficients) from which multi-point evaluation descends the subproduct tree
  // (stark_ctx_set_multipoint_tree_min); 0: stark::kDefaultMultipointTreeMin.
  size_t multipoint_tree_min = 0;
  // The interpolation plans that hold device memory on this context (poly.hip: interp_plan_build enters a plan,
  // interp_plan_release takes it out).  stark_ctx_destroy frees what is left and empties those plans, so a handle
  // or a circuit freed after its context finds nothing to free and touches no context memory.
  std::vector<stark::InterpPlan*> interp_plans;
  // The evaluation plans that hold device memory on this context (poly.hip: eval_plan_build / eval_plan_release),
  // kept and emptied in the same way.
  std::vector<stark::EvalPlan*> eval_plans;
  // stark_check_r1cs_circuit_batch (r1cs_check.hip): one chunk's working set (raw and Montgomery witness values,
  // failure bitmaps, counts and records), reused across calls and freed when the prove-batch cap is lowered below
  // what it holds; and the circuits' long-constraint lists that hold device memory on this context, entered and
  // emptied like the interpolation plans.
  stark::DevBuf witness_check;
  std::vector<stark::LongList*> long_lists;
};

namespace stark {

stark_status hip_fail(stark_ctx* ctx, hipError_t e, const char* what);
#define STARK_HIP(ctx, call)                                  \
  do {                                                        \
    hipError_t e_ = (call);                                   \
    if (e_ != hipSuccess) return ::stark::hip_fail(ctx, e_, #call); \
  } while (0)

#define STARK_TRY(expr)              \
  do {                               \
    stark_status st_ = (expr);       \
    if (st_ != STARK_OK) return st_; \
  } while (0)

// Poison: fill new device allocations and pinned buffers with poison_byte() (api.hip; diagnostics and tests:
// STARK_POISON=1 or stark_test_set_poison).  poison_dev is for an allocation just made, before its first use.
bool poison_on();
int poison_byte();
void poison_dev(void* p, size_t bytes);
// stark_test_poison_ctx's part for the context's trees and forests (merkle.hip): fills the digest area of the
// node buffer (a tree's last 32 bytes, its tail kernels' workgroup counter, stay) and returns the bytes held.
size_t merkle_poison_digests(stark_merkle_tree* t, int byte);
size_t forest_poison_digests(stark_merkle_forest* f, int byte);
stark_status ensure_buf(stark_ctx* ctx, DevBuf& b, size_t bytes);
// Cross-stream use of a context buffer (DevBuf::last): acquire before the first enqueued use on s (s
// waits for what the previous user's stream has enqueued so far), release after the last one.  A
// cached table filled on one stream and read on another: fill_mark records the fill's event, fill_wait
// makes another stream wait for it until it is known to be complete.
stark_status buf_acquire(stark_ctx* ctx, DevBuf& b, hipStream_t s);
stark_status buf_release(stark_ctx* ctx, DevBuf& b, hipStream_t s);
stark_status buf_drain(stark_ctx* ctx, DevBuf& b);  // host-waits for the last use's stream, forgets it
stark_status fill_wait(stark_ctx* ctx, hipEvent_t ev, hipStream_t& fill, hipStream_t s);
stark_status fill_mark(stark_ctx* ctx, hipEvent_t& ev, hipStream_t& fill, hipStream_t s);
// Bytes held by the context's cached tables (full twiddle tables and IDX extensions).
size_t cache_bytes(const stark_ctx* ctx);
// Makes room for `need` more cached bytes under ctx->cache_limit by freeing least recently used
// entries (after a device synchronisation: a kernel of any stream may still read them).  Full
// twiddle tables are always candidates; IDX extensions only with evict_ext (a proof's start, where
// no pointer into one is held).  False when the bytes cannot fit (the caller then does not cache).
bool cache_reserve(stark_ctx* ctx, size_t need, bool evict_ext);
// Context-owned pinned host scratch of at least `bytes` (async copy target).
// Slot 0: gather batches; slot 1: transcript values and roots; slot 2: the device trace builder's
// record-walk tables; slot 3: its upload staging (the raw .r1cs constraint section and witness); slot 4:
// the prover's small host-made uploads (constraint tables at 0, boundary constants from kPinned4ConstsOff),
// so they are asynchronous copies (a pageable copy blocks the host).  Slot 5: prove_low_degree_batch's roots
// and Last values (it grows with the batch; slot 1's fixed layout stays the single proof's).  Slot 6: the batched
// prover's transcript heads (kBatchHeadBytes per proof), then its small per-proof uploads and the witnesses' staging.
// Slot 7: the batched verifier's staging (the image of ctx->verify_batch, its ok bytes included).
constexpr size_t kBatchHeadBytes = 2048;
constexpr size_t kPinned4ConstsOff = 16384;
stark_status ctx_pinned(stark_ctx* ctx, int slot, size_t bytes, void** out);
// Pinned slot 1 (always this size, so no caller's pointer into it moves): [0, 2048) the prover's
// transcript head, [2048, 2560) FRI roots, [2560, 3584) two batch inverses' top levels, [3584, 3588) the
// trace builder's deferred flag, [4096, 16384) the last FRI layer's values.
constexpr size_t kPinned1Bytes = 16384;
constexpr size_t kPinned1InvTopOff = 2560;
constexpr size_t kPinned1TraceErrOff = 3584;
constexpr size_t kPinned1LastOff = 4096;

// Batch inverse (0 -> 0) in phases (field_ops.hip), so that one host round trip can serve two of them:
// multi_inv_up enqueues the up kernels, the caller synchronises its stream, multi_inv_top inverts the
// top level on the host, multi_inv_down enqueues the down kernels.  multi_inv_device does all four.
struct InvPlan {
  struct Level {
    uint64_t n;
    uint32_t chunk, wgs;
    const fe* in;
    fe *out, *pref, *others, *tot;
  };
  std::vector<Level> lv;
  fe* h_top = nullptr;
};
stark_status multi_inv_up(stark_ctx* ctx, const fe* d_in, fe* d_out, uint64_t n, hipStream_t s, DevBuf& buf,
                          fe* h_top, InvPlan& plan);
void multi_inv_top(const InvPlan& plan);
stark_status multi_inv_down(stark_ctx* ctx, const InvPlan& plan, hipStream_t s);
fe* multi_inv_h_top(stark_ctx* ctx, int k);  // top array k < 2 in pinned slot 1 (null: no pinned memory)
stark_status multi_inv_device(stark_ctx* ctx, const fe* d_in, fe* d_out, uint64_t n, hipStream_t s);
// out[i] = sum_k poly[k] xs[i]^k on device buffers (Horner, one point per thread; field_ops.hip).
stark_status eval_poly_device(stark_ctx* ctx, const fe* d_poly, uint64_t deg_plus_1, const fe* d_xs, uint64_t n,
                              fe* d_out, hipStream_t s);
// The same by the split Horner (field_ops.hip: a group of lanes per (coefficient chunk, point), partial sums added by
// further launches of the same kernel); mem holds eval_split_scratch_elems(deg_plus_1, n) elements.
size_t eval_split_scratch_elems(uint64_t deg_plus_1, uint64_t n);
stark_status eval_split_device(stark_ctx* ctx, const fe* d_poly, uint64_t deg_plus_1, const fe* d_xs, uint64_t n,
                               fe* d_out, fe* mem, hipStream_t s);

// The subproduct tree of zpoly / lagrange_interp (poly.hip): n points padded to N = 2^log_N, the top's
// coefficients in z (N), and the transforms of each of the `levels` NTT levels in zt (2 N per level).
struct PolyTree {
  size_t n = 0, N = 0;
  uint32_t log_N = 0, levels = 0;
  fe *z = nullptr, *zt = nullptr;
};
void poly_tree_plan(size_t n, PolyTree& t);
size_t poly_tree_elems(const PolyTree& t);  // elements of device memory a tree takes
stark_status poly_tree_build(stark_ctx* ctx, const fe* d_xs, PolyTree& t, fe* mem, hipStream_t s);
stark_status poly_tree_zpoly(stark_ctx* ctx, const PolyTree& t, fe* d_out, hipStream_t s);  // n + 1 coefficients
// The points are powers of a 2^log_order-th root: x_i = root^d_exps[i] (device exponents below the order;
// tw = the root's tables).  Z'(x_i) is then one transform of that size and a gather.
struct DomainHint {
  const Twiddles* tw = nullptr;
  uint32_t log_order = 0;
  const uint64_t* d_exps = nullptr;
};
// lagrange_interp (poly_utils.rs:409-439) on device buffers (canonical): n coefficients into d_out.  mem holds
// lagrange_scratch_elems(n, hint) elements; *z_out (optional) receives where zpoly(xs)'s n + 1 coefficients
// are in mem.  Asynchronous on s but for the batch inverse's host round trip.
size_t lagrange_scratch_elems(size_t n, const DomainHint* hint);
stark_status lagrange_interp_device(stark_ctx* ctx, const fe* d_xs, const fe* d_ys, size_t n, fe* d_out, fe* mem,
                                    hipStream_t s, const DomainHint* hint, fe** z_out);
// An interpolation plan: what lagrange_interp_device derives from the points alone, in a device buffer of its
// own (ctx->poly is every other call's): the points' Montgomery images (n), inv_den[i] = R^2 / Z'(x_i) (n; 0 for
// a repeated point: the product with a value as it is, any integer below 2^256, is c_i's Montgomery image) and the
// kept transforms of the tree's `levels` NTT levels (2 N each).  Its bytes count in the context's resident bytes.
// A plan that holds memory is entered in ctx->interp_plans by its address: it is not copied or moved while built.
struct InterpPlan {
  size_t n = 0, N = 0, bytes = 0;
  uint32_t log_N = 0, levels = 0;
  fe *mem = nullptr, *xs = nullptr, *inv_den = nullptr, *zt = nullptr;
};
// Builds the plan over the device points d_xs (canonical; hint as lagrange_interp_device's).  Takes ctx->poly for
// its temporaries and the batch inverse's host round trip; the plan is complete when it returns.
stark_status interp_plan_build(stark_ctx* ctx, const fe* d_xs, size_t n, const DomainHint* hint, InterpPlan& plan,
                               hipStream_t s);
// The same from host exponents: the points are root^exps[i] (root canonical, of order 2^log_order; exps checked).
stark_status interp_plan_build_domain(stark_ctx* ctx, const uint64_t root[4], uint32_t log_order, const uint64_t* exps,
                                      size_t n, InterpPlan& plan, hipStream_t s);
// Frees the buffer and takes the plan out of ctx->interp_plans.  A plan never built, or emptied by its context's
// destruction, holds nothing: a no-op that does not read ctx (which may be gone by then).
void interp_plan_release(stark_ctx* ctx, InterpPlan& plan);
// stark_ctx_destroy's part: frees every plan still entered and empties it.
void interp_plans_release_all(stark_ctx* ctx);
// Where a batch's values are: value i of proof b is the 32 bytes at base + b stride + 32 (index ? index[i] : i),
// 16-B aligned, taken as they are (any integer below 2^256).
struct InterpValues {
  const uint8_t* base = nullptr;
  uint64_t stride = 0;
  const uint32_t* index = nullptr;
};
// Where the coefficients go: proof b's n coefficients at base + b stride (16-B aligned), canonical or (mont) as
// Montgomery images, then zeros up to `fill` coefficients where fill > n.
struct InterpOut {
  uint8_t* base = nullptr;
  uint64_t stride = 0;
  bool mont = false;
  uint64_t fill = 0;
};
// lagrange_interp of `batch` value vectors over the plan's points: one fixed chain of launches per chunk of
// proofs (3 N elements of ctx->poly per proof, chunks under the context's prove-batch limit), no host
// synchronisation.
stark_status interp_plan_apply(stark_ctx* ctx, const InterpPlan& plan, const InterpValues& ys, uint32_t batch,
                               const InterpOut& out, hipStream_t s);
// g = 1 / h mod Y^(2^log_k) (canonical, 2^log_k coefficients into d_g; log_k >= 5) for h of hlen coefficients
// (the rest zero) with h(0) != 0: h0_inv = the Montgomery image of 1 / h(0).  A schoolbook phase in one workgroup
// up to the tree's leaf size, then Newton steps g <- g (2 - h g) by transforms on tree_twiddles' roots.  mem holds
// 4 2^log_k elements.
stark_status poly_recip_device(stark_ctx* ctx, const fe* d_h, size_t hlen, uint32_t log_k, const fe& h0_inv, fe* d_g,
                               fe* mem, hipStream_t s);
// f (deg_plus_1 >= 1 coefficients) at the points of a built tree, by the descent of the tree (the transpose of
// the interpolation's way up): n values into d_out.  d_xs are the points the tree was built from.  mem holds
// poly_descent_elems(t, deg_plus_1) elements; t.z is overwritten with the leaf level.  Fully asynchronous on s.
size_t poly_descent_elems(const PolyTree& t, size_t deg_plus_1);
stark_status poly_tree_eval(stark_ctx* ctx, const PolyTree& t, const fe* d_xs, const fe* d_f, size_t deg_plus_1,
                            fe* d_out, fe* mem, hipStream_t s);
// Multi-point evaluation on device buffers by the route stark_eval_poly_multipoint documents (takes ctx->poly).
stark_status eval_multipoint_device(stark_ctx* ctx, const fe* d_poly, size_t deg_plus_1, const fe* d_xs, size_t n,
                                    fe* d_out, hipStream_t s);
// An evaluation plan: what poly_tree_eval derives from the points and the degree bound alone, in a
// device buffer of its own: the points (n, canonical), the tree's leaf level z (N), the kept transforms of its
// `levels` NTT levels (2 N each), alpha = 1 / rev_N(Z_top) mod Y^K as coefficients (K = 2^log_K, the reciprocal's
// length for max_deg_plus_1 coefficients; a shorter polynomial uses a prefix) and alpha's transform of 2 K points,
// which an application at that K takes as it is.  Its bytes count in the context's resident bytes.  A plan that holds
// memory is entered in ctx->eval_plans by its address: it is not copied or moved while built.
struct EvalPlan {
  size_t n = 0, N = 0, K = 0, max_deg_plus_1 = 0, bytes = 0;
  uint32_t log_N = 0, levels = 0, log_K = 0;
  fe *mem = nullptr, *xs = nullptr, *z = nullptr, *zt = nullptr, *alpha = nullptr, *alpha_t = nullptr;
};
// STARK_ERR_BAD_LENGTH where max_deg_plus_1 + N is beyond the tree route's limit (before anything is allocated).
stark_status eval_plan_check(size_t n, size_t max_deg_plus_1);
// Builds the plan over the device points d_xs (canonical).  Takes ctx->poly for the tree and the reciprocal; no host
// round trip but the synchronisation at the end: the plan is complete when it returns.
stark_status eval_plan_build(stark_ctx* ctx, const fe* d_xs, size_t n, size_t max_deg_plus_1, EvalPlan& plan,
                             hipStream_t s);
// Frees the buffer and takes the plan out of ctx->eval_plans; as interp_plan_release for a plan that holds nothing.
void eval_plan_release(stark_ctx* ctx, EvalPlan& plan);
// stark_ctx_destroy's part: frees every plan still entered and empties it.
void eval_plans_release_all(stark_ctx* ctx);
// Scratch elements of ctx->poly an application takes per polynomial, K' = 2^log_k the reciprocal's length for its
// deg_plus_1: rev(f) (K'), its product with alpha (2 K'), the vector F (N) and its children's transforms (2 N).
// A chunk shares 2 K' more (alpha's transform) where K' is below the plan's K.
inline size_t eval_plan_poly_elems(size_t K1, size_t N) { return 3 * K1 + 3 * N; }
// Polynomials per chunk of an application (scratch under the prove-batch limit, at least one).
size_t eval_plan_chunk(const stark_ctx* ctx, const EvalPlan& plan, size_t deg_plus_1, uint32_t batch);
// Polynomial b's deg_plus_1 coefficients at d_polys + b poly_stride at the plan's points, its n values to
// d_out + b out_stride (strides in elements): poly_tree_eval's chain for a chunk at a time, the same number of
// launches as for one polynomial, no host synchronisation.  deg_plus_1 = 0 writes zeros.
stark_status eval_plan_apply(stark_ctx* ctx, const EvalPlan& plan, const fe* d_polys, size_t deg_plus_1,
                             size_t poly_stride, uint32_t batch, fe* d_out, size_t out_stride, hipStream_t s);
// d_xs[i] = root^d_exps[i], canonical (tw = the root's tables).
stark_status poly_domain_points(stark_ctx* ctx, const Twiddles& tw, const uint64_t* d_exps, size_t n, fe* d_xs,
                                hipStream_t s);

// Context-owned Merkle tree slot (created on first use).
stark_status ctx_tree(stark_ctx* ctx, int slot, stark_merkle_tree** out);
hipStream_t pick_stream(stark_ctx* ctx, void* stream);

// Returns tables for `root` (canonical limbs) of order exactly 2^log_n, or
// STARK_ERR_BAD_ROOT.  Cached per context.
stark_status get_twiddles(stark_ctx* ctx, const uint64_t root[4], uint32_t log_n, const Twiddles** out);

// Device NTT over `batch` contiguous transforms (in place, canonical values).
// post != nullptr: output k of each transform is multiplied by post[k] (Montgomery images, n entries)
// in the last pass's store (the one-exchange distributed NTT's twiddle, dist.hip).
stark_status ntt_device(stark_ctx* ctx, fe* d_data, uint32_t log_n, uint32_t batch, const Twiddles& tw,
                        bool inverse, hipStream_t stream, const fe* post = nullptr);
// Forward/inverse transform of src's batch columns of 2^(log_n - zero_log)
// elements, zero-extended to 2^log_n, into d_data (zero_log <= the plan's
// first radix); the zero tail is neither stored nor read.
uint32_t ntt_first_log_r(uint32_t log_n);  // log2 of the first pass's radix
stark_status ntt_device_from(stark_ctx* ctx, const fe* src, uint32_t zero_log, fe* d_data, uint32_t log_n,
                             uint32_t batch, const Twiddles& tw, bool inverse, hipStream_t stream,
                             const fe* post = nullptr);
// The forward transform's first pass alone over src's zero-extended columns (as ntt_device_from), stored
// transposed and canonical: out[c][t A + j] = sum_r src[c][j + r A] w_T^(r t), T = 2^*log_t (the plan's
// first radix), A = n / T, w_T = w^A.  Then X[c][i] = sum_j w^(i j) out[c][(i mod T) A + j]: one output of
// the whole transform is a dot product of length A over a contiguous run (the verifier's spot values).
stark_status ntt_first_pass_tmajor(stark_ctx* ctx, const fe* src, uint32_t zero_log, fe* out, uint32_t log_n,
                                   uint32_t batch, const Twiddles& tw, hipStream_t stream, uint32_t* log_t);

// First pass of a transform whose input is zero beyond its first n >> zero_log elements (best_fft's
// zero padding): skip = the number of leading radix-2 stages that are plain copies (<= zero_log,
// matching the pass's stage pairing); log_in = log2 of the compact input's batch stride.
struct Sparse {
  uint32_t skip, zero_log, log_in;
};

// Merkle internals (merkle.hip).
// Made by the kernel that makes a tree's root (merkle_build's root_fe, where that is the tail kernel; made
// tells whether it was): the root as a field element (fri.rs:135's special_x: the root's LE words reduced
// mod p, times r2) into *out, and the root's words into copy[0..8) (each when non-null).
struct RootFe {
  fe* out;
  fe r2;
  uint32_t* copy;
  bool made;
};
stark_status merkle_build(stark_ctx* ctx, stark_merkle_tree* t, const uint8_t* d_leaves, size_t n, size_t leaf_len,
                          hipStream_t stream, size_t plane_stride = 0, bool level0_ready = false,
                          RootFe* root_fe = nullptr);
stark_status merkle_level0(stark_ctx* ctx, stark_merkle_tree* t, size_t n, hipStream_t stream, uint32_t** level0);
stark_status merkle_root_d2h(stark_ctx* ctx, stark_merkle_tree* t, hipStream_t stream, uint8_t out[32]);
const uint8_t* merkle_root_dev(const stark_merkle_tree* t);
size_t merkle_device_bytes(const stark_merkle_tree* t);  // device memory the tree owns (0 for null)
stark_status merkle_gather(stark_ctx* ctx, stark_merkle_tree* t, const size_t* indices, size_t k,
                           uint8_t* leaves_out, uint8_t* nodes_out, hipStream_t stream, bool sync = true);

struct GatherReq {
  stark_merkle_tree* t;
  const size_t* idx;    // null: the indices are written on the device by `before_launch` (below)
  size_t k;
  uint8_t* leaves_out;  // k * leaf_len bytes
  uint8_t* nodes_out;   // k * depth * 32 bytes
};
// All requests in one pinned upload, one download, one synchronisation.  before_launch (optional) is
// called once the host's indices are in the pinned index array h_idx and before the gather is enqueued,
// with h_idx and each request's first slot in it; it enqueues on `stream` what writes the indices of
// the requests whose idx is null (they must be below the tree's leaf count).
using GatherHook = std::function<stark_status(uint64_t* h_idx, const std::vector<size_t>& first)>;
stark_status merkle_gather_batch(stark_ctx* ctx, const std::vector<GatherReq>& reqs, hipStream_t stream,
                                 const GatherHook& before_launch = GatherHook());

// Merkle forest internals (merkle.hip): `batch` trees of n leaves by one set of launches, tree b's leaves at
// d_leaves + b n leaf_len.  forest_level0 / forest_build(..., level0_ready) as merkle_level0 / merkle_build:
// tree b's leaf digests go to *level0 + b * *stride_words.  fe_out non-null: the launch that makes the roots
// writes root b as a field element (RootFe's role, with *r2) to fe_out[b]; *fe_made tells whether one did.
// plane_stride != 0 (with level0_ready only): tree b's leaves are rows stored as leaf_len / 32 planes of 32 B,
// plane c of row i at d_leaves + b n leaf_len + c plane_stride + 32 i, as merkle_build's; the gathers open them
// through tree b's view.
stark_status forest_level0(stark_ctx* ctx, stark_merkle_forest* f, size_t n, uint32_t batch, uint32_t** level0,
                           size_t* stride_words);
stark_status forest_build(stark_ctx* ctx, stark_merkle_forest* f, const uint8_t* d_leaves, size_t n, size_t leaf_len,
                          uint32_t batch, hipStream_t stream, bool level0_ready = false, fe* fe_out = nullptr,
                          const fe* r2 = nullptr, bool* fe_made = nullptr, size_t plane_stride = 0);
size_t forest_node_bytes(size_t n, uint32_t batch);  // device bytes of such a forest's nodes
// Frees a forest's device memory; the handle stays usable (the next build allocates again).
void forest_release(stark_merkle_forest* f);
// Tree b as the gather code and merkle_root_dev read a tree (owned by the forest, valid until its next build).
stark_merkle_tree* forest_tree(stark_merkle_forest* f, uint32_t b);
// Tree 0's nodes as words, with the words from a tree to the next and from a tree's first node to its root.
const uint32_t* forest_nodes_dev(const stark_merkle_forest* f, uint64_t* stride_words, uint64_t* root_word);
size_t forest_device_bytes(const stark_merkle_forest* f);  // device memory the forest owns (0 for null)

// A rendered JSON text: one uninitialised allocation written once (a std::string would be
// zero-filled first), so a multi-MB proof is assembled by several threads in parallel.
struct JsonText {
  std::unique_ptr<char[]> p;
  size_t n = 0;
  const char* data() const { return p.get(); }
  size_t size() const { return n; }
};

// serde_json text in pieces: fixed text, or a piece whose exact length is known before it is rendered
// (size) and which renders straight into its place (write: returns the end, writes nothing past it), so
// the whole text is sized once and its pieces written in parallel at their offsets (fri.hip).
struct JsonPieces {
  struct Piece {
    std::string text;                    // fixed (or prerendered) text when size is empty
    std::function<size_t()> size;
    std::function<char*(char*)> write;
  };
  std::vector<Piece> pieces;
  void text(const std::string& s);
  void bytes(const uint8_t* p, size_t n);  // p must outlive render()
  // rows of row_len bytes, "[..],[..]" (the caller writes the brackets)
  void byte_rows(const uint8_t* p, size_t rows, size_t row_len);
  void branches(const std::vector<uint8_t>& leaves, size_t leaf_len, const std::vector<uint8_t>& nodes, size_t k,
                size_t depth);
  void render(std::string& o);
  void render(JsonText& o);  // sized, then every piece written at its offset on the host workers
  // renders the pieces added so far into fixed text now (e.g. while the GPU still works)
  void prerender(unsigned max_threads = 16);
};
void fri_proof_json_pieces(const stark_fri_proof* proof, JsonPieces& j);
// The StarkProof's text up to and with "fri_proof": (utils.rs:122-130; fri.hip): the three roots and the
// two sets of openings, which must outlive render().
struct BranchSet {
  const std::vector<uint8_t>& leaves;
  size_t leaf_len;
  const std::vector<uint8_t>& nodes;
  size_t k, depth;
};
void stark_proof_json_head(const uint8_t m_root[32], const uint8_t l_root[32], const uint8_t a_root[32],
                           const BranchSet& main, const BranchSet& lcomb, JsonPieces& j);

// The four main-tree rows a spot check at position j opens (prove.rs:337-362, verify.rs:86-118): j, one
// step back, and the rows one and two thirds of the original steps ahead.
__host__ __device__ inline void spot_rows(size_t j, size_t os, size_t skips, size_t prec, size_t out[4]) {
  out[0] = j;
  out[1] = (j + prec - skips) % prec;
  out[2] = (j + os / 3 * skips) % prec;
  out[3] = (j + os / 3 * 2 * skips) % prec;
}

}  // namespace stark

// FRI and StarkProof values held by the library (fri.hip, r1cs.hip, group.hip).
struct stark_fri_layer {
  bool last = false;
  uint8_t root2[32];
  size_t col_depth = 0, poly_depth = 0;
  std::vector<size_t> col_idx, poly_idx;  // the prover's own indices (a verifier never reads them)
  size_t col_leaf_len = 32, poly_leaf_len = 32;  // (other than 32 only in a handle made from a caller's parts)
  std::vector<uint8_t> col_leaves, col_nodes;    // 32 B leaves, depth*32 B paths
  std::vector<uint8_t> poly_leaves, poly_nodes;
  std::vector<uint8_t> last_values;              // n * 32 B
};

struct stark_fri_proof {
  std::vector<stark_fri_layer> layers;
};

struct stark_r1cs_proof {
  uint8_t m_root[32], l_root[32], a_root[32];
  // The serde_json text: rendered by the prover, or (json_lazy, a handle of stark_r1cs_proof_from_parts) on the
  // first request, once (stark::r1cs_proof_text).
  mutable stark::JsonText json;
  mutable std::once_flag json_once;
  bool json_lazy = false;
  // The parts, for callers that build their own StarkProof value (stark_r1cs_proof_branches / _fri):
  // main and linear-combination openings (leaves, then depth siblings per opening, leaf to root).
  size_t depth = 0;
  // (A prover's handle has 256-B main leaves, 32-B L leaves and one depth; one made from a caller's parts holds
  // whatever it was given, l_depth included.)
  size_t m_leaf_len = 256, l_leaf_len = 32, l_depth = SIZE_MAX;
  size_t depth_of(int which) const { return which == 0 || l_depth == SIZE_MAX ? depth : l_depth; }
  std::vector<uint8_t> m_leaves, m_nodes, l_leaves, l_nodes;
  stark_fri_proof* fri = nullptr;
  ~stark_r1cs_proof() { stark_fri_proof_free(fri); }
};

namespace stark {
// The proof's serde_json text, rendered first where the handle holds parts only (fri.hip).
const JsonText& r1cs_proof_text(const stark_r1cs_proof* proof);
}  // namespace stark

namespace stark {

// R1CS v1 / wtns v2 headers (circom2bellman_core/src/reader.rs:4-89,
// r1cs-stark/src/reader.rs:7-42), r1cs_trace.hip.
struct R1csHeader {
  uint32_t n_wires, n_pub_out, n_pub_in, n_constraints;
  size_t cons_off;  // byte offset of the first constraint
};
struct WtnsHeader {
  uint32_t field_size, n_wit;
  size_t values_off;  // byte offset of witness value 0
};
stark_status parse_r1cs_header(const uint8_t* r1cs, size_t len, R1csHeader* h);
stark_status parse_wtns_header(const uint8_t* wtns, size_t len, WtnsHeader* h);

// The trace of one proof as the provers take it (prove.rs:14-26's arguments), whoever holds it: host arrays,
// a trace builder's columns, or a prepared circuit's with one witness' (r1cs.hip reads it, keeps nothing).
struct TraceView {
  // K F0 F1 F2 S P: coefficients, flags, witness and computational trace, os elements of 4 limbs each
  // (host or device pointers); F0-F2 are null when flag_bytes holds them.
  const uint64_t* col[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  // The flags as 3 x os bytes from a trace builder (calc_flags, run.rs:283-308; flag0 is 1 on every row: the
  // provers then take F0's shared extension instead of extending it), or null.
  const uint8_t* flag_bytes = nullptr;
  const size_t* perm = nullptr;  // permuted_indices, os slots
  size_t os = 0;
  const uint64_t* public_wires = nullptr;  // canonical limbs, 4 per wire
  size_t n_public = 0;
  const size_t* pfi = nullptr;  // public_first_indices, (wire, slot) pairs
  size_t n_pfi = 0;
  size_t n_constraints = 0, n_wires = 0;
  // Every column, the flag bytes and the permutation are device pointers that the single-GPU prover may
  // take with its one pack launch (stark_prove_r1cs_bytes only; a prepared circuit's proofs do not pack).
  bool dev_pack = false;
};

// The R1CS trace built on the device (r1cs_trace_dev.hip): the host
// builder's columns (coefficients, witness, computational as canonical
// elements; flags as bytes; permutation as u64 slots) in ctx->trace_arena,
// plus the small host-side public inputs.
struct DevTrace {
  size_t os = 0, n_constraints = 0, n_wires = 0;
  fe *coef = nullptr, *wit = nullptr, *comp = nullptr;
  uint8_t* flags = nullptr;
  uint64_t* perm = nullptr;
  std::vector<uint64_t> public_wires;       // canonical limbs, 4 per wire
  std::vector<size_t> public_first_indices;  // (wire, slot) pairs
  const uint32_t* d_err = nullptr;           // defer_err: the device's wire-id flag, not yet read
  TraceView view(bool dev_pack) const {
    return {{(const uint64_t*)coef, nullptr, nullptr, nullptr, (const uint64_t*)wit, (const uint64_t*)comp},
            flags, (const size_t*)perm, os, public_wires.data(), public_wires.size() / 4,
            public_first_indices.data(), public_first_indices.size() / 2, n_constraints, n_wires, dev_pack};
  }
};
// A device trace build whose host part (headers, public wires, record walk, the upload of the raw bytes)
// runs once for several contexts: the producer (a group's member 0) does it all and publishes its
// results and its device copies of the raw bytes and walk tables; each consumer waits for `ready`, copies
// those from the producer's device (peer copies, stream-ordered behind `ev`) and builds its own columns.
struct TraceShare {
  R1csHeader hd{};
  WtnsHeader wh{};
  size_t n_public = 0, cons_len = 0, o_raw_w = 0, wbytes = 0, fac_n = 0, base_n = 0;
  uint64_t a_len = 0;
  std::vector<uint64_t> public_wires;
  bool pf_ok = false;
  std::vector<uint64_t> pf_host;
  stark_ctx* src = nullptr;             // the producer's context
  const uint8_t* raw = nullptr;         // its raw bytes (constraint section, then the witness at o_raw_w)
  const uint32_t *fac = nullptr, *base = nullptr;  // its walk tables (device)
  hipEvent_t ev = nullptr;              // recorded on the producer's stream behind those copies
  stark_status status = STARK_OK;       // the producer's host stage (consumers stop on an error)
  std::promise<void> ready_p;           // set once the fields above are final
  std::shared_future<void> ready = ready_p.get_future().share();
};
// defer_err: no read-back when the host finds the public wires' first uses itself; the caller then
// reads d_err (non-zero: a wire id >= n_wires, STARK_ERR_BAD_ARG) at its own first synchronisation.
// share: null (a build of its own), or the group's shared host stage; producer: this call runs it.
stark_status r1cs_trace_device(stark_ctx* ctx, const uint8_t* r1cs, size_t r1cs_len, const uint8_t* wtns,
                               size_t wtns_len, DevTrace* out, bool defer_err = false, TraceShare* share = nullptr,
                               bool producer = false);
// The witness-independent columns of a circuit: the LDEs of K F0 F1 F2 IDX PIDX and the
// inverses of Zb2, Zb3 at the points rank + world j (8 x precision/world; K, F0-F2 and the
// inverses as Montgomery images).  world = 1: the whole domain.  with_zb = false (the verifier,
// which reads only the first six and evaluates Zb2 / Zb3 at its spot positions): 6 x P, no inverses.
stark_status circuit_lde(stark_ctx* ctx, const fe* coef, const uint8_t* flag_bytes, const uint64_t* perm, size_t os,
                         const size_t* public_first_indices, size_t n_pfi, uint32_t world, uint32_t rank, DevBuf& out,
                         hipStream_t s, bool with_zb = true, const fe** colp = nullptr,
                         uint32_t* spot_log_t = nullptr);
// mk_r1cs_proof on a trace view (r1cs.hip).  pre: null, or a prepared circuit's columns (circuit_lde for
// world 1; only S, P and A are extended then).
stark_status mk_r1cs_proof_view(stark_ctx* ctx, const TraceView& v, const fe* pre, stark_r1cs_proof** out);
// Opens the handle of rank `rank` of `world` on a trace view (r1cs.hip: the rank's share of mk_r1cs_proof up
// to the constraint rows).  pre: null, or a circuit's columns prepared for this (world, rank).  Columns a
// builder made on the context stream must be complete (the caller synchronises that stream first).
stark_status dprove_open(stark_ctx* ctx, uint32_t world, uint32_t rank, const TraceView& v, const fe* pre,
                         void* stream, stark_dprove** out);
// A circuit prepared for many proofs (r1cs_trace_dev.hip): everything of a proof that depends on
// the .r1cs alone.  lde = circuit_lde's columns for (world, rank).
struct PreparedCircuit;
// The six circuit columns K F0 F1 F2 IDX PIDX at n positions of the precision domain (a spot build):
// out[(k n + i) 32 ..] = column k at g2^positions[i], canonical little-endian.
stark_status circuit_spot_values(stark_ctx* ctx, const PreparedCircuit& c, const size_t* positions, size_t n,
                                 uint8_t* out, hipStream_t s);
// The constraints of more than kLongFactor slots of a prepared circuit (r1cs_check.hip: one wave each), built by
// the circuit's first witness check and freed with the circuit, or with its context if that goes first.
struct LongList {
  uint32_t* d = nullptr;
  uint32_t n = 0;
  size_t bytes = 0;
  bool built = false;
};
void long_list_release(stark_ctx* ctx, LongList& l);
void long_lists_release_all(stark_ctx* ctx);
struct PreparedCircuit {
  DevBuf arena, lde;
  size_t os = 0, n_wires = 0, n_public = 0;
  uint32_t n_c = 0;
  uint32_t world = 1, rank = 0;  // the points rank + world j of the precision domain (distributed prover)
  bool with_zb = true;           // false: lde holds K F0 F1 F2 IDX PIDX only (the verifier's cold build)
  // Where the six columns K F0 F1 F2 IDX PIDX are (slots of lde, or for the verifier's cold build
  // K's slot 1 and the shared F0 / IDX extensions); K F0-F2 are Montgomery images iff with_zb.
  const fe* col[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  // spot: the verifier's cold build holds no extensions, only the columns' first forward passes
  // (circuit_spot_values; first radix 2^spot_log_t).
  bool spot = false;
  uint32_t spot_log_t = 0;
  uint64_t a_len = 0;
  std::vector<size_t> pfi;
  const uint32_t* base = nullptr;
  const fe* coef = nullptr;
  const uint8_t* flags = nullptr;
  const uint64_t* perm = nullptr;
  const uint32_t* slot_wire = nullptr;
  // The interpolation plan over the boundary points g1^(w_k) (poly.hip), built by the first batched proof or
  // verification that takes it (circuit_public_plan) and freed with the circuit, or with its context if that goes
  // first.  mutable without a lock: a context, and with it its circuits, is driven by one thread at a time.
  mutable InterpPlan pub_plan;
  mutable LongList long_list;  // (as pub_plan: the first witness check builds it)
  // the circuit's columns with one witness' (circuit_witness: dt holds wit, comp and the public wires)
  TraceView view(const DevTrace& dt) const {
    return {{(const uint64_t*)coef, nullptr, nullptr, nullptr, (const uint64_t*)dt.wit, (const uint64_t*)dt.comp},
            flags, (const size_t*)perm, os, dt.public_wires.data(), dt.public_wires.size() / 4, pfi.data(),
            pfi.size() / 2, n_c, n_wires, false};
  }
};
stark_status circuit_build(stark_ctx* ctx, const uint8_t* r1cs, size_t r1cs_len, PreparedCircuit& c);
// The circuit's plan over its boundary points x_k = g1^(pfi[2 k + 1]), g1 = g2^skips of order 2^log_steps (r1cs.hip):
// the batched prover's and verifier's, whose points are the same.  Built on first use (one host round trip).
stark_status circuit_public_plan(stark_ctx* ctx, const PreparedCircuit& c, const HostFp& g2, uint64_t skips,
                                 uint32_t log_steps, hipStream_t s, const InterpPlan** out);
// ---- batched proofs of one prepared circuit (stark_prove_r1cs_circuit_batch) ----
// One witness of a batch, past circuit_witness's host checks: its values (field_size bytes each, value 0 first)
// and the public wires (canonical limbs, 4 per wire).
struct BatchWitness {
  const uint8_t* values = nullptr;
  uint32_t field_size = 0;
  std::vector<uint64_t> public_wires;
};
// The witness stage's device buffers for `batch` proofs, carved by the prover (r1cs.hip), everything batch-major.
// sp: proof b's S column at sp + 2 b steps and P at sp + (2 b + 1) steps (the caller zero-fills it: the columns'
// tails beyond the os trace rows).  h_stage: pinned staging of batch x n_wires x 32 B, the host's at the call.
struct WitnessBatchBufs {
  uint8_t* raw = nullptr;                      // batch x n_wires x 32 B
  fe *wcan = nullptr, *wmont = nullptr;        // batch x n_wires
  uint32_t *list = nullptr, *count = nullptr;  // batch x n_c long factors, batch counters
  fe* sp = nullptr;
  uint64_t steps = 0;
  uint8_t* h_stage = nullptr;
};
// circuit_witness's device part for a batch: one upload, then decode / fill / running sums with a proof coordinate.
stark_status circuit_witness_batch(stark_ctx* ctx, const PreparedCircuit& c, const BatchWitness* const* w,
                                   uint32_t batch, const WitnessBatchBufs& bufs, hipStream_t s);
// circuit_witness's host checks alone (what rejects a witness before anything is enqueued), with the public wires.
stark_status witness_host_checks(const PreparedCircuit& c, const uint8_t* wtns, size_t wtns_len, BatchWitness* out);
// The failing constraints of `batch` witnesses past the host checks (r1cs_check.hip), in consecutive chunks under
// the context's prove-batch limit: witness k's count goes to n_failed[at[k]] and its first min(count, cap) records
// to failures + at[k] cap.  witness_check_bytes: the device bytes one witness of a chunk takes.
stark_status check_r1cs_batch(stark_ctx* ctx, const PreparedCircuit& c, const BatchWitness* const* w,
                              const uint32_t* at, uint32_t batch, uint32_t* n_failed, stark_r1cs_failure* failures,
                              uint32_t cap);
size_t witness_check_bytes(const PreparedCircuit& c, uint32_t cap);
// mk_r1cs_proof for `batch` witnesses of a circuit prepared for world 1 through one launch chain (r1cs.hip
// prove_r1cs_batch), in consecutive chunks under the context's prove-batch limit.  statuses[b] / out[b]: proof
// b's status (STARK_OK, or STARK_ERR_CHECK from the constraint kernel's flags) and handle (null unless STARK_OK).
// The return value is an error of the chain as a whole (no out[b] is set then).
stark_status mk_r1cs_proof_batch(stark_ctx* ctx, const PreparedCircuit& c, const BatchWitness* const* w,
                                 uint32_t batch, stark_r1cs_proof** out, stark_status* statuses);
// lagrange_interp (fri/src/poly_utils.rs:409-439): coefficients, low degree first (r1cs.hip).
std::vector<HostFp> lagrange_interp(const std::vector<HostFp>& xs, const std::vector<HostFp>& ys);
// FRI prover on device values (fri.hip).  fri_enqueue puts every layer on the
// context stream with a device-side transcript and queues the roots' download;
// after the caller's stream synchronisation, fri_finish samples the indices
// and gathers all openings (with the caller's extra requests) in one batch.
struct FriPending;
struct FriPendingDeleter {
  void operator()(FriPending* p) const;
};
using FriPendingPtr = std::unique_ptr<FriPending, FriPendingDeleter>;
// ctx->fri_misc: 16 special_x slots (one per FRI layer; 15 is the distributed fold's) and 16 roots.
constexpr size_t kFriMiscBytes = 16 * sizeof(fe) + 16 * 32;
stark_status fri_enqueue(stark_ctx* ctx, const fe* d_values, size_t n, const uint64_t root[4], size_t max_deg_plus_1,
                         uint32_t excl, FriPendingPtr* out, stark_merkle_tree* tree0 = nullptr,
                         bool sx0_made = false);
stark_status fri_finish(stark_ctx* ctx, FriPending* p, std::vector<GatherReq>& extra, stark_fri_proof** out);
stark_status fri_prove_device(stark_ctx* ctx, const fe* d_values, size_t n, const uint64_t root[4],
                              size_t max_deg_plus_1, uint32_t excl, stark_fri_proof** out);
// prove_low_degree for `batch` vectors of n device values (vector b at d_values + b n) through one launch chain
// and one synchronisation (fri.hip): out[b] = fri_prove_device's proof of vector b; on an error no out[b] is set.
stark_status fri_prove_batch_device(stark_ctx* ctx, const fe* d_values, size_t n, uint32_t batch,
                                    const uint64_t root[4], size_t max_deg_plus_1, uint32_t excl,
                                    stark_fri_proof** out, stark_merkle_forest* forest0 = nullptr,
                                    const std::function<stark_status()>& mid = std::function<stark_status()>());
// forest0 non-null: the caller's forest over the batch vectors (the batched prover's L forest: layer 0's trees
// are not hashed twice), whose root launch wrote layer 0's special_x values where fri_batch_sx0 said.  mid
// (optional) is called once every layer is enqueued and before the openings are gathered: the caller's host
// work beside the FRI kernels.
// fri_batch_sx0 sizes ctx->fri_batch for such a call: special_x of (layer 0, proof b) goes to (*sx0)[b].
stark_status fri_batch_sx0(stark_ctx* ctx, size_t n, uint32_t batch, const uint64_t root[4], size_t max_deg_plus_1,
                           uint32_t excl, fe** sx0);
// Device bytes a batched FRI call holds beyond its input: the folded layers' forests and columns.
size_t fri_batch_bytes(size_t n, uint32_t batch, size_t max_deg_plus_1);
// prove_low_degree's argument checks alone (fri.hip): the status fri_enqueue returns for these arguments
// before it enqueues anything.  n_layers / tw_out may be null.
stark_status fri_check(stark_ctx* ctx, size_t n, const uint64_t root[4], size_t max_deg_plus_1, uint32_t excl,
                       size_t* n_layers, const Twiddles** tw_out);
// One FRI fold on a residue class (stark_fri_fold_dev / _dev_root, fri.hip): special_x from a host root
// (m_root) or a device-resident one (d_m_root).  d_digests non-null: the launch also writes the Blake2s of
// each folded value (n / (4 world) x 32 B, 16-B aligned), the leaf digests of the column's tree.
stark_status fri_fold(stark_ctx* ctx, const uint64_t* values, uint64_t* column, size_t n, const uint64_t root[4],
                      const uint8_t* m_root, const uint8_t* d_m_root, uint32_t world, uint32_t rank,
                      uint8_t* d_digests, void* stream);

// A Merkle tree over n leaves held by residue class over a group's members (member r: leaves r + G j),
// stark_amd/dprove.py DistTree (group.hip): digests hashed where the leaves are, one all-to-all of
// digests, member s builds the subtree of leaves [s nl, (s+1) nl), the subtree roots gathered to every
// member, and the top levels hashed on each (every member's next step reads the root on its own stream).
struct DTree {
  bool blocked = false;
  size_t n = 0, nl = 0, leaf_len = 0;
  std::vector<const uint8_t*> leaves;
  std::vector<stark_merkle_tree*> t;
  std::vector<uint8_t*> levels;  // blocked: G roots then the G - 1 above (root last); else the root
  std::vector<uint8_t> host;
  const uint8_t* d_root(size_t r, size_t G) const { return levels[r] + (blocked ? (2 * G - 2) * 32 : 0); }
  const uint8_t* root() const { return host.data() + host.size() - 32; }
  size_t level_width(size_t G, uint32_t lvl) const { return G >> lvl; }
  const uint8_t* level_node(size_t G, uint32_t lvl, size_t i) const {
    size_t at = 0;
    for (uint32_t l = 0; l < lvl; ++l) at += G >> l;
    return host.data() + 32 * (at + i);
  }
};
// leaves[r]: member r's nl leaves of leaf_len bytes (device).  dtree_commit hashes them;
// dtree_commit_digests takes their digests ready (digests[r]: nl x 32 B on member r, e.g. fri_fold's).
stark_status dtree_commit(stark_group* g, DTree& d, const std::vector<const uint8_t*>& leaves, size_t nl,
                          size_t leaf_len);
stark_status dtree_commit_digests(stark_group* g, DTree& d, const std::vector<const uint8_t*>& leaves, size_t nl,
                                  size_t leaf_len, const std::vector<uint8_t*>& digests);

// Montgomery image of a host value as a device fe (same bytes).
inline fe to_dev(const HostFp& x) {
  fe r;
  for (int i = 0; i < 4; ++i) {
    r.w[2 * i] = (uint32_t)x.v[i];
    r.w[2 * i + 1] = (uint32_t)(x.v[i] >> 32);
  }
  return r;
}

// Shoup pair of a constant w (tools/gen_fe_mul_asm.py shoup_stream): out[0] = w canonical,
// out[1] = wq = floor(w 2^256 / p).  With m = w R mod p (the Montgomery image, R = 2^256),
// w 2^256 = wq p + m exactly, so wq = (2^256 - m) p^-1 mod 2^256 (m = 0 <=> w = 0 <=> wq = 0).
inline void shoup_pair(const HostFp& x, fe out[2]) {
  static constexpr uint64_t kPinv256[4] = {0x3d1e0a6c10000001ull, 0x9a7979b4b396ee4cull, 0x1c6567d766f9dc6eull,
                                           0x8c07d0e2f27cbe4dull};
  uint64_t c[4];
  FieldHost::get().to_canonical(x, c);
  uint64_t neg[4], q[4] = {0, 0, 0, 0};
  unsigned __int128 borrow = 0;
  for (int i = 0; i < 4; ++i) {  // neg = 2^256 - m (mod 2^256)
    const unsigned __int128 d = (unsigned __int128)0 - x.v[i] - borrow;
    neg[i] = (uint64_t)d;
    borrow = (d >> 64) ? 1 : 0;
  }
  for (int i = 0; i < 4; ++i) {  // q = neg * pinv mod 2^256
    unsigned __int128 carry = 0;
    for (int j = 0; i + j < 4; ++j) {
      const unsigned __int128 t = (unsigned __int128)neg[i] * kPinv256[j] + q[i + j] + carry;
      q[i + j] = (uint64_t)t;
      carry = t >> 64;
    }
  }
  memcpy(out[0].w, c, 32);
  memcpy(out[1].w, q, 32);
}

// Digit-basis table of a constant w (fe_db.h): out[9 i + j] = 29-bit limb j of w 2^(32 i) mod p.
inline void db_table(const HostFp& x, uint32_t out[72]) {
  const FieldHost& F = FieldHost::get();
  const HostFp two32 = F.from_u64((uint64_t)1 << 32);
  HostFp cur = x;
  for (int i = 0; i < 8; ++i) {
    uint64_t c[4];
    F.to_canonical(cur, c);
    for (int j = 0; j < 9; ++j) {
      const int bit = 29 * j, word = bit >> 6, sh = bit & 63;
      uint64_t v = c[word] >> sh;
      if (sh > 35 && word < 3) v |= c[word + 1] << (64 - sh);
      out[9 * i + j] = (uint32_t)v & 0x1fffffffu;
    }
    cur = F.mul(cur, two32);
  }
}

}  // namespace stark

// A prepared circuit handle (stark_r1cs_circuit_new, r1cs_trace_dev.hip).
struct stark_r1cs_circuit {
  stark_ctx* ctx = nullptr;
  stark::PreparedCircuit c;
  ~stark_r1cs_circuit() {
    stark::interp_plan_release(ctx, c.pub_plan);
    stark::long_list_release(ctx, c.long_list);
    if (c.arena.ptr) hipFree(c.arena.ptr);
    if (c.lde.ptr) hipFree(c.lde.ptr);
  }
};
