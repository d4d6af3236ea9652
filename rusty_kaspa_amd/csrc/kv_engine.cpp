/* kv_engine.cpp — host side of the MI355X-native transaction-validation engine
 * (PRODUCT code). Implements the C-ABI in include/kaspa_engine_abi.h.
 *
 * The host is deliberately thin: device memory and stream management, batch
 * staging, and the MuHash finalization (one 3072-bit modular inverse per
 * block batch — host work by design, mirroring how the reference computes the
 * final commitment once per block: crypto/muhash/src/u3072.rs:157-183).
 * ALL per-signature and per-input compute runs in HIP kernels; there is no
 * CPU fallback — calls fail loudly when no GPU is present.
 */
#include "kaspa_engine_abi.h"
#include "kv_u3072.h"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <mutex>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <array>
#include <chrono>
#include <deque>
#include <unordered_map>

/* kernels compiled into this TU (single translation unit keeps the build to one
 * hipcc invocation, no -fgpu-rdc) */
#include "kv_secp_kernels.hip"
#include "kv_sighash_kernels.hip"
#include "kv_utxo_kernels.hip"
#include "kv_utxo_commit_kernels.hip"
#include "kv_utxo_rehash_kernels.hip"
#include "kv_utxo_journal_kernels.hip"
#include "kv_utxo_query_kernels.hip"
#include "kv_utxo_changes_kernels.hip"
#include "kv_validate_host.inc"
#include "kv_script_host.inc"

static thread_local std::string g_last_error;

static void set_error(const char *msg) { g_last_error = msg ? msg : ""; }

static void set_error_loc(const char *msg, const char *file, int line,
                          const char *expr) {
  g_last_error = std::string(msg ? msg : "") + " at " + file + ":" +
                 std::to_string(line) + " (" + expr + ")";
}

extern "C" const char *kv_last_error(void) { return g_last_error.c_str(); }

#define HIP_CHECK(expr)                                                        \
  do {                                                                         \
    hipError_t err_ = (expr);                                                  \
    if (err_ != hipSuccess) {                                                  \
      set_error_loc(hipGetErrorString(err_), __FILE__, __LINE__, #expr);       \
      return -2;                                                               \
    }                                                                          \
  } while (0)

struct kv_sig_key {
  uint64_t w[4];
  bool operator==(const kv_sig_key &o) const {
    return ((w[0] ^ o.w[0]) | (w[1] ^ o.w[1]) | (w[2] ^ o.w[2]) |
            (w[3] ^ o.w[3])) == 0;
  }
};
struct kv_sig_key_hash {
  size_t operator()(const kv_sig_key &k) const { return (size_t)k.w[0]; }
};

/* Batches of at least this many signatures run the ladder and the batched
 * finish as two kernels; smaller ones keep the fused kernel (a block-path batch
 * of ~10k signatures is latency-bound and gains nothing from a second launch).
 * Measured crossover: fused is ahead up to 131,072, split from
 * 262,144 on. KV_SCHNORR_SPLIT_MIN in the environment, read once in kv_create,
 * overrides it: 1 forces the split path, a huge value the fused one. */
#ifndef KV_SCHNORR_SPLIT_MIN_DEFAULT
#define KV_SCHNORR_SPLIT_MIN_DEFAULT ((size_t)1 << 18)
#endif

/* Owning, grow-on-demand buffers: every allocation of the engine is one of
 * these two, so a pointer is freed exactly once and never outlives its
 * capacity. OwnedBuf<false> is device memory, OwnedBuf<true> pinned host
 * memory. Non-copyable; moves and swaps hand the allocation over. */
template <bool PINNED> struct OwnedBuf {
  void *p = nullptr;
  size_t cap = 0;
  OwnedBuf() = default;
  OwnedBuf(const OwnedBuf &) = delete;
  OwnedBuf &operator=(const OwnedBuf &) = delete;
  OwnedBuf(OwnedBuf &&o) noexcept { swap(o); }
  OwnedBuf &operator=(OwnedBuf &&o) noexcept {
    swap(o);
    return *this;
  }
  ~OwnedBuf() { reset(); }
  void swap(OwnedBuf &o) noexcept {
    std::swap(p, o.p);
    std::swap(cap, o.cap);
  }
  void reset() {
    if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    cap = 0;
  }
  /* a fresh allocation of exactly `bytes`; the old one is freed first */
  int alloc(size_t bytes) {
    reset();
    if ((PINNED ? hipHostMalloc(&p, bytes) : hipMalloc(&p, bytes)) != hipSuccess) {
      p = nullptr;
      (void)hipGetLastError();
      set_error(PINNED ? "hipHostMalloc failed" : "hipMalloc failed");
      return -2;
    }
    cap = bytes;
    return 0;
  }
  /* at least `need` bytes; growing drops the contents */
  int ensure(size_t need) {
    return cap >= need ? 0 : alloc(need + need / 2 + 256);
  }
  template <class T = uint8_t> T *as() const { return (T *)p; }
};
using DeviceBuf = OwnedBuf<false>;
using PinnedBuf = OwnedBuf<true>;

/* One verify lane: the device chain jobs -> tuples -> bitmap/status of one
 * signature kind, plus the pinned landing buffer of its status readback. The
 * two kinds differ only in the constants of LaneDesc and in which verify
 * kernel runs. */
struct LaneDesc {
  uint32_t tuple_bytes; /* sig64 ‖ pk ‖ msg32 */
  uint32_t msg_off;
  int ecdsa;
  int tev_assemble, tev_verify; /* start event of the timing pair in kv_ctx::tev */
};
enum { LANE_SCHNORR = 0, LANE_ECDSA = 1 }; /* = kv_job::ecdsa */

struct VerifyLane {
  const LaneDesc d;
  DeviceBuf jobs, tuples, bitmap, status;
  /* PINNED: a pageable-dest hipMemcpyAsync blocks the enqueue thread until the
   * producing kernels finish, which serialized the three streams (measured
   * 7.7ms of 8.3ms in the enqueue phase) */
  PinnedBuf h_status;
};

/* per-context validate scratch. Per-ctx so two engine contexts in one process
 * never share device scratch. */
struct ValidateBufs {
  DeviceBuf blob, subhashes, elem_jobs, elements, partials_a, partials_b, tx_hashes;
  VerifyLane lane[2] = {{{128, 96, 0, 2, 6}}, {{132, 97, 1, 4, 8}}};
};

/* One undo record of the journal (kv_utxo_apply_diff): rows are the diff's
 * outpoints, removed side first. `fixed` is values (64 B a row) ‖ keys (36 B a
 * row) ‖ found bitmap (a bit a row), `blob` the long scripts among the values,
 * which refer to them by blob offset. Nothing here names a slot or a live
 * arena offset, so a rehash leaves it valid. */
struct JournalRecord {
  uint64_t token = 0;
  size_t n_removed = 0, n_added = 0;
  DeviceBuf fixed, blob;
  uint64_t blob_bytes = 0;
  size_t n() const { return n_removed + n_added; }
  size_t off_found() const { return (n() * (64 + 36) + 7) & ~(size_t)7; }
  size_t fixed_bytes() const { return off_found() + (n() + 63) / 64 * 8; }
  uint64_t device_bytes() const { return fixed.cap + blob.cap; }
  uint8_t *vals() const { return fixed.as<uint8_t>(); }
  uint8_t *keys() const { return fixed.as<uint8_t>() + n() * 64; }
  unsigned long long *found() const {
    return (unsigned long long *)(fixed.as<uint8_t>() + off_found());
  }
};

struct kv_ctx {
  kv_params params;
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr; /* ecdsa verify chain (overlaps the schnorr chain) */
  hipStream_t stream3 = nullptr; /* optimistic muhash chain (overlaps both) */
  hipEvent_t ev_blob = nullptr;  /* blob upload complete (sync-only, no timing) */
  hipEvent_t ev_sub = nullptr;   /* subhash kernel complete */
  std::mutex mu;
  /* KIP-21 seq-commitment accessor (kv_set_seq_commit_accessor) */
  kv_seq_commit_accessor_fn seqc_fn = nullptr;
  void *seqc_user = nullptr;
  ValidateBufs vb;
  /* per-kernel timing events of the last validate call (kv_get_validate_timings):
   * pairs (start,stop) for subhash, s-assemble, e-assemble, schnorr, ecdsa, muhash */
  hipEvent_t tev[12] = {};
  bool tev_init = false;
  kv_validate_timings last_timings = {};
  /* grow-on-demand device scratch */
  DeviceBuf d_in, d_bitmap, d_status;
  uint64_t cache_hits = 0, cache_misses = 0, cache_insertions = 0;
  /* sig cache ⇔ TransactionValidator sig_cache (crypto/txscript/src/caches.rs:
   * 57-82): verdicts of (txid, entries-digest, input, hash-type, sig, pk)
   * keyed checks survive across calls — the mempool→block revalidation dedup.
   * Key is a blake2b-256 so a collision is cryptographically excluded. */
  std::unordered_map<kv_sig_key, uint8_t, kv_sig_key_hash> sig_cache;
  /* reusable populate-path scratch (capacity persists across calls — a fresh
   * multi-MB vector per block showed up as page-fault spikes in the bench) */
  std::vector<uint8_t> pop_buf, ops_buf, ent_buf;
  /* per-call PINNED upload staging arena: hipMemcpyAsync from pageable host
   * memory blocks the enqueue thread (synchronous staging inside HIP); all
   * per-call H2D uploads bounce through this bump arena instead. Regions
   * stay valid until the call's final stream syncs. */
  PinnedBuf h_stage;
  size_t h_stage_off = 0;
  PinnedBuf h_mu_partial; /* pinned 768B muhash partial landing pad:
    a pageable-dest D2H of even 384B blocks the enqueue thread until the
    whole reduce chain drains (measured ~3.9ms) */
  std::vector<uint64_t> found_buf;
  /* GPU-resident UTXO set */
  DeviceBuf d_utxo;      /* kv::utxo_slot[utxo_cap] */
  uint64_t utxo_cap = 0; /* power of two */
  kv::utxo_slot *table() const { return d_utxo.as<kv::utxo_slot>(); }
  /* out-of-line spk arena (entries with spk_len > 36; flags bit1); its
   * capacity is d_arena.cap */
  DeviceBuf d_arena;
  uint64_t arena_head = 0;
  DeviceBuf d_gjobs, d_gout;
  DeviceBuf d_utxo_fail; /* int; per-ctx: a shared flag would race when two
                            contexts upsert concurrently */
  DeviceBuf d_op_in, d_val_in, d_ent_out;
  /* UTXO commitment scratch (kv_utxo_commit_kernels.hip): sized by the
   * compiled window, never by table capacity. d_cm_fixed holds, in order, the
   * copy-back record, the window's live count, the slot index list, the
   * running accumulators and the final reduce's two partial buffers. */
  DeviceBuf d_cm_fixed, d_cm_elems;
  /* table maintenance (kv_utxo_rehash_kernels.hip): the two small copy-back
   * records of kv_utxo_stats / kv_utxo_rehash, and the export walk's per-entry
   * script references */
  DeviceBuf d_tbl_rec, d_exp_refs;
  /* undo journal (kv_utxo_journal_kernels.hip): oldest record first; tokens
   * only grow. d_jrn_rec is the capture launch's copy-back record. */
  std::deque<JournalRecord> journal;
  uint64_t next_token = 1;
  DeviceBuf d_jrn_rec;
  double last_revert_ms = 0.0; /* kernel_ms of the last kv_utxo_revert */
  /* per-script changes of a record (kv_utxo_changes_kernels.hip): the copy-back
   * record, then the stored keys and staged records of one call. Bounded by
   * the record walked, never by table capacity. */
  DeviceBuf d_chg;
  /* queries by script public key (kv_utxo_query_kernels.hip): the query table
   * as built on the host and its device copy, the balance call's record and
   * per-query sums, the find walk's record, slot list and match records.
   * Bounded by KV_UTXO_QUERY_MAX, the scripts handed in and the scan window. */
  std::vector<uint8_t> q_host;
  DeviceBuf d_q_set, d_q_out, d_q_find;
  bool query_combine = true; /* KV_UTXO_QUERY_COMBINE, read once in kv_create */
  /* split Schnorr verify (launch_schnorr_verify): the ladder kernel's R limbs
   * and pre-status, 121 B per signature. One split verify is in flight per
   * context at a time (ctx->mu held, every caller syncs before the next). */
  DeviceBuf d_sfin;
  size_t schnorr_split_min = KV_SCHNORR_SPLIT_MIN_DEFAULT;

  /* handles are null until kv_create made them: it deletes a half-built
   * context on failure. The buffers free themselves after this body. */
  ~kv_ctx() {
    if (stream) (void)hipStreamDestroy(stream);
    if (stream2) (void)hipStreamDestroy(stream2);
    if (stream3) (void)hipStreamDestroy(stream3);
    if (ev_blob) (void)hipEventDestroy(ev_blob);
    if (ev_sub) (void)hipEventDestroy(ev_sub);
    if (tev_init)
      for (int i = 0; i < 12; i++) (void)hipEventDestroy(tev[i]);
  }
};

/* First line of every extern "C" entry that takes the lock: a null ctx is an
 * error (-1), the context is locked for the rest of the call, and any stale
 * per-thread HIP error is cleared so the launch-config checks below only see
 * THIS call's launches. */
#define KV_ENTER(ctx)                                                          \
  if (!(ctx)) {                                                                \
    set_error((std::string(__func__) + ": null ctx").c_str());                 \
    return -1;                                                                 \
  }                                                                            \
  std::lock_guard<std::mutex> lk((ctx)->mu);                                   \
  (void)hipGetLastError()

extern "C" kv_ctx *kv_create(const kv_params *params) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0) {
    set_error("kv_create: no HIP device available (the engine has no CPU fallback)");
    return nullptr;
  }
  int dev = params && params->device >= 0 ? params->device : 0;
  if (hipSetDevice(dev) != hipSuccess) {
    set_error("kv_create: hipSetDevice failed");
    return nullptr;
  }
  kv_ctx *ctx = new kv_ctx();
  if (params) ctx->params = *params;
  else
    ctx->params = kv_params{1000, 1000, 10000, 0};
  if (hipStreamCreate(&ctx->stream) != hipSuccess ||
      hipStreamCreate(&ctx->stream2) != hipSuccess ||
      hipStreamCreate(&ctx->stream3) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_blob, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_sub, hipEventDisableTiming) != hipSuccess) {
    set_error("kv_create: stream/event creation failed");
    delete ctx;
    return nullptr;
  }
  if (const char *e = getenv("KV_SCHNORR_SPLIT_MIN")) {
    char *end = nullptr;
    unsigned long long v = strtoull(e, &end, 10);
    if (end != e && v > 0) ctx->schnorr_split_min = (size_t)v;
  }
  /* the balance kernel sums a wave's matches first when they all pay into one
   * query (DESIGN.md §3.5 has the measurement); 0 turns that off */
  if (const char *e = getenv("KV_UTXO_QUERY_COMBINE")) ctx->query_combine = e[0] != '0';
  /* fill the shared fixed-base tables (idempotent: every context writes the
   * same final bytes): the two 8-bit tables on one lane, then the joint
   * 16-bit table with one lane per entry */
  hipLaunchKernelGGL(kv::kv_ec_table_init_kernel, dim3(1), dim3(64), 0, ctx->stream);
  hipLaunchKernelGGL(kv::kv_g_joint_init_kernel, dim3(KV_G_JOINT_ENTRIES / 256),
                     dim3(256), 0, ctx->stream);
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) {
    set_error("kv_create: G-table init failed");
    delete ctx;
    return nullptr;
  }
  return ctx;
}

extern "C" void kv_destroy(kv_ctx *ctx) {
  if (!ctx) return;
  delete ctx; /* handles, then every buffer */
  (void)hipGetLastError(); /* teardown calls are fire-and-forget; do not leave
      their errors sticky for the next engine's launch checks (a swallowed
      invalid-argument here surfaced as a spurious failure in the NEXT
      context's first kernel-launch check) */
}

/* ---------------- batched verify entry points ---------------- */

/* Every Schnorr verify launch goes through here (ctx->mu held): the fused
 * kernel below the split threshold, else ladder + batched finish back to back
 * on the same stream. Same outputs either way. */
static int launch_schnorr_verify(kv_ctx *ctx, hipStream_t stream,
                                 const uint8_t *d_tuples, size_t n,
                                 unsigned long long *d_bitmap, uint8_t *d_status) {
  if (n == 0) return 0;
  const unsigned long long grid = (n + 255) / 256;
  if (n < ctx->schnorr_split_min) {
    hipLaunchKernelGGL(kv::kv_schnorr_verify_kernel, dim3(grid), dim3(256), 0,
                       stream, d_tuples, (unsigned long long)n, d_bitmap,
                       d_status);
    return 0;
  }
  if (ctx->d_sfin.ensure(n * 121)) return -2;
  kv::u32 *limbs = ctx->d_sfin.as<kv::u32>();
  uint8_t *pre = ctx->d_sfin.as<uint8_t>() + n * 120;
  hipLaunchKernelGGL(kv::kv_schnorr_ladder_kernel, dim3(grid), dim3(256), 0,
                     stream, d_tuples, (unsigned long long)n, limbs, pre);
  const unsigned long long lanes =
      ((n + KV_FINISH_K - 1) / KV_FINISH_K + 63) / 64 * 64;
  hipLaunchKernelGGL(kv::kv_schnorr_finish_kernel, dim3(lanes / 64), dim3(64), 0,
                     stream, d_tuples, (unsigned long long)n,
                     (const kv::u32 *)limbs, (const uint8_t *)pre, lanes, d_bitmap,
                     d_status);
  return 0;
}

extern "C" int kv_schnorr_finish_batch(void) { return KV_FINISH_K; }

extern "C" int kv_g_comb_fetch(kv_ctx *ctx, uint32_t first, uint32_t count,
                               uint8_t *out64) {
  if (!ctx || (!out64 && count)) {
    set_error("kv_g_comb_fetch: null argument");
    return -1;
  }
  if (first > KV_G_JOINT_ENTRIES || count > KV_G_JOINT_ENTRIES - first) {
    set_error("kv_g_comb_fetch: range exceeds the 65,536-entry table");
    return -1;
  }
  if (count == 0) return 0;
  KV_ENTER(ctx);
  HIP_CHECK(hipMemcpyFromSymbolAsync(out64, HIP_SYMBOL(kv::KV_G_JOINT),
                                     (size_t)count * 64, (size_t)first * 64,
                                     hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return 0;
}

static int verify_batch(kv_ctx *ctx, const uint8_t *tuples, size_t n, size_t rec_size,
                        int ecdsa, uint64_t *bitmap_out, uint8_t *status_out) {
  if (n == 0) return 0;
  KV_ENTER(ctx);
  size_t words = (n + 63) / 64;
  if (ctx->d_in.ensure(n * rec_size) || ctx->d_bitmap.ensure(words * 8) ||
      ctx->d_status.ensure(n))
    return -2;
  uint8_t *d_in = ctx->d_in.as<uint8_t>();
  unsigned long long *d_bitmap = ctx->d_bitmap.as<unsigned long long>();
  uint8_t *d_status = status_out ? ctx->d_status.as<uint8_t>() : nullptr;
  HIP_CHECK(hipMemcpyAsync(d_in, tuples, n * rec_size, hipMemcpyHostToDevice,
                           ctx->stream));
  HIP_CHECK(hipMemsetAsync(d_bitmap, 0, words * 8, ctx->stream));
  int block = 256;
  unsigned long long grid = (n + block - 1) / block;
  if (ecdsa)
    hipLaunchKernelGGL(kv::kv_ecdsa_verify_kernel, dim3(grid), dim3(block), 0, ctx->stream,
                       d_in, (unsigned long long)n, d_bitmap, d_status);
  else if (launch_schnorr_verify(ctx, ctx->stream, d_in, n, d_bitmap, d_status))
    return -2;
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(bitmap_out, d_bitmap, words * 8, hipMemcpyDeviceToHost,
                           ctx->stream));
  if (status_out)
    HIP_CHECK(hipMemcpyAsync(status_out, d_status, n, hipMemcpyDeviceToHost,
                             ctx->stream));
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return 0;
}

extern "C" int kv_verify_schnorr_batch(kv_ctx *ctx, const uint8_t *tuples, size_t n,
                                       uint64_t *bitmap_out) {
  return verify_batch(ctx, tuples, n, 128, 0, bitmap_out, nullptr);
}

/* extended variant exposing per-signature status (valid/invalid/bad-pubkey/bad-sig)
 * — what the validate path consumes to distinguish script errors from false */
extern "C" int kv_verify_schnorr_batch_status(kv_ctx *ctx, const uint8_t *tuples,
                                              size_t n, uint64_t *bitmap_out,
                                              uint8_t *status_out) {
  return verify_batch(ctx, tuples, n, 128, 0, bitmap_out, status_out);
}

extern "C" int kv_verify_ecdsa_batch(kv_ctx *ctx, const uint8_t *tuples, size_t n,
                                     uint64_t *bitmap_out) {
  return verify_batch(ctx, tuples, n, 132, 1, bitmap_out, nullptr);
}

extern "C" int kv_verify_ecdsa_batch_status(kv_ctx *ctx, const uint8_t *tuples, size_t n,
                                            uint64_t *bitmap_out, uint8_t *status_out) {
  return verify_batch(ctx, tuples, n, 132, 1, bitmap_out, status_out);
}

/* ---------------- MuHash host finalization ---------------- */

/* ---- 3072-bit helpers for the modular inverse (binary extended gcd) ---- */

using kv::u3072;

static int big_cmp(const uint64_t *a, const uint64_t *b) {
  for (int i = KVU_LIMBS - 1; i >= 0; i--) {
    if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
  }
  return 0;
}

static void big_sub(uint64_t *a, const uint64_t *b) {
  uint64_t borrow = 0;
  for (int i = 0; i < KVU_LIMBS; i++) {
    uint64_t bi = b[i] + borrow;
    uint64_t nb = (bi < borrow) || (a[i] < bi);
    a[i] -= bi;
    borrow = nb;
  }
}

static void big_shr1(uint64_t *a, uint64_t top_bit) {
  for (int i = 0; i < KVU_LIMBS; i++) {
    uint64_t hi = (i + 1 < KVU_LIMBS) ? (a[i + 1] & 1) : top_bit;
    a[i] = (a[i] >> 1) | (hi << 63);
  }
}

static void prime_limbs(uint64_t *p) {
  for (int i = 0; i < KVU_LIMBS; i++) p[i] = ~0ULL;
  p[0] -= KVU_PRIME_DIFF - 1;
}

static void mod_half(uint64_t *x, const uint64_t *p) {
  if (x[0] & 1) {
    uint64_t c = 0;
    for (int i = 0; i < KVU_LIMBS; i++) x[i] = kv::kvu_addc(x[i], p[i], c);
    big_shr1(x, c);
  } else {
    big_shr1(x, 0);
  }
}

static void mod_sub(uint64_t *x, const uint64_t *y, const uint64_t *p) {
  /* x = (x - y) mod p, both < p */
  if (big_cmp(x, y) >= 0) {
    big_sub(x, y);
  } else {
    uint64_t t[KVU_LIMBS];
    memcpy(t, p, sizeof(t));
    big_sub(t, y); /* p - y */
    uint64_t c = 0;
    for (int i = 0; i < KVU_LIMBS; i++) x[i] = kv::kvu_addc(x[i], t[i], c);
    /* x + (p-y): may exceed p → subtract once */
    uint64_t pl[KVU_LIMBS];
    memcpy(pl, p, sizeof(pl));
    if (c || big_cmp(x, pl) >= 0) big_sub(x, pl);
  }
}

static void u3072_inverse(const u3072 &in, u3072 &out) {
  u3072 a = in;
  kv::u3072_canon(a);
  int zero = 1;
  for (int i = 0; i < KVU_LIMBS; i++)
    if (a.l[i]) zero = 0;
  if (zero) {
    memset(out.l, 0, sizeof(out.l));
    return;
  }
  uint64_t p[KVU_LIMBS], u[KVU_LIMBS], v[KVU_LIMBS], x1[KVU_LIMBS], x2[KVU_LIMBS];
  prime_limbs(p);
  memcpy(u, a.l, sizeof(u));
  memcpy(v, p, sizeof(v));
  memset(x1, 0, sizeof(x1));
  x1[0] = 1;
  memset(x2, 0, sizeof(x2));
  uint64_t one[KVU_LIMBS];
  memset(one, 0, sizeof(one));
  one[0] = 1;
  while (big_cmp(u, one) != 0 && big_cmp(v, one) != 0) {
    while (!(u[0] & 1)) {
      big_shr1(u, 0);
      mod_half(x1, p);
    }
    while (!(v[0] & 1)) {
      big_shr1(v, 0);
      mod_half(x2, p);
    }
    if (big_cmp(u, v) >= 0) {
      big_sub(u, v);
      mod_sub(x1, x2, p);
    } else {
      big_sub(v, u);
      mod_sub(x2, x1, p);
    }
  }
  memcpy(out.l, big_cmp(u, one) == 0 ? x1 : x2, sizeof(out.l));
}


extern "C" int kv_muhash_combine(kv_ctx *ctx, uint8_t *acc_partial768,
                                 const uint8_t *other_partial768) {
  (void)ctx;
  u3072 an, ad, bn, bd, r;
  memcpy(an.l, acc_partial768, 384);
  memcpy(ad.l, acc_partial768 + 384, 384);
  memcpy(bn.l, other_partial768, 384);
  memcpy(bd.l, other_partial768 + 384, 384);
  kv::u3072_mulmod(r, an, bn);
  memcpy(acc_partial768, r.l, 384);
  kv::u3072_mulmod(r, ad, bd);
  memcpy(acc_partial768 + 384, r.l, 384);
  return 0;
}

extern "C" int kv_muhash_finalize(kv_ctx *ctx, const uint8_t *partial768,
                                  uint8_t *hash32_out) {
  (void)ctx;
  u3072 num, den, dinv, r;
  memcpy(num.l, partial768, 384);
  memcpy(den.l, partial768 + 384, 384);
  u3072_inverse(den, dinv);
  kv::u3072_mulmod(r, num, dinv);
  kv::u3072_canon(r);
  uint8_t ser[384];
  memcpy(ser, r.l, 384); /* limbs are LE on all supported hosts */
  static const uint8_t KEY[] = "MuHashFinalize";
  kvhost::h_blake2b_keyed(KEY, sizeof(KEY) - 1, ser, 384, hash32_out);
  return 0;
}

extern "C" int kv_set_seq_commit_accessor(kv_ctx *ctx, kv_seq_commit_accessor_fn fn,
                                          void *user) {
  KV_ENTER(ctx);
  ctx->seqc_fn = fn;
  ctx->seqc_user = user;
  return 0;
}

extern "C" int kv_get_validate_timings(kv_ctx *ctx, kv_validate_timings *out) {
  if (!ctx || !out) return -1;
  KV_ENTER(ctx);
  *out = ctx->last_timings;
  return 0;
}

extern "C" int kv_sig_cache_stats(kv_ctx *ctx, kv_cache_stats *out) {
  out->insertions = ctx->cache_insertions;
  out->hits = ctx->cache_hits;
  out->misses = ctx->cache_misses;
  return 0;
}

/* ---------------- staged bench mode ----------------
 * Stage a tuple batch into HBM once; time repeated verify launches with the
 * inputs already resident (bench.py's timed region starts after staging —
 * the PCIe-inclusive rate of kv_verify_schnorr_batch is reported separately
 * in DESIGN.md). Kernel duration is measured with hipEvents on the engine's
 * OWN stream (torch.cuda.Event would watch torch's stream, not ours). */

extern "C" int kv_stage_tuples(kv_ctx *ctx, const uint8_t *tuples, size_t n,
                               int ecdsa) {
  KV_ENTER(ctx);
  size_t rec = ecdsa ? 132 : 128;
  size_t words = (n + 63) / 64;
  if (ctx->d_in.ensure(n * rec) || ctx->d_bitmap.ensure(words * 8)) return -2;
  HIP_CHECK(hipMemcpy(ctx->d_in.p, tuples, n * rec, hipMemcpyHostToDevice));
  return 0;
}

/* run one staged verify launch; writes kernel milliseconds to *kernel_ms.
 * Does NOT copy the bitmap back (kv_fetch_bitmap does). */
extern "C" int kv_verify_staged(kv_ctx *ctx, size_t n, int ecdsa, double *kernel_ms) {
  KV_ENTER(ctx);
  int block = 256;
  unsigned long long grid = (n + block - 1) / block;
  hipEvent_t t0, t1;
  HIP_CHECK(hipEventCreate(&t0));
  HIP_CHECK(hipEventCreate(&t1));
  HIP_CHECK(hipEventRecord(t0, ctx->stream));
  if (ecdsa)
    hipLaunchKernelGGL(kv::kv_ecdsa_verify_kernel, dim3(grid), dim3(block), 0,
                       ctx->stream, ctx->d_in.as<uint8_t>(), (unsigned long long)n,
                       ctx->d_bitmap.as<unsigned long long>(), nullptr);
  else if (launch_schnorr_verify(ctx, ctx->stream, ctx->d_in.as<uint8_t>(), n,
                                 ctx->d_bitmap.as<unsigned long long>(), nullptr))
    return -2; /* both kernels of the split path sit between t0 and t1 */
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(t1, ctx->stream));
  HIP_CHECK(hipEventSynchronize(t1));
  float ms = 0.f;
  HIP_CHECK(hipEventElapsedTime(&ms, t0, t1));
  if (kernel_ms) *kernel_ms = (double)ms;
  (void)hipEventDestroy(t0);
  (void)hipEventDestroy(t1);
  return 0;
}

extern "C" int kv_fetch_bitmap(kv_ctx *ctx, size_t n, uint64_t *bitmap_out) {
  KV_ENTER(ctx);
  size_t words = (n + 63) / 64;
  HIP_CHECK(hipMemcpy(bitmap_out, ctx->d_bitmap.p, words * 8, hipMemcpyDeviceToHost));
  return 0;
}

/* ---------------- full-block validate path ----------------
 * kv_validate_block ⇔ validate_populated_transaction_and_get_fee fanned out
 * per tx + the muhash monoid reduce (tx_validation_in_utxo_context.rs:37-67,
 * utxo_validation.rs:319-348). Host does the cheap integer checks and template
 * flattening; EVERY hash and EC verify runs on the GPU. */

using namespace kvhost;

namespace {

/* classify one input; appends jobs. Returns plan. */
/* non-template scripts: run the host general interpreter (kv_script_host.inc)
 * in collect mode. Signature-free scripts — hash puzzles, timelocks,
 * introspection/covenant logic, anyone-can-spend — resolve right here; a
 * script whose execution reaches a signature site suspends with its verify
 * requests in plan.pending and resolves over the GPU batch in the
 * interpreter-rounds phase of validate_block_impl. Only zk-precompile scripts
 * defer to the reference CPU interpreter (KV_TX_DEFER_TO_CPU). */
static void interp_classify(kv_ctx *ctx, const HTx &tx, const HInput &in,
                            uint32_t input_index, uint64_t sigop_units,
                            InputPlan &pl) {
  kvhost::KvsRunCtx rctx;
  rctx.memo = &pl.memo;
  rctx.pending = &pl.pending;
  rctx.seqc_fn = ctx->seqc_fn;
  rctx.seqc_user = ctx->seqc_user;
  int rc = kvh_run_input_script(tx, in, input_index, sigop_units, &rctx);
  if (rc == kvhost::KVH_SCRIPT_SUSPEND) {
    pl.kind = PLAN_INTERP;
    return;
  }
  int base = in.sig_script_len == 0 ? KV_ERR_SIGNATURE_EMPTY_BASE
                                    : KV_ERR_SIGNATURE_INVALID_BASE;
  if (rc == kvhost::KVH_SCRIPT_DEFER)
    pl.pre_code = KV_TX_DEFER_TO_CPU;
  else if (rc != 0)
    pl.pre_code = base + rc;
  else
    pl.pre_code = 0;
}

static InputPlan classify_input(kv_ctx *ctx, const HTx &tx, const HInput &in,
                                uint64_t sigop_units,
                                std::vector<kv::kv_job> &sjobs,
                                std::vector<kv::kv_job> &ejobs,
                                uint32_t tx_index, uint32_t input_index) {
  InputPlan pl;
  pl.limit_units = committed_limit(in);
  if (in.utxo_spk_version > 0) return pl; /* unknown version: accepted (lib.rs:655) */
  const uint8_t *spk = in.utxo_spk;
  uint32_t spklen = in.utxo_spk_len;
  /* oversized utxo spk charge (lib.rs:661-676) */
  if (spklen > 35) {
    uint64_t extra = (uint64_t)(spklen - 35) * KVH_UNITS_PER_GRAM;
    if (extra > pl.limit_units) {
      pl.pre_code = KV_ERR_SIGNATURE_INVALID_BASE + KV_SCRIPT_EXCEEDED_SCRIPT_UNITS;
      if (in.sig_script_len == 0)
        pl.pre_code = KV_ERR_SIGNATURE_EMPTY_BASE + KV_SCRIPT_EXCEEDED_SCRIPT_UNITS;
      return pl;
    }
    pl.spent_units += extra;
  }
  if (spklen == 0 && in.sig_script_len == 0) {
    pl.pre_code = KV_ERR_SIGNATURE_EMPTY_BASE + KV_SCRIPT_EVAL_FALSE;
    return pl;
  }
  int is_p2pk = spklen == 34 && spk[0] == 0x20 && spk[33] == 0xac;
  int is_p2pk_ecdsa = spklen == 35 && spk[0] == 0x21 && spk[34] == 0xab;
  int is_p2sh = spklen == 35 && spk[0] == 0xaa && spk[1] == 0x20 && spk[34] == 0x87;

  if (is_p2pk || is_p2pk_ecdsa) {
    const uint32_t siglen = 65; /* sig64 + type (both schnorr and ecdsa) */
    if (in.sig_script_len == 0) {
      /* spk alone: checksig pops 2 from a 1-deep stack */
      pl.pre_code = KV_ERR_SIGNATURE_EMPTY_BASE + KV_SCRIPT_INVALID_STACK_OPERATION;
      return pl;
    }
    if (in.sig_script_len != 1 + siglen || in.sig_script[0] != siglen) {
      interp_classify(ctx, tx, in, input_index, sigop_units, pl);
      return pl;
    }
    uint8_t type = in.sig_script[siglen];
    if (!valid_sighash_type(type)) {
      pl.pre_code = KV_ERR_SIGNATURE_INVALID_BASE + KV_SCRIPT_INVALID_SIG_HASH_TYPE;
      return pl;
    }
    if (sigop_units > pl.limit_units - pl.spent_units) {
      pl.pre_code = KV_ERR_SIGNATURE_INVALID_BASE + KV_SCRIPT_EXCEEDED_SCRIPT_UNITS;
      return pl;
    }
    pl.kind = PLAN_P2PK;
    pl.ecdsa = is_p2pk_ecdsa;
    kv::kv_job job;
    job.tx_index = tx_index;
    job.input_off = in.rec_off;
    job.input_index = input_index;
    job.sig_off = in.sig_script_off + 1;
    job.pk_off = in.utxo_spk_off + 1;
    job.hash_type = type;
    job.ecdsa = is_p2pk_ecdsa ? 1 : 0;
    job._pad = 0;
    if (is_p2pk_ecdsa) {
      pl.job = (int32_t)ejobs.size();
      ejobs.push_back(job);
    } else {
      pl.job = (int32_t)sjobs.size();
      sjobs.push_back(job);
    }
    return pl;
  }

  if (is_p2sh) {
    if (in.sig_script_len == 0) {
      /* spk alone: OpBlake2b pops from empty stack */
      pl.pre_code = KV_ERR_SIGNATURE_EMPTY_BASE + KV_SCRIPT_INVALID_STACK_OPERATION;
      return pl;
    }
    std::vector<std::pair<uint32_t, uint32_t>> pushes;
    if (!parse_pushes(nullptr, in.sig_script, in.sig_script_len, in.sig_script_off,
                      pushes) ||
        pushes.empty()) {
      interp_classify(ctx, tx, in, input_index, sigop_units, pl);
      return pl;
    }
    /* last push = redeem candidate (need the actual bytes: offset into blob is
     * relative; caller gave us pointers via in.sig_script) */
    auto redeem_pp = pushes.back();
    const uint8_t *redeem = in.sig_script + (redeem_pp.first - in.sig_script_off);
    uint32_t rlen = redeem_pp.second;
    /* p2sh hash check (spk exec): blake2b(redeem) == h32 — budget first */
    uint64_t blake_cost = (uint64_t)rlen * 2 + 32; /* data cost + pushed hash */
    if (pl.spent_units + blake_cost > pl.limit_units) {
      pl.pre_code = KV_ERR_SIGNATURE_INVALID_BASE + KV_SCRIPT_EXCEEDED_SCRIPT_UNITS;
      return pl;
    }
    pl.spent_units += blake_cost;
    uint8_t h[32];
    h_blake2b_keyed(nullptr, 0, redeem, rlen, h);
    if (memcmp(h, spk + 2, 32) != 0) {
      /* OpEqual pushes empty (0 units); check_error(false) → EvalFalse */
      pl.pre_code = KV_ERR_SIGNATURE_INVALID_BASE + KV_SCRIPT_EVAL_FALSE;
      return pl;
    }
    pl.spent_units += 1; /* OpEqual pushed [1] */
    /* parse canonical multisig redeem: OP_m (0x20 pk)×n OP_n 0xae */
    if (rlen < 3 || redeem[0] < 0x51 || redeem[0] > 0x60) {
      interp_classify(ctx, tx, in, input_index, sigop_units, pl);
      return pl;
    }
    int m = redeem[0] - 0x50;
    uint32_t rp = 1;
    std::vector<uint32_t> key_offs;
    while (rp + 33 <= rlen && redeem[rp] == 0x20) {
      key_offs.push_back(redeem_pp.first + rp + 1);
      rp += 33;
    }
    int n = (int)key_offs.size();
    if (rp + 2 != rlen || n < 1 || n > 20 || redeem[rp] != (uint8_t)(0x50 + n) ||
        redeem[rp + 1] != 0xae || m > n || m < 1) {
      interp_classify(ctx, tx, in, input_index, sigop_units, pl);
      return pl;
    }
    int nsigs = (int)pushes.size() - 1;
    if (nsigs != m) {
      /* stack mismatch: fewer → InvalidStackOperation when multisig pops;
       * more → extra entries → CleanStack at the end. Handle the simple
       * common cases; refuse others. */
      if (nsigs < m) {
        pl.pre_code = KV_ERR_SIGNATURE_INVALID_BASE + KV_SCRIPT_INVALID_STACK_OPERATION;
        return pl;
      }
      pl.extra_stack = true; /* resolved after matching */
    }
    pl.kind = PLAN_MULTISIG;
    pl.msig_m = m;
    pl.msig_n = n;
    pl.key_offs = key_offs;
    /* sigs = the last m pushes before the redeem (stack top-down ordering:
     * multisig pops the TOP m entries = the last m pushes).
     * A sig whose length is neither 0 nor 65 needs the current KEY's parse
     * status before its own length error (check order: cost, pubkey,
     * signature — lib.rs:884-890), which the template fast path cannot
     * provide; such inputs run through the general interpreter instead. */
    for (int si = nsigs - m; si < nsigs; si++) {
      uint32_t sl = pushes[si].second;
      if (sl != 0 && sl != 65) {
        pl = InputPlan();
        pl.limit_units = committed_limit(in);
        interp_classify(ctx, tx, in, input_index, sigop_units, pl);
        return pl;
      }
    }
    for (int si = nsigs - m; si < nsigs; si++) {
      MsigSig ms;
      ms.off = pushes[si].first;
      ms.len = pushes[si].second;
      ms.type = ms.len ? in.sig_script[ms.off - in.sig_script_off + ms.len - 1] : 0;
      ms.job0 = -1;
      if (ms.len == 65 && valid_sighash_type(ms.type)) {
        ms.job0 = (int32_t)sjobs.size();
        for (int ki = 0; ki < n; ki++) {
          kv::kv_job job;
          job.tx_index = tx_index;
          job.input_off = in.rec_off;
          job.input_index = input_index;
          job.sig_off = ms.off;
          job.pk_off = key_offs[ki];
          job.hash_type = ms.type;
          job.ecdsa = 0;
          job._pad = 0;
          sjobs.push_back(job);
        }
      }
      pl.msig_sigs.push_back(ms);
    }
    return pl;
  }

  interp_classify(ctx, tx, in, input_index, sigop_units, pl);
  return pl;
}

/* resolve one input after GPU statuses are back; returns full KV code or 0 */
static int resolve_input(const InputPlan &pl, const HInput &in, uint64_t sigop_units,
                         const uint8_t *s_status, const uint8_t *e_status) {
  int empty_base = in.sig_script_len == 0 ? KV_ERR_SIGNATURE_EMPTY_BASE
                                          : KV_ERR_SIGNATURE_INVALID_BASE;
  if (pl.pre_code) return pl.pre_code;
  if (pl.kind == PLAN_NONE) return 0;
  uint64_t spent = pl.spent_units;
  if (pl.kind == PLAN_P2PK) {
    uint8_t st = pl.ecdsa ? e_status[pl.job] : s_status[pl.job];
    spent += sigop_units; /* pre-checked to fit */
    if (st == 2) return empty_base + KV_SCRIPT_INVALID_PUBKEY;
    if (st == 3) return empty_base + KV_SCRIPT_INVALID_SIGNATURE;
    if (st == 0) {
      if (spent + 1 > pl.limit_units)
        return empty_base + KV_SCRIPT_EXCEEDED_SCRIPT_UNITS;
      return 0;
    }
    return empty_base + KV_SCRIPT_EVAL_FALSE;
  }
  /* multisig greedy matching (lib.rs:759-843) */
  int kp = 0;
  bool failed = false;
  int m = pl.msig_m, n = pl.msig_n;
  for (int si = 0; si < m; si++) {
    const MsigSig &ms = pl.msig_sigs[si];
    if (ms.len == 0) {
      failed = true;
      break;
    }
    if (!valid_sighash_type(ms.type))
      return empty_base + KV_SCRIPT_INVALID_SIG_HASH_TYPE;
    bool matched = false;
    while (true) {
      if (n - kp < m - si) {
        failed = true;
        break;
      }
      /* consume one sigop for this try */
      if (spent + sigop_units > pl.limit_units)
        return empty_base + KV_SCRIPT_EXCEEDED_SCRIPT_UNITS;
      spent += sigop_units;
      int key = kp++;
      if (ms.len != 65) /* sig blob wrong size: InvalidSignature error */
        return empty_base + KV_SCRIPT_INVALID_SIGNATURE;
      uint8_t st = s_status[ms.job0 + key];
      if (st == 2) return empty_base + KV_SCRIPT_INVALID_PUBKEY;
      if (st == 0) {
        matched = true;
        break;
      }
    }
    if (!matched) break;
  }
  bool any_nonempty = false;
  for (const auto &ms : pl.msig_sigs)
    if (ms.len) any_nonempty = true;
  if (failed && any_nonempty) return empty_base + KV_SCRIPT_NULL_FAIL;
  if (failed) {
    /* push false (0 units) → EvalFalse (or CleanStack first if extra) */
    if (pl.extra_stack) return empty_base + KV_SCRIPT_CLEAN_STACK;
    return empty_base + KV_SCRIPT_EVAL_FALSE;
  }
  if (spent + 1 > pl.limit_units)
    return empty_base + KV_SCRIPT_EXCEEDED_SCRIPT_UNITS;
  if (pl.extra_stack) return empty_base + KV_SCRIPT_CLEAN_STACK;
  return 0;
}

} // namespace

/* timing-event helpers (kv_get_validate_timings) */
static void tev_ensure(kv_ctx *ctx) {
  if (ctx->tev_init) return;
  for (int i = 0; i < 12; i++) (void)hipEventCreate(&ctx->tev[i]);
  ctx->tev_init = true;
}
static inline void tev_rec(kv_ctx *ctx, int i, hipStream_t stream = nullptr) {
  (void)hipEventRecord(ctx->tev[i], stream ? stream : ctx->stream);
}
static double tev_ms(kv_ctx *ctx, int pair) {
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, ctx->tev[2 * pair], ctx->tev[2 * pair + 1]) !=
      hipSuccess)
    return 0.0;
  return (double)ms;
}

/* reserve the per-call pinned staging arena (call while all streams are
 * idle — start of a validate call); returns -2 on allocation failure */
static int stage_reserve(kv_ctx *ctx, size_t need) {
  ctx->h_stage_off = 0;
  return ctx->h_stage.ensure(need);
}

/* copy src into the pinned arena and return the pinned pointer (NULL when the
 * arena is exhausted — callers then fall back to the pageable source) */
static const uint8_t *stage_push(kv_ctx *ctx, const void *src, size_t len) {
  if (!ctx->h_stage.p || ctx->h_stage_off + len > ctx->h_stage.cap) return nullptr;
  uint8_t *dst = ctx->h_stage.as<uint8_t>() + ctx->h_stage_off;
  memcpy(dst, src, len);
  ctx->h_stage_off += len;
  return dst;
}

/* stage-then-upload: pinned when the arena has room, pageable otherwise */
static inline int h2d_staged(kv_ctx *ctx, void *dst, const void *src, size_t len,
                             hipStream_t stream) {
  const uint8_t *p = stage_push(ctx, src, len);
  HIP_CHECK(hipMemcpyAsync(dst, p ? (const void *)p : src, len,
                           hipMemcpyHostToDevice, stream));
  return 0;
}

/* ---- the verify lane (VerifyLane): each step written once for both signature
 * kinds, enqueued on the stream the caller names; nothing here synchronises.
 * The blob and the subhashes must be resident in ctx->vb. `timed` is the
 * call's timing-pair flags, or NULL to leave the lane's timing events alone
 * (they describe phase 2 only). ---- */

/* upload `jobs` and assemble one tuple (sig ‖ pk ‖ sighash) per job */
static int lane_assemble(kv_ctx *ctx, VerifyLane &ln,
                         const std::vector<kv::kv_job> &jobs, hipStream_t stream,
                         bool *timed) {
  const size_t n = jobs.size();
  if (ln.jobs.ensure(n * sizeof(kv::kv_job)) ||
      ln.tuples.ensure(n * ln.d.tuple_bytes))
    return -2;
  if (h2d_staged(ctx, ln.jobs.p, jobs.data(), n * sizeof(kv::kv_job), stream))
    return -2;
  if (timed) tev_rec(ctx, ln.d.tev_assemble, stream);
  hipLaunchKernelGGL(kv::kv_sighash_assemble_kernel, dim3(((uint32_t)n + 255) / 256),
                     dim3(256), 0, stream, ctx->vb.blob.as<const uint8_t>(),
                     ctx->vb.subhashes.as<const uint8_t>(),
                     ln.jobs.as<const kv::kv_job>(), (uint32_t)n,
                     ln.tuples.as<uint8_t>(), ln.tuples.as<uint8_t>());
  if (timed) {
    tev_rec(ctx, ln.d.tev_assemble + 1, stream);
    timed[ln.d.tev_assemble / 2] = true;
  }
  return 0;
}

/* upload host-built tuples; `mjobs` name the tuples whose message is a sighash
 * the msg kernel still has to write in place (kv_job::sig_off = tuple slot) */
static int lane_upload(kv_ctx *ctx, VerifyLane &ln, const std::vector<uint8_t> &tuples,
                       const std::vector<kv::kv_job> &mjobs, hipStream_t stream) {
  if (ln.tuples.ensure(tuples.size()) ||
      ln.jobs.ensure(mjobs.size() * sizeof(kv::kv_job)))
    return -2;
  if (h2d_staged(ctx, ln.tuples.p, tuples.data(), tuples.size(), stream)) return -2;
  if (mjobs.empty()) return 0;
  if (h2d_staged(ctx, ln.jobs.p, mjobs.data(), mjobs.size() * sizeof(kv::kv_job),
                 stream))
    return -2;
  hipLaunchKernelGGL(kv::kv_sighash_msg_kernel,
                     dim3(((uint32_t)mjobs.size() + 255) / 256), dim3(256), 0, stream,
                     ctx->vb.blob.as<const uint8_t>(),
                     ctx->vb.subhashes.as<const uint8_t>(),
                     ln.jobs.as<const kv::kv_job>(), (uint32_t)mjobs.size(),
                     ln.tuples.as<uint8_t>(), ln.d.tuple_bytes, ln.d.msg_off);
  return 0;
}

/* verify the lane's first n tuples into its bitmap and status */
static int lane_verify(kv_ctx *ctx, VerifyLane &ln, size_t n, hipStream_t stream,
                       bool *timed) {
  if (ln.bitmap.ensure((n + 63) / 64 * 8) || ln.status.ensure(n)) return -2;
  if (timed) tev_rec(ctx, ln.d.tev_verify, stream);
  if (ln.d.ecdsa)
    hipLaunchKernelGGL(kv::kv_ecdsa_verify_kernel, dim3(((uint32_t)n + 255) / 256),
                       dim3(256), 0, stream, ln.tuples.as<const uint8_t>(),
                       (unsigned long long)n, ln.bitmap.as<unsigned long long>(),
                       ln.status.as<uint8_t>());
  else if (launch_schnorr_verify(ctx, stream, ln.tuples.as<const uint8_t>(), n,
                                 ln.bitmap.as<unsigned long long>(),
                                 ln.status.as<uint8_t>()))
    return -2;
  if (timed) {
    tev_rec(ctx, ln.d.tev_verify + 1, stream);
    timed[ln.d.tev_verify / 2] = true;
  }
  return 0;
}

/* queue the readback of n statuses into the lane's pinned landing buffer;
 * they are there once the caller has synchronised `stream` */
static int lane_readback(VerifyLane &ln, size_t n, hipStream_t stream) {
  if (ln.h_status.ensure(n)) return -2;
  HIP_CHECK(hipMemcpyAsync(ln.h_status.p, ln.status.p, n, hipMemcpyDeviceToHost,
                           stream));
  return 0;
}

extern "C" int kv_sighash_batch(kv_ctx *ctx, const uint8_t *blob, size_t blob_len,
                                const kv_sighash_job *jobs_in, size_t n,
                                uint8_t *hashes_out) {
  /* standalone sighash service over the blob (tests/parity). Jobs are split by
   * kind — the assemble kernel uses different tuple strides for schnorr (128B)
   * and ecdsa (132B). */
  KV_ENTER(ctx);
  ValidateBufs &vb = ctx->vb;
  vector<HTx> txs;
  if (parse_blob_host(blob, blob_len, txs) < 0) {
    set_error("kv_sighash_batch: malformed blob");
    return -1;
  }
  std::vector<kv::kv_job> jobs[2];
  std::vector<size_t> slots(n); /* index in its lane's array */
  for (size_t i = 0; i < n; i++) {
    const kv_sighash_job &j = jobs_in[i];
    if (j.tx_index >= txs.size() || j.input_index >= txs[j.tx_index].inputs.size()) {
      set_error("kv_sighash_batch: bad job index");
      return -1;
    }
    const HInput &in = txs[j.tx_index].inputs[j.input_index];
    std::vector<kv::kv_job> &lane_jobs = jobs[j.ecdsa ? LANE_ECDSA : LANE_SCHNORR];
    slots[i] = lane_jobs.size();
    lane_jobs.push_back(
        kv::kv_job{j.tx_index, in.rec_off, j.input_index, 0, 0, j.hash_type, j.ecdsa, 0});
  }
  uint32_t n_txs = (uint32_t)txs.size();
  if (vb.blob.ensure(blob_len) || vb.subhashes.ensure((size_t)n_txs * 160))
    return -2;
  HIP_CHECK(hipMemcpyAsync(vb.blob.p, blob, blob_len, hipMemcpyHostToDevice,
                           ctx->stream));
  hipLaunchKernelGGL(kv::kv_tx_subhash_kernel, dim3((n_txs + 255) / 256), dim3(256), 0,
                     ctx->stream, vb.blob.as<const uint8_t>(), n_txs,
                     vb.subhashes.as<uint8_t>());
  std::vector<uint8_t> tuples[2];
  for (int k = 0; k < 2; k++) {
    if (jobs[k].empty()) continue;
    VerifyLane &ln = vb.lane[k];
    tuples[k].resize(jobs[k].size() * ln.d.tuple_bytes);
    int rc = lane_assemble(ctx, ln, jobs[k], ctx->stream, nullptr);
    if (rc) return rc;
    HIP_CHECK(hipMemcpyAsync(tuples[k].data(), ln.tuples.p, tuples[k].size(),
                             hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < n; i++) {
    const int k = jobs_in[i].ecdsa ? LANE_ECDSA : LANE_SCHNORR;
    const LaneDesc &d = vb.lane[k].d;
    memcpy(hashes_out + 32 * i,
           tuples[k].data() + slots[i] * d.tuple_bytes + d.msg_off, 32);
  }
  return 0;
}

/* Enqueue the muhash element + reduce chain for txs with include[t] != 0 on
 * `stream`, fully async — the caller syncs the stream before reading outp.
 * The blob must already be resident in vb.blob. With no work the identity
 * partial is written synchronously and *launched stays false. */
static int enqueue_muhash(kv_ctx *ctx, const std::vector<HTx> &txs,
                          const uint8_t *include, uint64_t block_daa_score,
                          hipStream_t stream, bool *launched,
                          std::vector<kv::kv_elem_job> &jobs) {
  ValidateBufs &vb = ctx->vb;
  if (ctx->h_mu_partial.ensure(768)) return -2;
  uint8_t *outp = ctx->h_mu_partial.as<uint8_t>();
  jobs.clear();
  for (size_t t = 0; t < txs.size(); t++) {
    if (!include[t]) continue;
    const HTx &tx = txs[t];
    uint8_t cb = h_is_coinbase(tx) ? 1 : 0;
    for (uint32_t i = 0; i < tx.outputs.size(); i++)
      jobs.push_back(kv::kv_elem_job{(uint32_t)t, tx.output_offs[i], i, 1, cb, 0,
                                     block_daa_score});
  }
  size_t n_num = jobs.size();
  for (size_t t = 0; t < txs.size(); t++) {
    if (!include[t]) continue;
    const HTx &tx = txs[t];
    uint8_t cb = h_is_coinbase(tx) ? 1 : 0;
    for (auto &in : tx.inputs)
      jobs.push_back(kv::kv_elem_job{(uint32_t)t, in.rec_off, 0, 0, cb, 0,
                                     block_daa_score});
  }
  size_t n_all = jobs.size(), n_den = n_all - n_num;
  kv::u3072 one;
  kv::u3072_one(one);
  *launched = false;
  if (n_all == 0) {
    memcpy(outp, one.l, 384);
    memcpy(outp + 384, one.l, 384);
    return 0;
  }
  if (vb.elem_jobs.ensure(n_all * sizeof(kv::kv_elem_job)) ||
      vb.elements.ensure(n_all * KVU_LIMBS * 8) ||
      vb.partials_a.ensure(1024 * KVU_LIMBS * 8) ||
      vb.partials_b.ensure(1024 * KVU_LIMBS * 8))
    return -2;
  if (h2d_staged(ctx, vb.elem_jobs.p, jobs.data(),
                 n_all * sizeof(kv::kv_elem_job), stream))
    return -2;
  tev_rec(ctx, 10, stream);
  hipLaunchKernelGGL(kv::kv_muhash_element_kernel,
                     dim3(((uint32_t)n_all + 255) / 256), dim3(256), 0, stream,
                     vb.blob.as<const uint8_t>(),
                     vb.elem_jobs.as<const kv::kv_elem_job>(), (uint32_t)n_all,
                     vb.elements.as<uint64_t>());
  /* reduce numerator then denominator halves down to one value each; the
   * stride schedule is pure host arithmetic, so the whole chain enqueues
   * without any device->host round trip */
  for (int half = 0; half < 2; half++) {
    size_t cnt = half == 0 ? n_num : n_den;
    uint64_t *src = vb.elements.as<uint64_t>() + (half == 0 ? 0 : n_num * KVU_LIMBS);
    uint64_t *pa = vb.partials_a.as<uint64_t>();
    uint64_t *pb = vb.partials_b.as<uint64_t>();
    if (cnt == 0) {
      memcpy(outp + half * 384, one.l, 384);
      continue;
    }
    uint32_t n_cur = (uint32_t)cnt;
    uint64_t *cur = src;
    while (n_cur > 1) {
      /* wave-cooperative mulmod (one value per wave, limbs in registers).
       * Keep every pass parallel: each wave chains <=64 values, so the final
       * pass never degenerates into one wave grinding 512 serial mulmods. */
      uint32_t stride = n_cur > 64 ? (n_cur + 63) / 64 : 1;
      if (stride > 1024) stride = 1024;
      uint32_t waves_per_block = 4; /* 256 threads */
      uint32_t blocks = (stride + waves_per_block - 1) / waves_per_block;
      hipLaunchKernelGGL(kv_u3072_reduce_wave_kernel, dim3(blocks), dim3(256), 0,
                         stream, cur, n_cur, stride, pa);
      n_cur = stride;
      cur = pa;
      std::swap(pa, pb);
    }
    HIP_CHECK(hipMemcpyAsync(outp + half * 384, cur, 384, hipMemcpyDeviceToHost,
                             stream));
  }
  tev_rec(ctx, 11, stream);
  HIP_CHECK(hipGetLastError());
  *launched = true;
  return 0;
}

/* ---- validate_block_impl: the per-call state and its phases ---- */

using vt_clock = std::chrono::steady_clock;

/* host state of one verify lane during one validate call */
struct LaneCall {
  std::vector<kv::kv_job> jobs;   /* phase 1's jobs; after the cache probe, the misses */
  std::vector<uint8_t> status;    /* one verdict per phase-1 job (resolve_input) */
  std::vector<uint32_t> map;      /* cache on: miss k -> its phase-1 job index */
  std::vector<kv_sig_key> keys;   /* cache on: one key per phase-1 job */
};

struct ValidateCall {
  /* arguments */
  const uint8_t *blob = nullptr;
  size_t blob_len = 0;
  uint64_t pov_daa_score = 0, block_daa_score = 0;
  uint32_t flags = 0;
  const int32_t *pre_codes = nullptr;
  bool want_muhash = false;
  /* parsed txs and per-tx results */
  int n_txs = 0;
  uint64_t sigop_units = 0;
  vector<HTx> txs;
  std::vector<int32_t> codes;
  std::vector<uint64_t> fees;
  std::vector<std::vector<InputPlan>> plans;
  LaneCall lane[2];
  bool use_cache = false;
  /* device residency of this call's blob and subhashes */
  bool blob_uploaded = false, subhash_done = false;
  /* muhash: the include set of the enqueued chain */
  bool mu_opt_launched = false;
  std::vector<uint8_t> mu_inc;
  std::vector<kv::kv_elem_job> mu_jobs;
  bool tev_pair[6] = {}; /* which timing pairs of ctx->tev were recorded */
  /* host timing points (KV_TIMING) */
  vt_clock::time_point t_start, t_p1, t_enq, t_mu, t_rb, t_gpu, t_interp, t_resolve;
};

/* the call's blob into vb.blob, once per call: staged upload on ctx->stream,
 * ev_blob recorded behind it */
static int ensure_blob_resident(kv_ctx *ctx, ValidateCall &c) {
  if (c.blob_uploaded) return 0;
  if (ctx->vb.blob.ensure(c.blob_len)) return -2;
  if (h2d_staged(ctx, ctx->vb.blob.p, c.blob, c.blob_len, ctx->stream)) return -2;
  HIP_CHECK(hipEventRecord(ctx->ev_blob, ctx->stream));
  c.blob_uploaded = true;
  return 0;
}

/* the per-tx subhashes into vb.subhashes, once per call, on ctx->stream behind
 * the blob; ev_sub recorded behind the kernel */
static int ensure_subhashes(kv_ctx *ctx, ValidateCall &c) {
  if (c.subhash_done) return 0;
  if (ctx->vb.subhashes.ensure((size_t)c.n_txs * 160)) return -2;
  tev_rec(ctx, 0);
  hipLaunchKernelGGL(kv::kv_tx_subhash_kernel, dim3((c.n_txs + 255) / 256), dim3(256),
                     0, ctx->stream, ctx->vb.blob.as<const uint8_t>(),
                     (uint32_t)c.n_txs, ctx->vb.subhashes.as<uint8_t>());
  tev_rec(ctx, 1);
  c.tev_pair[0] = true;
  HIP_CHECK(hipEventRecord(ctx->ev_sub, ctx->stream));
  c.subhash_done = true;
  return 0;
}

/* per-call scratch: timing events and record, pinned staging arena */
static int validate_begin(kv_ctx *ctx, ValidateCall &c) {
  c.sigop_units = ctx->params.mass_per_sig_op * KVH_UNITS_PER_GRAM;
  tev_ensure(ctx);
  ctx->last_timings = kv_validate_timings{};
  /* generous upper bound: blob + verify jobs + muhash jobs */
  size_t n_units = 0;
  for (auto &tx : c.txs) n_units += tx.inputs.size() + tx.outputs.size();
  return stage_reserve(ctx, c.blob_len + n_units * (sizeof(kv::kv_job) +
                                                    sizeof(kv::kv_elem_job)) +
                                (size_t)c.n_txs * 64 + 65536);
}

/* phase 1 for one tx: integer checks, fee, and one plan per input */
static void phase1_tx(kv_ctx *ctx, ValidateCall &c, uint32_t t,
                      std::vector<kv::kv_job> &sjobs, std::vector<kv::kv_job> &ejobs) {
  HTx &tx = c.txs[t];
  if (c.codes[t]) return;
  if (h_is_coinbase(tx)) { /* coinbase never enters this path (utxo_validation.rs:297) */
    c.codes[t] = KV_ERR_BAD_BLOB;
    return;
  }
  int code = 0;
  for (auto &in : tx.inputs)
    if (in.utxo_is_coinbase &&
        in.utxo_daa_score + ctx->params.coinbase_maturity > c.pov_daa_score) {
      code = KV_ERR_IMMATURE_COINBASE;
      break;
    }
  uint64_t total_in = 0, total_out = 0;
  if (!code) {
    for (auto &in : tx.inputs) {
      if (total_in + in.utxo_amount < total_in) {
        code = KV_ERR_INPUT_AMOUNT_OVERFLOW;
        break;
      }
      total_in += in.utxo_amount;
      if (total_in > KVH_MAX_SOMPI) {
        code = KV_ERR_INPUT_AMOUNT_TOO_HIGH;
        break;
      }
    }
  }
  if (!code) {
    for (auto &o : tx.outputs) total_out += o.value;
    if (total_in < total_out) code = KV_ERR_SPEND_TOO_HIGH;
  }
  if (!code && c.flags != KV_FLAGS_SKIP_MASS_CHECK) {
    /* check_mass_commitment (tx_validation_in_utxo_context.rs:126-134) */
    uint64_t calc = 0;
    if (kvh_storage_mass(tx, false, &calc))
      code = KV_ERR_MASS_INCOMPUTABLE;
    else if (calc != tx.storage_mass)
      code = KV_ERR_WRONG_MASS;
  }
  if (!code) {
    for (auto &in : tx.inputs) {
      if ((in.sequence & KVH_SEQ_DISABLED) == KVH_SEQ_DISABLED) continue;
      int64_t lock = (int64_t)in.utxo_daa_score + (int64_t)(in.sequence & KVH_SEQ_MASK) - 1;
      if (lock >= (int64_t)c.pov_daa_score) {
        code = KV_ERR_SEQUENCE_LOCK;
        break;
      }
    }
  }
  if (!code && tx.version == 0)
    for (auto &o : tx.outputs)
      if (o.has_covenant) {
        /* the v0 wire form has no binding field (CovenantBindingInV0 belongs
         * to the isolation checks): such a blob cannot come from a node */
        code = KV_ERR_BAD_BLOB;
        break;
      }
  /* check_covenant_info (tx_validation_in_utxo_context.rs:58) */
  if (!code) code = kvh_check_covenant_info(tx);
  c.codes[t] = code;
  c.fees[t] = total_in - total_out;
  if (code || c.flags == KV_FLAGS_SKIP_SCRIPT_CHECKS) return;
  c.plans[t].reserve(tx.inputs.size());
  for (uint32_t i = 0; i < tx.inputs.size(); i++)
    c.plans[t].push_back(
        classify_input(ctx, tx, tx.inputs[i], c.sigop_units, sjobs, ejobs, t, i));
}

/* phase 1: host integer checks + classification, fanned over the host cores
 * (⇔ the reference's rayon pool) with per-chunk job lists so the GPU job
 * order after concatenation equals the serial order */
static void phase1_classify(kv_ctx *ctx, ValidateCall &c) {
  const uint32_t n_txs = (uint32_t)c.n_txs;
  c.plans.resize(n_txs);
  c.codes.assign(n_txs, 0);
  c.fees.assign(n_txs, 0);
  if (c.pre_codes) c.codes.assign(c.pre_codes, c.pre_codes + n_txs);
  unsigned P1T = kvh_threads(n_txs);
  uint32_t p1_chunk = (n_txs + P1T - 1) / P1T;
  std::vector<std::vector<kv::kv_job>> tl[2];
  tl[LANE_SCHNORR].resize(P1T);
  tl[LANE_ECDSA].resize(P1T);
  if (P1T == 1) {
    for (uint32_t t = 0; t < n_txs; t++)
      phase1_tx(ctx, c, t, tl[LANE_SCHNORR][0], tl[LANE_ECDSA][0]);
  } else {
    KvhPool::inst().run([&](unsigned p) {
      uint32_t lo = p * p1_chunk, hi = std::min(n_txs, lo + p1_chunk);
      for (uint32_t t = lo; t < hi; t++)
        phase1_tx(ctx, c, t, tl[LANE_SCHNORR][p], tl[LANE_ECDSA][p]);
    });
  }
  /* concatenate chunk job lists (serial order preserved) and rebase the
   * per-plan job indices by each chunk's offset */
  std::vector<size_t> base[2];
  for (int k = 0; k < 2; k++) {
    size_t total = 0;
    for (unsigned p = 0; p < P1T; p++) {
      base[k].push_back(total);
      total += tl[k][p].size();
    }
    c.lane[k].jobs.reserve(total);
    for (unsigned p = 0; p < P1T; p++)
      c.lane[k].jobs.insert(c.lane[k].jobs.end(), tl[k][p].begin(), tl[k][p].end());
  }
  if (P1T > 1)
    for (uint32_t t = 0; t < n_txs; t++) {
      unsigned p = t / p1_chunk;
      for (auto &pl : c.plans[t]) {
        if (pl.job >= 0)
          pl.job += (int32_t)base[pl.ecdsa ? LANE_ECDSA : LANE_SCHNORR][p];
        for (auto &ms : pl.msig_sigs)
          if (ms.job0 >= 0) ms.job0 += (int32_t)base[LANE_SCHNORR][p];
      }
    }
}

/* phase 1.5: sig cache ⇔ TransactionValidator sig_cache (caches.rs:57-82).
 * Key = blake2b-256(tx_id ‖ digest(all input entries) ‖ input_index ‖
 * hash_type ‖ ecdsa ‖ sig ‖ pk): tx_id pins everything else the sighash
 * commits to (it excludes sig scripts and utxo entries — those are keyed
 * explicitly). Hits skip the GPU entirely; the job lists are compacted to
 * the misses and statuses scattered back. */
static void probe_sig_cache(kv_ctx *ctx, ValidateCall &c) {
  for (auto &lc : c.lane) lc.status.resize(lc.jobs.size());
  c.use_cache = ctx->params.sig_cache_size > 0 &&
                c.lane[0].jobs.size() + c.lane[1].jobs.size() > 0;
  if (!c.use_cache) return;
  std::vector<uint8_t> need(c.n_txs, 0);
  for (auto &lc : c.lane)
    for (auto &j : lc.jobs) need[j.tx_index] = 1;
  std::vector<std::array<uint8_t, 32>> ed(c.n_txs);
  kvh_parallel_for((uint32_t)c.n_txs, [&](uint32_t t) {
    if (!need[t]) return;
    std::vector<uint8_t> buf;
    buf.reserve(c.txs[t].inputs.size() * 60);
    for (auto &in : c.txs[t].inputs) {
      uint8_t tmp[22];
      memcpy(tmp, &in.utxo_amount, 8);
      memcpy(tmp + 8, &in.utxo_daa_score, 8);
      tmp[16] = in.utxo_is_coinbase;
      tmp[17] = in.utxo_has_cov;
      memcpy(tmp + 18, &in.utxo_spk_version, 2);
      uint16_t sl = (uint16_t)in.utxo_spk_len;
      memcpy(tmp + 20, &sl, 2);
      buf.insert(buf.end(), tmp, tmp + 22);
      buf.insert(buf.end(), in.utxo_spk, in.utxo_spk + in.utxo_spk_len);
    }
    h_blake2b_keyed(nullptr, 0, buf.data(), buf.size(), ed[t].data());
  });
  for (auto &lc : c.lane) {
    lc.keys.resize(lc.jobs.size());
    kvh_parallel_for((uint32_t)lc.jobs.size(), [&](uint32_t i) {
      const kv::kv_job &j = lc.jobs[i];
      uint8_t buf[32 + 32 + 4 + 2 + 64 + 33];
      size_t o = 0;
      memcpy(buf + o, c.txs[j.tx_index].tx_id, 32);
      o += 32;
      memcpy(buf + o, ed[j.tx_index].data(), 32);
      o += 32;
      memcpy(buf + o, &j.input_index, 4);
      o += 4;
      buf[o++] = j.hash_type;
      buf[o++] = j.ecdsa;
      memcpy(buf + o, c.blob + j.sig_off, 64);
      o += 64;
      size_t pklen = j.ecdsa ? 33 : 32;
      memcpy(buf + o, c.blob + j.pk_off, pklen);
      o += pklen;
      uint8_t h[32];
      h_blake2b_keyed(nullptr, 0, buf, o, h);
      memcpy(lc.keys[i].w, h, 32);
    });
    std::vector<kv::kv_job> miss;
    miss.reserve(lc.jobs.size());
    for (size_t i = 0; i < lc.jobs.size(); i++) {
      auto it = ctx->sig_cache.find(lc.keys[i]);
      if (it != ctx->sig_cache.end()) {
        lc.status[i] = it->second;
        ctx->cache_hits++;
      } else {
        ctx->cache_misses++;
        lc.map.push_back((uint32_t)i);
        miss.push_back(lc.jobs[i]);
      }
    }
    lc.jobs.swap(miss);
  }
}

/* phase 2: GPU — subhashes, sighash+tuple assembly, EC verify (cache
 * misses only when the cache is on). Launches only; the readbacks follow the
 * muhash enqueue. */
static int enqueue_verify(kv_ctx *ctx, ValidateCall &c) {
  const size_t ns = c.lane[LANE_SCHNORR].jobs.size();
  const size_t ne = c.lane[LANE_ECDSA].jobs.size();
  if (ns + ne == 0) return 0;
  int rc = ensure_blob_resident(ctx, c);
  if (!rc) rc = ensure_subhashes(ctx, c);
  if (rc) return rc;
  if (ns) {
    VerifyLane &ln = ctx->vb.lane[LANE_SCHNORR];
    rc = lane_assemble(ctx, ln, c.lane[LANE_SCHNORR].jobs, ctx->stream, c.tev_pair);
    if (!rc) rc = lane_verify(ctx, ln, ns, ctx->stream, c.tev_pair);
    if (rc) return rc;
    ctx->last_timings.n_schnorr += ns;
  }
  if (ne) {
    /* ecdsa chain on stream2: at block-path sizes both verify kernels are
     * tiny latency-bound dispatches (a few hundred waves on a 2048-wave
     * machine) — overlapping them hides the whole ecdsa chain behind the
     * schnorr one */
    VerifyLane &ln = ctx->vb.lane[LANE_ECDSA];
    HIP_CHECK(hipStreamWaitEvent(ctx->stream2, ctx->ev_sub, 0));
    rc = lane_assemble(ctx, ln, c.lane[LANE_ECDSA].jobs, ctx->stream2, c.tev_pair);
    if (!rc) rc = lane_verify(ctx, ln, ne, ctx->stream2, c.tev_pair);
    if (rc) return rc;
    ctx->last_timings.n_ecdsa += ne;
  }
  HIP_CHECK(hipGetLastError());
  return 0;
}

/* optimistic muhash on stream3, overlapped with the verify chains: include
 * every tx that passed the phase-1 integer checks. Phase 4 consumes the
 * result when the final accept set matches (the overwhelmingly common
 * case) and re-enqueues the exact set otherwise. */
static int enqueue_optimistic_muhash(kv_ctx *ctx, ValidateCall &c) {
  if (!c.want_muhash) return 0;
  c.mu_inc.resize(c.n_txs);
  for (int t = 0; t < c.n_txs; t++) c.mu_inc[t] = c.codes[t] == 0;
  int rc = ensure_blob_resident(ctx, c);
  if (rc) return rc;
  HIP_CHECK(hipStreamWaitEvent(ctx->stream3, ctx->ev_blob, 0));
  return enqueue_muhash(ctx, c.txs, c.mu_inc.data(), c.block_daa_score, ctx->stream3,
                        &c.mu_opt_launched, c.mu_jobs);
}

/* status readbacks last (pinned, truly async) */
static int enqueue_status_readbacks(kv_ctx *ctx, ValidateCall &c) {
  hipStream_t streams[2] = {ctx->stream, ctx->stream2};
  for (int k = 0; k < 2; k++)
    if (size_t n = c.lane[k].jobs.size()) {
      int rc = lane_readback(ctx->vb.lane[k], n, streams[k]);
      if (rc) return rc;
    }
  return 0;
}

/* join the two verify streams */
static int wait_verify(kv_ctx *ctx, ValidateCall &c) {
  if (c.lane[0].jobs.size() + c.lane[1].jobs.size() == 0) return 0;
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  HIP_CHECK(hipStreamSynchronize(ctx->stream2));
  return 0;
}

/* scatter GPU statuses back and remember fresh verdicts */
static void collect_statuses(kv_ctx *ctx, ValidateCall &c) {
  const size_t cap = (size_t)ctx->params.sig_cache_size;
  for (int k = 0; k < 2; k++) {
    LaneCall &lc = c.lane[k];
    const size_t n = lc.jobs.size();
    const uint8_t *gpu = ctx->vb.lane[k].h_status.as<const uint8_t>();
    if (!c.use_cache) {
      if (n) memcpy(lc.status.data(), gpu, n);
      continue;
    }
    for (size_t i = 0; i < n; i++) {
      lc.status[lc.map[i]] = gpu[i];
      if (ctx->sig_cache.size() >= cap) ctx->sig_cache.erase(ctx->sig_cache.begin());
      ctx->sig_cache.emplace(lc.keys[lc.map[i]], gpu[i]);
      ctx->cache_insertions++;
    }
  }
}

/* phase 2.5: interpreter rounds — resolve suspended general-interpreter
 * scripts over the GPU verify batch, one signature site per script per
 * round (collect/replay protocol, kv_script_host.inc). Rounds =
 * max signature-site depth over this block's non-template scripts (almost
 * always 1); each round is one GPU batch over ALL suspended scripts, so
 * the launch count does not scale with signature count. */
static int interpreter_rounds(kv_ctx *ctx, ValidateCall &c) {
  if (c.flags == KV_FLAGS_SKIP_SCRIPT_CHECKS) return 0;
  ValidateBufs &vb = ctx->vb;
  std::vector<std::pair<uint32_t, uint32_t>> islots;
  for (int t = 0; t < c.n_txs; t++) {
    if (c.codes[t]) continue;
    for (uint32_t i = 0; i < c.plans[t].size(); i++)
      if (c.plans[t][i].kind == PLAN_INTERP) islots.emplace_back((uint32_t)t, i);
  }
  std::vector<uint8_t> tup[2]; /* host-side tuple arrays per round */
  while (!islots.empty()) {
    tup[0].clear();
    tup[1].clear();
    std::vector<kv::kv_job> mjobs[2]; /* sighash-msg jobs */
    struct ReqRef {
      uint8_t ecdsa;
      uint32_t idx;
    };
    std::vector<std::vector<ReqRef>> refs(islots.size());
    for (size_t sl = 0; sl < islots.size(); sl++) {
      uint32_t t = islots[sl].first, i = islots[sl].second;
      InputPlan &pl = c.plans[t][i];
      const HInput &in = c.txs[t].inputs[i];
      for (const auto &rq : pl.pending) {
        const uint8_t k = rq.ecdsa ? LANE_ECDSA : LANE_SCHNORR;
        const LaneDesc &d = vb.lane[k].d;
        uint32_t idx = (uint32_t)(tup[k].size() / d.tuple_bytes);
        tup[k].resize(tup[k].size() + d.tuple_bytes);
        uint8_t *tp = tup[k].data() + (size_t)idx * d.tuple_bytes;
        memcpy(tp, rq.sig, 64);
        memcpy(tp + 64, rq.pk, d.msg_off - 64); /* 32 B x-only, 33 B compressed */
        if (rq.literal)
          memcpy(tp + d.msg_off, rq.msg, 32);
        else /* sig_off carries the tuple slot for the msg kernel */
          mjobs[k].push_back(
              kv::kv_job{t, in.rec_off, i, idx, 0, rq.hash_type, k, 0});
        refs[sl].push_back({k, idx});
      }
    }
    const size_t n_i[2] = {tup[0].size() / vb.lane[0].d.tuple_bytes,
                           tup[1].size() / vb.lane[1].d.tuple_bytes};
    if (n_i[0] + n_i[1] > 0) {
      int rc = ensure_blob_resident(ctx, c);
      if (!rc) rc = ensure_subhashes(ctx, c);
      for (int k = 0; k < 2 && !rc; k++) {
        if (!n_i[k]) continue;
        VerifyLane &ln = vb.lane[k];
        rc = lane_upload(ctx, ln, tup[k], mjobs[k], ctx->stream);
        if (!rc) rc = lane_verify(ctx, ln, n_i[k], ctx->stream, nullptr);
        if (!rc) rc = lane_readback(ln, n_i[k], ctx->stream);
      }
      if (rc) return rc;
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    const uint8_t *st[2] = {vb.lane[0].h_status.as<const uint8_t>(),
                            vb.lane[1].h_status.as<const uint8_t>()};
    /* feed statuses back as this site's memo entry and replay */
    std::vector<uint8_t> survive(islots.size(), 0);
    kvh_parallel_for((uint32_t)islots.size(), [&](uint32_t sl) {
      uint32_t t = islots[sl].first, i = islots[sl].second;
      InputPlan &pl = c.plans[t][i];
      std::vector<uint8_t> entry(refs[sl].size());
      for (size_t r = 0; r < refs[sl].size(); r++)
        entry[r] = st[refs[sl][r].ecdsa][refs[sl][r].idx];
      pl.memo.push_back(std::move(entry));
      pl.pending.clear();
      kvhost::KvsRunCtx rctx;
      rctx.memo = &pl.memo;
      rctx.pending = &pl.pending;
      rctx.seqc_fn = ctx->seqc_fn;
      rctx.seqc_user = ctx->seqc_user;
      const HInput &in = c.txs[t].inputs[i];
      int rc = kvh_run_input_script(c.txs[t], in, i, c.sigop_units, &rctx);
      if (rc == kvhost::KVH_SCRIPT_SUSPEND) {
        survive[sl] = 1;
        return;
      }
      pl.kind = PLAN_NONE;
      if (rc == kvhost::KVH_SCRIPT_DEFER)
        pl.pre_code = KV_TX_DEFER_TO_CPU;
      else if (rc != 0)
        pl.pre_code = (in.sig_script_len == 0 ? KV_ERR_SIGNATURE_EMPTY_BASE
                                              : KV_ERR_SIGNATURE_INVALID_BASE) +
                      rc;
      else
        pl.pre_code = 0;
    });
    std::vector<std::pair<uint32_t, uint32_t>> next;
    for (size_t sl = 0; sl < islots.size(); sl++)
      if (survive[sl]) next.push_back(islots[sl]);
    islots.swap(next);
  }
  return 0;
}

/* phase 3: resolution (first failing input wins, sequential semantics);
 * read-only over the GPU statuses → fans over the host cores */
static void resolve_codes(ValidateCall &c) {
  kvh_parallel_for((uint32_t)c.n_txs, [&](uint32_t t) {
    if (c.codes[t] || c.flags == KV_FLAGS_SKIP_SCRIPT_CHECKS) return;
    for (uint32_t i = 0; i < c.txs[t].inputs.size(); i++) {
      int code = resolve_input(c.plans[t][i], c.txs[t].inputs[i], c.sigop_units,
                               c.lane[LANE_SCHNORR].status.data(),
                               c.lane[LANE_ECDSA].status.data());
      if (code) {
        c.codes[t] = code;
        break;
      }
    }
  });
}

/* phase 4: consume the optimistic muhash, or re-enqueue over the exact
 * accept set when some tx failed validation after the integer checks */
static int finish_muhash(kv_ctx *ctx, ValidateCall &c, uint8_t *muhash_partial_out) {
  if (!c.want_muhash) return 0;
  bool match = true;
  for (int t = 0; t < c.n_txs; t++)
    if ((c.codes[t] == 0) != (c.mu_inc[t] != 0)) {
      match = false;
      break;
    }
  HIP_CHECK(hipStreamSynchronize(ctx->stream3)); /* optimistic writes done */
  if (!match) {
    for (int t = 0; t < c.n_txs; t++) c.mu_inc[t] = c.codes[t] == 0;
    bool relaunched = false;
    int rc = enqueue_muhash(ctx, c.txs, c.mu_inc.data(), c.block_daa_score,
                            ctx->stream, &relaunched, c.mu_jobs);
    if (rc) return rc;
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    c.tev_pair[5] = relaunched;
  } else {
    c.tev_pair[5] = c.mu_opt_launched;
  }
  memcpy(muhash_partial_out, ctx->h_mu_partial.p, 768);
  return 0;
}

/* collect per-kernel timings (the stream is synchronized by now) */
static int collect_timings(kv_ctx *ctx, const ValidateCall &c) {
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  kv_validate_timings &lt = ctx->last_timings;
  if (c.tev_pair[0]) lt.subhash_ms = tev_ms(ctx, 0);
  if (c.tev_pair[1]) lt.s_assemble_ms = tev_ms(ctx, 1);
  if (c.tev_pair[2]) lt.e_assemble_ms = tev_ms(ctx, 2);
  if (c.tev_pair[3]) lt.schnorr_ms = tev_ms(ctx, 3);
  if (c.tev_pair[4]) lt.ecdsa_ms = tev_ms(ctx, 4);
  if (c.tev_pair[5]) lt.muhash_ms = tev_ms(ctx, 5);
  return 0;
}

/* caller holds ctx->mu; pre_codes (optional) pre-fails txs (e.g. missing
 * outpoints from the populate step) so they skip validation and muhash */
static int validate_block_impl(kv_ctx *ctx, const uint8_t *blob, size_t blob_len,
                               uint64_t pov_daa_score, uint64_t block_daa_score,
                               uint32_t flags, int32_t *tx_codes_out,
                               uint64_t *fees_out, uint8_t *muhash_partial_out,
                               const int32_t *pre_codes) {
  ValidateCall c;
  c.blob = blob;
  c.blob_len = blob_len;
  c.pov_daa_score = pov_daa_score;
  c.block_daa_score = block_daa_score;
  c.flags = flags;
  c.pre_codes = pre_codes;
  c.want_muhash = muhash_partial_out != nullptr;
  c.n_txs = parse_blob_host(blob, blob_len, c.txs);
  if (c.n_txs < 0) {
    set_error("kv_validate_block: malformed blob");
    return -1;
  }
  auto now = []() { return vt_clock::now(); };
  int rc;
  c.t_start = now();
  if ((rc = validate_begin(ctx, c))) return rc;
  phase1_classify(ctx, c);
  c.t_p1 = now();
  probe_sig_cache(ctx, c);
  if ((rc = enqueue_verify(ctx, c))) return rc;
  c.t_enq = now(); /* phase-2 launches done */
  if ((rc = enqueue_optimistic_muhash(ctx, c))) return rc;
  c.t_mu = now(); /* muhash enqueue done */
  if ((rc = enqueue_status_readbacks(ctx, c))) return rc;
  c.t_rb = now();
  if ((rc = wait_verify(ctx, c))) return rc;
  c.t_gpu = now();
  collect_statuses(ctx, c);
  if ((rc = interpreter_rounds(ctx, c))) return rc;
  c.t_interp = now();
  resolve_codes(c);
  c.t_resolve = now();
  if ((rc = finish_muhash(ctx, c, muhash_partial_out))) return rc;
  if ((rc = collect_timings(ctx, c))) return rc;

  for (int t = 0; t < c.n_txs; t++)
    if (c.codes[t]) c.fees[t] = 0; /* fee defined only for accepted txs */
  memcpy(tx_codes_out, c.codes.data(), (size_t)c.n_txs * 4);
  memcpy(fees_out, c.fees.data(), (size_t)c.n_txs * 8);
  if (getenv("KV_TIMING")) {
    auto ms = [](vt_clock::time_point a, vt_clock::time_point b) {
      return std::chrono::duration<double, std::milli>(b - a).count();
    };
    fprintf(stderr,
            "[kv_timing] validate: parse+p1 %.2f cache+enq %.2f (p2 %.2f mu %.2f "
            "rb %.2f) gpu-wait %.2f interp %.2f resolve %.2f muhash-wait %.2f "
            "total %.2f ms\n",
            ms(c.t_start, c.t_p1), ms(c.t_p1, c.t_rb), ms(c.t_p1, c.t_enq),
            ms(c.t_enq, c.t_mu), ms(c.t_mu, c.t_rb), ms(c.t_rb, c.t_gpu),
            ms(c.t_gpu, c.t_interp), ms(c.t_interp, c.t_resolve),
            ms(c.t_resolve, now()), ms(c.t_start, now()));
  }
  return 0;
}

extern "C" int kv_validate_block(kv_ctx *ctx, const uint8_t *blob, size_t blob_len,
                                 uint64_t pov_daa_score, uint64_t block_daa_score,
                                 uint32_t flags, int32_t *tx_codes_out,
                                 uint64_t *fees_out, uint8_t *muhash_partial_out) {
  KV_ENTER(ctx);
  return validate_block_impl(ctx, blob, blob_len, pov_daa_score, block_daa_score,
                             flags, tx_codes_out, fees_out, muhash_partial_out,
                             nullptr);
}


/* ---------------- GPU-resident UTXO set (kv_utxo_kernels.hip) ----------------
 * ⇔ utxo_collection.rs:5 HashMap + the populate/diff steps
 * (utxo_validation.rs:351-390, utxo_diff.rs:224). Entries are packed 64B
 * records: amount u64 ‖ daa u64 ‖ flags u16 (bit0 coinbase) ‖ spk_version u16 ‖
 * spk_len u32 ‖ spk[36] inline. */

extern "C" int kv_utxo_reset(kv_ctx *ctx, uint64_t capacity) {
  KV_ENTER(ctx);
  uint64_t cap = 64;
  while (cap < capacity * 2) cap <<= 1; /* ≤50% load factor */
  ctx->utxo_cap = 0;
  ctx->journal.clear(); /* undo records of the set that goes away */
  if (ctx->d_utxo.alloc(cap * sizeof(kv::utxo_slot))) return -2;
  ctx->utxo_cap = cap;
  HIP_CHECK(hipMemsetAsync(ctx->d_utxo.p, 0, cap * sizeof(kv::utxo_slot), ctx->stream));
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  ctx->arena_head = 0; /* the spk arena compacts on reset (allocation kept) */
  return 0;
}

static int utxo_stage(kv_ctx *ctx, const uint8_t *outpoints, const uint8_t *values,
                      size_t n) {
  if (ctx->d_op_in.ensure(n * 36)) return -2;
  HIP_CHECK(hipMemcpyAsync(ctx->d_op_in.p, outpoints, n * 36, hipMemcpyHostToDevice,
                           ctx->stream));
  if (values) {
    if (ctx->d_val_in.ensure(n * 64)) return -2;
    HIP_CHECK(hipMemcpyAsync(ctx->d_val_in.p, values, n * 64, hipMemcpyHostToDevice,
                             ctx->stream));
  }
  return 0;
}

/* a (start, stop) pair of timing events that cannot leak on an early return */
struct EventPair {
  hipEvent_t a = nullptr, b = nullptr;
  ~EventPair() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
  hipError_t init() {
    hipError_t e = hipEventCreate(&a);
    return e == hipSuccess ? hipEventCreate(&b) : e;
  }
  /* after a synchronisation of the stream both were recorded on */
  double ms() const {
    float v = 0.f;
    return hipEventElapsedTime(&v, a, b) == hipSuccess ? (double)v : 0.0;
  }
};

/* `timed` (optional, initialised by the caller) brackets the launch */
static int utxo_upsert_nolock(kv_ctx *ctx, const uint8_t *outpoints,
                              const uint8_t *entries64, size_t n,
                              const EventPair *timed = nullptr) {
  if (!ctx->d_utxo.p) {
    set_error("kv_utxo_upsert: call kv_utxo_reset first");
    return -1;
  }
  int rc = utxo_stage(ctx, outpoints, entries64, n);
  if (rc) return rc;
  if (ctx->d_utxo_fail.ensure(4)) return -2;
  int *d_fail = ctx->d_utxo_fail.as<int>();
  HIP_CHECK(hipMemsetAsync(d_fail, 0, 4, ctx->stream));
  if (timed) HIP_CHECK(hipEventRecord(timed->a, ctx->stream));
  hipLaunchKernelGGL(kv::kv_utxo_upsert_kernel, dim3(((uint32_t)n + 255) / 256),
                     dim3(256), 0, ctx->stream, ctx->table(), ctx->utxo_cap - 1,
                     ctx->d_op_in.as<uint8_t>(), ctx->d_val_in.as<uint8_t>(),
                     (unsigned long long)n, d_fail);
  if (timed) HIP_CHECK(hipEventRecord(timed->b, ctx->stream));
  int fail = 0;
  HIP_CHECK(hipMemcpyAsync(&fail, d_fail, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  if (fail) {
    set_error("kv_utxo_upsert: table full");
    return -3;
  }
  return 0;
}

extern "C" int kv_utxo_upsert(kv_ctx *ctx, const uint8_t *outpoints,
                              const uint8_t *entries64, size_t n) {
  KV_ENTER(ctx);
  /* a covenant id lives where an inline script would: kv_utxo_upsert_spk */
  for (size_t i = 0; i < n; i++) {
    uint16_t flags;
    memcpy(&flags, entries64 + i * 64 + 16, 2);
    if (flags & KV_UTXO_F_COVENANT) {
      set_error("kv_utxo_upsert: KV_UTXO_F_COVENANT needs kv_utxo_upsert_spk");
      return -1;
    }
  }
  return utxo_upsert_nolock(ctx, outpoints, entries64, n);
}

/* grow the spk arena to fit `need` more bytes; preserves contents */
static int arena_reserve(kv_ctx *ctx, uint64_t need) {
  uint64_t want = ctx->arena_head + need;
  if (want <= ctx->d_arena.cap) return 0;
  uint64_t nc = ctx->d_arena.cap ? ctx->d_arena.cap : (1u << 20);
  while (nc < want) nc *= 2;
  DeviceBuf na;
  if (na.alloc(nc)) return -2;
  if (ctx->arena_head)
    HIP_CHECK(hipMemcpyAsync(na.p, ctx->d_arena.p, ctx->arena_head,
                             hipMemcpyDeviceToDevice, ctx->stream));
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  ctx->d_arena.swap(na); /* the old arena goes with `na` */
  return 0;
}

/* does this ABI record's script travel in the spk blob (and live in the
 * arena)? Long scripts, and every covenant entry: its id takes bytes 28..60 */
static inline bool utxo_entry_needs_arena(const uint8_t *e) {
  uint16_t flags;
  uint32_t spk_len;
  memcpy(&flags, e + 16, 2);
  memcpy(&spk_len, e + 20, 4);
  return spk_len > 36 || (flags & KV_UTXO_F_COVENANT);
}

/* the argument rules of kv_utxo_upsert_spk: no script above KV_UTXO_MAX_SPK,
 * and spk_blob holds those of the arena entries. *long_total = their bytes,
 * *n_arena = their number. */
static int utxo_spk_args_check(const uint8_t *entries64, size_t spk_blob_len, size_t n,
                               uint64_t *long_total, size_t *n_arena) {
  *long_total = 0;
  *n_arena = 0;
  for (size_t i = 0; i < n; i++) {
    uint32_t spk_len;
    memcpy(&spk_len, entries64 + i * 64 + 20, 4);
    if (utxo_entry_needs_arena(entries64 + i * 64)) {
      ++*n_arena;
      if (spk_len > KV_UTXO_MAX_SPK) {
        set_error("kv_utxo_upsert_spk: spk exceeds KV_UTXO_MAX_SPK");
        return -1;
      }
      *long_total += spk_len;
    }
  }
  if (*long_total > spk_blob_len) {
    set_error("kv_utxo_upsert_spk: spk_blob shorter than the long entries");
    return -1;
  }
  return 0;
}

/* general upsert: spk_len > 36 entries spill their scripts to the arena
 * (bump-allocated; spans leak on remove until kv_utxo_reset or kv_utxo_rehash
 * — documented) */
static int utxo_upsert_spk_nolock(kv_ctx *ctx, const uint8_t *outpoints,
                                  const uint8_t *entries64, const uint8_t *spk_blob,
                                  size_t spk_blob_len, size_t n,
                                  const EventPair *timed = nullptr) {
  if (!ctx->d_utxo.p) {
    set_error("kv_utxo_upsert_spk: call kv_utxo_reset first");
    return -1;
  }
  uint64_t long_total = 0;
  size_t n_arena = 0;
  if (utxo_spk_args_check(entries64, spk_blob_len, n, &long_total, &n_arena)) return -1;
  if (n_arena == 0)
    return utxo_upsert_nolock(ctx, outpoints, entries64, n, timed);
  uint64_t base = ctx->arena_head;
  if (long_total) { /* covenant entries with empty scripts bring no bytes */
    int rc = arena_reserve(ctx, long_total);
    if (rc) return rc;
    HIP_CHECK(hipMemcpyAsync(ctx->d_arena.as<uint8_t>() + base, spk_blob, long_total,
                             hipMemcpyHostToDevice, ctx->stream));
    ctx->arena_head += long_total;
  }
  /* rewrite the arena entries: flags |= ARENA, spk[0..4) = arena offset; a
   * covenant entry keeps its id in 28..60 */
  std::vector<uint8_t> ents(entries64, entries64 + n * 64);
  uint64_t off = base;
  for (size_t i = 0; i < n; i++) {
    uint8_t *e = ents.data() + i * 64;
    uint32_t spk_len;
    memcpy(&spk_len, e + 20, 4);
    if (!utxo_entry_needs_arena(e)) continue;
    uint16_t flags;
    memcpy(&flags, e + 16, 2);
    flags |= KV_UTXO_F_SPK_ARENA;
    memcpy(e + 16, &flags, 2);
    uint32_t o32 = (uint32_t)off;
    memcpy(e + 24, &o32, 4);
    if (flags & KV_UTXO_F_COVENANT)
      memset(e + 60, 0, 4);
    else
      memset(e + 28, 0, 32);
    off += spk_len;
  }
  return utxo_upsert_nolock(ctx, outpoints, ents.data(), n, timed);
}

extern "C" int kv_utxo_upsert_spk(kv_ctx *ctx, const uint8_t *outpoints,
                                  const uint8_t *entries64, const uint8_t *spk_blob,
                                  size_t spk_blob_len, size_t n) {
  KV_ENTER(ctx);
  return utxo_upsert_spk_nolock(ctx, outpoints, entries64, spk_blob,
                                spk_blob_len, n);
}

static int utxo_remove_nolock(kv_ctx *ctx, const uint8_t *outpoints, size_t n) {
  if (!ctx->d_utxo.p) {
    set_error("kv_utxo_remove: call kv_utxo_reset first");
    return -1;
  }
  int rc = utxo_stage(ctx, outpoints, nullptr, n);
  if (rc) return rc;
  hipLaunchKernelGGL(kv::kv_utxo_remove_kernel, dim3(((uint32_t)n + 255) / 256),
                     dim3(256), 0, ctx->stream, ctx->table(), ctx->utxo_cap - 1,
                     ctx->d_op_in.as<uint8_t>(), (unsigned long long)n);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return 0;
}

extern "C" int kv_utxo_remove(kv_ctx *ctx, const uint8_t *outpoints, size_t n) {
  KV_ENTER(ctx);
  return utxo_remove_nolock(ctx, outpoints, n);
}

static int utxo_lookup_nolock(kv_ctx *ctx, const uint8_t *outpoints, size_t n,
                              uint8_t *entries_out, uint64_t *found_bitmap,
                              double *kernel_ms);

/* gather the arena spans of entries flagged KV_UTXO_F_SPK_ARENA (in entry
 * order) into host memory, rewriting each entry's spk field to its offset in
 * the gathered buffer. `take(i)` -> entry pointer or NULL to skip. */
template <class TakeFn>
static int arena_gather_nolock(kv_ctx *ctx, size_t n, TakeFn take,
                               std::vector<uint8_t> &out) {
  std::vector<kv::arena_gather_job> jobs;
  uint32_t dst = 0;
  for (size_t i = 0; i < n; i++) {
    uint8_t *e = take(i);
    if (!e) continue;
    uint16_t flags;
    memcpy(&flags, e + 16, 2);
    if (!(flags & KV_UTXO_F_SPK_ARENA)) continue;
    uint32_t spk_len, src;
    memcpy(&spk_len, e + 20, 4);
    memcpy(&src, e + 24, 4);
    if (spk_len) /* a covenant entry's script may be empty */
      jobs.push_back(kv::arena_gather_job{src, spk_len, dst, 0});
    memcpy(e + 24, &dst, 4); /* rewrite to the gathered-buffer offset */
    dst += spk_len;
  }
  out.resize(dst);
  if (jobs.empty()) return 0;
  if (ctx->d_gjobs.ensure(jobs.size() * sizeof(kv::arena_gather_job)) ||
      ctx->d_gout.ensure(dst))
    return -2;
  HIP_CHECK(hipMemcpyAsync(ctx->d_gjobs.p, jobs.data(),
                           jobs.size() * sizeof(kv::arena_gather_job),
                           hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(kv::kv_arena_gather_kernel, dim3((uint32_t)jobs.size()),
                     dim3(256), 0, ctx->stream, ctx->d_arena.as<uint8_t>(),
                     ctx->d_gjobs.as<const kv::arena_gather_job>(),
                     (uint32_t)jobs.size(), ctx->d_gout.as<uint8_t>());
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(out.data(), ctx->d_gout.p, dst, hipMemcpyDeviceToHost,
                           ctx->stream));
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return 0;
}

extern "C" int kv_utxo_lookup_spk(kv_ctx *ctx, const uint8_t *outpoints, size_t n,
                                  uint8_t *entries_out, uint64_t *found_bitmap,
                                  uint8_t *spk_out, size_t spk_cap,
                                  size_t *spk_used) {
  KV_ENTER(ctx);
  int rc = utxo_lookup_nolock(ctx, outpoints, n, entries_out, found_bitmap,
                              nullptr);
  if (rc) return rc;
  std::vector<uint8_t> gathered;
  rc = arena_gather_nolock(
      ctx, n,
      [&](size_t i) -> uint8_t * {
        int hit = (found_bitmap[i / 64] >> (i % 64)) & 1;
        return hit ? entries_out + i * 64 : nullptr;
      },
      gathered);
  if (rc) return rc;
  if (spk_used) *spk_used = gathered.size();
  if (gathered.empty()) return 0;
  if (gathered.size() > spk_cap) {
    set_error("kv_utxo_lookup_spk: spk_out too small");
    return -3;
  }
  memcpy(spk_out, gathered.data(), gathered.size());
  return 0;
}

static int utxo_lookup_nolock(kv_ctx *ctx, const uint8_t *outpoints, size_t n,
                              uint8_t *entries_out, uint64_t *found_bitmap,
                              double *kernel_ms) {
  if (!ctx->d_utxo.p) {
    set_error("kv_utxo_lookup: call kv_utxo_reset first");
    return -1;
  }
  const bool kvt = getenv("KV_TIMING") != nullptr;
  auto tn = []() { return std::chrono::steady_clock::now(); };
  auto t0_ = tn();
  int rc = utxo_stage(ctx, outpoints, nullptr, n);
  if (rc) return rc;
  auto t1_ = tn();
  size_t words = (n + 63) / 64;
  if (ctx->d_ent_out.ensure(n * 64) || ctx->d_bitmap.ensure(words * 8)) return -2;
  hipEvent_t t0, t1;
  HIP_CHECK(hipEventCreate(&t0));
  HIP_CHECK(hipEventCreate(&t1));
  HIP_CHECK(hipEventRecord(t0, ctx->stream));
  hipLaunchKernelGGL(kv::kv_utxo_lookup_kernel, dim3(((uint32_t)n + 255) / 256),
                     dim3(256), 0, ctx->stream, ctx->table(), ctx->utxo_cap - 1,
                     ctx->d_op_in.as<uint8_t>(), (unsigned long long)n,
                     ctx->d_ent_out.as<uint8_t>(),
                     ctx->d_bitmap.as<unsigned long long>());
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(t1, ctx->stream));
  if (entries_out)
    HIP_CHECK(hipMemcpyAsync(entries_out, ctx->d_ent_out.p, n * 64,
                             hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(hipMemcpyAsync(found_bitmap, ctx->d_bitmap.p, words * 8,
                           hipMemcpyDeviceToHost, ctx->stream));
  auto t2_ = tn();
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  if (kvt)
    fprintf(stderr, "[kv_timing] lookup inner: stage %.2f launch+copyq %.2f sync %.2f ms\n",
            std::chrono::duration<double, std::milli>(t1_ - t0_).count(),
            std::chrono::duration<double, std::milli>(t2_ - t1_).count(),
            std::chrono::duration<double, std::milli>(tn() - t2_).count());
  if (kernel_ms) {
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, t0, t1));
    *kernel_ms = ms;
  }
  (void)hipEventDestroy(t0);
  (void)hipEventDestroy(t1);
  return 0;
}

extern "C" int kv_utxo_lookup(kv_ctx *ctx, const uint8_t *outpoints, size_t n,
                              uint8_t *entries_out, uint64_t *found_bitmap,
                              double *kernel_ms) {
  KV_ENTER(ctx);
  return utxo_lookup_nolock(ctx, outpoints, n, entries_out, found_bitmap,
                            kernel_ms);
}

/* ---------------- UTXO-set commitment (kv_utxo_commit_kernels.hip) -----------
 * ⇔ the pruning-point import multiset (consensus/mod.rs:1139-1152,
 * processor.rs:1525-1538) and verify_expected_utxo_state
 * (utxo_validation.rs:188-195). */

namespace {
constexpr size_t CM_OFF_OUT = 0;      /* kv::commit_out */
constexpr size_t CM_OFF_COUNT = 512;  /* u32 live count of the current window */
constexpr size_t CM_OFF_IDX = 1024;   /* u32[KV_COMMIT_WINDOW] */
constexpr size_t CM_OFF_ACC = CM_OFF_IDX + (size_t)KV_COMMIT_WINDOW * 4;
constexpr size_t CM_OFF_PA = CM_OFF_ACC + (size_t)KV_COMMIT_LANES * KVU_LIMBS * 8;
constexpr size_t CM_OFF_PB = CM_OFF_PA + (size_t)1024 * KVU_LIMBS * 8;
constexpr size_t CM_FIXED_BYTES = CM_OFF_PB + (size_t)1024 * KVU_LIMBS * 8;
static_assert(sizeof(kv::commit_out) <= CM_OFF_COUNT, "commit_out outgrew its pad");
static_assert((KV_COMMIT_WINDOW & (KV_COMMIT_WINDOW - 1)) == 0 &&
                  KV_COMMIT_WINDOW >= 256,
              "KV_COMMIT_WINDOW must be a power of two >= 256");
} // namespace

extern "C" int kv_utxo_commitment_window(void) { return (int)KV_COMMIT_WINDOW; }

/* scratch for n_elems (<= KV_COMMIT_WINDOW) elements; the fixed part is one
 * allocation whose size depends on the compiled window alone */
static int commit_scratch(kv_ctx *ctx, size_t n_elems) {
  if (!ctx->d_cm_fixed.p && ctx->d_cm_fixed.alloc(CM_FIXED_BYTES)) return -2;
  return ctx->d_cm_elems.ensure(n_elems * KVU_LIMBS * 8);
}

/* zero the copy-back record and set `lanes` running accumulators to one */
static int commit_begin(kv_ctx *ctx, uint32_t lanes) {
  HIP_CHECK(hipMemsetAsync(ctx->d_cm_fixed.as<uint8_t>() + CM_OFF_OUT, 0, CM_OFF_COUNT,
                           ctx->stream));
  hipLaunchKernelGGL(kv::kv_u3072_fill_one_kernel,
                     dim3((lanes * KVU_LIMBS + 255) / 256), dim3(256), 0,
                     ctx->stream,
                     (uint64_t *)(ctx->d_cm_fixed.as<uint8_t>() + CM_OFF_ACC), lanes);
  return 0;
}

/* reduce the `lanes` accumulators to one value (host-known counts, the stride
 * schedule of enqueue_muhash), move it into the copy-back record and queue the
 * ONE device->host copy of the chain. The caller synchronises. */
static int commit_finish(kv_ctx *ctx, uint32_t lanes, kv::commit_out *h_out) {
  uint64_t *cur = (uint64_t *)(ctx->d_cm_fixed.as<uint8_t>() + CM_OFF_ACC);
  uint64_t *pa = (uint64_t *)(ctx->d_cm_fixed.as<uint8_t>() + CM_OFF_PA);
  uint64_t *pb = (uint64_t *)(ctx->d_cm_fixed.as<uint8_t>() + CM_OFF_PB);
  uint32_t n_cur = lanes;
  while (n_cur > 1) {
    uint32_t stride = n_cur > 64 ? (n_cur + 63) / 64 : 1;
    if (stride > 1024) stride = 1024;
    hipLaunchKernelGGL(kv_u3072_reduce_wave_kernel, dim3((stride + 3) / 4),
                       dim3(256), 0, ctx->stream, cur, n_cur, stride, pa);
    n_cur = stride;
    cur = pa;
    std::swap(pa, pb);
  }
  kv::commit_out *d_out = (kv::commit_out *)(ctx->d_cm_fixed.as<uint8_t>() + CM_OFF_OUT);
  hipLaunchKernelGGL(kv::kv_u3072_commit_out_kernel, dim3(1), dim3(64), 0,
                     ctx->stream, cur, d_out);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(h_out, d_out, sizeof(kv::commit_out),
                           hipMemcpyDeviceToHost, ctx->stream));
  return 0;
}

extern "C" int kv_utxo_commitment(kv_ctx *ctx, uint8_t partial768_out[768],
                                  uint64_t *n_live_out, double *kernel_ms) {
  if (!ctx || !partial768_out) {
    set_error("kv_utxo_commitment: null argument");
    return -1;
  }
  KV_ENTER(ctx);
  kv::u3072 one;
  kv::u3072_one(one);
  memcpy(partial768_out + 384, one.l, 384); /* denominator is always one */
  if (n_live_out) *n_live_out = 0;
  if (kernel_ms) *kernel_ms = 0.0;
  if (!ctx->d_utxo.p) { /* never reset: the empty set */
    memcpy(partial768_out, one.l, 384);
    return 0;
  }
  int rc = commit_scratch(ctx, KV_COMMIT_WINDOW);
  if (rc) return rc;
  uint8_t *fx = ctx->d_cm_fixed.as<uint8_t>();
  kv::commit_out *d_out = (kv::commit_out *)(fx + CM_OFF_OUT);
  uint32_t *d_count = (uint32_t *)(fx + CM_OFF_COUNT);
  uint32_t *d_idx = (uint32_t *)(fx + CM_OFF_IDX);
  uint64_t *d_acc = (uint64_t *)(fx + CM_OFF_ACC);
  hipEvent_t t0, t1;
  HIP_CHECK(hipEventCreate(&t0));
  HIP_CHECK(hipEventCreate(&t1));
  HIP_CHECK(hipEventRecord(t0, ctx->stream));
  rc = commit_begin(ctx, KV_COMMIT_LANES);
  for (uint64_t base = 0; !rc && base < ctx->utxo_cap; base += KV_COMMIT_WINDOW) {
    uint32_t n_slots = (uint32_t)std::min<uint64_t>(KV_COMMIT_WINDOW,
                                                    ctx->utxo_cap - base);
    dim3 grid((n_slots + 255) / 256);
    if (hipMemsetAsync(d_count, 0, 16, ctx->stream) != hipSuccess) rc = -2;
    hipLaunchKernelGGL(kv::kv_utxo_commit_compact_kernel, grid, dim3(256), 0,
                       ctx->stream, ctx->table(), base, n_slots, d_idx, d_count);
    hipLaunchKernelGGL(kv::kv_utxo_commit_element_kernel, grid, dim3(256), 0,
                       ctx->stream, ctx->table(), base, (const uint32_t *)d_idx,
                       (const uint32_t *)d_count, ctx->d_arena.as<const uint8_t>(),
                       ctx->arena_head, ctx->d_cm_elems.as<uint64_t>(), d_out);
    hipLaunchKernelGGL(kv_u3072_reduce_wave_acc_kernel,
                       dim3(KV_COMMIT_LANES / 4), dim3(256), 0, ctx->stream,
                       ctx->d_cm_elems.as<const uint64_t>(), (const uint32_t *)d_count,
                       0u, KV_COMMIT_LANES, d_acc, d_out);
  }
  kv::commit_out h_out;
  if (!rc) rc = commit_finish(ctx, KV_COMMIT_LANES, &h_out);
  hipError_t e1 = hipEventRecord(t1, ctx->stream);
  /* the single synchronisation of the chain */
  hipError_t e2 = hipStreamSynchronize(ctx->stream);
  float ms = 0.f;
  if (!rc && e1 == hipSuccess && e2 == hipSuccess)
    (void)hipEventElapsedTime(&ms, t0, t1);
  (void)hipEventDestroy(t0);
  (void)hipEventDestroy(t1);
  if (rc) return rc;
  HIP_CHECK(e1);
  HIP_CHECK(e2);
  if (h_out.fail) {
    set_error("kv_utxo_commitment: a table entry's script reference is out of range");
    return -3;
  }
  memcpy(partial768_out, h_out.limbs, 384);
  if (n_live_out) *n_live_out = h_out.n_live;
  if (kernel_ms) *kernel_ms = ms;
  return 0;
}

extern "C" int kv_utxo_import_chunk(kv_ctx *ctx, const uint8_t *outpoints,
                                    const uint8_t *entries64, const uint8_t *spk_blob,
                                    size_t spk_blob_len, size_t n,
                                    uint8_t acc_partial768[768]) {
  if (!ctx || !acc_partial768) {
    set_error("kv_utxo_import_chunk: null argument");
    return -1;
  }
  if (n == 0) return 0;
  if (n > 0xffffffffu) {
    set_error("kv_utxo_import_chunk: chunk too large");
    return -1;
  }
  KV_ENTER(ctx);
  int rc = utxo_upsert_spk_nolock(ctx, outpoints, entries64, spk_blob,
                                  spk_blob_len, n);
  if (rc) return rc;
  /* the chunk is still staged in d_op_in / d_val_in, long entries already
   * rewritten to their arena offsets: hash it from there, scripts in place */
  size_t batch = std::min<size_t>(n, KV_COMMIT_WINDOW);
  rc = commit_scratch(ctx, batch);
  if (rc) return rc;
  uint8_t *fx = ctx->d_cm_fixed.as<uint8_t>();
  kv::commit_out *d_out = (kv::commit_out *)(fx + CM_OFF_OUT);
  uint64_t *d_acc = (uint64_t *)(fx + CM_OFF_ACC);
  /* about 8 elements per first-pass wave, at most KV_COMMIT_LANES waves */
  uint32_t lanes = (uint32_t)std::min<size_t>((n + 7) / 8, KV_COMMIT_LANES);
  rc = commit_begin(ctx, lanes);
  if (rc) return rc;
  for (size_t off = 0; off < n; off += batch) {
    uint32_t m = (uint32_t)std::min(batch, n - off);
    hipLaunchKernelGGL(kv::kv_utxo_chunk_element_kernel, dim3((m + 255) / 256),
                       dim3(256), 0, ctx->stream,
                       ctx->d_op_in.as<const uint8_t>() + off * 36,
                       ctx->d_val_in.as<const uint8_t>() + off * 64, m,
                       ctx->d_arena.as<const uint8_t>(), ctx->arena_head,
                       ctx->d_cm_elems.as<uint64_t>(), d_out);
    hipLaunchKernelGGL(kv_u3072_reduce_wave_acc_kernel, dim3((lanes + 3) / 4),
                       dim3(256), 0, ctx->stream, ctx->d_cm_elems.as<const uint64_t>(),
                       (const uint32_t *)nullptr, m, lanes, d_acc, d_out);
  }
  kv::commit_out h_out;
  rc = commit_finish(ctx, lanes, &h_out);
  if (rc) return rc;
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  if (h_out.fail) {
    set_error("kv_utxo_import_chunk: an entry's script reference is out of range");
    return -3;
  }
  u3072 prod, an, r;
  memcpy(prod.l, h_out.limbs, 384);
  memcpy(an.l, acc_partial768, 384);
  kv::u3072_mulmod(r, an, prod);
  memcpy(acc_partial768, r.l, 384);
  return 0;
}

/* ---------------- table maintenance (kv_utxo_rehash_kernels.hip) -------------
 * stats, rehash / grow / shrink / compaction, and the export walk ⇔
 * get_pruning_point_utxos / get_virtual_utxos (consensus/mod.rs:1067-1108). */

namespace {
constexpr size_t TR_OFF_SCAN = 0;    /* kv::table_scan_rec */
constexpr size_t TR_OFF_REHASH = 64; /* kv::rehash_rec */
constexpr size_t TR_BYTES = 128;
static_assert(sizeof(kv::table_scan_rec) <= TR_OFF_REHASH &&
                  TR_OFF_REHASH + sizeof(kv::rehash_rec) <= TR_BYTES,
              "table records outgrew their pads");
} // namespace

/* the stats pass on ctx->stream: one kernel, one 40 B record back, one
 * synchronisation. Needs a table. */
static int utxo_scan_nolock(kv_ctx *ctx, kv::table_scan_rec *h_rec, float *ms) {
  if (ctx->d_tbl_rec.ensure(TR_BYTES)) return -2;
  kv::table_scan_rec *d_rec =
      (kv::table_scan_rec *)(ctx->d_tbl_rec.as<uint8_t>() + TR_OFF_SCAN);
  uint32_t blocks = (uint32_t)std::min<uint64_t>((ctx->utxo_cap + 255) / 256,
                                                 KV_STATS_MAX_BLOCKS);
  hipEvent_t t0, t1;
  HIP_CHECK(hipEventCreate(&t0));
  if (hipEventCreate(&t1) != hipSuccess) {
    (void)hipEventDestroy(t0);
    set_error("kv_utxo_stats: hipEventCreate failed");
    return -2;
  }
  hipError_t e = hipEventRecord(t0, ctx->stream);
  if (e == hipSuccess)
    e = hipMemsetAsync(d_rec, 0, sizeof(kv::table_scan_rec), ctx->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(kv::kv_utxo_stats_kernel, dim3(blocks), dim3(256), 0,
                       ctx->stream, ctx->table(),
                       ctx->utxo_cap, d_rec);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipEventRecord(t1, ctx->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(h_rec, d_rec, sizeof(kv::table_scan_rec),
                       hipMemcpyDeviceToHost, ctx->stream);
  hipError_t e2 = hipStreamSynchronize(ctx->stream);
  if (ms) {
    *ms = 0.f;
    if (e == hipSuccess && e2 == hipSuccess) (void)hipEventElapsedTime(ms, t0, t1);
  }
  (void)hipEventDestroy(t0);
  (void)hipEventDestroy(t1);
  HIP_CHECK(e);
  HIP_CHECK(e2);
  return 0;
}

extern "C" int kv_utxo_stats(kv_ctx *ctx, kv_utxo_table_stats *out) {
  if (!ctx || !out) {
    set_error("kv_utxo_stats: null argument");
    return -1;
  }
  KV_ENTER(ctx);
  memset(out, 0, sizeof(*out));
  if (!ctx->d_utxo.p) return 0; /* never reset */
  kv::table_scan_rec rec;
  int rc = utxo_scan_nolock(ctx, &rec, nullptr);
  if (rc) return rc;
  out->slots = ctx->utxo_cap;
  out->n_live = rec.n_live;
  out->n_tomb = rec.n_tomb;
  out->n_empty = rec.n_empty;
  out->arena_used = ctx->arena_head;
  out->arena_live_bytes = rec.arena_live_bytes;
  out->arena_cap = ctx->d_arena.cap;
  return 0;
}

extern "C" int kv_utxo_rehash(kv_ctx *ctx, uint64_t capacity, double *kernel_ms) {
  KV_ENTER(ctx);
  if (kernel_ms) *kernel_ms = 0.0;
  if (!ctx->d_utxo.p) {
    set_error("kv_utxo_rehash: call kv_utxo_reset first");
    return -1;
  }
  kv::table_scan_rec scan;
  float scan_ms = 0.f;
  int rc = utxo_scan_nolock(ctx, &scan, &scan_ms);
  if (rc) return rc;
  uint64_t new_cap = ctx->utxo_cap; /* capacity 0: a pure compaction */
  if (capacity) {
    if (capacity > (1ULL << 40)) {
      set_error("kv_utxo_rehash: capacity out of range");
      return -1;
    }
    new_cap = 64;
    while (new_cap < capacity * 2) new_cap <<= 1; /* as kv_utxo_reset */
    if (new_cap < 2 * scan.n_live) {
      set_error("kv_utxo_rehash: capacity too small for the live set");
      return -3;
    }
  }
  if (scan.arena_live_bytes > 0xffffffffULL || scan.n_arena > 0xffffffffULL) {
    set_error("kv_utxo_rehash: compacted arena exceeds a u32 offset");
    return -3;
  }
  /* the fresh arena: arena_reserve's rounding (1 MiB doubled until it fits);
   * a context that already owns an arena keeps at least that minimum */
  uint64_t new_arena_cap = 0;
  if (ctx->d_arena.p || scan.arena_live_bytes) {
    new_arena_cap = 1u << 20;
    while (new_arena_cap < scan.arena_live_bytes) new_arena_cap *= 2;
  }
  const uint32_t jobs_cap = (uint32_t)scan.n_arena;
  rc = commit_scratch(ctx, 0); /* index list and count word */
  if (rc) return rc;
  if (ctx->d_gjobs.ensure((size_t)jobs_cap * sizeof(kv::arena_gather_job)))
    return -2;

  /* the new table and arena live in locals until the chain has run clean:
   * every failure below leaves the old table in place and frees these */
  DeviceBuf nt, na;
  if (nt.alloc(new_cap * sizeof(kv::utxo_slot))) return -2;
  if (new_arena_cap && na.alloc(new_arena_cap)) return -2;
  hipEvent_t t0 = nullptr, t1 = nullptr;
  uint8_t *fx = ctx->d_cm_fixed.as<uint8_t>();
  uint32_t *d_count = (uint32_t *)(fx + CM_OFF_COUNT);
  uint32_t *d_idx = (uint32_t *)(fx + CM_OFF_IDX);
  kv::rehash_rec *d_rec =
      (kv::rehash_rec *)(ctx->d_tbl_rec.as<uint8_t>() + TR_OFF_REHASH);
  kv::rehash_rec h_rec;
  hipError_t e = hipEventCreate(&t0);
  if (e == hipSuccess) e = hipEventCreate(&t1);
  if (e == hipSuccess) e = hipEventRecord(t0, ctx->stream);
  if (e == hipSuccess)
    e = hipMemsetAsync(nt.p, 0, new_cap * sizeof(kv::utxo_slot), ctx->stream);
  if (e == hipSuccess)
    e = hipMemsetAsync(d_rec, 0, sizeof(kv::rehash_rec), ctx->stream);
  for (uint64_t base = 0; e == hipSuccess && base < ctx->utxo_cap;
       base += KV_COMMIT_WINDOW) {
    uint32_t n_slots = (uint32_t)std::min<uint64_t>(KV_COMMIT_WINDOW,
                                                    ctx->utxo_cap - base);
    dim3 grid((n_slots + 255) / 256);
    e = hipMemsetAsync(d_count, 0, 16, ctx->stream);
    if (e != hipSuccess) break;
    hipLaunchKernelGGL(kv::kv_utxo_commit_compact_kernel, grid, dim3(256), 0,
                       ctx->stream, ctx->table(), base, n_slots, d_idx, d_count);
    hipLaunchKernelGGL(kv::kv_utxo_rehash_insert_kernel, grid, dim3(256), 0,
                       ctx->stream, ctx->table(), base,
                       (const uint32_t *)d_idx, (const uint32_t *)d_count,
                       nt.as<kv::utxo_slot>(), new_cap - 1, ctx->arena_head,
                       new_arena_cap,
                       ctx->d_gjobs.as<kv::arena_gather_job>(), jobs_cap, d_rec);
    e = hipGetLastError();
  }
  if (e == hipSuccess && jobs_cap) {
    hipLaunchKernelGGL(kv::kv_arena_copy_jobs_kernel, dim3(jobs_cap), dim3(256), 0,
                       ctx->stream, ctx->d_arena.as<const uint8_t>(),
                       ctx->d_gjobs.as<const kv::arena_gather_job>(),
                       (const uint32_t *)&d_rec->n_jobs, jobs_cap,
                       na.as<uint8_t>());
    e = hipGetLastError();
  }
  if (e == hipSuccess)
    e = hipMemcpyAsync(&h_rec, d_rec, sizeof(kv::rehash_rec), hipMemcpyDeviceToHost,
                       ctx->stream);
  if (e == hipSuccess) e = hipEventRecord(t1, ctx->stream);
  /* the single synchronisation of the chain */
  hipError_t e2 = hipStreamSynchronize(ctx->stream);
  float ms = 0.f;
  if (e == hipSuccess && e2 == hipSuccess) (void)hipEventElapsedTime(&ms, t0, t1);
  if (t0) (void)hipEventDestroy(t0);
  if (t1) (void)hipEventDestroy(t1);
  HIP_CHECK(e);
  HIP_CHECK(e2);
  if (h_rec.fail || h_rec.inserted != scan.n_live ||
      h_rec.arena_head != scan.arena_live_bytes) {
    set_error(h_rec.fail
                  ? "kv_utxo_rehash: an entry could not be placed (script reference "
                    "out of range, or no room)"
                  : "kv_utxo_rehash: inserted count differs from the live count");
    return -3;
  }
  /* device work complete and clean: swap; the old allocations go with the
   * locals */
  ctx->d_utxo.swap(nt);
  ctx->utxo_cap = new_cap;
  ctx->d_arena.swap(na);
  ctx->arena_head = h_rec.arena_head;
  if (kernel_ms) *kernel_ms = (double)scan_ms + (double)ms;
  return 0;
}

extern "C" int kv_utxo_export_chunk(kv_ctx *ctx, uint64_t *cursor, size_t max_entries,
                                    uint8_t *outpoints_out, uint8_t *entries_out,
                                    uint8_t *spk_out, size_t spk_cap, size_t *spk_used,
                                    size_t *n_out) {
  if (!ctx || !cursor || !n_out) {
    set_error("kv_utxo_export_chunk: null argument");
    return -1;
  }
  *n_out = 0;
  if (spk_used) *spk_used = 0;
  if (spk_cap < KV_UTXO_MAX_SPK || !spk_out) {
    set_error("kv_utxo_export_chunk: spk_cap below KV_UTXO_MAX_SPK");
    return -1;
  }
  KV_ENTER(ctx);
  if (*cursor >= ctx->utxo_cap) { /* the walk is over (or there is no table) */
    *cursor = ctx->utxo_cap;
    return 0;
  }
  if (max_entries == 0) return 0;
  if (!outpoints_out || !entries_out) {
    set_error("kv_utxo_export_chunk: null argument");
    return -1;
  }
  /* the span: about max_entries live slots at the 50% design load, at least
   * 4096 slots so a sparse table is not walked a handful of slots per call,
   * at most one window, never past the end or across a window boundary */
  const uint64_t base = *cursor;
  uint64_t want = max_entries > KV_COMMIT_WINDOW ? KV_COMMIT_WINDOW : 2 * max_entries;
  want = std::max<uint64_t>(want, 4096);
  uint64_t to_boundary = KV_COMMIT_WINDOW - (base & (KV_COMMIT_WINDOW - 1));
  const uint32_t span = (uint32_t)std::min<uint64_t>(
      std::min<uint64_t>(want, to_boundary), ctx->utxo_cap - base);
  int rc = commit_scratch(ctx, 0);
  if (rc) return rc;
  if (ctx->d_op_in.ensure((size_t)span * 36) ||
      ctx->d_ent_out.ensure((size_t)span * 64) ||
      ctx->d_exp_refs.ensure((size_t)span * 8))
    return -2;
  uint8_t *fx = ctx->d_cm_fixed.as<uint8_t>();
  uint32_t *d_count = (uint32_t *)(fx + CM_OFF_COUNT);
  uint32_t *d_idx = (uint32_t *)(fx + CM_OFF_IDX);
  dim3 grid((span + 255) / 256);
  HIP_CHECK(hipMemsetAsync(d_count, 0, 16, ctx->stream));
  hipLaunchKernelGGL(kv::kv_utxo_commit_compact_kernel, grid, dim3(256), 0,
                     ctx->stream, ctx->table(), base, span, d_idx, d_count);
  hipLaunchKernelGGL(kv::kv_utxo_export_gather_kernel, grid, dim3(256), 0,
                     ctx->stream, ctx->table(), base,
                     (const uint32_t *)d_idx, (const uint32_t *)d_count,
                     ctx->arena_head, ctx->d_op_in.as<uint8_t>(),
                     ctx->d_ent_out.as<uint8_t>(),
                     ctx->d_exp_refs.as<unsigned long long>());
  HIP_CHECK(hipGetLastError());
  uint32_t count = 0;
  HIP_CHECK(hipMemcpyAsync(&count, d_count, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  if (count > span) {
    set_error("kv_utxo_export_chunk: compaction count out of range");
    return -2;
  }
  if (count == 0) {
    *cursor = base + span;
    return 0;
  }
  std::vector<uint32_t> idx(count);
  std::vector<unsigned long long> refs(count);
  std::vector<uint8_t> &keys = ctx->ops_buf, &vals = ctx->ent_buf;
  keys.resize((size_t)count * 36);
  vals.resize((size_t)count * 64);
  HIP_CHECK(hipMemcpyAsync(idx.data(), d_idx, (size_t)count * 4,
                           hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(hipMemcpyAsync(refs.data(), ctx->d_exp_refs.p, (size_t)count * 8,
                           hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(hipMemcpyAsync(keys.data(), ctx->d_op_in.p, (size_t)count * 36,
                           hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(hipMemcpyAsync(vals.data(), ctx->d_ent_out.p, (size_t)count * 64,
                           hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  /* compaction order is whatever the waves' atomics made it: sort into slot
   * order, then take the prefix that fits max_entries and spk_cap */
  std::vector<uint32_t> order(count);
  for (uint32_t i = 0; i < count; i++) order[i] = i;
  std::sort(order.begin(), order.end(),
            [&](uint32_t a, uint32_t b) { return idx[a] < idx[b]; });
  std::vector<kv::arena_gather_job> jobs;
  size_t m = 0;
  uint32_t used = 0;
  for (; m < count && m < max_entries; m++) {
    uint32_t p = order[m];
    if (refs[p] == KV_EXPORT_REF_BAD) {
      set_error("kv_utxo_export_chunk: a table entry's script reference is out of range");
      return -3;
    }
    uint32_t spk_len = (uint32_t)(refs[p] >> 32);
    if (spk_len) {
      if ((size_t)used + spk_len > spk_cap) break; /* next chunk starts here */
      jobs.push_back(kv::arena_gather_job{(uint32_t)refs[p], spk_len, used, 0});
      used += spk_len;
    }
    memcpy(outpoints_out + m * 36, keys.data() + (size_t)p * 36, 36);
    memcpy(entries_out + m * 64, vals.data() + (size_t)p * 64, 64);
  }
  if (!jobs.empty()) {
    if (ctx->d_gjobs.ensure(jobs.size() * sizeof(kv::arena_gather_job)) ||
        ctx->d_gout.ensure(used))
      return -2;
    HIP_CHECK(hipMemcpyAsync(ctx->d_gjobs.p, jobs.data(),
                             jobs.size() * sizeof(kv::arena_gather_job),
                             hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(kv::kv_arena_gather_kernel, dim3((uint32_t)jobs.size()),
                       dim3(256), 0, ctx->stream, ctx->d_arena.as<uint8_t>(),
                       ctx->d_gjobs.as<const kv::arena_gather_job>(),
                       (uint32_t)jobs.size(), ctx->d_gout.as<uint8_t>());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(spk_out, ctx->d_gout.p, used, hipMemcpyDeviceToHost,
                             ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
  }
  /* m >= 1 here: the first entry always fits (spk_cap >= KV_UTXO_MAX_SPK) */
  *cursor = m == count ? base + span : base + (uint64_t)idx[order[m - 1]] + 1;
  *n_out = m;
  if (spk_used) *spk_used = used;
  return 0;
}

/* ---------------- queries by script public key (kv_utxo_query_kernels.hip) ---
 * ⇔ UtxoIndexApi (indexes/utxoindex/src/core/api/mod.rs:23-30), served by a
 * filtered scan of the table instead of the reference's second database
 * (indexes/utxoindex/src/stores/indexed_utxos.rs:156-198). */

/* where the parts of the query table lie in ctx->q_host and ctx->d_q_set:
 * hash ‖ qidx ‖ heads ‖ offsets ‖ blob */
struct QueryLayout {
  uint32_t slots;
  size_t n_q, off_qidx, off_q, off_off, off_blob, bytes;
};

/* Validate the queries and build their table in ctx->q_host with the device
 * file's own spk_query_build. Returns -1 on any refusal of the contract. */
static int query_set_build(kv_ctx *ctx, const char *who, const kv_spk_query *q,
                           size_t n_q, const uint8_t *spk_blob, size_t spk_blob_len,
                           QueryLayout *L) {
  if ((n_q && !q) || (spk_blob_len && !spk_blob) ||
      kv::spk_query_check(q, n_q, spk_blob_len)) {
    set_error((std::string(who) + ": too many queries, a script over "
               "KV_UTXO_MAX_SPK, a non-zero `zero` field, or a blob length that "
               "is not the sum of the script lengths").c_str());
    return -1;
  }
  L->slots = kv::spk_query_slots(n_q);
  L->n_q = n_q;
  L->off_qidx = (size_t)L->slots * 8;
  L->off_q = L->off_qidx + (size_t)L->slots * 4;
  L->off_off = L->off_q + n_q * sizeof(kv_spk_query);
  L->off_blob = L->off_off + n_q * 4;
  L->bytes = L->off_blob + spk_blob_len;
  ctx->q_host.resize(L->bytes);
  uint8_t *h = ctx->q_host.data();
  if (n_q) memcpy(h + L->off_q, q, n_q * sizeof(kv_spk_query));
  if (spk_blob_len) memcpy(h + L->off_blob, spk_blob, spk_blob_len);
  if (kv::spk_query_build(q, n_q, spk_blob, (uint32_t *)(h + L->off_off),
                          (uint64_t *)h, (uint32_t *)(h + L->off_qidx), L->slots)) {
    set_error((std::string(who) + ": two identical queries").c_str());
    return -1;
  }
  return 0;
}

/* queue the upload of the table query_set_build made; *S gets the device view.
 * ctx->q_host stays as it is until the caller's synchronisation. */
static int query_set_upload(kv_ctx *ctx, const QueryLayout &L, kv::spk_query_set *S) {
  if (ctx->d_q_set.ensure(L.bytes)) return -2;
  HIP_CHECK(hipMemcpyAsync(ctx->d_q_set.p, ctx->q_host.data(), L.bytes,
                           hipMemcpyHostToDevice, ctx->stream));
  const uint8_t *d = ctx->d_q_set.as<const uint8_t>();
  S->hash = (const uint64_t *)d;
  S->qidx = (const uint32_t *)(d + L.off_qidx);
  S->q = (const kv_spk_query *)(d + L.off_q);
  S->off = (const uint32_t *)(d + L.off_off);
  S->blob = d + L.off_blob;
  S->mask = L.slots - 1;
  S->n_q = (uint32_t)L.n_q;
  return 0;
}

extern "C" int kv_utxo_balance_by_spk(kv_ctx *ctx, const kv_spk_query *q, size_t n_q,
                                      const uint8_t *spk_blob, size_t spk_blob_len,
                                      uint64_t *balances_out, uint64_t *counts_out,
                                      uint64_t *total_amount_out, uint64_t *n_live_out,
                                      double *kernel_ms) {
  KV_ENTER(ctx);
  if (n_q && n_q <= KV_UTXO_QUERY_MAX && !balances_out) {
    set_error("kv_utxo_balance_by_spk: null argument");
    return -1;
  }
  QueryLayout L;
  int rc = query_set_build(ctx, "kv_utxo_balance_by_spk", q, n_q, spk_blob,
                           spk_blob_len, &L);
  if (rc) return rc;
  double ms = 0.0;
  kv::query_rec h_rec = {};
  std::vector<uint64_t> sums(2 * n_q, 0); /* balances ‖ counts */
  if (ctx->d_utxo.p) { /* else never reset: the empty set */
    kv::spk_query_set S;
    rc = query_set_upload(ctx, L, &S);
    if (rc) return rc;
    const size_t out_bytes = 64 + 16 * n_q;
    if (ctx->d_q_out.ensure(out_bytes)) return -2;
    kv::query_rec *d_rec = ctx->d_q_out.as<kv::query_rec>();
    unsigned long long *d_bal =
        (unsigned long long *)(ctx->d_q_out.as<uint8_t>() + 64);
    EventPair ev;
    HIP_CHECK(ev.init());
    HIP_CHECK(hipMemsetAsync(d_rec, 0, out_bytes, ctx->stream));
    uint32_t blocks = (uint32_t)std::min<uint64_t>((ctx->utxo_cap + 255) / 256,
                                                   KV_STATS_MAX_BLOCKS);
    HIP_CHECK(hipEventRecord(ev.a, ctx->stream));
    hipLaunchKernelGGL(kv::kv_utxo_balance_kernel, dim3(blocks), dim3(256), 0,
                       ctx->stream, ctx->table(), ctx->utxo_cap, S,
                       ctx->d_arena.as<const uint8_t>(), ctx->arena_head, d_bal,
                       d_bal + n_q, ctx->query_combine ? 1 : 0, d_rec);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ev.b, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(&h_rec, d_rec, sizeof(h_rec), hipMemcpyDeviceToHost,
                             ctx->stream));
    if (n_q)
      HIP_CHECK(hipMemcpyAsync(sums.data(), d_bal, 16 * n_q, hipMemcpyDeviceToHost,
                               ctx->stream));
    /* the single synchronisation of the call */
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    ms = ev.ms();
    if (h_rec.fail) {
      set_error("kv_utxo_balance_by_spk: a table entry's script reference is out "
                "of range");
      return -3;
    }
  }
  if (n_q) memcpy(balances_out, sums.data(), 8 * n_q);
  if (n_q && counts_out) memcpy(counts_out, sums.data() + n_q, 8 * n_q);
  if (total_amount_out) *total_amount_out = h_rec.total;
  if (n_live_out) *n_live_out = h_rec.n_live;
  if (kernel_ms) *kernel_ms = ms;
  return 0;
}

extern "C" int kv_utxo_find_by_spk(kv_ctx *ctx, uint64_t *cursor, const kv_spk_query *q,
                                   size_t n_q, const uint8_t *spk_blob,
                                   size_t spk_blob_len, size_t max_entries,
                                   uint8_t *matches_out, size_t *n_out) {
  KV_ENTER(ctx);
  if (!cursor || !n_out || !matches_out || max_entries == 0) {
    set_error("kv_utxo_find_by_spk: null argument, or max_entries == 0");
    return -1;
  }
  QueryLayout L;
  int rc = query_set_build(ctx, "kv_utxo_find_by_spk", q, n_q, spk_blob, spk_blob_len,
                           &L);
  if (rc) return rc;
  if (!ctx->d_utxo.p || *cursor >= ctx->utxo_cap || n_q == 0) {
    /* nothing to scan: never reset (the cursor stays), the walk is over, or
     * there is no query to match */
    *n_out = 0;
    if (ctx->d_utxo.p) *cursor = ctx->utxo_cap;
    return 0;
  }
  kv::spk_query_set S;
  rc = query_set_upload(ctx, L, &S);
  if (rc) return rc;
  *n_out = 0;
  const uint32_t max_e = (uint32_t)std::min<size_t>(max_entries, KV_COMMIT_WINDOW);
  const uint32_t out_cap = max_e + KV_COMMIT_WINDOW;
  const size_t off_slots = 64, off_recs = off_slots + (size_t)out_cap * 8;
  /* exactly the bound: (max_entries + one window) × 104 B */
  const size_t need = off_recs + (size_t)out_cap * KV_QUERY_MATCH_BYTES;
  if (ctx->d_q_find.cap < need && ctx->d_q_find.alloc(need)) return -2;
  uint8_t *fb = ctx->d_q_find.as<uint8_t>();
  kv::query_rec *d_rec = (kv::query_rec *)fb;
  unsigned long long *d_slots = (unsigned long long *)(fb + off_slots);
  uint8_t *d_recs = fb + off_recs;
  const uint64_t start = *cursor, end = ctx->utxo_cap;
  HIP_CHECK(hipMemsetAsync(d_rec, 0, sizeof(kv::query_rec), ctx->stream));
  HIP_CHECK(hipMemsetAsync(&d_rec->first_skipped, 0xff, 4, ctx->stream));
  /* window w of this walk starts at win_start(w); the first may be partial */
  auto win_start = [&](uint64_t w) {
    return w == 0 ? start : (start / KV_COMMIT_WINDOW + w) * (uint64_t)KV_COMMIT_WINDOW;
  };
  uint32_t w = 0;
  for (uint64_t base = start; base < end; w++) {
    const uint32_t n_slots = (uint32_t)std::min<uint64_t>(
        KV_COMMIT_WINDOW - (base & (KV_COMMIT_WINDOW - 1)), end - base);
    /* the stop rule's snapshot: what the windows before this one stored */
    HIP_CHECK(hipMemcpyAsync(&d_rec->seen, &d_rec->count, 4, hipMemcpyDeviceToDevice,
                             ctx->stream));
    hipLaunchKernelGGL(kv::kv_utxo_find_kernel, dim3((n_slots + 255) / 256), dim3(256),
                       0, ctx->stream, ctx->table(), base, n_slots, S,
                       ctx->d_arena.as<const uint8_t>(), ctx->arena_head, max_e, w,
                       out_cap, d_slots, d_recs, d_rec);
    base += n_slots;
  }
  HIP_CHECK(hipGetLastError());
  kv::query_rec h_rec;
  HIP_CHECK(hipMemcpyAsync(&h_rec, d_rec, sizeof(h_rec), hipMemcpyDeviceToHost,
                           ctx->stream));
  /* the single synchronisation of the chain */
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  if (h_rec.fail) {
    set_error("kv_utxo_find_by_spk: a table entry's script reference is out of range");
    return -3;
  }
  if (h_rec.count >= out_cap) {
    set_error("kv_utxo_find_by_spk: match count out of range");
    return -2;
  }
  /* every window below `limit` ran and stored all of its matches */
  const uint64_t limit =
      h_rec.first_skipped == 0xffffffffu ? end : win_start(h_rec.first_skipped);
  const uint32_t stored = h_rec.count;
  if (stored == 0) {
    *cursor = limit;
    return 0;
  }
  std::vector<unsigned long long> slots(stored);
  HIP_CHECK(hipMemcpy(slots.data(), d_slots, (size_t)stored * 8, hipMemcpyDeviceToHost));
  /* positions are whatever the waves' atomics made them: sort by slot and take
   * the first max_entries; the rest is found again by the next call */
  std::vector<uint32_t> order(stored);
  for (uint32_t i = 0; i < stored; i++) order[i] = i;
  std::sort(order.begin(), order.end(),
            [&](uint32_t a, uint32_t b) { return slots[a] < slots[b]; });
  const uint32_t m = std::min(stored, max_e);
  uint32_t hi = 0; /* one past the last buffer position among those returned */
  for (uint32_t i = 0; i < m; i++) hi = std::max(hi, order[i] + 1);
  std::vector<uint8_t> &recs = ctx->ent_buf;
  recs.resize((size_t)hi * KV_QUERY_MATCH_BYTES);
  HIP_CHECK(hipMemcpy(recs.data(), d_recs, recs.size(), hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < m; i++)
    memcpy(matches_out + (size_t)i * KV_QUERY_MATCH_BYTES,
           recs.data() + (size_t)order[i] * KV_QUERY_MATCH_BYTES, KV_QUERY_MATCH_BYTES);
  *cursor = m < stored ? slots[order[m - 1]] + 1 : limit;
  *n_out = m;
  return 0;
}

/* ---------------- undo journal (kv_utxo_journal_kernels.hip) -----------------
 * ⇔ the stored chain-block diffs of calculate_utxo_state_relatively
 * (processor.rs:393-437): kv_utxo_apply_diff ⇔ write_diff_batch
 * (utxo_set.rs:107-112) with the inverse kept, kv_utxo_revert ⇔
 * with_diff_in_place(as_reversed) (processor.rs:410, utxo_diff.rs:71). */

/* are the na + nb outpoints distinct? A host-side open-addressing set of row
 * numbers, hashed like the table. */
static bool ops_distinct(const uint8_t *a, size_t na, const uint8_t *b, size_t nb) {
  const size_t n = na + nb;
  if (n < 2) return true;
  size_t cap = 16;
  while (cap < 2 * n) cap <<= 1;
  std::vector<uint32_t> rows(cap, 0); /* row + 1; 0 = free */
  auto at = [&](size_t i) { return i < na ? a + i * 36 : b + (i - na) * 36; };
  for (size_t i = 0; i < n; i++) {
    const uint8_t *op = at(i);
    uint64_t h;
    uint32_t idx;
    memcpy(&h, op, 8);
    memcpy(&idx, op + 32, 4);
    h ^= 0x9e3779b97f4a7c15ULL * (idx + 1);
    size_t slot = (size_t)(h ^ (h >> 32)) & (cap - 1);
    for (; rows[slot]; slot = (slot + 1) & (cap - 1))
      if (!memcmp(at(rows[slot] - 1), op, 36)) return false;
    rows[slot] = (uint32_t)i + 1;
  }
  return true;
}

/* caller holds ctx->mu. Plays the newest record back (see kv_utxo_revert) and
 * pops it. */
static int journal_revert_nolock(kv_ctx *ctx, uint64_t token) {
  if (ctx->journal.empty() || ctx->journal.back().token != token) {
    set_error("kv_utxo_revert: not the newest unreverted record");
    return -1;
  }
  JournalRecord &r = ctx->journal.back();
  const size_t n = r.n();
  const uint64_t base = ctx->arena_head;
  EventPair ev;
  HIP_CHECK(ev.init());
  if (r.blob_bytes) {
    if (base + r.blob_bytes > 0xffffffffULL) {
      set_error("kv_utxo_revert: arena exceeds a u32 offset; kv_utxo_rehash first");
      return -3;
    }
    int rc = arena_reserve(ctx, r.blob_bytes);
    if (rc) return rc;
  }
  if (ctx->d_utxo_fail.ensure(4)) return -2;
  int *d_fail = ctx->d_utxo_fail.as<int>();
  int fail = 0;
  HIP_CHECK(hipEventRecord(ev.a, ctx->stream));
  if (r.blob_bytes)
    HIP_CHECK(hipMemcpyAsync(ctx->d_arena.as<uint8_t>() + base, r.blob.p, r.blob_bytes,
                             hipMemcpyDeviceToDevice, ctx->stream));
  HIP_CHECK(hipMemsetAsync(d_fail, 0, 4, ctx->stream));
  if (r.n_added)
    hipLaunchKernelGGL(kv::kv_utxo_journal_unadd_kernel,
                       dim3(((uint32_t)r.n_added + 255) / 256), dim3(256), 0,
                       ctx->stream, ctx->table(), ctx->utxo_cap - 1,
                       (const uint8_t *)r.keys(),
                       (const unsigned long long *)r.found(),
                       (unsigned long long)r.n_removed, (unsigned long long)n);
  if (n)
    hipLaunchKernelGGL(kv::kv_utxo_journal_restore_kernel,
                       dim3(((uint32_t)n + 255) / 256), dim3(256), 0, ctx->stream,
                       ctx->table(), ctx->utxo_cap - 1, (const uint8_t *)r.keys(),
                       (const uint8_t *)r.vals(), (const unsigned long long *)r.found(),
                       (unsigned long long)n, base, r.blob_bytes, base + r.blob_bytes,
                       d_fail);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(ev.b, ctx->stream));
  HIP_CHECK(hipMemcpyAsync(&fail, d_fail, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  ctx->arena_head = base + r.blob_bytes; /* restored values refer to these bytes */
  ctx->last_revert_ms = ev.ms();
  if (fail) {
    set_error("kv_utxo_revert: table full (the set is not in the state the apply "
              "left it in)");
    return -3;
  }
  ctx->journal.pop_back();
  return 0;
}

/* caller holds ctx->mu; see kv_utxo_apply_diff */
static int journal_apply_nolock(kv_ctx *ctx, const uint8_t *removed_ops, size_t n_removed,
                                const uint8_t *added_ops, const uint8_t *added_entries64,
                                const uint8_t *spk_blob, size_t spk_blob_len,
                                size_t n_added, kv_utxo_diff_result *res_out,
                                uint64_t *undo_token_out) {
  if (!undo_token_out || (n_removed && !removed_ops) ||
      (n_added && (!added_ops || !added_entries64))) {
    set_error("kv_utxo_apply_diff: null argument");
    return -1;
  }
  if (!ctx->d_utxo.p) {
    set_error("kv_utxo_apply_diff: call kv_utxo_reset first");
    return -1;
  }
  if (n_removed > (1u << 30) || n_added > (1u << 30)) {
    set_error("kv_utxo_apply_diff: diff too large");
    return -1;
  }
  /* every -1 of the upsert that follows the remove is decided here, before
   * anything changes */
  uint64_t long_total = 0;
  size_t n_arena = 0;
  if (utxo_spk_args_check(added_entries64, spk_blob_len, n_added, &long_total, &n_arena))
    return -1;
  if (!ops_distinct(removed_ops, n_removed, added_ops, n_added)) {
    set_error("kv_utxo_apply_diff: outpoints are not distinct across removed and added");
    return -1;
  }
  JournalRecord r;
  r.n_removed = n_removed;
  r.n_added = n_added;
  const size_t n = r.n();
  if (n && r.fixed.alloc(r.fixed_bytes())) return -2;
  if (ctx->d_jrn_rec.ensure(sizeof(kv::journal_rec)) ||
      ctx->d_gjobs.ensure(n * sizeof(kv::arena_gather_job)))
    return -2;
  kv::journal_rec *d_rec = ctx->d_jrn_rec.as<kv::journal_rec>();
  kv::journal_rec h_rec = {};
  EventPair ev_cap, ev_copy, ev_up;
  HIP_CHECK(ev_cap.init());
  HIP_CHECK(ev_copy.init());
  HIP_CHECK(ev_up.init());

  /* capture (and tombstone the removed side): one launch, one 32 B record
   * back, one synchronisation */
  if (n_removed)
    HIP_CHECK(hipMemcpyAsync(r.keys(), removed_ops, n_removed * 36,
                             hipMemcpyHostToDevice, ctx->stream));
  if (n_added)
    HIP_CHECK(hipMemcpyAsync(r.keys() + n_removed * 36, added_ops, n_added * 36,
                             hipMemcpyHostToDevice, ctx->stream));
  HIP_CHECK(hipEventRecord(ev_cap.a, ctx->stream));
  HIP_CHECK(hipMemsetAsync(d_rec, 0, sizeof(kv::journal_rec), ctx->stream));
  if (n) {
    hipLaunchKernelGGL(kv::kv_utxo_journal_capture_kernel,
                       dim3(((uint32_t)n + 255) / 256), dim3(256), 0, ctx->stream,
                       ctx->table(), ctx->utxo_cap - 1, (const uint8_t *)r.keys(),
                       (unsigned long long)n, (unsigned long long)n_removed,
                       ctx->arena_head, r.vals(), r.found(),
                       ctx->d_gjobs.as<kv::arena_gather_job>(), (uint32_t)n, d_rec);
    HIP_CHECK(hipGetLastError());
  }
  HIP_CHECK(hipEventRecord(ev_cap.b, ctx->stream));
  HIP_CHECK(hipMemcpyAsync(&h_rec, d_rec, sizeof(kv::journal_rec), hipMemcpyDeviceToHost,
                           ctx->stream));
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  double ms = ev_cap.ms();

  /* the record's own copy of the long scripts it captured, one block a script */
  r.blob_bytes = h_rec.blob_bytes;
  if (r.blob_bytes) {
    if (r.blob.alloc(r.blob_bytes)) return -2;
    HIP_CHECK(hipEventRecord(ev_copy.a, ctx->stream));
    hipLaunchKernelGGL(kv::kv_arena_copy_jobs_kernel,
                       dim3(std::min<uint32_t>(h_rec.n_jobs, (uint32_t)n)), dim3(256), 0,
                       ctx->stream, ctx->d_arena.as<const uint8_t>(),
                       ctx->d_gjobs.as<const kv::arena_gather_job>(),
                       (const uint32_t *)&d_rec->n_jobs, (uint32_t)n,
                       r.blob.as<uint8_t>());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ev_copy.b, ctx->stream));
  }
  int rc = 0;
  if (h_rec.fail) {
    set_error("kv_utxo_apply_diff: a table entry's script reference is out of range");
    rc = -3;
  }
  /* the diff's upsert; it ends in a synchronisation, which the script copy
   * needs too */
  if (!rc && n_added)
    rc = utxo_upsert_spk_nolock(ctx, added_ops, added_entries64, spk_blob, spk_blob_len,
                                n_added, &ev_up);
  else
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
  if (rc && rc != -3) return rc; /* a HIP error: nothing more can be done */
  if (r.blob_bytes) ms += ev_copy.ms();
  if (!rc && n_added) ms += ev_up.ms();

  r.token = ctx->next_token++;
  const uint64_t token = r.token, bytes = r.device_bytes();
  ctx->journal.push_back(std::move(r));
  if (rc) {
    /* failure atomicity: undo what was done from the record just captured */
    const std::string why = g_last_error;
    int rr = journal_revert_nolock(ctx, token);
    if (rr) {
      set_error((why + "; undoing the partial diff failed too: record " +
                 std::to_string(token) + " kept")
                    .c_str());
      return rr;
    }
    set_error(why.c_str());
    return rc;
  }
  if (res_out) {
    res_out->n_removed_missing = h_rec.n_removed_missing;
    res_out->n_added_overwrote = h_rec.n_added_overwrote;
    res_out->journal_bytes = bytes;
    res_out->kernel_ms = ms;
  }
  *undo_token_out = token;
  return 0;
}

extern "C" int kv_utxo_apply_diff(kv_ctx *ctx, const uint8_t *removed_ops,
                                  size_t n_removed, const uint8_t *added_ops,
                                  const uint8_t *added_entries64, const uint8_t *spk_blob,
                                  size_t spk_blob_len, size_t n_added,
                                  kv_utxo_diff_result *res_out,
                                  uint64_t *undo_token_out) {
  KV_ENTER(ctx);
  return journal_apply_nolock(ctx, removed_ops, n_removed, added_ops, added_entries64,
                              spk_blob, spk_blob_len, n_added, res_out, undo_token_out);
}

extern "C" int kv_utxo_revert(kv_ctx *ctx, uint64_t token) {
  KV_ENTER(ctx);
  return journal_revert_nolock(ctx, token);
}

extern "C" int kv_utxo_journal_drop(kv_ctx *ctx, uint64_t upto_token) {
  KV_ENTER(ctx);
  /* no record is in use on the stream: every apply and revert ends synchronised */
  while (!ctx->journal.empty() && ctx->journal.front().token <= upto_token)
    ctx->journal.pop_front();
  return 0;
}

extern "C" int kv_utxo_journal_stats(kv_ctx *ctx, kv_utxo_journal_info *out) {
  if (!ctx || !out) {
    set_error("kv_utxo_journal_stats: null argument");
    return -1;
  }
  KV_ENTER(ctx);
  memset(out, 0, sizeof(*out));
  out->n_records = ctx->journal.size();
  if (!ctx->journal.empty()) {
    out->oldest_token = ctx->journal.front().token;
    out->newest_token = ctx->journal.back().token;
  }
  for (const JournalRecord &r : ctx->journal) out->device_bytes += r.device_bytes();
  out->last_revert_kernel_ms = ctx->last_revert_ms;
  return 0;
}

/* ---------------- per-script changes of a record (kv_utxo_changes_kernels.hip)
 * ⇔ UtxoIndexChanges::update_utxo_diff (indexes/utxoindex/src/
 * update_container.rs:29-51) filtered as filter_utxo_set does
 * (indexes/core/src/notification.rs:81-127), with the supply change of
 * indexes/utxoindex/src/index.rs:98. */

/* launch the block-per-script gather over `src` into ctx->d_gout (the caller
 * sized it) for the jobs of one source; queued, not synchronised */
static int changes_gather(kv_ctx *ctx, const uint8_t *src,
                          const std::vector<kv::arena_gather_job> &jobs, size_t at) {
  if (jobs.empty()) return 0;
  kv::arena_gather_job *d_jobs = ctx->d_gjobs.as<kv::arena_gather_job>() + at;
  HIP_CHECK(hipMemcpyAsync(d_jobs, jobs.data(), jobs.size() * sizeof(kv::arena_gather_job),
                           hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(kv::kv_arena_gather_kernel, dim3((uint32_t)jobs.size()), dim3(256),
                     0, ctx->stream, src, (const kv::arena_gather_job *)d_jobs,
                     (uint32_t)jobs.size(), ctx->d_gout.as<uint8_t>());
  HIP_CHECK(hipGetLastError());
  return 0;
}

extern "C" int kv_utxo_changes_by_spk(kv_ctx *ctx, uint64_t token, uint32_t flags,
                                      uint64_t *cursor, const kv_spk_query *q, size_t n_q,
                                      const uint8_t *spk_blob, size_t spk_blob_len,
                                      size_t max_entries, uint8_t *changes_out,
                                      uint8_t *spk_out, size_t spk_cap, size_t *spk_used,
                                      size_t *n_out, kv_utxo_changes_result *res_out) {
  KV_ENTER(ctx);
  if (!cursor || !n_out || !res_out || !changes_out || max_entries == 0) {
    set_error("kv_utxo_changes_by_spk: null argument, or max_entries == 0");
    return -1;
  }
  const bool all = flags & KV_UTXO_CHANGES_ALL;
  if ((flags & ~(KV_UTXO_CHANGES_REVERSED | KV_UTXO_CHANGES_ALL)) || (all && n_q)) {
    set_error("kv_utxo_changes_by_spk: unknown flag bits, or KV_UTXO_CHANGES_ALL with "
              "queries");
    return -1;
  }
  if (spk_out && spk_cap < KV_UTXO_MAX_SPK) {
    set_error("kv_utxo_changes_by_spk: spk_cap below KV_UTXO_MAX_SPK");
    return -1;
  }
  const JournalRecord *r = nullptr;
  for (const JournalRecord &jr : ctx->journal)
    if (jr.token == token) r = &jr;
  if (!r) {
    set_error("kv_utxo_changes_by_spk: no such record in the journal");
    return -1;
  }
  const uint64_t total = (uint64_t)r->n_removed + 2 * (uint64_t)r->n_added;
  const uint64_t start = *cursor;
  if (start > total) {
    set_error("kv_utxo_changes_by_spk: cursor past cursor_end");
    return -1;
  }
  QueryLayout L;
  int rc = query_set_build(ctx, "kv_utxo_changes_by_spk", q, n_q, spk_blob, spk_blob_len,
                           &L);
  if (rc) return rc;

  /* Scratch: 64 B for the copy-back record, then 144 B (staged record) + 8 B
   * (key) per lane that can store, cursor_end - *cursor of them at most and
   * none when there is no query to match: bounded by the record, never by
   * table capacity. The query table (query_set_upload) comes on top. The
   * staged records come first: they are written 16 bytes at a time. */
  const uint64_t out_cap64 = (all || n_q) ? total - start : 0;
  const uint32_t out_cap = (uint32_t)out_cap64; /* total < 2^32: see apply_diff */
  const size_t off_staged = 64,
               off_keys = off_staged + (size_t)out_cap * KV_CHANGE_STAGED_BYTES;
  const size_t need = off_keys + (size_t)out_cap * 8;
  kv::changes_rec h_rec = {};
  double ms = 0.0;
  uint8_t *cb = nullptr;
  if (total) { /* else both sides are empty: zeros, and the walk is over */
    kv::spk_query_set S;
    rc = query_set_upload(ctx, L, &S);
    if (rc) return rc;
    if (ctx->d_chg.ensure(need)) return -2;
    cb = ctx->d_chg.as<uint8_t>();
    kv::changes_rec *d_rec = (kv::changes_rec *)cb;
    EventPair ev;
    HIP_CHECK(ev.init());
    HIP_CHECK(hipMemsetAsync(d_rec, 0, sizeof(kv::changes_rec), ctx->stream));
    HIP_CHECK(hipEventRecord(ev.a, ctx->stream));
    hipLaunchKernelGGL(kv::kv_utxo_changes_kernel, dim3((uint32_t)((total + 255) / 256)),
                       dim3(256), 0, ctx->stream, ctx->table(), ctx->utxo_cap - 1,
                       (const uint8_t *)r->keys(), (const uint8_t *)r->vals(),
                       (const unsigned long long *)r->found(),
                       (unsigned long long)r->n_removed, (unsigned long long)total,
                       r->blob.as<const uint8_t>(), r->blob_bytes,
                       ctx->d_arena.as<const uint8_t>(), ctx->arena_head, S, flags,
                       (unsigned long long)start, out_cap,
                       (unsigned long long *)(cb + off_keys), cb + off_staged, d_rec);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ev.b, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(&h_rec, d_rec, sizeof(h_rec), hipMemcpyDeviceToHost,
                             ctx->stream));
    /* the single synchronisation of the launch */
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    ms = ev.ms();
    if (h_rec.fail) {
      set_error("kv_utxo_changes_by_spk: a value's script reference is out of range");
      return -3;
    }
    if (h_rec.stored > out_cap) {
      set_error("kv_utxo_changes_by_spk: stored count out of range");
      return -2;
    }
  }

  /* positions are whatever the waves' atomics made them: sort the keys (change
   * index, script length above it) and cut the prefix that fits max_entries
   * and spk_cap */
  const uint32_t stored = h_rec.stored;
  std::vector<unsigned long long> keys(stored);
  if (stored)
    HIP_CHECK(hipMemcpy(keys.data(), cb + off_keys, (size_t)stored * 8,
                        hipMemcpyDeviceToHost));
  const unsigned long long idx_mask = (1ULL << KV_CHANGE_KEY_LEN_SHIFT) - 1;
  std::vector<uint32_t> order(stored);
  for (uint32_t i = 0; i < stored; i++) order[i] = i;
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    return (keys[a] & idx_mask) < (keys[b] & idx_mask);
  });
  size_t m = 0, used = 0;
  uint32_t lo = stored, hi = 0; /* the buffer positions among those returned */
  for (; m < stored && m < max_entries; m++) {
    const size_t len = (size_t)(keys[order[m]] >> KV_CHANGE_KEY_LEN_SHIFT);
    if (spk_out && used + len > spk_cap) break; /* the next chunk starts here */
    used += len;
    lo = std::min(lo, order[m]);
    hi = std::max(hi, order[m] + 1);
  }
  /* m >= 1 when anything is stored: the first script always fits */
  std::vector<uint8_t> &staged = ctx->ent_buf;
  std::vector<uint8_t> gathered;
  if (m) {
    staged.resize((size_t)(hi - lo) * KV_CHANGE_STAGED_BYTES);
    HIP_CHECK(hipMemcpy(staged.data(),
                        cb + off_staged + (size_t)lo * KV_CHANGE_STAGED_BYTES,
                        staged.size(), hipMemcpyDeviceToHost));
  }
  auto staged_at = [&](size_t i) {
    return staged.data() + (size_t)(order[i] - lo) * KV_CHANGE_STAGED_BYTES;
  };
  if (m && spk_out && used) {
    /* out-of-line scripts: one gather per source, both into d_gout at the
     * offsets the scripts take in spk_out */
    std::vector<kv::arena_gather_job> from_blob, from_arena;
    uint32_t at = 0;
    for (size_t i = 0; i < m; i++) {
      uint32_t w[36];
      memcpy(w, staged_at(i), sizeof(w));
      const uint32_t len = w[15];
      if (len && w[24] == KV_CHANGE_SPK_BLOB)
        from_blob.push_back(kv::arena_gather_job{w[25], len, at, 0});
      else if (len && w[24] == KV_CHANGE_SPK_ARENA)
        from_arena.push_back(kv::arena_gather_job{w[25], len, at, 0});
      at += len;
    }
    const size_t n_jobs = from_blob.size() + from_arena.size();
    if (n_jobs) {
      if (ctx->d_gjobs.ensure(n_jobs * sizeof(kv::arena_gather_job)) ||
          ctx->d_gout.ensure(used))
        return -2;
      EventPair ev;
      HIP_CHECK(ev.init());
      HIP_CHECK(hipEventRecord(ev.a, ctx->stream));
      rc = changes_gather(ctx, r->blob.as<const uint8_t>(), from_blob, 0);
      if (!rc)
        rc = changes_gather(ctx, ctx->d_arena.as<const uint8_t>(), from_arena,
                            from_blob.size());
      if (rc) return rc;
      HIP_CHECK(hipEventRecord(ev.b, ctx->stream));
      gathered.resize(used);
      HIP_CHECK(hipMemcpyAsync(gathered.data(), ctx->d_gout.p, used,
                               hipMemcpyDeviceToHost, ctx->stream));
      HIP_CHECK(hipStreamSynchronize(ctx->stream));
      ms += ev.ms();
    }
  }
  /* nothing can fail from here on: write the outputs */
  size_t at = 0;
  for (size_t i = 0; i < m; i++) {
    const uint8_t *s = staged_at(i);
    memcpy(changes_out + i * KV_CHANGE_BYTES, s, KV_CHANGE_BYTES);
    if (!spk_out) continue;
    uint32_t len, kind;
    memcpy(&len, s + 60, 4);
    memcpy(&kind, s + 96, 4);
    if (len) /* inline: the value's own field, words 26.. of the staged record */
      memcpy(spk_out + at, kind == KV_CHANGE_SPK_INLINE ? s + 104 : gathered.data() + at,
             len);
    at += len;
  }
  *cursor = m < stored ? (keys[order[m - 1]] & idx_mask) + 1 : total;
  *n_out = m;
  if (spk_out && spk_used) *spk_used = used;
  const int rev = (flags & KV_UTXO_CHANGES_REVERSED) ? 1 : 0;
  res_out->cursor_end = total;
  res_out->added_amount = h_rec.amount[1 - rev];
  res_out->removed_amount = h_rec.amount[rev];
  res_out->n_added = h_rec.count[1 - rev];
  res_out->n_removed = h_rec.count[rev];
  res_out->n_added_gone = h_rec.n_added_gone;
  res_out->kernel_ms = ms;
  return 0;
}

static int populate_blob_nolock(kv_ctx *ctx, const uint8_t *blob, size_t blob_len,
                                std::vector<kvhost::HTx> &txs, int n_txs,
                                std::vector<int32_t> &pre_codes);

/* ---------------- mempool batch validation ----------------
 * ⇔ validate_mempool_transaction_in_utxo_context (utxo_validation.rs:418-457)
 * fanned over a batch: entries resolve inline from the blob (from_utxo_table
 * = 0, the caller populated) or from the GPU-resident table (= 1; a missing
 * outpoint fails that tx with KV_ERR_MISSING_OUTPOINT, mirroring
 * populate_mempool_transaction_in_utxo_context:392-415). The contextual
 * storage mass is COMPUTED per tx (the carried commitment is ignored — the
 * mempool sets it), validation runs with SkipMassCheck, and the optional
 * feerate threshold rejects fee / normalized_max(mass) <= threshold with
 * KV_ERR_FEERATE_TOO_LOW (tx_validation_in_utxo_context.rs:69-77). */
extern "C" int kv_validate_mempool(kv_ctx *ctx, const uint8_t *blob,
                                   size_t blob_len, uint64_t pov_daa_score,
                                   double feerate_threshold, int from_utxo_table,
                                   int32_t *tx_codes_out, uint64_t *fees_out) {
  KV_ENTER(ctx);
  vector<HTx> txs;
  int n_txs = parse_blob_host(blob, blob_len, txs);
  if (n_txs < 0) {
    set_error("kv_validate_mempool: malformed blob");
    return -1;
  }
  std::vector<int32_t> pre_codes(n_txs, 0);
  const uint8_t *vblob = blob;
  size_t vlen = blob_len;
  vector<HTx> ptxs;
  const vector<HTx> *use_txs = &txs;
  if (from_utxo_table) {
    if (!ctx->d_utxo.p) {
      set_error("kv_validate_mempool: call kv_utxo_reset first");
      return -1;
    }
    int rc = populate_blob_nolock(ctx, blob, blob_len, txs, n_txs, pre_codes);
    if (rc) return rc;
    vblob = ctx->pop_buf.data();
    vlen = ctx->pop_buf.size();
    if (parse_blob_host(vblob, vlen, ptxs) != n_txs) {
      set_error("kv_validate_mempool: internal rebuild parse");
      return -1;
    }
    use_txs = &ptxs;
  }
  int rc = validate_block_impl(ctx, vblob, vlen, pov_daa_score, pov_daa_score,
                               KV_FLAGS_SKIP_MASS_CHECK, tx_codes_out, fees_out,
                               nullptr, pre_codes.data());
  if (rc) return rc;
  /* contextual mass + feerate post-pass (mass computed BEFORE validation in
   * the reference, so MassIncomputable wins over any validation error) */
  for (int t = 0; t < n_txs; t++) {
    const HTx &tx = (*use_txs)[t];
    if (pre_codes[t]) continue; /* populate failure stands */
    uint64_t storage = 0;
    if (kvh_storage_mass(tx, h_is_coinbase(tx), &storage)) {
      tx_codes_out[t] = KV_ERR_MASS_INCOMPUTABLE;
      fees_out[t] = 0;
    } else if (feerate_threshold > 0 &&
               (tx_codes_out[t] == 0 || tx_codes_out[t] == KV_ERR_COVENANT_AUTH_INPUT ||
                tx_codes_out[t] == KV_ERR_COVENANT_GENESIS_ID)) {
      /* the reference checks the feerate (:57) before the covenant bindings
       * (:58), so it wins over them. A covenant failure cleared the fee, but
       * the amount checks before it passed: the fee is the plain difference. */
      uint64_t fee = fees_out[t];
      if (tx_codes_out[t]) {
        fee = 0;
        for (const auto &in : tx.inputs) fee += in.utxo_amount;
        for (const auto &o : tx.outputs) fee -= o.value;
      }
      uint64_t m = kvh_normalized_mass(tx, storage);
      if (m > 0 && (double)fee / (double)m <= feerate_threshold) {
        tx_codes_out[t] = KV_ERR_FEERATE_TOO_LOW;
        fees_out[t] = 0;
      }
    }
  }
  return 0;
}

/* ---------------- merkle root + body-in-isolation batch ----------------
 * ⇔ validate_body_in_isolation (consensus/src/pipeline/body_processor/
 * body_validation_in_isolation.rs): calc_hash_merkle_root (:38 via
 * consensus/core/src/merkle.rs:5 → crypto/merkle/src/lib.rs:31-52) over the
 * GPU-computed tx hashes, plus check_duplicate_transactions (:152),
 * check_block_double_spends (:126) and check_no_chained_transactions (:136).
 * The leaf hashes (one keyed blake2b per tx over the full serialization) run
 * on device; the log-depth fold and the set checks run on the host pool. */
extern "C" int kv_block_body_check(kv_ctx *ctx, const uint8_t *blob,
                                   size_t blob_len, uint8_t merkle_root_out[32],
                                   int32_t *rule_code_out) {
  KV_ENTER(ctx);
  ValidateBufs &vb = ctx->vb;
  vector<HTx> txs;
  int n_txs = parse_blob_host(blob, blob_len, txs);
  if (n_txs < 0) {
    set_error("kv_block_body_check: malformed blob");
    return -1;
  }
  /* leaf hashes on device */
  std::vector<uint8_t> hashes((size_t)n_txs * 32);
  if (n_txs > 0) {
    if (vb.blob.ensure(blob_len) || vb.tx_hashes.ensure((size_t)n_txs * 32))
      return -2;
    HIP_CHECK(hipMemcpyAsync(vb.blob.p, blob, blob_len, hipMemcpyHostToDevice,
                             ctx->stream));
    hipLaunchKernelGGL(kv::kv_tx_hash_kernel, dim3((n_txs + 255) / 256),
                       dim3(256), 0, ctx->stream, (const uint8_t *)vb.blob.p,
                       (uint32_t)n_txs, (uint8_t *)vb.tx_hashes.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(hashes.data(), vb.tx_hashes.p,
                             (size_t)n_txs * 32, hipMemcpyDeviceToHost,
                             ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
  }
  /* merkle fold (crypto/merkle/src/lib.rs:31-52): pad to a power of two,
   * absent left → absent parent, absent right → ZERO_HASH */
  if (merkle_root_out) {
    if (n_txs == 0) {
      memset(merkle_root_out, 0, 32);
    } else if (n_txs == 1) {
      memcpy(merkle_root_out, hashes.data(), 32);
    } else {
      size_t pot = 1;
      while (pot < (size_t)n_txs) pot <<= 1;
      std::vector<uint8_t> cur(pot * 32, 0), pres(pot, 0);
      memcpy(cur.data(), hashes.data(), (size_t)n_txs * 32);
      for (int i = 0; i < n_txs; i++) pres[i] = 1;
      static const uint8_t ZERO[32] = {0};
      size_t width = pot;
      /* each level is written into its own buffer: with 256 or more parents
       * the level is fanned over the host threads, and parent o of one thread
       * sits where another thread still reads children 2o', 2o'+1 */
      std::vector<uint8_t> nxt(pot / 2 * 32, 0), npres(pot / 2, 0);
      while (width > 1) {
        kvh_parallel_for((uint32_t)(width / 2), [&](uint32_t o) {
          size_t i = 2 * (size_t)o;
          if (!pres[i]) {
            npres[o] = 0;
            return;
          }
          uint8_t buf[64];
          memcpy(buf, cur.data() + i * 32, 32);
          memcpy(buf + 32, pres[i + 1] ? cur.data() + (i + 1) * 32 : ZERO, 32);
          uint8_t h[32];
          static const uint8_t MKEY[] = "MerkleBranchHash";
          h_blake2b_keyed(MKEY, sizeof(MKEY) - 1, buf, 64, h);
          memcpy(nxt.data() + o * 32, h, 32);
          npres[o] = 1;
        });
        cur.swap(nxt);
        pres.swap(npres);
        width /= 2;
      }
      memcpy(merkle_root_out, cur.data(), 32);
    }
  }
  /* body rule checks (first violation wins, reference order) */
  int32_t code = 0;
  {
    std::vector<std::array<uint8_t, 32>> ids(n_txs);
    for (int t = 0; t < n_txs; t++) memcpy(ids[t].data(), txs[t].tx_id, 32);
    std::sort(ids.begin(), ids.end());
    for (int t = 0; t + 1 < n_txs; t++)
      if (ids[t] == ids[t + 1]) {
        code = KV_ERR_BODY_DUP_TX;
        break;
      }
  }
  if (!code) {
    std::vector<std::array<uint8_t, 36>> ops;
    for (auto &tx : txs)
      for (auto &in : tx.inputs) {
        std::array<uint8_t, 36> o;
        memcpy(o.data(), in.prev_tx_id, 32);
        memcpy(o.data() + 32, &in.prev_index, 4);
        ops.push_back(o);
      }
    std::sort(ops.begin(), ops.end());
    for (size_t i = 0; i + 1 < ops.size(); i++)
      if (ops[i] == ops[i + 1]) {
        code = KV_ERR_BODY_DOUBLE_SPEND;
        break;
      }
    if (!code) {
      std::vector<std::array<uint8_t, 36>> created;
      for (auto &tx : txs)
        for (uint32_t i = 0; i < tx.outputs.size(); i++) {
          std::array<uint8_t, 36> o;
          memcpy(o.data(), tx.tx_id, 32);
          memcpy(o.data() + 32, &i, 4);
          created.push_back(o);
        }
      std::sort(created.begin(), created.end());
      for (auto &tx : txs) {
        for (auto &in : tx.inputs) {
          std::array<uint8_t, 36> key;
          memcpy(key.data(), in.prev_tx_id, 32);
          memcpy(key.data() + 32, &in.prev_index, 4);
          if (std::binary_search(created.begin(), created.end(), key)) {
            code = KV_ERR_BODY_CHAINED;
            break;
          }
        }
        if (code) break;
      }
    }
  }
  if (rule_code_out) *rule_code_out = code;
  return 0;
}

/* ---------------- populate + validate + diff-apply ----------------
 * ⇔ the virtual processor's populate step (utxo_validation.rs:351-390:
 * each input's UtxoEntry is resolved from the virtual UTXO set; a missing
 * outpoint fails the tx) followed by validation and utxo_diff application
 * (utxo_diff.rs:224 add_transaction: remove spent, add created).
 *
 * The incoming blob uses the same format but every input's UtxoEntry fields
 * are ignored (builders write zeros, utxo_spk_len = 0). Entries come from the
 * GPU-resident table (kv_utxo_reset/upsert); the engine rebuilds a populated
 * blob internally (one linear pass — the entry fields are the only part that
 * moves) and runs the standard pipeline on it. */
/* caller holds ctx->mu. Resolves every input's entry from the GPU table into
 * a rebuilt populated blob (ctx->pop_buf); missing outpoints pre-fail their tx
 * with KV_ERR_MISSING_OUTPOINT in pre_codes. */
static int populate_blob_nolock(kv_ctx *ctx, const uint8_t *blob, size_t blob_len,
                                vector<HTx> &txs, int n_txs,
                                std::vector<int32_t> &pre_codes) {

  /* populate: one GPU lookup over every input's outpoint. The gather and the
   * blob rebuild fan over the host pool (per-tx prefix-summed offsets). */
  std::vector<size_t> in_base(n_txs + 1, 0);
  for (int t = 0; t < n_txs; t++)
    in_base[t + 1] = in_base[t] + txs[t].inputs.size();
  size_t n_in_total = in_base[n_txs];
  std::vector<uint8_t> &ops = ctx->ops_buf;
  ops.resize(n_in_total * 36);
  kvh_parallel_for((uint32_t)n_txs, [&](uint32_t t) {
    uint8_t *dst = ops.data() + in_base[t] * 36;
    for (auto &in : txs[t].inputs) {
      memcpy(dst, in.prev_tx_id, 32);
      memcpy(dst + 32, &in.prev_index, 4);
      dst += 36;
    }
  });
  std::vector<uint8_t> &entries = ctx->ent_buf;
  entries.resize(n_in_total * 64);
  std::vector<uint64_t> &found = ctx->found_buf;
  found.assign((n_in_total + 63) / 64, 0);
  const bool kv_timing = getenv("KV_TIMING") != nullptr;
  auto tnow = []() { return std::chrono::steady_clock::now(); };
  auto tms = [](std::chrono::steady_clock::time_point a,
                std::chrono::steady_clock::time_point b) {
    return std::chrono::duration<double, std::milli>(b - a).count();
  };
  auto t_a = tnow();
  std::vector<uint8_t> gathered; /* out-of-line spk bytes, entry order */
  if (n_in_total) {
    int rc = utxo_lookup_nolock(ctx, ops.data(), n_in_total, entries.data(),
                                found.data(), nullptr);
    if (rc) return rc;
    rc = arena_gather_nolock(
        ctx, n_in_total,
        [&](size_t i) -> uint8_t * {
          int hit = (found[i / 64] >> (i % 64)) & 1;
          return hit ? entries.data() + i * 64 : nullptr;
        },
        gathered);
    if (rc) return rc;
  }
  auto t_b = tnow();

  /* rebuild the blob with populated entries; pre-fail txs with missing inputs */
  std::vector<size_t> new_off(n_txs + 1, 0);
  kvh_parallel_for((uint32_t)n_txs, [&](uint32_t t) {
    const HTx &tx = txs[t];
    uint32_t tx_end = ((int)t + 1 < n_txs) ? txs[t + 1].off : (uint32_t)blob_len;
    size_t sz;
    if (tx.inputs.empty()) {
      sz = tx_end - tx.off;
    } else {
      sz = tx.inputs[0].rec_off - tx.off; /* header + payload */
      size_t ii = in_base[t];
      for (auto &in : tx.inputs) {
        int hit = (found[ii / 64] >> (ii % 64)) & 1;
        uint32_t spk_len = 0;
        uint16_t eflags = 0;
        if (hit) {
          memcpy(&spk_len, entries.data() + ii * 64 + 20, 4);
          memcpy(&eflags, entries.data() + ii * 64 + 16, 2);
        } else if (!pre_codes[t]) {
          pre_codes[t] = KV_ERR_MISSING_OUTPOINT;
        }
        sz += 52 + in.sig_script_len + 24 + spk_len +
              ((eflags & KV_UTXO_F_COVENANT) ? 32 : 0);
        ii++;
      }
      uint32_t outs_start = tx.outputs.empty() ? tx_end : tx.output_offs[0];
      sz += tx_end - outs_start;
    }
    new_off[t + 1] = sz; /* size for now; prefixed below */
  });
  size_t hdr_len = 4 + 4ull * n_txs;
  new_off[0] = hdr_len;
  for (int t = 0; t < n_txs; t++) new_off[t + 1] += new_off[t];
  std::vector<uint8_t> &pop = ctx->pop_buf;
  pop.resize(new_off[n_txs]);
  memcpy(pop.data(), blob, 4);
  kvh_parallel_for((uint32_t)n_txs, [&](uint32_t t) {
    const HTx &tx = txs[t];
    uint32_t off32 = (uint32_t)new_off[t];
    memcpy(pop.data() + 4 + 4ull * t, &off32, 4);
    uint8_t *dst = pop.data() + new_off[t];
    uint32_t tx_end = ((int)t + 1 < n_txs) ? txs[t + 1].off : (uint32_t)blob_len;
    if (tx.inputs.empty()) {
      memcpy(dst, blob + tx.off, tx_end - tx.off);
      return;
    }
    size_t hp = tx.inputs[0].rec_off - tx.off;
    memcpy(dst, blob + tx.off, hp);
    dst += hp;
    size_t ii = in_base[t];
    for (auto &in : tx.inputs) {
      size_t pre = 52 + in.sig_script_len;
      memcpy(dst, blob + in.rec_off, pre);
      dst += pre;
      int hit = (found[ii / 64] >> (ii % 64)) & 1;
      const uint8_t *e = entries.data() + ii * 64;
      uint64_t amount = 0, daa = 0;
      uint16_t eflags = 0, spkv = 0;
      uint32_t spk_len = 0;
      if (hit) {
        memcpy(&amount, e, 8);
        memcpy(&daa, e + 8, 8);
        memcpy(&eflags, e + 16, 2);
        memcpy(&spkv, e + 18, 2);
        memcpy(&spk_len, e + 20, 4);
      }
      memcpy(dst, &amount, 8);
      memcpy(dst + 8, &daa, 8);
      dst[16] = (uint8_t)(eflags & 1);
      dst[17] = (eflags & KV_UTXO_F_COVENANT) ? 1 : 0;
      memcpy(dst + 18, &spkv, 2);
      memcpy(dst + 20, &spk_len, 4);
      dst += 24;
      if (spk_len) {
        if (eflags & KV_UTXO_F_SPK_ARENA) {
          uint32_t go;
          memcpy(&go, e + 24, 4);
          memcpy(dst, gathered.data() + go, spk_len);
        } else {
          memcpy(dst, e + 24, spk_len);
        }
        dst += spk_len;
      }
      if (eflags & KV_UTXO_F_COVENANT) { /* utxo_covenant_id follows the script */
        memcpy(dst, e + 28, 32);
        dst += 32;
      }
      ii++;
    }
    uint32_t outs_start = tx.outputs.empty() ? tx_end : tx.output_offs[0];
    memcpy(dst, blob + outs_start, tx_end - outs_start);
  });

  if (kv_timing)
    fprintf(stderr, "[kv_timing] utxo populate: lookup %.2fms rebuild %.2fms\n",
            tms(t_a, t_b), tms(t_b, tnow()));
  return 0;
}

/* the diff of a validated block ⇔ utxo_diff.rs:224 add_transaction per accepted
 * tx: its inputs' outpoints to remove, its outputs to upsert (in the input
 * format of kv_utxo_upsert_spk) */
struct BlockDiff {
  std::vector<uint8_t> del_ops, add_ops, add_ents, add_spk;
};

static int build_block_diff(const vector<HTx> &txs, int n_txs, const int32_t *tx_codes,
                            uint64_t block_daa_score, BlockDiff &d) {
  for (int t = 0; t < n_txs; t++) {
    const HTx &tx = txs[t];
    if (tx_codes[t] != 0) continue;
    for (auto &in : tx.inputs) {
      uint8_t op[36];
      memcpy(op, in.prev_tx_id, 32);
      memcpy(op + 32, &in.prev_index, 4);
      d.del_ops.insert(d.del_ops.end(), op, op + 36);
    }
    for (uint32_t i = 0; i < tx.outputs.size(); i++) {
      const HOutput &o = tx.outputs[i];
      if (o.spk_len > KV_UTXO_MAX_SPK) {
        set_error("kv_validate_block_utxo: created spk exceeds KV_UTXO_MAX_SPK");
        return -4;
      }
      d.add_ops.insert(d.add_ops.end(), tx.tx_id, tx.tx_id + 32);
      const uint8_t *ix = (const uint8_t *)&i;
      d.add_ops.insert(d.add_ops.end(), ix, ix + 4);
      uint8_t e[64] = {0};
      memcpy(e, &o.value, 8);
      memcpy(e + 8, &block_daa_score, 8);
      /* flags: coinbase txs never enter this path → bit0 = 0 */
      memcpy(e + 18, &o.spk_version, 2);
      memcpy(e + 20, &o.spk_len, 4);
      if (o.has_covenant) { /* the id takes the inline field: script out of line */
        const uint16_t f = KV_UTXO_F_COVENANT;
        memcpy(e + 16, &f, 2);
        memcpy(e + 28, o.cov_id, 32);
      }
      if (o.spk_len <= 36 && !o.has_covenant)
        memcpy(e + 24, o.spk, o.spk_len);
      else /* out-of-line: bytes go to the arena via upsert_spk */
        d.add_spk.insert(d.add_spk.end(), o.spk, o.spk + o.spk_len);
      d.add_ents.insert(d.add_ents.end(), e, e + 64);
    }
  }
  return 0;
}

/* caller holds ctx->mu. undo_token_out != NULL: the diff is applied through
 * the journal (and apply_diff is taken as set). */
static int validate_block_utxo_nolock(kv_ctx *ctx, const uint8_t *blob, size_t blob_len,
                                      uint64_t pov_daa_score, uint64_t block_daa_score,
                                      uint32_t flags, int apply_diff,
                                      int32_t *tx_codes_out, uint64_t *fees_out,
                                      uint8_t *muhash_partial_out,
                                      uint64_t *undo_token_out) {
  if (!ctx->d_utxo.p) {
    set_error("kv_validate_block_utxo: call kv_utxo_reset first");
    return -1;
  }
  vector<HTx> txs;
  int n_txs = parse_blob_host(blob, blob_len, txs);
  if (n_txs < 0) {
    set_error("kv_validate_block_utxo: malformed blob");
    return -1;
  }
  std::vector<int32_t> pre_codes(n_txs, 0);
  int rc = populate_blob_nolock(ctx, blob, blob_len, txs, n_txs, pre_codes);
  if (rc) return rc;
  std::vector<uint8_t> &pop = ctx->pop_buf;
  rc = validate_block_impl(ctx, pop.data(), pop.size(), pov_daa_score,
                           block_daa_score, flags, tx_codes_out, fees_out,
                           muhash_partial_out, pre_codes.data());
  if (rc || (!apply_diff && !undo_token_out)) return rc;

  /* diff apply for accepted txs: remove spent, upsert created */
  BlockDiff d;
  rc = build_block_diff(txs, n_txs, tx_codes_out, block_daa_score, d);
  if (rc) return rc;
  if (undo_token_out)
    return journal_apply_nolock(ctx, d.del_ops.data(), d.del_ops.size() / 36,
                                d.add_ops.data(), d.add_ents.data(), d.add_spk.data(),
                                d.add_spk.size(), d.add_ops.size() / 36, nullptr,
                                undo_token_out);
  if (!d.del_ops.empty()) {
    rc = utxo_remove_nolock(ctx, d.del_ops.data(), d.del_ops.size() / 36);
    if (rc) return rc;
  }
  if (!d.add_ops.empty()) {
    rc = utxo_upsert_spk_nolock(ctx, d.add_ops.data(), d.add_ents.data(),
                                d.add_spk.data(), d.add_spk.size(),
                                d.add_ops.size() / 36);
    if (rc) return rc;
  }
  return 0;
}

extern "C" int kv_validate_block_utxo(kv_ctx *ctx, const uint8_t *blob,
                                      size_t blob_len, uint64_t pov_daa_score,
                                      uint64_t block_daa_score, uint32_t flags,
                                      int apply_diff, int32_t *tx_codes_out,
                                      uint64_t *fees_out,
                                      uint8_t *muhash_partial_out) {
  KV_ENTER(ctx);
  return validate_block_utxo_nolock(ctx, blob, blob_len, pov_daa_score, block_daa_score,
                                    flags, apply_diff, tx_codes_out, fees_out,
                                    muhash_partial_out, nullptr);
}

extern "C" int kv_validate_block_utxo_undo(kv_ctx *ctx, const uint8_t *blob,
                                           size_t blob_len, uint64_t pov_daa_score,
                                           uint64_t block_daa_score, uint32_t flags,
                                           int32_t *tx_codes_out, uint64_t *fees_out,
                                           uint8_t *muhash_partial_out,
                                           uint64_t *undo_token_out) {
  KV_ENTER(ctx);
  if (!undo_token_out) {
    set_error("kv_validate_block_utxo_undo: null undo_token_out");
    return -1;
  }
  return validate_block_utxo_nolock(ctx, blob, blob_len, pov_daa_score, block_daa_score,
                                    flags, 1, tx_codes_out, fees_out,
                                    muhash_partial_out, undo_token_out);
}

/* ---- direct mass-vector test exports (tests/golden/mass.json, extracted from
 * consensus/core/src/mass/mod.rs:531-953). These expose the engine's OWN mass
 * helpers (kv_validate_host.inc) so the CPU suite can pin them against the
 * reference's vectors without a GPU. ---- */

extern "C" uint64_t kv_test_plurality(uint32_t spk_len, int has_cov) {
  return kvh_plurality(spk_len, has_cov != 0);
}

extern "C" uint64_t kv_test_normalized_max(uint64_t storage_mass, uint64_t compute_mass,
                                           uint64_t transient_mass, uint64_t limit_storage,
                                           uint64_t limit_compute,
                                           uint64_t limit_transient) {
  return kvh_normalized_max_limits(storage_mass, compute_mass, transient_mass,
                                   limit_storage, limit_compute, limit_transient);
}

extern "C" int kv_test_storage_mass(uint32_t n_ins, const uint64_t *in_amounts,
                                    const uint32_t *in_spk_lens, const uint8_t *in_has_cov,
                                    uint32_t n_outs, const uint64_t *out_amounts,
                                    const uint32_t *out_spk_lens,
                                    const uint8_t *out_has_cov, uint64_t *mass_out) {
  HTx tx;
  tx.version = 1;
  for (uint32_t i = 0; i < n_ins; i++) {
    HInput in{};
    in.utxo_amount = in_amounts[i];
    in.utxo_spk_len = in_spk_lens ? in_spk_lens[i] : 0;
    in.utxo_has_cov = (in_has_cov && in_has_cov[i]) ? 1 : 0;
    tx.inputs.push_back(in);
  }
  for (uint32_t i = 0; i < n_outs; i++) {
    HOutput o{};
    o.value = out_amounts[i];
    o.spk_len = out_spk_lens ? out_spk_lens[i] : 0;
    o.has_covenant = (out_has_cov && out_has_cov[i]) ? 1 : 0;
    tx.outputs.push_back(o);
  }
  return kvh_storage_mass(tx, /*is_coinbase=*/false, mass_out);
}

/* ---- direct reduce-kernel test export (tests/test_gpu_u3072_wave.py): one
 * launch of the wave-cooperative U3072 reduce over caller-supplied operands,
 * with the launch shape every production site uses ((stride+3)/4 blocks of
 * 256). acc_in == NULL runs kv_u3072_reduce_wave_kernel; otherwise the
 * `stride` accumulators are uploaded and kv_u3072_reduce_wave_acc_kernel runs
 * with a host-known count. out receives the `stride` results. ---- */

extern "C" int kv_test_u3072_reduce(kv_ctx *ctx, const uint64_t *elements, uint32_t n,
                                    uint32_t stride, const uint64_t *acc_in,
                                    uint64_t *out, uint64_t *n_live_out) {
  if (!ctx || !out || stride == 0 || (n && !elements)) {
    set_error("kv_test_u3072_reduce: bad argument");
    return -1;
  }
  KV_ENTER(ctx);
  const size_t elem_bytes = KVU_LIMBS * sizeof(uint64_t);
  DeviceBuf d_elems, d_res, d_rec;
  kv::commit_out h_rec;
  if (d_elems.ensure((n ? n : 1) * elem_bytes) || d_res.ensure(stride * elem_bytes) ||
      d_rec.ensure(sizeof(kv::commit_out)))
    return -2;
  if (n)
    HIP_CHECK(hipMemcpyAsync(d_elems.p, elements, n * elem_bytes,
                             hipMemcpyHostToDevice, ctx->stream));
  if (acc_in) {
    HIP_CHECK(hipMemcpyAsync(d_res.p, acc_in, stride * elem_bytes,
                             hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(hipMemsetAsync(d_rec.p, 0, sizeof(kv::commit_out), ctx->stream));
    hipLaunchKernelGGL(kv_u3072_reduce_wave_acc_kernel, dim3((stride + 3) / 4),
                       dim3(256), 0, ctx->stream, d_elems.as<const uint64_t>(),
                       (const uint32_t *)nullptr, n, stride, d_res.as<uint64_t>(),
                       d_rec.as<kv::commit_out>());
  } else {
    hipLaunchKernelGGL(kv_u3072_reduce_wave_kernel, dim3((stride + 3) / 4), dim3(256),
                       0, ctx->stream, d_elems.as<const uint64_t>(), n, stride,
                       d_res.as<uint64_t>());
  }
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  HIP_CHECK(hipMemcpy(out, d_res.p, stride * elem_bytes, hipMemcpyDeviceToHost));
  if (n_live_out) {
    *n_live_out = 0;
    if (acc_in) {
      HIP_CHECK(hipMemcpy(&h_rec, d_rec.p, sizeof(h_rec), hipMemcpyDeviceToHost));
      *n_live_out = h_rec.n_live;
    }
  }
  return 0;
}
