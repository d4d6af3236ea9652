/* kv_validate_host.inc — included by kv_engine.cpp (single TU).
 *
 * Host orchestration of kv_validate_block: blob parsing, template
 * classification (the "script micro-interpreter / template dispatcher" of
 * SURVEY.md §2 item 8 — host flattens standard script classes into (msg,pk,sig)
 * work items; the GPU does every hash and EC verify), the runtime resource
 * meter (⇔ crypto/txscript/src/runtime_resource_meter.rs), the multisig
 * greedy-matching loop (⇔ crypto/txscript/src/lib.rs:759-843), and the muhash
 * reduction pipeline (⇔ utxo_validation.rs:319-348).
 *
 * Round-1 template coverage (anything else → KV_SCRIPT_UNSUPPORTED_OPCODE,
 * documented in DESIGN.md):
 *   - P2PK schnorr  : spk = 0x20‖pk32‖0xac, sig_script = 0x41‖sig64‖type
 *   - P2PK ECDSA    : spk = 0x21‖pk33‖0xab, sig_script = 0x42‖sig64‖type
 *   - P2SH multisig : spk = 0xaa‖0x20‖h32‖0x87; sig_script = sig pushes +
 *                     redeem push; redeem = OP_m (0x20‖pk32)×n OP_n 0xae
 */

#include <algorithm>
#include <cmath>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace kvhost {

using std::vector;

/* ---- meter constants (consensus/core/src/mass/units.rs) ---- */
#define KVH_UNITS_PER_GRAM 100ULL
#define KVH_UNITS_PER_SIGOP_COUNT (1000ULL * 100ULL)
#define KVH_UNITS_PER_BUDGET (100ULL * 100ULL)
#define KVH_FREE_UNITS (KVH_UNITS_PER_BUDGET - 1)
#define KVH_MAX_SOMPI (29000000000ULL * 100000000ULL)
#define KVH_SEQ_DISABLED (1ULL << 63)
#define KVH_SEQ_MASK 0x00000000ffffffffULL

struct HInput {
  uint32_t rec_off;
  const uint8_t *prev_tx_id;
  uint32_t prev_index;
  uint64_t sequence;
  uint8_t commit_kind;
  uint16_t commit_value;
  const uint8_t *sig_script;
  uint32_t sig_script_len;
  uint32_t sig_script_off;
  uint64_t utxo_amount;
  uint64_t utxo_daa_score;
  uint8_t utxo_is_coinbase;
  uint8_t utxo_has_cov;
  uint16_t utxo_spk_version;
  const uint8_t *utxo_spk;
  uint32_t utxo_spk_len;
  uint32_t utxo_spk_off;
  const uint8_t *utxo_cov_id; /* 32B, valid when utxo_has_cov */
};

struct HOutput {
  uint64_t value;
  uint16_t spk_version;
  const uint8_t *spk;
  uint32_t spk_len;
  uint8_t has_covenant;
  uint16_t cov_auth_input;
  const uint8_t *cov_id; /* 32B, valid when has_covenant */
};

struct HTx {
  uint32_t off;
  uint16_t version;
  uint64_t storage_mass;
  uint64_t lock_time;
  const uint8_t *subnetwork_id;
  uint64_t gas;
  uint32_t payload_len;
  const uint8_t *tx_id;
  const uint8_t *payload;
  vector<HInput> inputs;
  vector<HOutput> outputs;
  vector<uint32_t> output_offs;
};

static bool h_is_coinbase(const HTx &tx) {
  if (tx.subnetwork_id[0] != 1) return false;
  for (int i = 1; i < 20; i++)
    if (tx.subnetwork_id[i]) return false;
  return true;
}

/* Persistent host worker pool (the reference fans the same work across a
 * rayon pool, utxo_validation.rs:319). Spawn-per-call was measured to cost
 * more than it saved at block-batch sizes, so workers live for the process
 * and park on a condition variable between calls. Deterministic chunking so
 * job order after per-chunk concatenation equals the serial order. */
struct KvhPool {
  std::mutex run_mu; /* serializes concurrent run() callers */
  std::mutex m;
  std::condition_variable cv_work, cv_done;
  std::vector<std::thread> workers;
  std::function<void(unsigned)> task;
  uint64_t gen = 0;
  unsigned n_active = 0;
  unsigned T;
  bool stop = false;

  static KvhPool &inst() {
    static KvhPool p;
    return p;
  }

  KvhPool() {
    unsigned hc = std::thread::hardware_concurrency();
    T = hc > 32 ? 32 : (hc < 1 ? 1 : hc);
    for (unsigned k = 1; k < T; k++)
      workers.emplace_back([this, k]() { loop(k); });
  }

  ~KvhPool() {
    {
      std::lock_guard<std::mutex> l(m);
      stop = true;
    }
    cv_work.notify_all();
    for (auto &w : workers) w.join();
  }

  void loop(unsigned k) {
    uint64_t seen = 0;
    for (;;) {
      std::function<void(unsigned)> f;
      {
        std::unique_lock<std::mutex> l(m);
        cv_work.wait(l, [&] { return stop || gen != seen; });
        if (stop) return;
        seen = gen;
        f = task;
      }
      f(k);
      {
        std::lock_guard<std::mutex> l(m);
        if (--n_active == 0) cv_done.notify_all();
      }
    }
  }

  /* f(k) runs once per worker index 0..T-1; caller participates as worker 0 */
  template <class F>
  void run(F &&f) {
    if (T == 1) {
      f(0);
      return;
    }
    std::lock_guard<std::mutex> rl(run_mu);
    {
      std::lock_guard<std::mutex> l(m);
      task = f;
      n_active = T - 1;
      gen++;
    }
    cv_work.notify_all();
    f(0);
    std::unique_lock<std::mutex> l(m);
    cv_done.wait(l, [&] { return n_active == 0; });
  }
};

static inline unsigned kvh_threads(uint32_t n) {
  return n < 256 ? 1 : KvhPool::inst().T;
}

template <class F>
static void kvh_parallel_for(uint32_t n, F f) {
  unsigned T = kvh_threads(n);
  if (T == 1) {
    for (uint32_t i = 0; i < n; i++) f(i);
    return;
  }
  uint32_t chunk = (n + T - 1) / T;
  KvhPool::inst().run([&](unsigned k) {
    uint32_t lo = k * chunk, hi = std::min(n, lo + chunk);
    for (uint32_t i = lo; i < hi; i++) f(i);
  });
}

static bool parse_one_tx(const uint8_t *blob, size_t blob_len, uint32_t off,
                         HTx &tx) {
  const uint8_t *end = blob + blob_len;
  if (off + 88 > blob_len) return false;
  {
    const uint8_t *p = blob + off;
    tx.off = off;
    uint16_t n_in, n_out;
    memcpy(&tx.version, p, 2);
    memcpy(&n_in, p + 2, 2);
    memcpy(&n_out, p + 4, 2);
    memcpy(&tx.lock_time, p + 8, 8);
    tx.subnetwork_id = p + 16;
    memcpy(&tx.payload_len, p + 36, 4);
    memcpy(&tx.gas, p + 40, 8);
    memcpy(&tx.storage_mass, p + 48, 8);
    tx.tx_id = p + 56;
    p += 88;
    tx.payload = p;
    if (p + tx.payload_len > end) return false;
    p += tx.payload_len;
    tx.inputs.resize(n_in);
    for (uint32_t i = 0; i < n_in; i++) {
      HInput &in = tx.inputs[i];
      if (p + 52 > end) return false;
      in.rec_off = (uint32_t)(p - blob);
      in.prev_tx_id = p;
      memcpy(&in.prev_index, p + 32, 4);
      memcpy(&in.sequence, p + 36, 8);
      in.commit_kind = p[44];
      memcpy(&in.commit_value, p + 46, 2);
      memcpy(&in.sig_script_len, p + 48, 4);
      in.sig_script = p + 52;
      in.sig_script_off = (uint32_t)(p + 52 - blob);
      p += 52;
      if (p + in.sig_script_len + 24 > end) return false;
      p += in.sig_script_len;
      memcpy(&in.utxo_amount, p, 8);
      memcpy(&in.utxo_daa_score, p + 8, 8);
      in.utxo_is_coinbase = p[16];
      in.utxo_has_cov = p[17];
      memcpy(&in.utxo_spk_version, p + 18, 2);
      memcpy(&in.utxo_spk_len, p + 20, 4);
      in.utxo_spk = p + 24;
      in.utxo_spk_off = (uint32_t)(p + 24 - blob);
      in.utxo_cov_id = in.utxo_spk + in.utxo_spk_len;
      p += 24 + in.utxo_spk_len + (in.utxo_has_cov ? 32 : 0);
      if (p > end) return false;
    }
    tx.outputs.resize(n_out);
    tx.output_offs.resize(n_out);
    for (uint32_t i = 0; i < n_out; i++) {
      HOutput &o = tx.outputs[i];
      if (p + 16 > end) return false;
      tx.output_offs[i] = (uint32_t)(p - blob);
      memcpy(&o.value, p, 8);
      memcpy(&o.spk_version, p + 8, 2);
      memcpy(&o.spk_len, p + 12, 4);
      o.spk = p + 16;
      p += 16 + o.spk_len;
      if (p + 1 > end) return false;
      o.has_covenant = *p++;
      o.cov_auth_input = 0;
      o.cov_id = nullptr;
      if (o.has_covenant) {
        if (p + 34 > end) return false;
        memcpy(&o.cov_auth_input, p, 2);
        o.cov_id = p + 2;
        p += 34;
      }
    }
  }
  return true;
}

static int parse_blob_host(const uint8_t *blob, size_t blob_len, vector<HTx> &txs) {
  if (blob_len < 4) return -1;
  uint32_t n_txs;
  memcpy(&n_txs, blob, 4);
  if (blob_len < 4 + 4ull * n_txs) return -1;
  txs.resize(n_txs);
  std::atomic<int> bad{0};
  kvh_parallel_for(n_txs, [&](uint32_t t) {
    uint32_t off;
    memcpy(&off, blob + 4 + 4ull * t, 4);
    if (!parse_one_tx(blob, blob_len, off, txs[t]))
      bad.store(1, std::memory_order_relaxed);
  });
  return bad.load() ? -1 : (int)n_txs;
}


/* host keyed blake2b-256 (RFC 7693) — product host code */
static const uint64_t H_IV[8] = {0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL,
                                 0x3c6ef372fe94f82bULL, 0xa54ff53a5f1d36f1ULL,
                                 0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL,
                                 0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL};
static const uint8_t H_SIG[12][16] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15},
    {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
    {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4},
    {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
    {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13},
    {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
    {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11},
    {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
    {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5},
    {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0},
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15},
    {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3}};

static inline uint64_t rot64(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }

static void h_b2b_compress(uint64_t h[8], const uint8_t blk[128], uint64_t t, int last) {
  uint64_t v[16], m[16];
  for (int i = 0; i < 16; i++) memcpy(&m[i], blk + 8 * i, 8);
  for (int i = 0; i < 8; i++) v[i] = h[i];
  for (int i = 0; i < 8; i++) v[i + 8] = H_IV[i];
  v[12] ^= t;
  if (last) v[14] = ~v[14];
#define HG(a, b, c, d, x, y)                                                   \
  v[a] += v[b] + (x); v[d] = rot64(v[d] ^ v[a], 32); v[c] += v[d];             \
  v[b] = rot64(v[b] ^ v[c], 24); v[a] += v[b] + (y);                           \
  v[d] = rot64(v[d] ^ v[a], 16); v[c] += v[d]; v[b] = rot64(v[b] ^ v[c], 63);
  for (int r = 0; r < 12; r++) {
    const uint8_t *s = H_SIG[r];
    HG(0, 4, 8, 12, m[s[0]], m[s[1]]); HG(1, 5, 9, 13, m[s[2]], m[s[3]]);
    HG(2, 6, 10, 14, m[s[4]], m[s[5]]); HG(3, 7, 11, 15, m[s[6]], m[s[7]]);
    HG(0, 5, 10, 15, m[s[8]], m[s[9]]); HG(1, 6, 11, 12, m[s[10]], m[s[11]]);
    HG(2, 7, 8, 13, m[s[12]], m[s[13]]); HG(3, 4, 9, 14, m[s[14]], m[s[15]]);
  }
#undef HG
  for (int i = 0; i < 8; i++) h[i] ^= v[i] ^ v[i + 8];
}

static void h_blake2b_keyed(const uint8_t *key, size_t keylen, const uint8_t *data,
                            size_t len, uint8_t out[32]) {
  uint64_t h[8];
  for (int i = 0; i < 8; i++) h[i] = H_IV[i];
  h[0] ^= 32ULL | ((uint64_t)keylen << 8) | (1ULL << 16) | (1ULL << 24);
  uint8_t blk[128];
  uint64_t t = 0;
  if (keylen) {
    memset(blk, 0, 128);
    memcpy(blk, key, keylen);
    if (len == 0) {
      h_b2b_compress(h, blk, 128, 1);
      goto fin;
    }
    t = 128;
    h_b2b_compress(h, blk, 128, 0);
  }
  while (len > 128) {
    t += 128;
    h_b2b_compress(h, data, t, 0);
    data += 128;
    len -= 128;
  }
  memset(blk, 0, 128);
  memcpy(blk, data, len);
  t += len;
  h_b2b_compress(h, blk, t, 1);
fin:
  for (int i = 0; i < 32; i++) out[i] = (uint8_t)(h[i / 8] >> (8 * (i % 8)));
}


/* ---- covenant bindings ⇔ CovenantsContext::from_tx
 * (crypto/txscript/src/covenants.rs:101-163), called from
 * check_covenant_info (tx_validation_in_utxo_context.rs:58,176).
 *
 * An output with a binding is a CONTINUATION when its authorizing input's
 * entry carries the same covenant id; only those reach the script engine's
 * contexts (input_ctxs / shared_ctxs). Every other bound output is a GENESIS
 * output of the group (authorizing_input, covenant_id), and the group's id
 * must equal consensus/core/src/hashing/covenant_id.rs over the authorizing
 * input's outpoint and the group's outputs in ascending index. */
static bool h_cov_is_continuation(const HTx &tx, const HOutput &o) {
  if (!o.has_covenant || o.cov_auth_input >= tx.inputs.size()) return false;
  const HInput &in = tx.inputs[o.cov_auth_input];
  return in.utxo_has_cov && !memcmp(in.utxo_cov_id, o.cov_id, 32);
}

static const uint8_t H_KEY_COVENANT_ID[10] = {'C', 'o', 'v', 'e', 'n',
                                              'a', 'n', 't', 'I', 'D'};

static void h_put_le(vector<uint8_t> &v, uint64_t x, int bytes) {
  for (int i = 0; i < bytes; i++) v.push_back((uint8_t)(x >> (8 * i)));
}

/* 0, KV_ERR_COVENANT_AUTH_INPUT or KV_ERR_COVENANT_GENESIS_ID. The reference
 * walks its genesis groups in HashMap order, so which of two failures it
 * reports is unspecified there; here an out-of-bounds authorizing input wins
 * (the reference returns it from the first loop, before any hashing). Every
 * failing group gives the same code, so the order the groups are hashed in
 * (by authorizing input, then id) cannot show. Sorting keeps a transaction of
 * many one-output groups at n log n. */
static int kvh_check_covenant_info(const HTx &tx) {
  vector<uint32_t> gen; /* genesis outputs */
  for (uint32_t i = 0; i < tx.outputs.size(); i++) {
    const HOutput &o = tx.outputs[i];
    if (!o.has_covenant) continue;
    if (o.cov_auth_input >= tx.inputs.size()) return KV_ERR_COVENANT_AUTH_INPUT;
    if (!h_cov_is_continuation(tx, o)) gen.push_back(i);
  }
  if (gen.empty()) return 0;
  auto group_cmp = [&](uint32_t a, uint32_t b) {
    const HOutput &x = tx.outputs[a], &y = tx.outputs[b];
    if (x.cov_auth_input != y.cov_auth_input)
      return x.cov_auth_input < y.cov_auth_input ? -1 : 1;
    return memcmp(x.cov_id, y.cov_id, 32);
  };
  /* ties keep ascending output index: the order the id hashes a group in */
  std::sort(gen.begin(), gen.end(), [&](uint32_t a, uint32_t b) {
    int c = group_cmp(a, b);
    return c ? c < 0 : a < b;
  });
  vector<uint8_t> buf;
  for (size_t lo = 0, hi; lo < gen.size(); lo = hi) {
    for (hi = lo + 1; hi < gen.size() && group_cmp(gen[lo], gen[hi]) == 0;) hi++;
    const HOutput &first = tx.outputs[gen[lo]];
    const HInput &in = tx.inputs[first.cov_auth_input];
    buf.clear();
    buf.insert(buf.end(), in.prev_tx_id, in.prev_tx_id + 32);
    h_put_le(buf, in.prev_index, 4);
    h_put_le(buf, hi - lo, 8);
    for (size_t k = lo; k < hi; k++) {
      const HOutput &o = tx.outputs[gen[k]];
      h_put_le(buf, gen[k], 4);
      h_put_le(buf, o.value, 8);
      h_put_le(buf, o.spk_version, 2);
      h_put_le(buf, o.spk_len, 8);
      buf.insert(buf.end(), o.spk, o.spk + o.spk_len);
    }
    uint8_t id[32];
    h_blake2b_keyed(H_KEY_COVENANT_ID, sizeof H_KEY_COVENANT_ID, buf.data(), buf.size(),
                    id);
    if (memcmp(id, first.cov_id, 32)) return KV_ERR_COVENANT_GENESIS_ID;
  }
  return 0;
}


/* ---- mempool feerate mass (validate_mempool_transaction_in_utxo_context,
 * utxo_validation.rs:418-457). Product-side restatement of
 * transaction_estimated_serialized_size + calc_non_contextual_masses
 * (mass/mod.rs:21-78,336-368) and normalized_max over the mainnet cofactors
 * (limits {compute 500k, storage 500k, transient 1M} → storage 1.0,
 * transient 0.5; params.rs:623-626). */
static uint64_t kvh_estimated_size(const HTx &tx) {
  uint64_t size = 2 + 8 + 8 + 8 + 20 + 8 + 32 + 8 + tx.payload_len;
  for (const auto &in : tx.inputs) {
    size += 32 + 4 + 8 + in.sig_script_len + 8;
    if (tx.version >= 1) size += 2;
  }
  for (const auto &o : tx.outputs) {
    size += 8 + 2 + 8 + o.spk_len;
    if (o.has_covenant) size += 2 + 32;
  }
  return size;
}

/* Generic normalized_max over per-dimension limits ⇔ Mass::normalized_max +
 * MassCofactors::new (mass/mod.rs:258-265,298-308): cofactor_i = Lc/L_i (f64),
 * normalized = ceil(m_i · cofactor_i), result = max over dimensions. */
static uint64_t kvh_normalized_max_limits(uint64_t storage_mass, uint64_t compute_mass,
                                          uint64_t transient_mass,
                                          uint64_t limit_storage, uint64_t limit_compute,
                                          uint64_t limit_transient) {
  double cs = (double)limit_compute / (double)limit_storage;
  double ct = (double)limit_compute / (double)limit_transient;
  uint64_t sn = (uint64_t)ceil((double)storage_mass * cs);
  uint64_t tn = (uint64_t)ceil((double)transient_mass * ct);
  uint64_t m = sn;
  if (compute_mass > m) m = compute_mass;
  if (tn > m) m = tn;
  return m;
}

static uint64_t kvh_normalized_mass(const HTx &tx, uint64_t storage_mass) {
  if (h_is_coinbase(tx)) return storage_mass;
  uint64_t size = kvh_estimated_size(tx);
  uint64_t spk_bytes = 0;
  for (const auto &o : tx.outputs) spk_bytes += 2 + o.spk_len;
  uint64_t script_mass = 0;
  for (const auto &in : tx.inputs) {
    if (tx.version >= 1)
      script_mass += 100ull * (in.commit_kind == 1 ? in.commit_value : 0);
    else
      script_mass += 1000ull * (in.commit_kind == 0 ? in.commit_value : 0);
  }
  uint64_t compute = size * 1 + spk_bytes * 10 + script_mass;
  /* mainnet limits {storage 500k, compute 500k, transient 1M}, params.rs:626 */
  return kvh_normalized_max_limits(storage_mass, compute, size * 4, 500000, 500000,
                                   1000000);
}

/* ---- storage mass (KIP-0009) ⇔ consensus/core/src/mass/mod.rs:385-514 ----
 * Product-side implementation (independent of the oracle's). */
#define KVH_STORM_PARAM (100000000ULL * 10000ULL)

static uint64_t kvh_plurality(uint32_t spk_len, bool has_cov) {
  uint64_t sz = 63ull + spk_len + (has_cov ? 32 : 0);
  return (sz + 99) / 100;
}

/* 0 ok, -1 incomputable */
static int kvh_storage_mass(const HTx &tx, bool is_coinbase, uint64_t *out) {
  if (is_coinbase) {
    *out = 0;
    return 0;
  }
  uint64_t outs_p = 0, harm_outs = 0;
  for (const auto &o : tx.outputs) {
    uint64_t p = kvh_plurality(o.spk_len, o.has_covenant != 0);
    if (o.value == 0) return -1;
    uint64_t cp, cpp, h;
    if (__builtin_mul_overflow(KVH_STORM_PARAM, p, &cp)) return -1;
    if (__builtin_mul_overflow(cp, p, &cpp)) return -1;
    if (__builtin_add_overflow(harm_outs, cpp / o.value, &h)) return -1;
    harm_outs = h;
    outs_p += p;
  }
  bool relaxed;
  if (outs_p == 1) {
    relaxed = true;
  } else if (tx.inputs.size() > 2) {
    relaxed = false;
  } else {
    uint64_t ins_p = 0;
    for (const auto &in : tx.inputs)
      ins_p += kvh_plurality(in.utxo_spk_len, in.utxo_has_cov != 0);
    relaxed = ins_p == 1 || (outs_p == 2 && ins_p == 2);
  }
  if (relaxed) {
    uint64_t harm_ins = 0;
    for (const auto &in : tx.inputs) {
      uint64_t p = kvh_plurality(in.utxo_spk_len, in.utxo_has_cov != 0);
      if (in.utxo_amount == 0) return -1;
      uint64_t c = KVH_STORM_PARAM * p * p / in.utxo_amount;
      uint64_t s = harm_ins + c;
      harm_ins = s < harm_ins ? UINT64_MAX : s;
    }
    *out = harm_outs > harm_ins ? harm_outs - harm_ins : 0;
    return 0;
  }
  uint64_t ins_p = 0, sum_ins = 0;
  for (const auto &in : tx.inputs) {
    ins_p += kvh_plurality(in.utxo_spk_len, in.utxo_has_cov != 0);
    sum_ins += in.utxo_amount;
  }
  uint64_t mean = sum_ins / ins_p;
  if (mean == 0) mean = 1;
  uint64_t arith;
  if (__builtin_mul_overflow(ins_p, KVH_STORM_PARAM / mean, &arith)) arith = UINT64_MAX;
  *out = harm_outs > arith ? harm_outs - arith : 0;
  return 0;
}

static bool valid_sighash_type(uint8_t t) {
  return t == 0x01 || t == 0x02 || t == 0x04 || t == 0x81 || t == 0x82 || t == 0x84;
}

/* ---- per-input plan ---- */
enum PlanKind : uint8_t {
  PLAN_NONE = 0,     /* no jobs (unknown spk version accepted, or pre-error) */
  PLAN_P2PK,
  PLAN_MULTISIG,
  PLAN_INTERP,       /* general interpreter, suspended at a signature site */
};

struct MsigSig {
  uint32_t off;   /* byte offset of push data in blob */
  uint32_t len;   /* push data length (0 = empty sig) */
  uint8_t type;   /* last byte when len >= 1 */
  int32_t job0;   /* first pair-job index (this sig × key 0), -1 if no jobs */
};

/* one EC verify request collected at a signature site */
struct KvSigReq {
  uint8_t ecdsa;     /* 0 = schnorr (BIP-340), 1 = ECDSA */
  uint8_t literal;   /* 1 = msg[] is the literal 32B digest (OpCheckSigFromStack);
                        0 = msg is sighash(hash_type) of this (tx, input) */
  uint8_t hash_type; /* when literal == 0 */
  uint8_t _pad;
  uint8_t sig[64];   /* zeroed when the popped sig length was invalid (the
                        status is then only consulted for the pubkey) */
  uint8_t pk[33];    /* x-only 32B (schnorr, pk[32]=0) or compressed 33B */
  uint8_t msg[32];   /* literal digest when literal == 1 */
};

/* per-run context threading the memo/pending protocol + the KIP-21 accessor */
struct KvsRunCtx {
  const std::vector<std::vector<uint8_t>> *memo = nullptr; /* resolved sites */
  std::vector<KvSigReq> *pending = nullptr; /* filled at suspension */
  int (*seqc_fn)(void *, const uint8_t *, uint8_t *) = nullptr;
  void *seqc_user = nullptr;
};

struct InputPlan {
  PlanKind kind = PLAN_NONE;
  int pre_code = 0;      /* nonzero: decided without GPU (full KV code) */
  bool ecdsa = false;
  int32_t job = -1;      /* P2PK: job index in its (schnorr|ecdsa) array */
  uint64_t limit_units = 0;
  uint64_t spent_units = 0; /* units consumed before any sigop */
  /* multisig */
  int msig_m = 0, msig_n = 0;
  vector<MsigSig> msig_sigs;
  vector<uint32_t> key_offs; /* blob offsets of the n keys */
  bool extra_stack = false;  /* unexpected leftover stack entries → CleanStack */
  /* general interpreter (collect/replay rounds over the GPU verify batch) */
  std::vector<std::vector<uint8_t>> memo; /* resolved sig-site statuses */
  std::vector<KvSigReq> pending;          /* the suspended site's requests */
};

static uint64_t committed_limit(const HInput &in) {
  uint64_t units = in.commit_kind == 0
                       ? (uint64_t)in.commit_value * KVH_UNITS_PER_SIGOP_COUNT
                       : (uint64_t)in.commit_value * KVH_UNITS_PER_BUDGET;
  uint64_t lim = units + KVH_FREE_UNITS;
  if (lim < units) lim = UINT64_MAX;
  return lim;
}

/* parse a push-only script into (off,len) pairs; returns false if any opcode is
 * not a plain data push 0x00..0x4e (keeps round-1 templates canonical) */
static bool parse_pushes(const uint8_t *blob, const uint8_t *s, uint32_t len,
                         uint32_t base_off, vector<std::pair<uint32_t, uint32_t>> &out) {
  uint32_t pc = 0;
  while (pc < len) {
    uint8_t op = s[pc++];
    uint32_t dlen, doff;
    if (op == 0x00) {
      dlen = 0;
      doff = base_off + pc;
    } else if (op >= 0x01 && op <= 0x4b) {
      dlen = op;
      doff = base_off + pc;
      if (pc + dlen > len) return false;
      pc += dlen;
    } else if (op >= 0x4c && op <= 0x4e) {
      uint32_t szlen = op == 0x4c ? 1 : (op == 0x4d ? 2 : 4);
      if (pc + szlen > len) return false;
      dlen = 0;
      for (uint32_t i = 0; i < szlen; i++) dlen |= (uint32_t)s[pc + i] << (8 * i);
      pc += szlen;
      doff = base_off + pc;
      if (pc + dlen > len) return false;
      pc += dlen;
    } else {
      return false;
    }
    out.push_back({doff, dlen});
  }
  return true;
}

} // namespace kvhost
