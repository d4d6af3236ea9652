/* kv_script_host.inc — PRODUCT host-side general script interpreter.
 *
 * Executes the full TxScriptEngine opcode set (crypto/txscript/src/lib.rs +
 * opcodes/mod.rs) for scripts OUTSIDE the GPU template classes. The
 * signature-check family (OpCheckSig / OpCheckSigECDSA / OpCheckMultiSig* /
 * OpCheckSigVerify / OpCheckSigFromStack*) executes through a collect/replay
 * protocol so the GPU keeps every EC verification while control flow stays
 * exact:
 *
 *   - Execution is deterministic given the verdicts of earlier signature
 *     sites. Each executed sig-site gets an index in execution order.
 *   - When execution reaches site k and the caller-provided memo holds only
 *     k entries, the site's verify requests (one for a single checksig, all
 *     collected (sig,key) pairs for a multisig) are appended to `pending` and
 *     the run returns KVH_SCRIPT_SUSPEND.
 *   - The driver resolves the requests (GPU kernels in the engine; the
 *     host-compiled product verify functions in the CPU test shim), appends
 *     the status vector as memo entry k, and re-runs from scratch. Replay is
 *     cheap (scripts are <=10KB, metered) and converges in max-site-depth
 *     rounds, so a whole block of such scripts costs one GPU batch per depth
 *     level, not per signature.
 *   - Statuses use the engine's verify status bytes: 0 valid / 1 invalid /
 *     2 pubkey-parse-error / 3 sig-parse-error; host-side length checks are
 *     applied in the reference's own order (cost, pubkey, signature) during
 *     replay, so error-variant parity holds (lib.rs:846-905).
 *
 * Only OpZkPrecompile still returns KVH_SCRIPT_DEFER (routed to the CPU
 * reference via KV_TX_DEFER_TO_CPU). OpChainblockSeqCommit resolves through
 * the kv_seq_commit_accessor_fn callback (NULL → InvalidOpcode, matching a
 * None accessor). Blake3 ops run right here.
 *
 * Independent product implementation: written against the same reference
 * sources the oracle restates (lib.rs:617-905 engine loop + sig checks,
 * opcodes/mod.rs semantics, runtime_resource_meter.rs metering,
 * data_stack.rs numbers), with a different structure (C++ value stacks).
 * Parity is established by the canonical script-vector suite and an
 * oracle-differential fuzzer in tests/test_host_interpreter.py — never by
 * linking the oracle.
 */

#include <string>
#include <vector>

namespace kvhost {

enum : int {
  KVH_SCRIPT_DEFER = -100,  /* zk precompile: engine does not decide */
  KVH_SCRIPT_SUSPEND = -101 /* sig site needs verdicts: resolve pending, re-run */
};


/* limits (crypto/txscript/src/lib.rs:74-80, runtime_resource_meter.rs) */
#define KVS_MAX_STACK 244 /* lib.rs:76 */
#define KVS_MAX_OPS 1000000
#define KVS_MAX_SCRIPTS_SIZE 1000000u
#define KVS_MAX_ELEMENT 1000000u
#define KVS_UNITS_PER_SIGOP_COUNT 100000ull /* 1000 grams * 100 */
#define KVS_UNITS_PER_BUDGET 10000ull
#define KVS_FREE_UNITS 9999ull

typedef std::vector<uint8_t> KEnt;

struct KScript {
  std::vector<KEnt> d, a; /* data / alt stacks */
  const HTx *tx;
  const HInput *input;
  uint32_t idx;
  uint64_t sigop_units;
  uint64_t remaining;
  int32_t num_ops = 0;
  const KvsRunCtx *rctx = nullptr; /* memo/pending protocol + accessors */
  uint32_t site = 0;               /* next signature-site index this run */
  std::vector<uint8_t> cond; /* 1 = executing, 0 = skipping */

  uint64_t op_pushed = 0; /* metered bytes of the CURRENT op; charged by the
                             executor after the op succeeds (reference order:
                             the op's own error wins over metering) */
  int consume(uint64_t units) {
    if (units > remaining) return KV_SCRIPT_EXCEEDED_SCRIPT_UNITS;
    remaining -= units;
    return 0;
  }
  int push(KEnt v, bool metered = true) {
    if (v.size() > KVS_MAX_ELEMENT) return KV_SCRIPT_ELEMENT_TOO_BIG;
    if (metered) op_pushed += v.size();
    if (d.size() >= KVS_MAX_STACK) return KV_SCRIPT_STACK_SIZE_EXCEEDED;
    d.push_back(std::move(v));
    return 0;
  }
  int push_alt(KEnt v) { /* alt-stack moves are unmetered */
    if (a.size() >= KVS_MAX_STACK) return KV_SCRIPT_STACK_SIZE_EXCEEDED;
    a.push_back(std::move(v));
    return 0;
  }
  bool exec_active() const {
    for (uint8_t c : cond)
      if (!c) return false;
    return true;
  }
};

static KEnt kvs_num(int64_t v) {
  KEnt out;
  if (v == 0) return out;
  bool neg = v < 0;
  uint64_t mag = neg ? (uint64_t)(-(v + 1)) + 1 : (uint64_t)v;
  while (mag) {
    out.push_back((uint8_t)(mag & 0xff));
    mag >>= 8;
  }
  if (out.back() & 0x80)
    out.push_back(neg ? 0x80 : 0);
  else if (neg)
    out.back() |= 0x80;
  return out;
}

/* deserialize_i64 (data_stack.rs:164-178): <=8 bytes, sign-magnitude LE */
static int kvs_to_num(const KEnt &e, int64_t *out) {
  if (e.size() > 8) return KV_SCRIPT_NUMBER_TOO_BIG; /* SizedEncodeInt<8> */
  if (e.empty()) {
    *out = 0;
    return 0;
  }
  uint8_t msb = e.back();
  int64_t sign = (msb & 0x80) ? -1 : 1;
  uint64_t acc = msb & 0x7f;
  for (size_t i = e.size() - 1; i-- > 0;) acc = (acc << 8) | e[i];
  *out = sign * (int64_t)acc;
  return 0;
}

static bool kvs_bool(const KEnt &e) {
  if (e.empty()) return false;
  if (e.back() & 0x7f) return true;
  for (size_t i = 0; i + 1 < e.size(); i++)
    if (e[i]) return true;
  return false;
}

static int kvs_pop(KScript &S, KEnt *out) {
  if (S.d.empty()) return KV_SCRIPT_INVALID_STACK_OPERATION;
  *out = std::move(S.d.back());
  S.d.pop_back();
  return 0;
}

static int kvs_pop_num(KScript &S, int64_t *out) {
  KEnt e;
  int rc = kvs_pop(S, &e);
  if (rc) return rc;
  return kvs_to_num(e, out);
}

static int kvs_pop_i32(KScript &S, int32_t *out) {
  int64_t v;
  int rc = kvs_pop_num(S, &v);
  if (rc) return rc;
  if (v > INT32_MAX || v < INT32_MIN) return KV_SCRIPT_NUMBER_TOO_BIG;
  *out = (int32_t)v;
  return 0;
}

static int kvs_push_num(KScript &S, int64_t v, bool metered = true) {
  if (v == INT64_MIN) return KV_SCRIPT_NUMBER_TOO_BIG; /* 9-byte serialize */
  return S.push(kvs_num(v), metered);
}

/* substring() (opcodes/mod.rs:196-203) */
static int kvs_substr(KScript &S, const uint8_t *data, uint32_t len,
                      int32_t start, int32_t end) {
  if (start < 0 || end < 0) return KV_SCRIPT_INVALID_INDEX;
  if (end < start) return KV_SCRIPT_INVALID_RANGE;
  if ((uint32_t)(end - start) > KVS_MAX_ELEMENT)
    return KV_SCRIPT_ELEMENT_TOO_BIG;
  if ((uint32_t)end > len) return KV_SCRIPT_INVALID_SOURCE;
  return S.push(KEnt(data + start, data + end));
}

/* host sha256 (FIPS 180-4; OpSHA256 only — the hot path hashes on device) */
static const uint32_t KVS_SHA_K[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1,
    0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3,
    0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786,
    0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
    0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
    0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13,
    0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b,
    0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
    0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a,
    0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
    0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};

static void kvs_sha256(const uint8_t *data, size_t len, uint8_t out[32]) {
  uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a,
                   0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
  uint64_t total = (uint64_t)len * 8;
  std::vector<uint8_t> buf(data, data + len);
  buf.push_back(0x80);
  while (buf.size() % 64 != 56) buf.push_back(0);
  for (int i = 7; i >= 0; i--) buf.push_back((uint8_t)(total >> (8 * i)));
  for (size_t off = 0; off < buf.size(); off += 64) {
    uint32_t w[64];
    for (int i = 0; i < 16; i++)
      w[i] = ((uint32_t)buf[off + 4 * i] << 24) | ((uint32_t)buf[off + 4 * i + 1] << 16) |
             ((uint32_t)buf[off + 4 * i + 2] << 8) | buf[off + 4 * i + 3];
    for (int i = 16; i < 64; i++) {
      uint32_t s0 = (w[i - 15] >> 7 | w[i - 15] << 25) ^
                    (w[i - 15] >> 18 | w[i - 15] << 14) ^ (w[i - 15] >> 3);
      uint32_t s1 = (w[i - 2] >> 17 | w[i - 2] << 15) ^
                    (w[i - 2] >> 19 | w[i - 2] << 13) ^ (w[i - 2] >> 10);
      w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t a = h[0], b = h[1], c = h[2], dd = h[3], e = h[4], f = h[5],
             g = h[6], hh = h[7];
    for (int i = 0; i < 64; i++) {
      uint32_t S1 = (e >> 6 | e << 26) ^ (e >> 11 | e << 21) ^ (e >> 25 | e << 7);
      uint32_t ch = (e & f) ^ (~e & g);
      uint32_t t1 = hh + S1 + ch + KVS_SHA_K[i] + w[i];
      uint32_t S0 = (a >> 2 | a << 30) ^ (a >> 13 | a << 19) ^ (a >> 22 | a << 10);
      uint32_t mj = (a & b) ^ (a & c) ^ (b & c);
      uint32_t t2 = S0 + mj;
      hh = g; g = f; f = e; e = dd + t1;
      dd = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += dd;
    h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
  }
  for (int i = 0; i < 8; i++) {
    out[4 * i] = (uint8_t)(h[i] >> 24);
    out[4 * i + 1] = (uint8_t)(h[i] >> 16);
    out[4 * i + 2] = (uint8_t)(h[i] >> 8);
    out[4 * i + 3] = (uint8_t)h[i];
  }
}

static bool kvs_is_executing(const KScript &S) {
  return S.cond.empty() || S.cond.back() == 1; /* top-only; nested Ifs push
                                                  skip markers */
}

/* ---- host BLAKE3 (the blake3 crate the reference links for OpBlake3 /
 * OpBlake3WithKey, opcodes/mod.rs:1457-1476) — independent product
 * implementation from the BLAKE3 spec; full chunk-tree for inputs beyond
 * 1024B (stack elements can reach 1MB). ---- */
static const uint32_t KVS_B3_IV[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u,
                                      0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu,
                                      0x1F83D9ABu, 0x5BE0CD19u};
static const uint8_t KVS_B3_PERM[16] = {2, 6, 3, 10, 7, 0, 4, 13,
                                        1, 11, 12, 5, 9, 14, 15, 8};
#define KVS_B3_CHUNK_START 1u
#define KVS_B3_CHUNK_END 2u
#define KVS_B3_PARENT 4u
#define KVS_B3_ROOT 8u
#define KVS_B3_KEYED 16u

static inline uint32_t kvs_rotr32(uint32_t x, int n) {
  return (x >> n) | (x << (32 - n));
}

static void kvs_b3_compress(const uint32_t cv[8], const uint32_t mw[16], uint64_t ctr,
                            uint32_t blen, uint32_t flags, uint32_t out8[8]) {
  uint32_t st[16];
  for (int i = 0; i < 8; i++) st[i] = cv[i];
  for (int i = 0; i < 4; i++) st[8 + i] = KVS_B3_IV[i];
  st[12] = (uint32_t)ctr;
  st[13] = (uint32_t)(ctr >> 32);
  st[14] = blen;
  st[15] = flags;
  uint32_t m[16];
  memcpy(m, mw, 64);
#define KB3G(a, b, c, d, x, y)                                                 \
  st[a] += st[b] + (x); st[d] = kvs_rotr32(st[d] ^ st[a], 16);                 \
  st[c] += st[d]; st[b] = kvs_rotr32(st[b] ^ st[c], 12);                       \
  st[a] += st[b] + (y); st[d] = kvs_rotr32(st[d] ^ st[a], 8);                  \
  st[c] += st[d]; st[b] = kvs_rotr32(st[b] ^ st[c], 7);
  for (int r = 0;; r++) {
    KB3G(0, 4, 8, 12, m[0], m[1]) KB3G(1, 5, 9, 13, m[2], m[3])
    KB3G(2, 6, 10, 14, m[4], m[5]) KB3G(3, 7, 11, 15, m[6], m[7])
    KB3G(0, 5, 10, 15, m[8], m[9]) KB3G(1, 6, 11, 12, m[10], m[11])
    KB3G(2, 7, 8, 13, m[12], m[13]) KB3G(3, 4, 9, 14, m[14], m[15])
    if (r == 6) break;
    uint32_t nm[16];
    for (int i = 0; i < 16; i++) nm[i] = m[KVS_B3_PERM[i]];
    memcpy(m, nm, 64);
  }
#undef KB3G
  for (int i = 0; i < 8; i++) out8[i] = st[i] ^ st[i + 8];
}

/* the final node, kept un-compressed so ROOT can be OR-ed in at extraction */
struct KvB3Out {
  uint32_t cv[8];
  uint32_t blk[16];
  uint32_t blen;
  uint64_t ctr;
  uint32_t flags;
};

static void kvs_blake3(const uint8_t *key32 /* nullable */, const uint8_t *data,
                       size_t len, uint8_t out32[32]) {
  uint32_t key[8];
  uint32_t base = 0;
  if (key32) {
    for (int i = 0; i < 8; i++) memcpy(&key[i], key32 + 4 * i, 4);
    base = KVS_B3_KEYED;
  } else {
    memcpy(key, KVS_B3_IV, 32);
  }
  uint32_t stack[54][8];
  int sp = 0;
  uint64_t chunk_idx = 0;
  size_t off = 0;
  KvB3Out node;
  for (;;) {
    size_t clen = len - off;
    if (clen > 1024) clen = 1024;
    bool last_chunk = (off + clen == len);
    uint32_t cv[8];
    memcpy(cv, key, 32);
    size_t nblocks = clen == 0 ? 1 : (clen + 63) / 64;
    for (size_t b = 0; b < nblocks; b++) {
      size_t blen = clen - b * 64;
      if (blen > 64) blen = 64;
      uint8_t buf[64];
      memset(buf, 0, 64);
      memcpy(buf, data + off + b * 64, blen);
      uint32_t mw[16];
      for (int i = 0; i < 16; i++) memcpy(&mw[i], buf + 4 * i, 4);
      uint32_t flags = base;
      if (b == 0) flags |= KVS_B3_CHUNK_START;
      if (b == nblocks - 1) flags |= KVS_B3_CHUNK_END;
      if (b == nblocks - 1 && last_chunk) {
        /* final chunk's last block becomes the output node */
        memcpy(node.cv, cv, 32);
        memcpy(node.blk, mw, 64);
        node.blen = (uint32_t)blen;
        node.ctr = chunk_idx;
        node.flags = flags;
      } else {
        kvs_b3_compress(cv, mw, chunk_idx, (uint32_t)blen, flags, cv);
      }
    }
    if (last_chunk) break;
    /* completed non-final chunk: fold into the CV stack by chunk count */
    chunk_idx++;
    uint64_t total = chunk_idx;
    while ((total & 1) == 0) {
      uint32_t blk[16];
      memcpy(blk, stack[--sp], 32);
      memcpy(blk + 8, cv, 32);
      kvs_b3_compress(key, blk, 0, 64, base | KVS_B3_PARENT, cv);
      total >>= 1;
    }
    memcpy(stack[sp++], cv, 32);
    off += clen;
  }
  /* merge remaining left siblings over the output node */
  while (sp > 0) {
    uint32_t right[8];
    kvs_b3_compress(node.cv, node.blk, node.ctr, node.blen, node.flags, right);
    memcpy(node.blk, stack[--sp], 32);
    memcpy(node.blk + 8, right, 32);
    memcpy(node.cv, key, 32);
    node.blen = 64;
    node.ctr = 0;
    node.flags = base | KVS_B3_PARENT;
  }
  uint32_t root[8];
  kvs_b3_compress(node.cv, node.blk, node.ctr, node.blen,
                  node.flags | KVS_B3_ROOT, root);
  for (int i = 0; i < 8; i++) memcpy(out32 + 4 * i, &root[i], 4);
}

enum { KVC_FALSE = 0, KVC_TRUE = 1, KVC_SKIP = 2 };

/* ---- signature-check family (collect/replay protocol, see header) ----
 * Mirrors check_schnorr_signature / check_ecdsa_signature (lib.rs:846-905)
 * and the opcode wrappers (opcodes/mod.rs:804-875, 1438-1455). */

static bool kvs_sighash_type_valid(uint8_t t) {
  return t == 0x01 || t == 0x02 || t == 0x04 || t == 0x81 || t == 0x82 || t == 0x84;
}

/* Resolve sig-site k: memo hit returns the site's status vector; otherwise
 * the caller must queue its requests into S.rctx->pending and return SUSPEND.
 * Called LAZILY — only when an op actually needs a verify status — so ops
 * whose outcome is host-decidable (zero sigs, length errors before any curve
 * check) never allocate a site and never cost a round. */
static int kvs_site_statuses(KScript &S, const std::vector<uint8_t> **sts) {
  uint32_t k = S.site++;
  if (S.rctx && S.rctx->memo && k < S.rctx->memo->size()) {
    *sts = &(*S.rctx->memo)[k];
    return 0;
  }
  *sts = nullptr;
  return S.rctx && S.rctx->pending ? KVH_SCRIPT_SUSPEND : KVH_SCRIPT_DEFER;
}

static void kvs_queue_req(KScript &S, bool ecdsa, bool literal, uint8_t hash_type,
                          const KEnt &sig, const KEnt &key, const uint8_t *msg32) {
  KvSigReq r;
  memset(&r, 0, sizeof(r));
  r.ecdsa = ecdsa ? 1 : 0;
  r.literal = literal ? 1 : 0;
  r.hash_type = hash_type;
  if (sig.size() == 64) memcpy(r.sig, sig.data(), 64); /* else zeroed: status
                         consulted for the pubkey only (length error wins) */
  size_t pklen = ecdsa ? 33 : 32;
  if (key.size() == pklen) memcpy(r.pk, key.data(), pklen);
  if (literal && msg32) memcpy(r.msg, msg32, 32);
  S.rctx->pending->push_back(r);
}

/* host-decidable prefix of check_*_signature (lib.rs:857-860, 888-890):
 * sig-op cost, then the pubkey LENGTH error. Curve/parse statuses need GPU. */
static int kvs_sig_check_pre(KScript &S, bool ecdsa, const KEnt &key) {
  int rc = S.consume(S.sigop_units);
  if (rc) return rc;
  if (!ecdsa) {
    if (key.size() != 32) return KV_SCRIPT_INVALID_PUBKEY;
  } else {
    if (key.size() != 33) return KV_SCRIPT_PUBKEY_FORMAT;
  }
  return 0;
}

/* status-dependent tail: curve check (status 2), signature length, then
 * signature parse (status 3), then the verdict. */
static int kvs_sig_check_post(size_t sig_len, uint8_t st, bool *valid) {
  if (st == 2) return KV_SCRIPT_INVALID_PUBKEY;
  if (sig_len != 64) return KV_SCRIPT_INVALID_SIGNATURE;
  if (st == 3) return KV_SCRIPT_INVALID_SIGNATURE;
  *valid = st == 0;
  return 0;
}

/* OpCheckSig (0xac) / OpCheckSigECDSA (0xab), opcodes/mod.rs:804-850 */
static int kvs_op_checksig(KScript &S, bool ecdsa) {
  if (S.d.size() < 2) return KV_SCRIPT_INVALID_STACK_OPERATION;
  KEnt key, sig;
  kvs_pop(S, &key);
  kvs_pop(S, &sig);
  if (sig.empty()) return S.push(KEnt()); /* push false */
  uint8_t type = sig.back();
  sig.pop_back();
  if (!kvs_sighash_type_valid(type)) return KV_SCRIPT_INVALID_SIG_HASH_TYPE;
  int rc = kvs_sig_check_pre(S, ecdsa, key);
  if (rc) return rc;
  const std::vector<uint8_t> *sts;
  rc = kvs_site_statuses(S, &sts);
  if (rc) {
    if (rc == KVH_SCRIPT_SUSPEND) kvs_queue_req(S, ecdsa, false, type, sig, key, nullptr);
    return rc;
  }
  bool valid = false;
  rc = kvs_sig_check_post(sig.size(), sts->empty() ? 1 : (*sts)[0], &valid);
  if (rc) return rc;
  return S.push(valid ? KEnt{1} : KEnt());
}

/* OpCheckSigFromStack (0xd7) / ...ECDSA (0xd8), opcodes/mod.rs:1438-1455:
 * pops [signature, msg_hash, pubkey] (pubkey on top); no hash-type byte. */
static int kvs_op_checksig_from_stack(KScript &S, bool ecdsa) {
  if (S.d.size() < 3) return KV_SCRIPT_INVALID_STACK_OPERATION;
  KEnt key, msg, sig;
  kvs_pop(S, &key);
  kvs_pop(S, &msg);
  kvs_pop(S, &sig);
  if (msg.size() != 32) return KV_SCRIPT_INVALID_STATE; /* Hash::try_from */
  int rc = kvs_sig_check_pre(S, ecdsa, key);
  if (rc) return rc;
  const std::vector<uint8_t> *sts;
  rc = kvs_site_statuses(S, &sts);
  if (rc) {
    if (rc == KVH_SCRIPT_SUSPEND)
      kvs_queue_req(S, ecdsa, true, 0, sig, key, msg.data());
    return rc;
  }
  bool valid = false;
  rc = kvs_sig_check_post(sig.size(), sts->empty() ? 1 : (*sts)[0], &valid);
  if (rc) return rc;
  return S.push(valid ? KEnt{1} : KEnt());
}

/* OpCheckMultiSig (0xae) / OpCheckMultiSigECDSA (0xa9)
 * ⇔ op_check_multisig_schnorr_or_ecdsa (lib.rs:759-843). At collection the
 * site queues sig-major rows of n statuses for every sig up to (exclusive)
 * the first empty or invalid-hash-type sig — later sigs are never checked
 * before an error or break. Replay walks the reference's greedy loop over
 * those rows. */
static int kvs_op_multisig(KScript &S, bool ecdsa) {
  int rc;
  int32_t num_keys;
  if ((rc = kvs_pop_i32(S, &num_keys))) return rc;
  if (num_keys < 0 || num_keys > 20) return KV_SCRIPT_INVALID_PUBKEY_COUNT;
  S.num_ops += num_keys;
  if (S.num_ops > KVS_MAX_OPS) return KV_SCRIPT_TOO_MANY_OPERATIONS;
  if (S.d.size() < (size_t)num_keys) return KV_SCRIPT_INVALID_STACK_OPERATION;
  std::vector<KEnt> keys(S.d.end() - num_keys, S.d.end());
  S.d.resize(S.d.size() - num_keys);
  int32_t num_sigs;
  if ((rc = kvs_pop_i32(S, &num_sigs))) return rc;
  if (num_sigs < 0 || num_sigs > num_keys) return KV_SCRIPT_INVALID_SIGNATURE_COUNT;
  if (S.d.size() < (size_t)num_sigs) return KV_SCRIPT_INVALID_STACK_OPERATION;
  std::vector<KEnt> sigs(S.d.end() - num_sigs, S.d.end());
  S.d.resize(S.d.size() - num_sigs);

  /* Greedy loop (lib.rs:794-836) with LAZY site allocation: the status
   * vector is consulted only when a pair reaches the curve-check point; an
   * op that errors or completes before that (zero sigs, empty first sig,
   * length/type errors, budget) never allocates a site. The tuple layout is
   * a function of stack data only (sig-major rows of num_keys statuses for
   * sigs up to the first empty/invalid-type), so replay indexes match. */
  const std::vector<uint8_t> *sts = nullptr;
  bool failed = false;
  int kp = 0;
  size_t row = 0; /* row base into the status vector, num_keys wide */
  for (int si = 0; si < num_sigs; si++) {
    if (sigs[si].empty()) {
      failed = true;
      break;
    }
    uint8_t type = sigs[si].back();
    if (!kvs_sighash_type_valid(type)) return KV_SCRIPT_INVALID_SIG_HASH_TYPE;
    size_t sig_len = sigs[si].size() - 1;
    size_t base = row;
    row += num_keys;
    bool matched = false;
    while (true) {
      if (num_keys - kp < num_sigs - si) {
        failed = true;
        break;
      }
      int ki = kp++;
      rc = kvs_sig_check_pre(S, ecdsa, keys[ki]);
      if (rc) return rc;
      if (!sts) { /* first curve-check of this op: resolve or collect */
        rc = kvs_site_statuses(S, &sts);
        if (rc) {
          if (rc == KVH_SCRIPT_SUSPEND) {
            for (int cs = 0; cs < num_sigs; cs++) {
              if (sigs[cs].empty()) break;
              uint8_t ct = sigs[cs].back();
              if (!kvs_sighash_type_valid(ct)) break;
              KEnt body(sigs[cs].begin(), sigs[cs].end() - 1);
              for (int ck = 0; ck < num_keys; ck++)
                kvs_queue_req(S, ecdsa, false, ct, body, keys[ck], nullptr);
            }
          }
          return rc;
        }
      }
      uint8_t st = base + ki < sts->size() ? (*sts)[base + ki] : 1;
      bool valid = false;
      rc = kvs_sig_check_post(sig_len, st, &valid);
      if (rc) return rc;
      if (valid) {
        matched = true;
        break;
      }
    }
    if (!matched) break; /* failed set inside */
  }
  bool any_nonempty = false;
  for (const auto &s : sigs)
    if (!s.empty()) any_nonempty = true;
  if (failed && any_nonempty) return KV_SCRIPT_NULL_FAIL;
  return S.push(failed ? KEnt() : KEnt{1});
}

/* pop the result of a *Verify wrapper (opcodes/mod.rs:851-858, 866-875) */
static int kvs_verify_top(KScript &S) {
  KEnt v;
  int rc = kvs_pop(S, &v);
  if (rc) return rc;
  return kvs_bool(v) ? 0 : KV_SCRIPT_VERIFY_ERROR;
}

/* one opcode (payload already parsed). Mirrors the reference's execute_opcode
 * dispatch; pushes METER into op_pushed and the caller charges after the op
 * (runtime_resource_meter.rs ordering: the op's own error wins over its
 * metering). */
static int kvs_exec_op(KScript &S, uint8_t op, const uint8_t *data,
                       uint32_t dlen);
static int kvs_exec_introspection(KScript &S, uint8_t op);

static int kvs_run_one_script(KScript &S, const uint8_t *script, uint32_t slen,
                              bool verify_only_push) {
  uint32_t pc = 0;
  int rc = 0;
  while (pc < slen) {
    uint8_t op = script[pc++];
    const uint8_t *data = nullptr;
    uint32_t dlen = 0;
    if (op >= 0x01 && op <= 0x4b) {
      dlen = op;
      if (pc + dlen > slen) return KV_SCRIPT_MALFORMED_PUSH;
      data = script + pc;
      pc += dlen;
    } else if (op >= 0x4c && op <= 0x4e) {
      uint32_t szlen = op == 0x4c ? 1 : (op == 0x4d ? 2 : 4);
      if (pc + szlen > slen) return KV_SCRIPT_MALFORMED_PUSH;
      for (uint32_t i = 0; i < szlen; i++)
        dlen |= (uint32_t)script[pc + i] << (8 * i);
      pc += szlen;
      if (dlen > slen || pc + dlen > slen) return KV_SCRIPT_MALFORMED_PUSH;
      data = script + pc;
      pc += dlen;
    }
    bool is_push = op <= 0x60;
    if (op == 0x80 || op == 0x81 || op == 0x8d || op == 0x8e || op == 0x98 ||
        op == 0x99)
      return KV_SCRIPT_OPCODE_DISABLED;
    if (op == 0x65 || op == 0x66) return KV_SCRIPT_OPCODE_RESERVED;
    if (verify_only_push && !is_push) return KV_SCRIPT_NOT_PUSH_ONLY;
    if (!is_push) {
      if (++S.num_ops > KVS_MAX_OPS) return KV_SCRIPT_TOO_MANY_OPERATIONS;
    } else if (dlen > KVS_MAX_ELEMENT) {
      return KV_SCRIPT_ELEMENT_TOO_BIG;
    }
    bool conditional = op >= 0x63 && op <= 0x68;
    if (kvs_is_executing(S) || conditional) {
      S.op_pushed = 0;
      rc = kvs_exec_op(S, op, data, dlen);
      if (rc) return rc;
      rc = S.consume(S.op_pushed);
      if (rc) return rc;
    }
    if (S.d.size() + S.a.size() > KVS_MAX_STACK)
      return KV_SCRIPT_STACK_SIZE_EXCEEDED;
  }
  if (!S.cond.empty()) return KV_SCRIPT_UNBALANCED_CONDITIONAL;
  /* alt stack and op count do not persist across scripts (lib.rs:646-648) */
  S.a.clear();
  S.num_ops = 0;
  return 0;
}

#define KVS_POP2(a, b)                                                         \
  int64_t a, b;                                                                \
  {                                                                            \
    if (S.d.size() < 2) return KV_SCRIPT_INVALID_STACK_OPERATION;              \
    int rc2;                                                                   \
    if ((rc2 = kvs_pop_num(S, &b))) return rc2;                                \
    if ((rc2 = kvs_pop_num(S, &a))) return rc2;                                \
  }

static int kvs_exec_op(KScript &S, uint8_t op, const uint8_t *data,
                       uint32_t dlen) {
  int rc;
  const HTx &tx = *S.tx;
  switch (op) {
    case 0x00:
      return S.push(KEnt(), false);
    case 0x4f:
      return kvs_push_num(S, -1, false);
    case 0x50:
    case 0x62:
    case 0x89:
    case 0x8a:
      return KV_SCRIPT_OPCODE_RESERVED;
    case 0x61:
      return 0; /* nop */
    case 0x63:
    case 0x64: { /* if / notif */
      int cond = KVC_SKIP;
      if (kvs_is_executing(S)) {
        KEnt e;
        if ((rc = kvs_pop(S, &e))) return rc;
        bool b = kvs_bool(e);
        if (op == 0x64) b = !b;
        cond = b ? KVC_TRUE : KVC_FALSE;
      }
      if (S.cond.size() >= 4096) return KV_SCRIPT_INVALID_STATE;
      S.cond.push_back((uint8_t)cond);
      return 0;
    }
    case 0x67: /* else */
      if (S.cond.empty()) return KV_SCRIPT_INVALID_STATE;
      {
        uint8_t &c = S.cond.back();
        c = c == KVC_TRUE ? KVC_FALSE : (c == KVC_FALSE ? KVC_TRUE : KVC_SKIP);
      }
      return 0;
    case 0x68: /* endif */
      if (S.cond.empty()) return KV_SCRIPT_INVALID_STATE;
      S.cond.pop_back();
      return 0;
    case 0x69: { /* verify */
      KEnt e;
      if ((rc = kvs_pop(S, &e))) return rc;
      return kvs_bool(e) ? 0 : KV_SCRIPT_VERIFY_ERROR;
    }
    case 0x6a:
      return KV_SCRIPT_EARLY_RETURN;
    case 0x6b: { /* toaltstack */
      KEnt e;
      if ((rc = kvs_pop(S, &e))) return rc;
      return S.push_alt(std::move(e));
    }
    case 0x6c: { /* fromaltstack */
      if (S.a.empty()) return KV_SCRIPT_EMPTY_STACK;
      KEnt e = std::move(S.a.back());
      S.a.pop_back();
      return S.push(std::move(e), false);
    }
    case 0x6d: /* 2drop */
      if (S.d.size() < 2) return KV_SCRIPT_INVALID_STACK_OPERATION;
      S.d.pop_back();
      S.d.pop_back();
      return 0;
    case 0x6e: { /* 2dup */
      if (S.d.size() < 2) return KV_SCRIPT_INVALID_STACK_OPERATION;
      KEnt a = S.d[S.d.size() - 2], b = S.d[S.d.size() - 1];
      if ((rc = S.push(std::move(a)))) return rc;
      return S.push(std::move(b));
    }
    case 0x6f: { /* 3dup */
      if (S.d.size() < 3) return KV_SCRIPT_INVALID_STACK_OPERATION;
      size_t base = S.d.size();
      for (int k = 3; k >= 1; k--) {
        KEnt c = S.d[base - k];
        if ((rc = S.push(std::move(c)))) return rc;
      }
      return 0;
    }
    case 0x70: { /* 2over */
      if (S.d.size() < 4) return KV_SCRIPT_INVALID_STACK_OPERATION;
      size_t base = S.d.size();
      for (int k = 4; k >= 3; k--) {
        KEnt c = S.d[base - k];
        if ((rc = S.push(std::move(c)))) return rc;
      }
      return 0;
    }
    case 0x71: { /* 2rot */
      if (S.d.size() < 6) return KV_SCRIPT_INVALID_STACK_OPERATION;
      size_t n = S.d.size();
      KEnt a = std::move(S.d[n - 6]), b = std::move(S.d[n - 5]);
      S.d.erase(S.d.begin() + (n - 6), S.d.begin() + (n - 4));
      S.d.push_back(std::move(a));
      S.d.push_back(std::move(b));
      return 0;
    }
    case 0x72: { /* 2swap */
      if (S.d.size() < 4) return KV_SCRIPT_INVALID_STACK_OPERATION;
      size_t n = S.d.size();
      std::swap(S.d[n - 4], S.d[n - 2]);
      std::swap(S.d[n - 3], S.d[n - 1]);
      return 0;
    }
    case 0x73: { /* ifdup */
      if (S.d.empty()) return KV_SCRIPT_INVALID_STACK_OPERATION;
      if (kvs_bool(S.d.back())) {
        KEnt c = S.d.back();
        return S.push(std::move(c));
      }
      return 0;
    }
    case 0x74: /* depth */
      return kvs_push_num(S, (int64_t)S.d.size());
    case 0x75: /* drop */
      if (S.d.empty()) return KV_SCRIPT_INVALID_STACK_OPERATION;
      S.d.pop_back();
      return 0;
    case 0x76: { /* dup */
      if (S.d.empty()) return KV_SCRIPT_INVALID_STACK_OPERATION;
      KEnt c = S.d.back();
      return S.push(std::move(c));
    }
    case 0x77: /* nip */
      if (S.d.size() < 2) return KV_SCRIPT_INVALID_STACK_OPERATION;
      S.d.erase(S.d.end() - 2);
      return 0;
    case 0x78: { /* over */
      if (S.d.size() < 2) return KV_SCRIPT_INVALID_STACK_OPERATION;
      KEnt c = S.d[S.d.size() - 2];
      return S.push(std::move(c));
    }
    case 0x79: { /* pick */
      int32_t loc;
      if ((rc = kvs_pop_i32(S, &loc))) return rc;
      if (loc < 0 || (size_t)loc >= S.d.size()) return KV_SCRIPT_INVALID_STATE;
      KEnt c = S.d[S.d.size() - 1 - loc];
      return S.push(std::move(c));
    }
    case 0x7a: { /* roll */
      int32_t loc;
      if ((rc = kvs_pop_i32(S, &loc))) return rc;
      if (loc < 0 || (size_t)loc >= S.d.size()) return KV_SCRIPT_INVALID_STATE;
      KEnt c = std::move(S.d[S.d.size() - 1 - loc]);
      S.d.erase(S.d.end() - 1 - loc);
      /* a roll re-push is metered (it went through push in the reference) */
      return S.push(std::move(c));
    }
    case 0x7b: { /* rot */
      if (S.d.size() < 3) return KV_SCRIPT_INVALID_STACK_OPERATION;
      size_t n = S.d.size();
      KEnt c = std::move(S.d[n - 3]);
      S.d.erase(S.d.end() - 3);
      S.d.push_back(std::move(c));
      return 0;
    }
    case 0x7c: /* swap */
      if (S.d.size() < 2) return KV_SCRIPT_INVALID_STACK_OPERATION;
      std::swap(S.d[S.d.size() - 2], S.d[S.d.size() - 1]);
      return 0;
    case 0x7d: { /* tuck */
      if (S.d.size() < 2) return KV_SCRIPT_INVALID_STACK_OPERATION;
      KEnt c = S.d.back();
      S.op_pushed += c.size();
      if (S.d.size() >= KVS_MAX_STACK) return KV_SCRIPT_STACK_SIZE_EXCEEDED;
      S.d.insert(S.d.end() - 2, std::move(c));
      return 0;
    }
    case 0x7e: { /* cat */
      if (S.d.size() < 2) return KV_SCRIPT_EMPTY_STACK;
      KEnt b, a;
      (void)kvs_pop(S, &b);
      (void)kvs_pop(S, &a);
      a.insert(a.end(), b.begin(), b.end());
      return S.push(std::move(a));
    }
    case 0x7f: { /* substr */
      int64_t start64, end64;
      if (S.d.size() < 2) return KV_SCRIPT_INVALID_STACK_OPERATION;
      if ((rc = kvs_pop_num(S, &end64))) return rc;
      if ((rc = kvs_pop_num(S, &start64))) return rc;
      if (start64 > INT32_MAX || start64 < INT32_MIN || end64 > INT32_MAX ||
          end64 < INT32_MIN)
        return KV_SCRIPT_NUMBER_TOO_BIG;
      if (S.d.empty()) return KV_SCRIPT_EMPTY_STACK;
      KEnt e;
      (void)kvs_pop(S, &e);
      if (start64 < 0 || end64 < 0) return KV_SCRIPT_INVALID_INDEX;
      uint64_t start = (uint64_t)start64, end = (uint64_t)end64;
      if (end < start) return KV_SCRIPT_INVALID_RANGE;
      if (end - start > KVS_MAX_ELEMENT) return KV_SCRIPT_ELEMENT_TOO_BIG;
      if (end > e.size()) return KV_SCRIPT_INVALID_RANGE;
      return S.push(KEnt(e.begin() + start, e.begin() + end));
    }
    case 0x82: /* size */
      if (S.d.empty()) return KV_SCRIPT_INVALID_STACK_OPERATION;
      return kvs_push_num(S, (int64_t)S.d.back().size());
    case 0x83: { /* invert (in place, metered as a push) */
      if (S.d.empty()) return KV_SCRIPT_EMPTY_STACK;
      for (auto &x : S.d.back()) x = (uint8_t)~x;
      S.op_pushed += S.d.back().size();
      return 0;
    }
    case 0x84:
    case 0x85:
    case 0x86: { /* and / or / xor */
      if (S.d.size() < 2) return KV_SCRIPT_EMPTY_STACK;
      KEnt b, a;
      (void)kvs_pop(S, &b);
      (void)kvs_pop(S, &a);
      if (a.size() != b.size()) return KV_SCRIPT_INVALID_STATE;
      for (size_t i = 0; i < a.size(); i++)
        a[i] = op == 0x84 ? (a[i] & b[i]) : op == 0x85 ? (a[i] | b[i])
                                                       : (a[i] ^ b[i]);
      return S.push(std::move(a));
    }
    case 0x87: { /* equal */
      if (S.d.size() < 2) return KV_SCRIPT_INVALID_STACK_OPERATION;
      KEnt b, a;
      (void)kvs_pop(S, &b);
      (void)kvs_pop(S, &a);
      return S.push(a == b ? KEnt{1} : KEnt{});
    }
    case 0x88: { /* equalverify */
      if (S.d.size() < 2) return KV_SCRIPT_INVALID_STACK_OPERATION;
      KEnt b, a;
      (void)kvs_pop(S, &b);
      (void)kvs_pop(S, &a);
      return a == b ? 0 : KV_SCRIPT_VERIFY_ERROR;
    }
    case 0x8b: { /* 1add */
      int64_t v;
      if ((rc = kvs_pop_num(S, &v))) return rc;
      if (v == INT64_MAX) return KV_SCRIPT_NUMBER_TOO_BIG;
      return kvs_push_num(S, v + 1);
    }
    case 0x8c: { /* 1sub */
      int64_t v;
      if ((rc = kvs_pop_num(S, &v))) return rc;
      if (v == INT64_MIN) return KV_SCRIPT_NUMBER_TOO_BIG;
      return kvs_push_num(S, v - 1);
    }
    case 0x8f: { /* negate */
      int64_t v;
      if ((rc = kvs_pop_num(S, &v))) return rc;
      if (v == INT64_MIN) return KV_SCRIPT_NUMBER_TOO_BIG;
      return kvs_push_num(S, -v);
    }
    case 0x90: { /* abs */
      int64_t v;
      if ((rc = kvs_pop_num(S, &v))) return rc;
      if (v == INT64_MIN) return KV_SCRIPT_NUMBER_TOO_BIG;
      return kvs_push_num(S, v < 0 ? -v : v);
    }
    case 0x91: { /* not */
      int64_t v;
      if ((rc = kvs_pop_num(S, &v))) return rc;
      return kvs_push_num(S, v == 0);
    }
    case 0x92: { /* 0notequal */
      int64_t v;
      if ((rc = kvs_pop_num(S, &v))) return rc;
      return kvs_push_num(S, v != 0);
    }
    case 0x93: { /* add */
      KVS_POP2(a, b);
      if ((b > 0 && a > INT64_MAX - b) || (b < 0 && a < INT64_MIN - b))
        return KV_SCRIPT_NUMBER_TOO_BIG;
      return kvs_push_num(S, a + b);
    }
    case 0x94: { /* sub */
      KVS_POP2(a, b);
      if ((b < 0 && a > INT64_MAX + b) || (b > 0 && a < INT64_MIN + b))
        return KV_SCRIPT_NUMBER_TOO_BIG;
      return kvs_push_num(S, a - b);
    }
    case 0x95: { /* mul */
      KVS_POP2(a, b);
      if (a != 0 && b != 0) {
        int64_t r = (int64_t)((uint64_t)a * (uint64_t)b);
        if ((a == INT64_MIN && b == -1) || r / b != a)
          return KV_SCRIPT_NUMBER_TOO_BIG;
        return kvs_push_num(S, r);
      }
      return kvs_push_num(S, 0);
    }
    case 0x96: { /* div */
      KVS_POP2(a, b);
      if (b == 0 || (a == INT64_MIN && b == -1)) return KV_SCRIPT_INVALID_STATE;
      return kvs_push_num(S, a / b);
    }
    case 0x97: { /* mod */
      KVS_POP2(a, b);
      if (b == 0 || (a == INT64_MIN && b == -1)) return KV_SCRIPT_INVALID_STATE;
      return kvs_push_num(S, a % b);
    }
    case 0x9a: { KVS_POP2(a, b); return kvs_push_num(S, a != 0 && b != 0); }
    case 0x9b: { KVS_POP2(a, b); return kvs_push_num(S, a != 0 || b != 0); }
    case 0x9c: { KVS_POP2(a, b); return kvs_push_num(S, a == b); }
    case 0x9d: { KVS_POP2(a, b); return a == b ? 0 : KV_SCRIPT_VERIFY_ERROR; }
    case 0x9e: { KVS_POP2(a, b); return kvs_push_num(S, a != b); }
    case 0x9f: { KVS_POP2(a, b); return kvs_push_num(S, a < b); }
    case 0xa0: { KVS_POP2(a, b); return kvs_push_num(S, a > b); }
    case 0xa1: { KVS_POP2(a, b); return kvs_push_num(S, a <= b); }
    case 0xa2: { KVS_POP2(a, b); return kvs_push_num(S, a >= b); }
    case 0xa3: { KVS_POP2(a, b); return kvs_push_num(S, a < b ? a : b); }
    case 0xa4: { KVS_POP2(a, b); return kvs_push_num(S, a > b ? a : b); }
    case 0xa5: { /* within */
      int64_t x, l, u;
      if (S.d.size() < 3) return KV_SCRIPT_INVALID_STACK_OPERATION;
      if ((rc = kvs_pop_num(S, &u))) return rc;
      if ((rc = kvs_pop_num(S, &l))) return rc;
      if ((rc = kvs_pop_num(S, &x))) return rc;
      return kvs_push_num(S, x >= l && x < u);
    }
    case 0xa7: { /* blake2b with key */
      if (S.d.size() < 2) return KV_SCRIPT_INVALID_STACK_OPERATION;
      KEnt key, msg;
      (void)kvs_pop(S, &key);
      (void)kvs_pop(S, &msg);
      if (key.size() > 64) return KV_SCRIPT_ELEMENT_TOO_BIG;
      if ((rc = S.consume((uint64_t)msg.size() * 2))) return rc;
      uint8_t h[32];
      h_blake2b_keyed(key.data(), key.size(), msg.data(), msg.size(), h);
      return S.push(KEnt(h, h + 32));
    }
    case 0xa8: { /* sha256 */
      KEnt e;
      if ((rc = kvs_pop(S, &e))) return rc;
      if ((rc = S.consume(e.size()))) return rc;
      uint8_t h[32];
      kvs_sha256(e.data(), e.size(), h);
      return S.push(KEnt(h, h + 32));
    }
    case 0xaa: { /* blake2b */
      KEnt e;
      if ((rc = kvs_pop(S, &e))) return rc;
      if ((rc = S.consume((uint64_t)e.size() * 2))) return rc;
      uint8_t h[32];
      h_blake2b_keyed(nullptr, 0, e.data(), e.size(), h);
      return S.push(KEnt(h, h + 32));
    }
    case 0xb0: { /* checklocktimeverify */
      KEnt e;
      if ((rc = kvs_pop(S, &e))) return rc;
      if (e.size() > 8) return KV_SCRIPT_NUMBER_TOO_BIG;
      uint64_t lt = 0;
      for (size_t i = 0; i < e.size(); i++) lt |= (uint64_t)e[i] << (8 * i);
      const uint64_t THRESH = 500000000000ull;
      if ((S.tx->lock_time < THRESH) != (lt < THRESH))
        return KV_SCRIPT_UNSATISFIED_LOCKTIME;
      if (lt > S.tx->lock_time) return KV_SCRIPT_UNSATISFIED_LOCKTIME;
      if (S.input->sequence == UINT64_MAX) return KV_SCRIPT_UNSATISFIED_LOCKTIME;
      return 0;
    }
    case 0xb1: { /* checksequenceverify */
      KEnt e;
      if ((rc = kvs_pop(S, &e))) return rc;
      if (e.size() > 8) return KV_SCRIPT_NUMBER_TOO_BIG;
      uint64_t st = 0;
      for (size_t i = 0; i < e.size(); i++) st |= (uint64_t)e[i] << (8 * i);
      if (st & (1ull << 63)) return 0;
      if (S.input->sequence & (1ull << 63))
        return KV_SCRIPT_UNSATISFIED_LOCKTIME;
      if ((st & 0xffffffffull) > (S.input->sequence & 0xffffffffull))
        return KV_SCRIPT_UNSATISFIED_LOCKTIME;
      return 0;
    }
    default:
      break;
  }
  /* literal pushes (unmetered) */
  if (op <= 0x4e)
    return S.push(KEnt(data, data + dlen), false);
  if (op >= 0x51 && op <= 0x60)
    return kvs_push_num(S, op - 0x50, false);
  /* signature-check family (collect/replay; GPU resolves the verdicts) */
  switch (op) {
    case 0xa9: /* OpCheckMultiSigECDSA */
      return kvs_op_multisig(S, true);
    case 0xab: /* OpCheckSigECDSA */
      return kvs_op_checksig(S, true);
    case 0xac: /* OpCheckSig */
      return kvs_op_checksig(S, false);
    case 0xad: /* OpCheckSigVerify */
      if ((rc = kvs_op_checksig(S, false))) return rc;
      return kvs_verify_top(S);
    case 0xae: /* OpCheckMultiSig */
      return kvs_op_multisig(S, false);
    case 0xaf: /* OpCheckMultiSigVerify */
      if ((rc = kvs_op_multisig(S, false))) return rc;
      return kvs_verify_top(S);
    case 0xd7: /* OpCheckSigFromStack */
      return kvs_op_checksig_from_stack(S, false);
    case 0xd8: /* OpCheckSigFromStackECDSA */
      return kvs_op_checksig_from_stack(S, true);
    case 0xd9: { /* OpBlake3 (opcodes/mod.rs:1457-1462; 1 unit/byte) */
      KEnt e;
      if ((rc = kvs_pop(S, &e))) return rc;
      if ((rc = S.consume(e.size()))) return rc;
      uint8_t h[32];
      kvs_blake3(nullptr, e.data(), e.size(), h);
      return S.push(KEnt(h, h + 32));
    }
    case 0xda: { /* OpBlake3WithKey (key exactly 32B, :1466-1476) */
      if (S.d.size() < 2) return KV_SCRIPT_INVALID_STACK_OPERATION;
      KEnt key, e;
      kvs_pop(S, &key);
      kvs_pop(S, &e);
      if (key.size() != 32) return KV_SCRIPT_MALFORMED_PUSH;
      if ((rc = S.consume(e.size()))) return rc;
      uint8_t h[32];
      kvs_blake3(key.data(), e.data(), e.size(), h);
      return S.push(KEnt(h, h + 32));
    }
    case 0xd4: { /* OpChainblockSeqCommit (KIP-21, :1389-1405) via the
                    kv_seq_commit_accessor_fn callback */
      if (!S.rctx || !S.rctx->seqc_fn)
        return KV_SCRIPT_INVALID_OPCODE; /* accessor None */
      KEnt blk;
      if ((rc = kvs_pop(S, &blk))) return rc;
      if (blk.size() != 32) return KV_SCRIPT_INVALID_STATE; /* Hash::try_from */
      uint8_t commit[32];
      if (S.rctx->seqc_fn(S.rctx->seqc_user, blk.data(), commit) != 0)
        return KV_SCRIPT_INVALID_SOURCE; /* not selected / pruned / too deep */
      return S.push(KEnt(commit, commit + 32));
    }
    case 0xa6: /* OpZkPrecompile: the engine does not decide zk proofs */
      return KVH_SCRIPT_DEFER;
    default:
      break;
  }
  /* tx introspection (KIP-10) */
  return kvs_exec_introspection(S, op);
}

/* KIP-10 introspection + covenant introspection (opcodes/mod.rs:969-1445),
 * reading the parsed HTx directly */
static int kvs_in_at(KScript &S, const HInput **out) {
  int32_t idx;
  int rc = kvs_pop_i32(S, &idx);
  if (rc) return rc;
  if (idx < 0) return KV_SCRIPT_INVALID_INDEX;
  if ((size_t)idx >= S.tx->inputs.size()) return KV_SCRIPT_INVALID_INPUT_INDEX;
  *out = &S.tx->inputs[idx];
  return 0;
}

static int kvs_out_at(KScript &S, const HOutput **out) {
  int32_t idx;
  int rc = kvs_pop_i32(S, &idx);
  if (rc) return rc;
  if (idx < 0) return KV_SCRIPT_INVALID_INDEX;
  if ((size_t)idx >= S.tx->outputs.size()) return KV_SCRIPT_INVALID_INPUT_INDEX;
  *out = &S.tx->outputs[idx];
  return 0;
}

static int kvs_push_spk(KScript &S, uint16_t version, const uint8_t *spk,
                        uint32_t len) {
  KEnt v;
  v.reserve(2 + len);
  v.push_back((uint8_t)(version & 0xff));
  v.push_back((uint8_t)(version >> 8));
  v.insert(v.end(), spk, spk + len);
  return S.push(std::move(v));
}

static int kvs_exec_introspection(KScript &S, uint8_t op) {
  int rc;
  const HTx &tx = *S.tx;
  switch (op) {
    case 0xb2:
      return kvs_push_num(S, (int64_t)tx.version);
    case 0xb3:
      return kvs_push_num(S, (int64_t)tx.inputs.size());
    case 0xb4:
      return kvs_push_num(S, (int64_t)tx.outputs.size());
    case 0xb5:
      return kvs_push_num(S, (int64_t)tx.lock_time);
    case 0xb6:
      return S.push(KEnt(tx.subnetwork_id, tx.subnetwork_id + 20));
    case 0xb7:
      return kvs_push_num(S, (int64_t)tx.gas);
    case 0xb8: { /* payload substr */
      int32_t se[2];
      if ((rc = kvs_pop_i32(S, &se[1]))) return rc;
      if ((rc = kvs_pop_i32(S, &se[0]))) return rc;
      return kvs_substr(S, tx.payload, tx.payload_len, se[0], se[1]);
    }
    case 0xb9:
      return kvs_push_num(S, (int64_t)S.idx);
    case 0xba: {
      const HInput *in2;
      if ((rc = kvs_in_at(S, &in2))) return rc;
      return S.push(KEnt(in2->prev_tx_id, in2->prev_tx_id + 32));
    }
    case 0xbb: {
      const HInput *in2;
      if ((rc = kvs_in_at(S, &in2))) return rc;
      return kvs_push_num(S, (int64_t)in2->prev_index);
    }
    case 0xbc: { /* sig-script substr */
      int32_t se[2];
      if ((rc = kvs_pop_i32(S, &se[1]))) return rc;
      if ((rc = kvs_pop_i32(S, &se[0]))) return rc;
      const HInput *in2;
      if ((rc = kvs_in_at(S, &in2))) return rc;
      return kvs_substr(S, in2->sig_script, in2->sig_script_len, se[0], se[1]);
    }
    case 0xbd: { /* sequence: raw 8B LE */
      const HInput *in2;
      if ((rc = kvs_in_at(S, &in2))) return rc;
      KEnt v(8);
      for (int i = 0; i < 8; i++) v[i] = (uint8_t)(in2->sequence >> (8 * i));
      return S.push(std::move(v));
    }
    case 0xbe: {
      const HInput *in2;
      if ((rc = kvs_in_at(S, &in2))) return rc;
      if (in2->utxo_amount > (uint64_t)INT64_MAX) return KV_SCRIPT_NUMBER_TOO_BIG;
      return kvs_push_num(S, (int64_t)in2->utxo_amount);
    }
    case 0xbf: {
      const HInput *in2;
      if ((rc = kvs_in_at(S, &in2))) return rc;
      return kvs_push_spk(S, in2->utxo_spk_version, in2->utxo_spk,
                          in2->utxo_spk_len);
    }
    case 0xc0: {
      const HInput *in2;
      if ((rc = kvs_in_at(S, &in2))) return rc;
      return kvs_push_num(S, (int64_t)in2->utxo_daa_score);
    }
    case 0xc1: {
      const HInput *in2;
      if ((rc = kvs_in_at(S, &in2))) return rc;
      return kvs_push_num(S, in2->utxo_is_coinbase ? 1 : 0);
    }
    case 0xc2: {
      const HOutput *o2;
      if ((rc = kvs_out_at(S, &o2))) return rc;
      if (o2->value > (uint64_t)INT64_MAX) return KV_SCRIPT_NUMBER_TOO_BIG;
      return kvs_push_num(S, (int64_t)o2->value);
    }
    case 0xc3: {
      const HOutput *o2;
      if ((rc = kvs_out_at(S, &o2))) return rc;
      return kvs_push_spk(S, o2->spk_version, o2->spk, o2->spk_len);
    }
    case 0xc4:
      return kvs_push_num(S, (int64_t)tx.payload_len);
    case 0xc5: {
      const HInput *in2;
      if ((rc = kvs_in_at(S, &in2))) return rc;
      return kvs_push_num(S, 2 + (int64_t)in2->utxo_spk_len);
    }
    case 0xc6: {
      int32_t se[2];
      if ((rc = kvs_pop_i32(S, &se[1]))) return rc;
      if ((rc = kvs_pop_i32(S, &se[0]))) return rc;
      const HInput *in2;
      if ((rc = kvs_in_at(S, &in2))) return rc;
      KEnt v;
      v.push_back((uint8_t)(in2->utxo_spk_version & 0xff));
      v.push_back((uint8_t)(in2->utxo_spk_version >> 8));
      v.insert(v.end(), in2->utxo_spk, in2->utxo_spk + in2->utxo_spk_len);
      return kvs_substr(S, v.data(), (uint32_t)v.size(), se[0], se[1]);
    }
    case 0xc7: {
      const HOutput *o2;
      if ((rc = kvs_out_at(S, &o2))) return rc;
      return kvs_push_num(S, 2 + (int64_t)o2->spk_len);
    }
    case 0xc8: {
      int32_t se[2];
      if ((rc = kvs_pop_i32(S, &se[1]))) return rc;
      if ((rc = kvs_pop_i32(S, &se[0]))) return rc;
      const HOutput *o2;
      if ((rc = kvs_out_at(S, &o2))) return rc;
      KEnt v;
      v.push_back((uint8_t)(o2->spk_version & 0xff));
      v.push_back((uint8_t)(o2->spk_version >> 8));
      v.insert(v.end(), o2->spk, o2->spk + o2->spk_len);
      return kvs_substr(S, v.data(), (uint32_t)v.size(), se[0], se[1]);
    }
    case 0xc9: {
      const HInput *in2;
      if ((rc = kvs_in_at(S, &in2))) return rc;
      return kvs_push_num(S, (int64_t)in2->sig_script_len);
    }
    case 0xcd: { /* num2bin */
      int32_t size;
      if ((rc = kvs_pop_i32(S, &size))) return rc;
      if (size < 0) return KV_SCRIPT_INVALID_INDEX;
      if (size > 8) return KV_SCRIPT_NOT_MINIMAL_DATA;
      int64_t v;
      if ((rc = kvs_pop_num(S, &v))) return rc;
      KEnt out;
      bool neg = v < 0;
      uint64_t mag = neg ? (uint64_t)(-(v + 1)) + 1 : (uint64_t)v;
      bool sat = false;
      while (mag) {
        out.push_back((uint8_t)(mag & 0xff));
        sat = (out.back() & 0x80) != 0;
        mag >>= 8;
      }
      if (sat) out.push_back(0);
      if (out.size() > (size_t)size) return KV_SCRIPT_NUMBER_TOO_BIG;
      out.resize(size, 0);
      if (neg) out.back() |= 0x80;
      return S.push(std::move(out));
    }
    case 0xce: { /* bin2num */
      int64_t v;
      if ((rc = kvs_pop_num(S, &v))) return rc;
      return kvs_push_num(S, v);
    }
    case 0xcb: { /* auth output count */
      int32_t ii;
      if ((rc = kvs_pop_i32(S, &ii))) return rc;
      if (ii < 0) return KV_SCRIPT_INVALID_INDEX;
      if ((size_t)ii >= tx.inputs.size()) return KV_SCRIPT_INVALID_INPUT_INDEX;
      /* input_ctxs hold continuation outputs only (covenants.rs:124-143) */
      int64_t cnt = 0;
      for (auto &o : tx.outputs)
        if (o.cov_auth_input == (uint16_t)ii && h_cov_is_continuation(tx, o)) cnt++;
      return kvs_push_num(S, cnt);
    }
    case 0xcc: { /* auth output idx */
      int32_t k, ii;
      if ((rc = kvs_pop_i32(S, &k))) return rc;
      if ((rc = kvs_pop_i32(S, &ii))) return rc;
      if (ii < 0 || k < 0) return KV_SCRIPT_INVALID_INDEX;
      if ((size_t)ii >= tx.inputs.size()) return KV_SCRIPT_INVALID_INPUT_INDEX;
      int64_t seen = 0;
      for (size_t o = 0; o < tx.outputs.size(); o++)
        if (tx.outputs[o].cov_auth_input == (uint16_t)ii &&
            h_cov_is_continuation(tx, tx.outputs[o])) {
          if (seen == k) return kvs_push_num(S, (int64_t)o);
          seen++;
        }
      return KV_SCRIPT_INVALID_SOURCE;
    }
    case 0xcf: { /* input covenant id */
      const HInput *in2;
      if ((rc = kvs_in_at(S, &in2))) return rc;
      KEnt v(32, 0);
      if (in2->utxo_has_cov) v.assign(in2->utxo_cov_id, in2->utxo_cov_id + 32);
      return S.push(std::move(v));
    }
    case 0xd0:
    case 0xd1:
    case 0xd2:
    case 0xd3: { /* covenant input/output count/idx */
      KEnt id;
      if ((rc = kvs_pop(S, &id))) return rc;
      if (id.size() != 32) return KV_SCRIPT_INVALID_STATE;
      int32_t k = 0;
      bool want_idx = op == 0xd1 || op == 0xd3;
      if (want_idx) {
        if ((rc = kvs_pop_i32(S, &k))) return rc;
        if (k < 0) return KV_SCRIPT_INVALID_INDEX;
      }
      int64_t seen = 0;
      int found = -1;
      if (op == 0xd0 || op == 0xd1) {
        for (size_t i = 0; i < tx.inputs.size(); i++)
          if (tx.inputs[i].utxo_has_cov &&
              !memcmp(tx.inputs[i].utxo_cov_id, id.data(), 32)) {
            if (want_idx && seen == k) found = (int)i;
            seen++;
          }
      } else { /* shared_ctxs list continuation outputs only */
        for (size_t o = 0; o < tx.outputs.size(); o++)
          if (h_cov_is_continuation(tx, tx.outputs[o]) &&
              !memcmp(tx.outputs[o].cov_id, id.data(), 32)) {
            if (want_idx && seen == k) found = (int)o;
            seen++;
          }
      }
      if (!want_idx) return kvs_push_num(S, seen);
      if (found < 0) return KV_SCRIPT_INVALID_SOURCE;
      return kvs_push_num(S, (int64_t)found);
    }
    case 0xd5: { /* output covenant id */
      const HOutput *o2;
      if ((rc = kvs_out_at(S, &o2))) return rc;
      KEnt v(32, 0);
      if (o2->has_covenant) v.assign(o2->cov_id, o2->cov_id + 32);
      return S.push(std::move(v));
    }
    case 0xd6: { /* output authorizing input (-1 without covenant) */
      const HOutput *o2;
      if ((rc = kvs_out_at(S, &o2))) return rc;
      return kvs_push_num(S, o2->has_covenant ? (int64_t)o2->cov_auth_input
                                              : -1);
    }
    default:
      return KV_SCRIPT_INVALID_OPCODE; /* 0xca, 0xdb..0xff */
  }
}

/* final / intermediate result check (lib.rs:726-744): the stack must hold a
 * truthy top; at the END, exactly one element (CleanStack) */
static int kvs_check_result(KScript &S, bool final_check) {
  if (final_check && S.d.size() > 1) return KV_SCRIPT_CLEAN_STACK;
  if (S.d.empty()) return KV_SCRIPT_EMPTY_STACK;
  bool ok = kvs_bool(S.d.back());
  S.d.pop_back();
  return ok ? 0 : KV_SCRIPT_EVAL_FALSE;
}

/* Run the full [sig_script, spk(, p2sh redeem)] engine for one input
 * (⇔ TxScriptEngine::execute, lib.rs:653-760). Returns 0 / KV_SCRIPT_* /
 * KVH_SCRIPT_SUSPEND (sig site collected into rctx->pending — resolve and
 * re-run with the status vector appended to rctx->memo) / KVH_SCRIPT_DEFER
 * (zk precompile; or a sig site reached with no collect context). */
static int kvh_run_input_script(const HTx &tx, const HInput &in, uint32_t idx,
                                uint64_t sigop_units,
                                const KvsRunCtx *rctx = nullptr) {
  KScript S;
  S.tx = &tx;
  S.input = &in;
  S.idx = idx;
  S.rctx = rctx;
  S.sigop_units = sigop_units;
  uint64_t committed = in.commit_kind == 0
                           ? (uint64_t)in.commit_value * KVS_UNITS_PER_SIGOP_COUNT
                           : (uint64_t)in.commit_value * KVS_UNITS_PER_BUDGET;
  uint64_t limit = committed + KVS_FREE_UNITS;
  if (limit < committed) limit = UINT64_MAX;
  S.remaining = limit;

  if (in.utxo_spk_version > 0) return 0; /* unknown version accepted */
  bool is_p2sh = in.utxo_spk_len == 35 && in.utxo_spk[0] == 0xaa &&
                 in.utxo_spk[1] == 0x20 && in.utxo_spk[34] == 0x87;
  uint64_t extra = in.utxo_spk_len > 35 ? (uint64_t)(in.utxo_spk_len - 35) : 0;
  int rc = S.consume(extra * 100);
  if (rc) return rc;
  if (in.sig_script_len == 0 && in.utxo_spk_len == 0)
    return KV_SCRIPT_EVAL_FALSE;
  if (in.sig_script_len > KVS_MAX_SCRIPTS_SIZE ||
      in.utxo_spk_len > KVS_MAX_SCRIPTS_SIZE)
    return KV_SCRIPT_SCRIPT_SIZE;

  std::vector<KEnt> saved;
  bool have_saved = false;
  const uint8_t *scripts[2] = {in.sig_script, in.utxo_spk};
  uint32_t lens[2] = {in.sig_script_len, in.utxo_spk_len};
  for (int i = 0; i < 2; i++) {
    if (lens[i] == 0) continue;
    if (is_p2sh && i == 1) {
      saved = S.d;
      have_saved = true;
    }
    rc = kvs_run_one_script(S, scripts[i], lens[i], i == 0);
    if (rc) return rc;
  }
  if (is_p2sh) {
    rc = kvs_check_result(S, false);
    if (rc) return rc;
    if (!have_saved) return KV_SCRIPT_EMPTY_STACK;
    S.d = std::move(saved);
    if (S.d.empty()) return KV_SCRIPT_EMPTY_STACK;
    KEnt redeem = std::move(S.d.back());
    S.d.pop_back();
    rc = kvs_run_one_script(S, redeem.data(), (uint32_t)redeem.size(), false);
    if (rc) return rc;
  }
  return kvs_check_result(S, true);
}

} // namespace kvhost
