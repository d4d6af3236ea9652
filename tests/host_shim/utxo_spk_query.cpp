/* Host shim for the script-public-key query functions of
 * kv_utxo_query_kernels.hip (test_utxo_spk_query_host.py): spk_hash,
 * spk_query_check, spk_query_build and spk_query_match compile with g++
 * (KV_HOST_TEST drops the kernels, which need wave intrinsics and the table's
 * slot type). With KV_SPK_HASH_CONST every script hash is equal and every
 * result must stay what it was. With KV_SPK_QUERY_MAIN it is a stand-alone
 * program that runs the same kinds of cases against a linear search, for runs
 * under host sanitizers: the arena is a heap block of exactly arena_len bytes,
 * so a read past a script, or through a bad reference, is caught. */
#include "shim.h"
#include "kv_utxo_commit_kernels.hip"
#include "kv_utxo_query_kernels.hip"

extern "C" uint32_t host_spk_query_slots(size_t n_q) { return kv::spk_query_slots(n_q); }

extern "C" uint64_t host_spk_hash(uint16_t version, uint32_t len, const uint8_t *spk) {
  return kv::spk_hash(version, len, spk);
}

extern "C" int host_spk_query_check(const kv_spk_query *q, size_t n_q, size_t blob_len) {
  return kv::spk_query_check(q, n_q, blob_len);
}

extern "C" int host_spk_query_build(const kv_spk_query *q, size_t n_q,
                                    const uint8_t *blob, uint32_t *off, uint64_t *hash,
                                    uint32_t *qidx, uint32_t slots) {
  return kv::spk_query_build(q, n_q, blob, off, hash, qidx, slots);
}

extern "C" int32_t host_spk_query_match(const uint8_t *val64, const uint8_t *arena,
                                        uint64_t arena_len, const uint64_t *hash,
                                        const uint32_t *qidx, const kv_spk_query *q,
                                        const uint32_t *off, const uint8_t *blob,
                                        uint32_t slots, uint32_t n_q) {
  kv::spk_query_set S = {hash, qidx, q, off, blob, slots - 1, n_q};
  return kv::spk_query_match(val64, arena, arena_len, S);
}

#ifdef KV_SPK_QUERY_MAIN
#include <stdio.h>
#include <stdlib.h>
#include <vector>

typedef std::vector<uint8_t> bytes;

static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
static uint64_t rnd() {
  rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
  return rng_state;
}
static bytes rand_bytes(size_t n) {
  bytes b(n);
  for (auto &x : b) x = (uint8_t)rnd();
  return b;
}

struct Script {
  uint16_t version;
  bytes spk;
  bool operator==(const Script &o) const {
    return version == o.version && spk == o.spk;
  }
};

struct Entry {
  Script s;
  bool covenant;
  uint8_t val[64];
};

/* the packed table value of an entry; arena scripts are appended to `arena`
 * behind a few unrelated bytes, so offsets are odd */
static void pack(Entry &e, bytes &arena) {
  uint64_t amount = rnd(), daa = rnd();
  uint16_t flags = 0;
  uint32_t len = (uint32_t)e.s.spk.size();
  memset(e.val, 0, 64);
  if (e.covenant || len > 36) {
    flags |= KV_UTXO_F_SPK_ARENA;
    if (e.covenant) flags |= KV_UTXO_F_COVENANT;
    for (int i = 0; i < 3; i++) arena.push_back((uint8_t)rnd());
    uint32_t off = (uint32_t)arena.size();
    arena.insert(arena.end(), e.s.spk.begin(), e.s.spk.end());
    memcpy(e.val + 24, &off, 4);
    if (e.covenant)
      for (int i = 28; i < 60; i++) e.val[i] = (uint8_t)rnd();
  } else if (len) {
    memcpy(e.val + 24, e.s.spk.data(), len);
  }
  memcpy(e.val, &amount, 8);
  memcpy(e.val + 8, &daa, 8);
  memcpy(e.val + 16, &flags, 2);
  memcpy(e.val + 18, &e.s.version, 2);
  memcpy(e.val + 20, &len, 4);
}

struct Table {
  std::vector<kv_spk_query> q;
  bytes blob;
  std::vector<uint32_t> off, qidx;
  std::vector<uint64_t> hash;
  uint32_t slots;
  int build_rc;
};

static Table build(const std::vector<Script> &qs) {
  Table t;
  for (auto &s : qs) {
    t.q.push_back(kv_spk_query{(uint32_t)s.spk.size(), s.version, 0});
    t.blob.insert(t.blob.end(), s.spk.begin(), s.spk.end());
  }
  t.slots = kv::spk_query_slots(qs.size());
  t.off.resize(qs.size() + 1);
  t.qidx.resize(t.slots);
  t.hash.resize(t.slots);
  t.build_rc = host_spk_query_check(t.q.data(), qs.size(), t.blob.size());
  if (t.build_rc == 0)
    t.build_rc = host_spk_query_build(t.q.data(), qs.size(), t.blob.data(),
                                      t.off.data(), t.hash.data(), t.qidx.data(),
                                      t.slots);
  return t;
}

static int32_t match(const Table &t, const uint8_t *val, const uint8_t *arena,
                     uint64_t arena_len) {
  return host_spk_query_match(val, arena, arena_len, t.hash.data(), t.qidx.data(),
                              t.q.data(), t.off.data(), t.blob.data(), t.slots,
                              (uint32_t)t.q.size());
}

int main() {
  int bad = 0, n = 0;
  std::vector<Entry> entries;
  const size_t lens[] = {0, 1, 35, 36, 37, 64, 200, 10000};
  for (size_t len : lens) entries.push_back(Entry{{0, rand_bytes(len)}, false, {}});
  entries.push_back(Entry{{1, entries[2].s.spk}, false, {}}); /* version only */
  entries.push_back(Entry{{0, bytes{'a', 'b', 'c'}}, false, {}});
  entries.push_back(Entry{{0, bytes{'a', 'b', 'c', 0}}, false, {}});
  bytes longer = entries[3].s.spk; /* 37 bytes sharing the inline 36 */
  longer.push_back(7);
  entries.push_back(Entry{{0, longer}, false, {}});
  entries.push_back(Entry{{0, rand_bytes(20)}, true, {}}); /* covenant, arena */
  entries.push_back(Entry{{0, bytes{}}, true, {}});        /* covenant, empty */
  bytes arena_v;
  for (auto &e : entries) pack(e, arena_v);
  const uint64_t arena_len = arena_v.size();
  uint8_t *arena = (uint8_t *)malloc(arena_len); /* exactly arena_len bytes */
  memcpy(arena, arena_v.data(), arena_len);

  const size_t counts[] = {0, 1, 2, 3, 64, 1000};
  for (size_t n_q : counts) {
    std::vector<Script> qs;
    for (size_t i = 0; qs.size() < n_q; i++) {
      Script s;
      if (i < entries.size() && i % 3 != 2) {
        s = entries[i].s; /* present */
      } else if (i < 2 * entries.size()) {
        s = entries[i % entries.size()].s; /* a near miss of a present one */
        if (i % 2 && !s.spk.empty()) s.spk.back() ^= 1;
        else s.version += 2;
      } else {
        s = Script{(uint16_t)(rnd() % 3), rand_bytes(rnd() % 70)};
      }
      bool dup = false;
      for (auto &o : qs) dup |= o == s;
      if (!dup) qs.push_back(s);
    }
    Table t = build(qs);
    bad += t.build_rc != 0, n++;
    for (auto &e : entries) {
      int32_t want = KV_SPK_MATCH_NONE;
      for (size_t i = 0; i < qs.size(); i++)
        if (qs[i] == e.s) want = (int32_t)i;
      bad += match(t, e.val, arena, arena_len) != want, n++;
    }
  }

  /* the duplicate detector */
  Script a{0, rand_bytes(34)}, b = a, c = a;
  b.spk[33] ^= 0x80;
  c.version = 1;
  bad += build({a, b, c, entries[9].s, entries[10].s}).build_rc != 0, n++;
  bad += build({a, b, a}).build_rc != 1, n++;
  bad += build({entries[0].s, a, entries[0].s}).build_rc != 1, n++; /* two empty */
  bad += build({entries[7].s, entries[7].s}).build_rc != 1, n++;    /* 10,000 B */

  /* the argument rules */
  kv_spk_query one{KV_UTXO_MAX_SPK + 1, 0, 0};
  bad += host_spk_query_check(&one, 1, KV_UTXO_MAX_SPK + 1) != -1, n++;
  one = kv_spk_query{3, 0, 1};
  bad += host_spk_query_check(&one, 1, 3) != -1, n++;
  one = kv_spk_query{3, 0, 0};
  bad += host_spk_query_check(&one, 1, 4) != -1, n++;
  bad += host_spk_query_check(&one, 1, 3) != 0, n++;
  bad += host_spk_query_check(nullptr, 0, 0) != 0, n++;
  bad += host_spk_query_check(nullptr, (size_t)KV_UTXO_QUERY_MAX + 1, 0) != -1, n++;

  /* bad script references are reported, never followed */
  Table t = build({entries[6].s, entries[1].s});
  uint8_t val[64];
  memcpy(val, entries[6].val, 64); /* 200 bytes in the arena */
  uint32_t off = (uint32_t)arena_len - 199;
  memcpy(val + 24, &off, 4);
  bad += match(t, val, arena, arena_len) != KV_SPK_MATCH_BAD, n++;
  off = 0xfffffff0u;
  memcpy(val + 24, &off, 4);
  bad += match(t, val, arena, arena_len) != KV_SPK_MATCH_BAD, n++;
  bad += match(t, entries[6].val, arena, 0) != KV_SPK_MATCH_BAD, n++;
  off = (uint32_t)arena_len - 200; /* the last 200 bytes: in range, no match */
  memcpy(val + 24, &off, 4);
  bad += match(t, val, arena, arena_len) != KV_SPK_MATCH_NONE, n++;
  memcpy(val, entries[1].val, 64);
  uint32_t len = 37; /* inline, but longer than the field */
  memcpy(val + 20, &len, 4);
  bad += match(t, val, arena, arena_len) != KV_SPK_MATCH_BAD, n++;
  memcpy(val, entries[1].val, 64);
  uint16_t flags = KV_UTXO_F_COVENANT; /* a covenant id where the script would be */
  memcpy(val + 16, &flags, 2);
  bad += match(t, val, arena, arena_len) != KV_SPK_MATCH_BAD, n++;
  /* ... also with no query at all */
  bad += match(build({}), val, arena, arena_len) != KV_SPK_MATCH_BAD, n++;
  bad += match(build({}), entries[1].val, arena, arena_len) != KV_SPK_MATCH_NONE, n++;

  free(arena);
  printf("spk_query: %d cases, %d bad\n", n, bad);
  return bad != 0;
}
#endif
