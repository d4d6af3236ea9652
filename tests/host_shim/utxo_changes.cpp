/* Host shim for the functions of kv_utxo_changes_kernels.hip that need no wave
 * intrinsics and no slot type (test_utxo_changes_host.py): utxo_change_locate,
 * the change-index mapping, and utxo_change_pack, the 96-byte record. g++
 * compiles them under KV_HOST_TEST, which drops the kernel. With
 * KV_UTXO_CHANGES_MAIN it is a stand-alone program that runs the same kinds of
 * cases against a restatement written here, for runs under host sanitizers:
 * keys, values and records are heap blocks of exactly 36, 64 and 96 bytes, so
 * a read or write past any of them is caught. */
#include "shim.h"
#include "kv_utxo_changes_kernels.hip"

/* out3: row, live, removed */
extern "C" void host_utxo_change_locate(uint64_t c, uint64_t n_removed, uint32_t flags,
                                        uint64_t *out3) {
  kv::utxo_change_loc loc = kv::utxo_change_locate(c, n_removed, flags);
  out3[0] = loc.row;
  out3[1] = (uint64_t)loc.live;
  out3[2] = (uint64_t)loc.removed;
}

extern "C" void host_utxo_change_pack(const uint8_t *op36, const uint8_t *val64,
                                      uint32_t query_index, int removed,
                                      uint8_t *out96) {
  uint32_t key[9], val[16], out[24];
  memcpy(key, op36, 36);
  memcpy(val, val64, 64);
  kv::utxo_change_pack(out, key, val, query_index, removed);
  memcpy(out96, out, 96);
}

#ifdef KV_UTXO_CHANGES_MAIN
#include <stdio.h>
#include <stdlib.h>

static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
static uint64_t rnd() {
  rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
  return rng_state;
}

/* a packed 64-byte table value with random amount, daa score, script field
 * and tail; heap block of exactly 64 bytes */
static uint8_t *value(uint16_t flags, uint16_t version, uint32_t len) {
  uint8_t *v = (uint8_t *)malloc(64);
  for (int i = 0; i < 64; i++) v[i] = (uint8_t)rnd();
  memcpy(v + 16, &flags, 2);
  memcpy(v + 18, &version, 2);
  memcpy(v + 20, &len, 4);
  return v;
}

/* the record, restated byte by byte */
static void want_record(const uint8_t *op, const uint8_t *v, uint32_t qi, int removed,
                        uint8_t *out) {
  memset(out, 0, 96);
  memcpy(out, op, 36);
  memcpy(out + 36, &qi, 4);
  memcpy(out + 40, v, 16);
  uint16_t flags;
  memcpy(&flags, v + 16, 2);
  uint16_t f = (uint16_t)((flags & (KV_UTXO_F_COINBASE | KV_UTXO_F_COVENANT)) |
                          (removed ? KV_UTXO_CHANGE_F_REMOVED : 0));
  memcpy(out + 56, &f, 2);
  memcpy(out + 58, v + 18, 2);
  memcpy(out + 60, v + 20, 4);
  if (flags & KV_UTXO_F_COVENANT) memcpy(out + 64, v + 28, 32);
}

int main() {
  int bad = 0, n = 0;
  const uint64_t sizes[] = {0, 1, 2, 63, 64, 65};
  for (uint64_t nr : sizes)
    for (uint64_t na : sizes)
      for (uint32_t flags = 0; flags < 4; flags++) {
        const int rev = flags & KV_UTXO_CHANGES_REVERSED;
        uint64_t c = 0, out[3];
        for (uint64_t i = 0; i < nr; i++, c++, n++) {
          host_utxo_change_locate(c, nr, flags, out);
          bad += out[0] != i || out[1] != 0 || out[2] != (uint64_t)!rev;
        }
        for (uint64_t k = 0; k < na; k++)
          for (int live = 0; live < 2; live++, c++, n++) {
            host_utxo_change_locate(c, nr, flags, out);
            bad += out[0] != nr + k || out[1] != (uint64_t)live ||
                   out[2] != (uint64_t)(live ? rev != 0 : !rev);
          }
        bad += c != nr + 2 * na, n++;
      }

  struct {
    uint16_t flags;
    uint32_t len;
  } cases[] = {{0, 0}, {0, 1}, {0, 35}, {0, 36}, {KV_UTXO_F_COINBASE, 34},
               {KV_UTXO_F_SPK_ARENA, 37}, {KV_UTXO_F_SPK_ARENA, 10000},
               {KV_UTXO_F_SPK_ARENA | KV_UTXO_F_COVENANT, 5},
               {KV_UTXO_F_SPK_ARENA | KV_UTXO_F_COVENANT | KV_UTXO_F_COINBASE, 0}};
  for (auto &cs : cases)
    for (int removed = 0; removed < 2; removed++)
      for (int q = 0; q < 4; q++) {
        const uint32_t qis[4] = {0u, 7u, 65535u, 0xffffffffu}, qi = qis[q];
        uint8_t *op = (uint8_t *)malloc(36), *got = (uint8_t *)malloc(96), want[96];
        for (int i = 0; i < 36; i++) op[i] = (uint8_t)rnd();
        uint8_t *v = value(cs.flags, (uint16_t)rnd(), cs.len);
        memset(got, 0xa5, 96);
        host_utxo_change_pack(op, v, qi, removed, got);
        want_record(op, v, qi, removed, want);
        bad += memcmp(got, want, 96) != 0, n++;
        free(op), free(got), free(v);
      }
  printf("utxo_changes: %d cases, %d bad\n", n, bad);
  return bad != 0;
}
#endif
