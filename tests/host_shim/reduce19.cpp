/* Host shim for fe26_reduce19 on RAW column sums
 * (test_fe26_reduce_columns_host.py). The device header compiles as it does
 * for the other shims (KV_HOST_TEST on: the precondition and every bound of
 * the reduction's header comment are asserted). With KV_REDUCE19_MAIN it is a
 * stand-alone program that checks the same edge columns and a random sweep
 * against a plain wide-integer reference, for runs under host sanitizers. */
#include "shim.h"
#include "kv_secp_device.h"

extern "C" void host_fe26_reduce19(const uint64_t t[19], uint32_t r[10]) {
  kv::fe26 fr;
  kv::fe26_reduce19(fr, t);
  for (int i = 0; i < 10; i++) r[i] = fr.l[i];
}

#ifdef KV_REDUCE19_MAIN
#include <stdio.h>

typedef unsigned __int128 u128;

static uint64_t cap(int k) { return (uint64_t)(k < 10 ? k + 1 : 19 - k) << 60; }

/* reference: digits of sum t[k]*2^(26k), high digits folded by
 * 2^260 == 0x3D10 + 2^36 until none is left, then the canonical form */
static void reference(const uint64_t t[19], uint32_t out[10]) {
  u128 d[24];
  for (int k = 0; k < 24; k++) d[k] = k < 19 ? t[k] : 0;
  for (;;) {
    u128 c = 0;
    for (int k = 0; k < 24; k++) {
      u128 v = d[k] + c;
      d[k] = v & 0x3FFFFFF;
      c = v >> 26;
    }
    bool high = false;
    for (int k = 10; k < 24; k++) high |= d[k] != 0;
    if (!high) break;
    for (int k = 10; k < 24; k++) {
      d[k - 10] += d[k] * 0x3D10;
      d[k - 9] += d[k] << 10;
      d[k] = 0;
    }
  }
  kv::fe26 f;
  for (int i = 0; i < 10; i++) f.l[i] = (uint32_t)d[i];
  kv::fe26_normalize(f);
  for (int i = 0; i < 10; i++) out[i] = f.l[i];
}

static int check(const uint64_t t[19]) {
  uint32_t r[10], want[10];
  host_fe26_reduce19(t, r);
  for (int i = 0; i < 9; i++)
    if (r[i] > (1u << 26)) return 1;
  if (r[9] >= (1u << 22)) return 1;
  kv::fe26 f;
  for (int i = 0; i < 10; i++) f.l[i] = r[i];
  kv::fe26_normalize(f);
  reference(t, want);
  for (int i = 0; i < 10; i++)
    if (f.l[i] != want[i]) return 1;
  return 0;
}

int main() {
  uint64_t t[19];
  int bad = 0, n = 0;
  for (int k = 0; k < 19; k++)
    for (int one = 0; one < 2; one++) {
      for (int i = 0; i < 19; i++) t[i] = 0;
      t[k] = one ? 1 : cap(k);
      bad += check(t), n++;
    }
  for (int i = 0; i < 19; i++) t[i] = cap(i);
  bad += check(t), n++;
  for (int i = 0; i < 19; i++) t[i] = (cap(i) - ((uint64_t)1 << 32)) | 0xFFFFFFFFu;
  bad += check(t), n++;
  for (int i = 0; i < 19; i++) t[i] = cap(i) & ~(uint64_t)0xFFFFFFFFu;
  bad += check(t), n++;
  uint64_t x = 0x9E3779B97F4A7C15ULL;
  for (int it = 0; it < 20000; it++) {
    for (int i = 0; i < 19; i++) {
      x ^= x << 13, x ^= x >> 7, x ^= x << 17;
      t[i] = x % (cap(i) + 1);
    }
    bad += check(t), n++;
  }
  printf("reduce19: %d cases, %d bad\n", n, bad);
  return bad != 0;
}
#endif
