/* Host shim for the engine's U3072 arithmetic (test_u3072_host.py): exposes
 * u3072_mulmod and u3072_canon from kv_u3072.h, compiled with g++. The header
 * is plain C++ off the HIP compiler, so nothing is stubbed. */
#include "kv_u3072.h"

extern "C" void host_u3072_mulmod(const uint64_t *a48, const uint64_t *b48,
                                  uint64_t *r48) {
  kv::u3072 a, b, r;
  memcpy(a.l, a48, sizeof(a.l));
  memcpy(b.l, b48, sizeof(b.l));
  kv::u3072_mulmod(r, a, b);
  memcpy(r48, r.l, sizeof(r.l));
}

extern "C" void host_u3072_canon(uint64_t *a48) {
  kv::u3072 a;
  memcpy(a.l, a48, sizeof(a.l));
  kv::u3072_canon(a);
  memcpy(a48, a.l, sizeof(a.l));
}
