/* Host shim for the verify ladder's building blocks (test_ladder_host.py):
 * the zero predicate, the inversion-free P table and ecmult_double. It sits on
 * top of main.cpp so the device sources compile exactly as they do there
 * (KV_HOST_TEST on: magnitude asserts live) and host_init_gtable is shared. */
#include "main.cpp"

static void put26(uint32_t *out, kv::fe26 v) {
  kv::fe26_normalize(v);
  for (int i = 0; i < 10; i++) out[i] = v.l[i];
}

static kv::fe26 get26(const uint32_t *in) {
  kv::fe26 v;
  for (int i = 0; i < 10; i++) v.l[i] = in[i];
  return v;
}

extern "C" int host_fe26_normalizes_to_zero(const uint32_t a[10]) {
  return kv::fe26_normalizes_to_zero(get26(a));
}

/* out: KV_PTAB_MAX entries of (x, y), canonical limbs; zg: canonical limbs */
extern "C" int host_ptab_build(const uint32_t px[10], const uint32_t py[10],
                               uint32_t *out, uint32_t zg_out[10]) {
  kv::ge P;
  P.x = get26(px);
  P.y = get26(py);
  kv::ge ptab[KV_PTAB_MAX + 1];
  kv::ladder_consts lc;
  kv::fe26 zg;
  kv::ecmult_ptab_build(ptab, lc, zg, P);
  for (int k = 1; k <= KV_PTAB_MAX; k++) {
    /* magnitude discipline: table entries stay <= 2 */
    for (int i = 0; i < 10; i++) {
      if (ptab[k].x.l[i] > 2 * (1u << 26) || ptab[k].y.l[i] > 2 * (1u << 26))
        return -1;
    }
    put26(out + 20 * (k - 1), ptab[k].x);
    put26(out + 20 * (k - 1) + 10, ptab[k].y);
  }
  put26(zg_out, zg);
  return KV_PTAB_MAX;
}

/* R = gs·G + ps·P as canonical Jacobian (X, Y, Z) limbs; returns 1 if R is
 * infinity by the kernel's own test */
extern "C" int host_ecmult_double(const uint64_t gs[4], const uint64_t ps[4],
                                  const uint32_t px[10], const uint32_t py[10],
                                  uint32_t out[30]) {
  kv::sc g, p;
  memcpy(g.d, gs, 32);
  memcpy(p.d, ps, 32);
  kv::ge P;
  P.x = get26(px);
  P.y = get26(py);
  kv::gej R;
  kv::ecmult_double(R, g, p, P);
  int inf = kv::gej_is_infinity(R);
  put26(out, R.x);
  put26(out + 10, R.y);
  put26(out + 20, R.z);
  return inf;
}
