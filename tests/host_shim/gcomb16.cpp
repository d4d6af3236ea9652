/* Host shim for the joint 16-bit fixed-base table (test_gcomb16_host.py): the
 * per-entry build routine, the unpack, the H multiples the host accessor
 * derives from KV_G_TABLE8, and ecmult_double on top of them. It sits on
 * main.cpp so the device sources compile exactly as they do there
 * (KV_HOST_TEST on: magnitude asserts live) and host_init_gtable is shared. */
#include "main.cpp"

static void put26c(uint32_t *out, kv::fe26 v) {
  kv::fe26_normalize(v);
  for (int i = 0; i < 10; i++) out[i] = v.l[i];
}

/* raw: the entry's 16 packed words, built by the init kernel's per-entry
 * routine. xy: the unpack of those words, limbs AS UNPACKED (no normalise, so
 * the test sees the magnitude-1 claim). Returns 0, or -1 for a bad index. */
extern "C" int host_g16_entry(uint32_t idx, uint32_t raw[16], uint32_t xy[20]) {
  if (idx >= KV_G_JOINT_ENTRIES) return -1;
  kv::ge e;
  kv::g16_fetch(e, 1); /* makes the accessor derive the H multiples */
  kv::g16_entry t;
  kv::g16_build_entry(t, idx, kv::KV_G_TABLE8, kv::KV_H_TABLE8);
  for (int i = 0; i < 16; i++) raw[i] = t.w[i];
  kv::g16_unpack(e, t);
  for (int i = 0; i < 10; i++) {
    xy[i] = e.x.l[i];
    xy[10 + i] = e.y.l[i];
  }
  /* the ladder's own accessor must hand out the same point */
  kv::ge f;
  kv::g16_fetch(f, idx);
  for (int i = 0; i < 10; i++)
    if (f.x.l[i] != e.x.l[i] || f.y.l[i] != e.y.l[i]) return -2;
  return 0;
}

/* out: 256 entries of (x, y) limbs as stored; entry 0 is H itself */
extern "C" int host_h_table(uint32_t *out) {
  kv::ge e;
  kv::g16_fetch(e, 1);
  for (int k = 0; k < 256; k++)
    for (int i = 0; i < 10; i++) {
      out[20 * k + i] = kv::KV_H_TABLE8[k].x.l[i];
      out[20 * k + 10 + i] = kv::KV_H_TABLE8[k].y.l[i];
    }
  return 256;
}

/* R = gs·G + ps·P as canonical Jacobian (X, Y, Z) limbs; returns 1 if R is
 * infinity by the kernel's own test */
extern "C" int host_g16_ecmult_double(const uint64_t gs[4], const uint64_t ps[4],
                                      const uint32_t px[10],
                                      const uint32_t py[10], uint32_t out[30]) {
  kv::sc g, p;
  memcpy(g.d, gs, 32);
  memcpy(p.d, ps, 32);
  kv::ge P;
  for (int i = 0; i < 10; i++) {
    P.x.l[i] = px[i];
    P.y.l[i] = py[i];
  }
  kv::gej R;
  kv::ecmult_double(R, g, p, P);
  int inf = kv::gej_is_infinity(R);
  put26c(out, R.x);
  put26c(out + 10, R.y);
  put26c(out + 20, R.z);
  return inf;
}

/* 1 when the ladder was compiled with the joint table (the default) */
extern "C" int host_g16_joint_ladder(void) {
#ifdef KV_G_JOINT_LADDER
  return 1;
#else
  return 0;
#endif
}
