/* MI355X-native batched signature verification kernels (gfx950, PRODUCT code).
 *
 * kv_schnorr_verify_kernel ⇔ secp256k1::schnorr::Signature::verify at
 *   crypto/txscript/src/lib.rs:869 (BIP-340), one signature per lane.
 * kv_ecdsa_verify_kernel   ⇔ secp256k1::ecdsa::Signature::verify at
 *   crypto/txscript/src/lib.rs:899 (low-S enforced like libsecp256k1).
 *
 * Layout: tuples are 128B (Schnorr: r‖s‖pk_x‖msg) / 129B-padded-to-132
 * (ECDSA: r‖s‖pk33‖msg, see engine) records in HBM; loads are a handful of
 * dwordx4 per lane against ~5k 256-bit field multiplies of ALU work — this
 * kernel is integer-ALU bound by ~300 ops/byte, so layout
 * matters far less than VGPR pressure and carry-chain depth.
 *
 * Verdicts are wave-ballot-compressed: each 64-lane wave writes one u64 of the
 * bitmap with a single store (no atomics).
 */
#include "kv_hash_device.h"
#include "kv_secp_device.h"

namespace kv {

/* SHA-256 midstate after compressing tag_hash‖tag_hash for
 * tag = "BIP0340/challenge" (fixed by BIP-340; precomputed, verified against a
 * full SHA-256 at build time in tests). */
__device__ __constant__ static const uint32_t BIP340_CHALLENGE_MID[8] = {
    0x9cecba11u, 0x23925381u, 0x11679112u, 0xd1627e0fu,
    0x97c87550u, 0x003cc765u, 0x90f61164u, 0x33e9b66au};

/* status codes (engine-internal, align with KV_SCRIPT_* mapping in host) */
enum : uint8_t {
  KVS_VALID = 0,
  KVS_INVALID = 1,
  KVS_BAD_PUBKEY = 2,
  KVS_BAD_SIG = 3,
};

__device__ __forceinline__ void fe_from_be(fe &r, const uint8_t b[32]) {
#pragma unroll
  for (int i = 0; i < 4; i++) {
    u64 w = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) w = (w << 8) | b[8 * (3 - i) + j];
    r.n[i] = w;
  }
}

__device__ __forceinline__ int fe_gte_p_full(const fe &a) {
  return (a.n[3] == KV_P1) & (a.n[2] == KV_P1) & (a.n[1] == KV_P1) &
         (a.n[0] >= KV_P0);
}

/* lift x (BE bytes) to an affine point with chosen y parity; 0 on failure.
 * The >= p overflow check runs on the exact 4xu64 form; the curve equation
 * and sqrt run on fe26. */
__device__ inline int lift_x_parity(ge &P, const uint8_t xb[32], u32 want_odd) {
  fe xu;
  fe_from_be(xu, xb);
  if (fe_gte_p_full(xu)) return 0;
  fe26 x, x3, y2, y;
  fe26_from_fe(x, xu);
  fe26_sqr(x3, x);
  fe26_mul(x3, x3, x);
  fe26 seven;
  fe26_set_int(seven, 7);
  fe26_add(y2, x3, seven);
  if (!fe26_sqrt(y, y2)) return 0;
  fe26_normalize(y);
  fe26 ny;
  fe26_neg(ny, y, 1);
  fe26_cmov(y, ny, (y.l[0] & 1) ^ want_odd);
  P.x = x;
  P.y = y; /* magnitude <= 2 */
  return 1;
}

__device__ inline int lift_x_even(ge &P, const uint8_t xb[32]) {
  return lift_x_parity(P, xb, 0);
}

/* parse 33-byte compressed pubkey; 0 on failure */
__device__ inline int parse_compressed(ge &P, const uint8_t pk[33]) {
  if (pk[0] != 0x02 && pk[0] != 0x03) return 0;
  return lift_x_parity(P, pk + 1, pk[0] == 0x03);
}

/* affine G (4xu64 limbs; converted to fe26 once in the table-init kernel) */
__device__ __constant__ static const u64 GE_G_X[4] = {
    0x59F2815B16F81798ULL, 0x029BFCDB2DCE28D9ULL, 0x55A06295CE870B07ULL,
    0x79BE667EF9DCBBACULL};
__device__ __constant__ static const u64 GE_G_Y[4] = {
    0x9C47D08FFB10D4B8ULL, 0xFD17B448A6855419ULL, 0x5DA4FBFC0E1108A8ULL,
    0x483ADA7726A3C465ULL};

/* 8-bit fixed-base tables: KV_G_TABLE8[d] = d·G and KV_H_TABLE8[d] = d·H with
 * H = 2^128·G, d = 1..255 (entry 0 = the base point, never selected as a
 * digit). They are the inputs of the joint table below; under -DKV_NO_G_JOINT
 * the ladder's G/φG streams read KV_G_TABLE8 directly. */
__device__ ge KV_G_TABLE8[256];
__device__ ge KV_H_TABLE8[256];
__device__ static fe26 KV_G8_X[256];    /* init-time scratch */
__device__ static fe26 KV_G8_Y[256];    /* init-time scratch */
__device__ static fe26 KV_G8_Z[256];    /* init-time scratch */
__device__ static fe26 KV_G8_PREF[256]; /* init-time scratch */

/* Joint 16-bit fixed-base table: KV_G_JOINT[hi << 8 | lo] = lo·G + hi·H.
 * G is FIXED, so its scalar needs no GLV split: s = s_lo + 2^128·s_hi (a plain
 * bit split), and byte j of s_lo with byte j of s_hi select ONE entry whose add
 * lands on 4-bit window 2j — 16 mixed adds per verify where the two 8-bit
 * G/φG streams took 34. lo == 0 or hi == 0 gives the other term alone; entry 0
 * is G (discarded by the digit-0 cmov, but a well-formed point).
 *
 * An entry is the affine point as canonical 256-bit x then y, 8 little-endian
 * u32 words each: 64 bytes, 64-byte aligned, so one entry is one half of a
 * 128-byte line and the whole table is 4 MiB (one XCD's L2; far inside the
 * Infinity Cache). The 80-byte ge layout would save the unpack's ~40 shifts
 * and masks per add against 25% more lines touched and entries that straddle
 * lines; the packed form was kept. */
struct alignas(64) g16_entry {
  u32 w[16];
};
#define KV_G_JOINT_ENTRIES 65536u
#ifndef KV_HOST_TEST
__device__ g16_entry KV_G_JOINT[KV_G_JOINT_ENTRIES];
#endif

/* Joint G table is the DEFAULT; -DKV_NO_G_JOINT restores the two-stream 8-bit
 * comb (GLV-split G scalar, 34 adds) for experiments. The tables above are
 * built either way. */
#ifndef KV_NO_G_JOINT
#define KV_G_JOINT_LADDER 1
#endif

/* tab[d] = d·B affine with canonical limbs, d = 1..255, tab[0] = B. One
 * Montgomery batch inversion over all 255 Zs instead of 255 Fermat chains (the
 * serial per-entry form cost ~35ms of every kv_create). Only FINAL values are
 * stored to tab, so a context created while another one's kernels read the
 * tables rewrites identical bytes. sx/sy/sz/pref: 256-entry scratch. */
__device__ inline void g8_table_fill(ge *tab, fe26 *sx, fe26 *sy, fe26 *sz,
                                     fe26 *pref, const ge &B) {
  gej acc;
  acc.x = B.x;
  acc.y = B.y;
  fe26_set_int(acc.z, 1);
  for (int k = 1; k <= 255; k++) {
    sx[k] = acc.x;
    sy[k] = acc.y;
    sz[k] = acc.z;
    gej t;
    gej_add_ge(t, acc, B);
    acc = t;
  }
  pref[1] = sz[1];
  for (int k = 2; k <= 255; k++) fe26_mul(pref[k], pref[k - 1], sz[k]);
  fe26 inv;
  fe26_inv(inv, pref[255]);
  for (int k = 255; k >= 1; k--) {
    fe26 zi;
    if (k > 1) {
      fe26_mul(zi, inv, pref[k - 1]);
      fe26_mul(inv, inv, sz[k]);
    } else {
      zi = inv;
    }
    fe26 zi2, zi3;
    ge e;
    fe26_sqr(zi2, zi);
    fe26_mul(zi3, zi2, zi);
    fe26_mul(e.x, sx[k], zi2);
    fe26_mul(e.y, sy[k], zi3);
    fe26_normalize(e.x);
    fe26_normalize(e.y);
    tab[k] = e;
  }
  tab[0] = tab[1];
}

/* H = 2^128·G as a canonical affine point, from G by 128 doublings */
__device__ inline void g8_h_base(ge &H, const ge &G) {
  gej acc;
  acc.x = G.x;
  acc.y = G.y;
  fe26_set_int(acc.z, 1);
  for (int k = 0; k < 128; k++) {
    gej t;
    gej_double(t, acc);
    acc = t;
  }
  fe26 zi, zi2, zi3;
  fe26_inv(zi, acc.z);
  fe26_sqr(zi2, zi);
  fe26_mul(zi3, zi2, zi);
  fe26_mul(H.x, acc.x, zi2);
  fe26_mul(H.y, acc.y, zi3);
  fe26_normalize(H.x);
  fe26_normalize(H.y);
}

/* canonical fe26 limbs -> 8 little-endian u32 words of the 256-bit value */
__device__ __forceinline__ void g16_pack_fe(u32 w[8], const fe26 &a) {
  fe f;
  fe26_to_fe(f, a);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    w[2 * i] = (u32)f.n[i];
    w[2 * i + 1] = (u32)(f.n[i] >> 32);
  }
}

/* 8 little-endian u32 words of a value < p -> fe26 limbs (magnitude 1) */
__device__ __forceinline__ void g16_unpack_fe(fe26 &r, const u32 w[8]) {
#pragma unroll
  for (int i = 0; i < 10; i++) {
    int bit = 26 * i;
    int k = bit >> 5, sh = bit & 31;
    u32 v = w[k] >> sh;
    if (sh > 6 && k < 7) v |= w[k + 1] << (32 - sh);
    r.l[i] = v & KV26_M;
  }
}

__device__ __forceinline__ void g16_unpack(ge &e, const g16_entry &t) {
  g16_unpack_fe(e.x, t.w);
  g16_unpack_fe(e.y, t.w + 8);
}

/* One joint entry from the two 8-bit tables: the routine every lane of
 * kv_g_joint_init_kernel runs, and the host build's table accessor. For lo and
 * hi both non-zero it is one mixed add, one inversion, a normalise and a pack.
 * lo·G and hi·H are never equal or opposite there: that needs
 * lo ∓ hi·2^128 ≡ 0 (mod n), and 0 < |lo ∓ hi·2^128| < 2^136 < n. (The mixed
 * add handles both cases anyway.) */
__device__ inline void g16_build_entry(g16_entry &out, u32 idx, const ge *g8,
                                       const ge *h8) {
  u32 lo = idx & 255, hi = (idx >> 8) & 255;
  ge e;
  if (hi == 0) {
    e = g8[lo]; /* lo == 0: g8[0] = G */
  } else if (lo == 0) {
    e = h8[hi];
  } else {
    gej a, s;
    a.x = g8[lo].x;
    a.y = g8[lo].y;
    fe26_set_int(a.z, 1);
    gej_add_ge(s, a, h8[hi]);
    fe26 zi, zi2, zi3;
    fe26_inv(zi, s.z);
    fe26_sqr(zi2, zi);
    fe26_mul(zi3, zi2, zi);
    fe26_mul(e.x, s.x, zi2);
    fe26_mul(e.y, s.y, zi3);
    fe26_normalize(e.x);
    fe26_normalize(e.y);
  }
  g16_pack_fe(out.w, e.x);
  g16_pack_fe(out.w + 8, e.y);
}

/* Table init, phase one (single lane): the two 8-bit tables. */
extern "C" __global__ void kv_ec_table_init_kernel() {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  ge G, H;
  {
    fe gx, gy;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      gx.n[i] = GE_G_X[i];
      gy.n[i] = GE_G_Y[i];
    }
    fe26_from_fe(G.x, gx);
    fe26_from_fe(G.y, gy);
  }
  g8_table_fill(KV_G_TABLE8, KV_G8_X, KV_G8_Y, KV_G8_Z, KV_G8_PREF, G);
  g8_h_base(H, G);
  g8_table_fill(KV_H_TABLE8, KV_G8_X, KV_G8_Y, KV_G8_Z, KV_G8_PREF, H);
}

#ifndef KV_HOST_TEST
/* Table init, phase two: one lane per joint entry (grid covers exactly
 * KV_G_JOINT_ENTRIES lanes; the guard keeps any other launch in bounds). */
extern "C" __global__ void __launch_bounds__(256) kv_g_joint_init_kernel() {
  u32 idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= KV_G_JOINT_ENTRIES) return;
  g16_entry e;
  g16_build_entry(e, idx, KV_G_TABLE8, KV_H_TABLE8);
  KV_G_JOINT[idx] = e;
}

__device__ __forceinline__ void g16_fetch(ge &e, u32 idx) {
  g16_unpack(e, KV_G_JOINT[idx & (KV_G_JOINT_ENTRIES - 1)]);
}
#else
/* Host build: the shims fill KV_G_TABLE8 only, so the accessor builds the H
 * multiples from it (again whenever its base entry changed) and computes the
 * requested entry on demand with the init kernel's per-entry routine. */
static inline void g16_fetch(ge &e, u32 idx) {
  static ge base;
  static bool have = false;
  static fe26 sx[256], sy[256], sz[256], pref[256];
  bool same = have;
  for (int i = 0; same && i < 10; i++)
    same = base.x.l[i] == KV_G_TABLE8[1].x.l[i] &&
           base.y.l[i] == KV_G_TABLE8[1].y.l[i];
  if (!same) {
    ge H;
    base = KV_G_TABLE8[1];
    g8_h_base(H, base);
    g8_table_fill(KV_H_TABLE8, sx, sy, sz, pref, H);
    have = true;
  }
  g16_entry t;
  g16_build_entry(t, idx & (KV_G_JOINT_ENTRIES - 1), KV_G_TABLE8, KV_H_TABLE8);
  g16_unpack(e, t);
}
#endif

/* ---------------- GLV endomorphism scalar decomposition ----------------
 * secp256k1 has an efficient endomorphism φ(x,y) = (β·x, y) with φ(P) = λ·P.
 * Splitting each 256-bit scalar k into k1 + k2·λ with |k1|,|k2| ≤ 2^129 halves
 * the doubling ladder (33 4-bit windows instead of 64). All constants below
 * were DERIVED in-repo (cube roots of unity via Tonelli–Shanks, lattice basis
 * via extended Euclid) and verified against φ(G) = λ·G — see the derivation
 * script output quoted in DESIGN.md. Decomposition uses the shift method:
 * c_i = (g_i·k) >> 384, k1 = k − c1·a1 − c2·a2, k2 = −(c1·b1 + c2·b2),
 * computed in 256-bit two's complement. */

__device__ __constant__ static const u64 GLV_BETA[4] = {
    0xc1396c28719501eeULL, 0x9cf0497512f58995ULL, 0x6e64479eac3434e9ULL,
    0x7ae96a2b657c0710ULL};
__device__ __constant__ static const u64 GLV_G1[4] = {
    0xe893209a45dbb031ULL, 0x3daa8a1471e8ca7fULL, 0xe86c90e49284eb15ULL,
    0x3086d221a7d46bcdULL};
__device__ __constant__ static const u64 GLV_G2[4] = {
    0x1571b4ae8ac47f71ULL, 0x221208ac9df506c6ULL, 0x6f547fa90abfe4c4ULL,
    0xe4437ed6010e8828ULL};
__device__ __constant__ static const u64 GLV_A1[4] = {
    0xe86c90e49284eb15ULL, 0x3086d221a7d46bcdULL, 0x0000000000000000ULL,
    0x0000000000000000ULL};
__device__ __constant__ static const u64 GLV_B1[4] = {
    0x90ab8056f5401b3dULL, 0x1bbc8129fef177d7ULL, 0xffffffffffffffffULL,
    0xffffffffffffffffULL};
__device__ __constant__ static const u64 GLV_A2[4] = {
    0x57c1108d9d44cfd8ULL, 0x14ca50f7a8e2f3f6ULL, 0x0000000000000001ULL,
    0x0000000000000000ULL};
__device__ __constant__ static const u64 GLV_B2[4] = {
    0xe86c90e49284eb15ULL, 0x3086d221a7d46bcdULL, 0x0000000000000000ULL,
    0x0000000000000000ULL};

/* low-256 product r = (a*b) mod 2^256 (two's-complement arithmetic) */
__device__ __forceinline__ void mul_low256(u64 r[4], const u64 a[4], const u64 b[4]) {
  u64 t[8];
  fe_mul_inner(t, a, b);
#pragma unroll
  for (int i = 0; i < 4; i++) r[i] = t[i];
}

/* c = (g*k) >> 384, a 128-bit result */
__device__ __forceinline__ void mul_shift384(u64 c[2], const u64 g[4], const u64 k[4]) {
  u64 t[8];
  fe_mul_inner(t, g, k);
  c[0] = t[6];
  c[1] = t[7];
}

struct glv_half {
  u64 d[3];  /* |k_i|, ≤ 2^129 */
  u64 neg;   /* 1 if k_i < 0 */
};

__device__ inline void glv_split(const sc &k, glv_half &h1, glv_half &h2) {
  u64 c1[4] = {0, 0, 0, 0}, c2[4] = {0, 0, 0, 0};
  mul_shift384(c1, GLV_G1, k.d);
  mul_shift384(c2, GLV_G2, k.d);
  u64 t1[4], t2[4], k1[4], k2[4];
  /* k1 = k − c1·a1 − c2·a2 (mod 2^256) */
  mul_low256(t1, c1, GLV_A1);
  mul_low256(t2, c2, GLV_A2);
  {
    u64 borrow = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) k1[i] = subb(k.d[i], t1[i], borrow);
    borrow = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) k1[i] = subb(k1[i], t2[i], borrow);
  }
  /* k2 = −(c1·b1 + c2·b2), all mod 2^256 two's complement */
  mul_low256(t1, c1, GLV_B1);
  mul_low256(t2, c2, GLV_B2);
  {
    u64 carry = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) t1[i] = addc(t1[i], t2[i], carry);
    u64 borrow = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) k2[i] = subb(0, t1[i], borrow);
  }
  /* two's-complement abs */
  u64 n1 = k1[3] >> 63, n2 = k2[3] >> 63;
  u64 carry = 1;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    u64 v = n1 ? ~k1[i] : k1[i];
    u128 s = (u128)v + (n1 ? carry : 0);
    if (n1) {
      k1[i] = (u64)s;
      carry = (u64)(s >> 64);
    } else {
      k1[i] = v;
    }
  }
  carry = 1;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    u64 v = n2 ? ~k2[i] : k2[i];
    u128 s = (u128)v + (n2 ? carry : 0);
    if (n2) {
      k2[i] = (u64)s;
      carry = (u64)(s >> 64);
    } else {
      k2[i] = v;
    }
  }
  h1.d[0] = k1[0]; h1.d[1] = k1[1]; h1.d[2] = k1[2]; h1.neg = n1;
  h2.d[0] = k2[0]; h2.d[1] = k2[1]; h2.d[2] = k2[2]; h2.neg = n2;
}

__device__ __forceinline__ u64 glv_digit(const glv_half &h, int w) {
  int bit = w * 4;
  int limb = bit >> 6, sh = bit & 63;
  u64 v = h.d[limb] >> sh;
  if (sh > 60 && limb < 2) v |= h.d[limb + 1] << (64 - sh);
  return v & 15;
}

/* 8-bit digit at 4-bit-window position w (w even): bits [4w, 4w+8) */
__device__ __forceinline__ u64 glv_digit8(const glv_half &h, int w) {
  int bit = w * 4;
  int limb = bit >> 6, sh = bit & 63;
  u64 v = h.d[limb] >> sh;
  if (sh > 56 && limb < 2) v |= h.d[limb + 1] << (64 - sh);
  return v & 255;
}

/* Signed fixed-window P digits are the DEFAULT (measured 43.8M vs 39.1M
 * verifies/s: the 8-entry table halves the per-lane scratch table and its
 * build cost); -DKV_NO_SIGNED_PTAB restores unsigned 15-entry windows. */
#ifndef KV_NO_SIGNED_PTAB
#define KV_SIGNED_PTAB 1
#endif

#ifdef KV_SIGNED_PTAB
/* signed fixed 4-bit recode: 33 digits in [-8, 8] (LSB order). |h| < 2^130,
 * so the top digit (<= 4) absorbs the final carry without overflow. */
__device__ __forceinline__ void glv_recode_signed(const glv_half &h,
                                                  int8_t dig[33]) {
  u64 carry = 0;
#pragma unroll 1
  for (int w = 0; w < 33; w++) {
    u64 v = glv_digit(h, w) + carry;
    carry = v > 8;
    dig[w] = (int8_t)((long long)v - (long long)(carry << 4));
  }
}
#endif

/* Signed windows need 1P..8P, unsigned ones 1P..15P. */
#ifdef KV_SIGNED_PTAB
#define KV_PTAB_MAX 8
#else
#define KV_PTAB_MAX 15
#endif

/* Per-verify ladder constants, handed to the window frames by one reference.
 * The ladder runs on the curve y² = x³ + 7·Zg⁶ ("effective affine"), where the
 * per-lane P table needs no inversion; (x, y) on secp256k1 maps to
 * (x·Zg², y·Zg³) there. */
struct ladder_consts {
  fe26 beta; /* GLV β */
  fe26 zg2;  /* Zg² */
  fe26 zg3;  /* Zg³ */
#ifndef KV_G_JOINT_LADDER
  fe26 bzg2; /* β·Zg² */
#endif
};

/* The G digits of one even ladder window, as the frames pass them along: the
 * joint table's 16-bit index, or the two 8-bit comb digits with their signs. */
#ifdef KV_G_JOINT_LADDER
struct g_digits {
  u32 idx;
};
#else
struct g_digits {
  u64 d1, n1, d2, n2;
};
#endif

/* Per-lane P table without an inversion. The chain acc_k = acc_{k-1} + P has
 * Z_k = Z_{k-1}·zr_k, so with Zg = Z_max and m_k = ∏_{j>k} zr_j = Zg/Z_k the
 * pair (X_k·m_k², Y_k·m_k³) is k·P over the COMMON denominator Zg: affine on
 * the isomorphic curve above. 5 field ops per entry instead of one Fermat
 * inversion plus back-substitution; the caller pays Zg back into the result's
 * z. Entries are mul outputs (magnitude <= 2). zg is Zg, magnitude <= 2. */
__device__ inline void ecmult_ptab_build(ge *ptab, ladder_consts &lc, fe26 &zg,
                                         const ge &P) {
  fe26 zr[KV_PTAB_MAX + 1];
  gej acc;
  acc.x = P.x;
  acc.y = P.y;
  fe26_set_int(acc.z, 1);
#pragma unroll 1
  for (int k = 2; k <= KV_PTAB_MAX; k++) {
    gej t;
    gej_add_ge_zr(t, zr[k], acc, P); /* k == 2 is the equal-x doubling path */
    acc = t;
    ptab[k].x = acc.x;
    ptab[k].y = acc.y;
  }
  zg = acc.z;
  fe26 m = zr[KV_PTAB_MAX]; /* m_{max-1} */
#pragma unroll 1
  for (int k = KV_PTAB_MAX - 1; k >= 2; k--) {
    fe26 m2, m3;
    fe26_sqr(m2, m);
    fe26_mul(m3, m2, m);
    fe26_mul(ptab[k].x, ptab[k].x, m2);
    fe26_mul(ptab[k].y, ptab[k].y, m3);
    if (k > 2) fe26_mul(m, m, zr[k]);
  }
  /* entry 1 is P itself: m_1 = Zg */
  fe26_sqr(lc.zg2, zg);
  fe26_mul(lc.zg3, lc.zg2, zg);
  fe26_mul(ptab[1].x, P.x, lc.zg2);
  fe26_mul(ptab[1].y, P.y, lc.zg3);
  ptab[0] = ptab[1]; /* digit 0: add computed then discarded by cmov — a
                        well-formed point keeps magnitudes in range */
}

/* table entry -> the point a ladder stream adds: G entries are mapped onto the
 * ladder's curve first (P entries already live there), then φ (β·x) and the
 * stream's sign are applied */
template <bool IS_G, bool PHI>
__device__ __forceinline__ void ladder_entry(ge &e, const ge &tab,
                                             const ladder_consts &lc, u64 neg) {
  e = tab;
#ifndef KV_G_JOINT_LADDER
  if (IS_G) { /* one multiply per coordinate: φ's β rides on Zg² */
    fe26 mx, my;
    fe26_mul(mx, e.x, PHI ? lc.bzg2 : lc.zg2);
    fe26_mul(my, e.y, lc.zg3);
    e.x = mx;
    e.y = my;
  } else
#endif
  if (PHI) {
    fe26 bx;
    fe26_mul(bx, e.x, lc.beta);
    e.x = bx;
  }
  fe26 ny;
  fe26_neg(ny, e.y, 2);
  fe26_cmov(e.y, ny, (u32)neg);
}

template <bool IS_G, bool PHI>
__device__ __forceinline__ void ladder_add(gej &R, const ge &tab,
                                           const ladder_consts &lc, u64 digit,
                                           u64 neg) {
  ge e;
  gej t;
  ladder_entry<IS_G, PHI>(e, tab, lc, neg);
  gej_add_ge_impl(t, R, e);
  gej_cmov(R, t, (u64)(digit != 0));
}

/* the G adds of one even window */
__device__ __forceinline__ void ladder_add_g(gej &R, const ladder_consts &lc,
                                             const g_digits &g) {
#ifdef KV_G_JOINT_LADDER
  /* one add of lo·G + hi·H: a 64-byte gather, the unpack (magnitude 1) and
   * the map onto the ladder's curve; no sign and no β apply */
  ge e, m;
  gej t;
  g16_fetch(e, g.idx);
  fe26_mul(m.x, e.x, lc.zg2);
  fe26_mul(m.y, e.y, lc.zg3);
  gej_add_ge_impl(t, R, m);
  gej_cmov(R, t, (u64)(g.idx != 0));
#else
  ladder_add<true, false>(R, KV_G_TABLE8[g.d1], lc, g.d1, g.n1); /* G (8-bit) */
  ladder_add<true, true>(R, KV_G_TABLE8[g.d2], lc, g.d2, g.n2);  /* φG */
#endif
}

/* One full ladder window in ONE call frame: 4 doublings + the stream adds
 * (G on even windows, then P, φP). The group ops inline INSIDE this body, so
 * the accumulator crosses the noinline ABI once per window instead of once per
 * group op — the r02 PMC showed the per-call scratch spills of R/temps were
 * the kernel's dominant memory traffic (~119KB/verify). Full kernel-wide
 * inlining is not an option: it reproducibly hangs gfx950 (measured again this
 * round); this bounded body (~5k instructions) stays under that cliff. */
template <bool DOUBLE, bool G_ACTIVE>
__device__ __forceinline__ void gej_window_impl(gej &R, const ge *ptab,
                                                const ladder_consts &lc,
                                                const g_digits &g, u64 dp1,
                                                u64 np1, u64 dp2, u64 np2) {
  if (DOUBLE) {
    gej t;
    gej_double_impl(t, R);
    gej_double_impl(R, t);
    gej_double_impl(t, R);
    gej_double_impl(R, t);
  }
  if (G_ACTIVE) ladder_add_g(R, lc, g); /* G adds land on every second window */
  ladder_add<false, false>(R, ptab[dp1], lc, dp1, np1); /* P */
  ladder_add<false, true>(R, ptab[dp2], lc, dp2, np2);  /* φP */
}

__device__ KV_GROUP_ATTR void gej_window_step(gej &R, const ge *ptab,
                                              const ladder_consts &lc,
                                              u64 g_active, g_digits g, u64 dp1,
                                              u64 np1, u64 dp2, u64 np2) {
  if (g_active) /* wave-uniform */
    gej_window_impl<true, true>(R, ptab, lc, g, dp1, np1, dp2, np2);
  else
    gej_window_impl<true, false>(R, ptab, lc, g, dp1, np1, dp2, np2);
}

/* The ladder's top window: R starts at infinity, so its four doublings would
 * double infinity. This frame sets R and runs the window's adds only (all
 * digits zero leaves R at infinity). With the joint table the G scalar's
 * halves are exactly 128 bits and window 32 carries P digits alone. */
__device__ KV_GROUP_ATTR void gej_window_first(gej &R, const ge *ptab,
                                               const ladder_consts &lc,
#ifndef KV_G_JOINT_LADDER
                                               g_digits g,
#endif
                                               u64 dp1, u64 np1, u64 dp2,
                                               u64 np2) {
  gej r; /* frame-local, stored once: see gej_window_step2 */
  gej_set_infinity(r);
#ifdef KV_G_JOINT_LADDER
  gej_window_impl<false, false>(r, ptab, lc, g_digits{0}, dp1, np1, dp2, np2);
#else
  gej_window_impl<false, true>(r, ptab, lc, g, dp1, np1, dp2, np2);
#endif
  R = r;
}

/* Pair-window frames are the DEFAULT (measured 41.1M vs 39.6M verifies/s);
 * -DKV_NO_PAIR_WINDOWS restores one-window frames for experiments. */
#ifndef KV_NO_PAIR_WINDOWS
#define KV_PAIR_WINDOWS 1
#endif

#ifdef KV_PAIR_WINDOWS
/* Two ladder windows per call frame: 8 doublings + both windows' stream adds
 * (the G add lands only on the even window: 5 adds with the joint table).
 * Halves the accumulator's ABI crossings (17 frames vs 33) at the cost of a
 * ~2x body — under the gfx950 long-body hang cliff (full inlining still
 * hangs). */
__device__ __forceinline__ void gej_window_pair_impl(
    gej &R, const ge *ptab, const ladder_consts &lc, const g_digits &g,
    u64 hp1, u64 hn1, u64 hp2, u64 hn2, /* odd-window P digits + negs */
    u64 lp1, u64 ln1, u64 lp2, u64 ln2 /* even-window P digits + negs */) {
  /* odd window: P streams only */
  gej_window_impl<true, false>(R, ptab, lc, g, hp1, hn1, hp2, hn2);
  /* even window: G + P streams */
  gej_window_impl<true, true>(R, ptab, lc, g, lp1, ln1, lp2, ln2);
}

__device__ KV_GROUP_ATTR void gej_window_step2(gej &R, const ge *ptab,
                                               const ladder_consts &lc,
                                               g_digits g, u64 hp1, u64 hn1,
                                               u64 hp2, u64 hn2, u64 lp1,
                                               u64 ln1, u64 lp2, u64 ln2) {
  /* frame-local accumulator: R may alias ptab and lc as far as the compiler
   * can tell, so working through the reference stores R after every add */
  gej r = R;
  gej_window_pair_impl(r, ptab, lc, g, hp1, hn1, hp2, hn2, lp1, ln1, lp2, ln2);
  R = r;
}

#ifdef KV_QUAD_WINDOWS
/* four windows (two pairs) per frame: 9 frames per ladder */
__device__ KV_GROUP_ATTR void gej_window_step4(gej &R, const ge *ptab,
                                               const ladder_consts &lc,
                                               g_digits ga, g_digits gb,
                                               const u64 a[8], const u64 b[8]) {
  gej_window_pair_impl(R, ptab, lc, ga, a[0], a[1], a[2], a[3], a[4], a[5],
                       a[6], a[7]);
  gej_window_pair_impl(R, ptab, lc, gb, b[0], b[1], b[2], b[3], b[4], b[5],
                       b[6], b[7]);
}
#endif
#endif

/* R = gs·G + ps·P. ps is GLV-split into two signed 129-bit halves read as
 * 4-bit windows: 33 window steps (the top one without doublings, R being
 * infinity there) of 4 doublings + the P and φP adds (φ applied at add time as
 * one β·x field multiply; negative half-scalars negate the added point's y).
 * gs is split at bit 128 and adds one joint-table entry on every second
 * window (see KV_G_JOINT); under KV_NO_G_JOINT it is GLV-split too and feeds
 * two 8-bit comb streams, G and φG. */
__device__ inline void ecmult_double(gej &R, const sc &gs, const sc &ps,
                                     const ge &P) {
  glv_half p1h, p2h;
  glv_split(ps, p1h, p2h);
#ifndef KV_G_JOINT_LADDER
  glv_half g1h, g2h;
  glv_split(gs, g1h, g2h);
#endif
  /* Per-lane P table, affine over the common denominator Zg (80B entries:
   * the working set fits MALL and the P streams are MIXED adds, 11 vs 16
   * fe_muls). The ladder runs on the isomorphic curve where these entries
   * are affine; Zg is paid back into R.z below. */
  ge ptab[KV_PTAB_MAX + 1];
  ladder_consts lc;
  fe26 zg;
  ecmult_ptab_build(ptab, lc, zg, P);
#ifdef KV_SIGNED_PTAB
  int8_t dp1[33], dp2[33];
  glv_recode_signed(p1h, dp1);
  glv_recode_signed(p2h, dp2);
#endif
  {
    fe bu;
#pragma unroll
    for (int i = 0; i < 4; i++) bu.n[i] = GLV_BETA[i];
    fe26_from_fe(lc.beta, bu);
#ifndef KV_G_JOINT_LADDER
    fe26_mul(lc.bzg2, lc.beta, lc.zg2);
#endif
  }
  /* per-stream digit/neg accessors: unsigned fixed windows by default,
   * signed fixed windows (8-entry table) under KV_SIGNED_PTAB */
#ifdef KV_SIGNED_PTAB
#define KV_DP1(w) ((u64)(dp1[w] < 0 ? -dp1[w] : dp1[w]))
#define KV_DN1(w) ((u64)((dp1[w] < 0) ^ (int)p1h.neg))
#define KV_DP2(w) ((u64)(dp2[w] < 0 ? -dp2[w] : dp2[w]))
#define KV_DN2(w) ((u64)((dp2[w] < 0) ^ (int)p2h.neg))
#else
#define KV_DP1(w) glv_digit(p1h, w)
#define KV_DN1(w) (p1h.neg)
#define KV_DP2(w) glv_digit(p2h, w)
#define KV_DN2(w) (p2h.neg)
#endif
  /* G digits of even window w */
#ifdef KV_G_JOINT_LADDER
  /* byte w/2 of the high half over byte w/2 of the low half */
#define KV_GD(w)                                                               \
  (g_digits{(u32)((gs.d[2 + ((w) >> 4)] >> (((w) & 14) << 2)) & 255) << 8 |    \
            (u32)((gs.d[(w) >> 4] >> (((w) & 14) << 2)) & 255)})
#else
#define KV_GD(w)                                                               \
  (g_digits{glv_digit8(g1h, w), g1h.neg, glv_digit8(g2h, w), g2h.neg})
#endif
  /* window 32 alone: R starts at infinity, so this frame has adds only */
  gej_window_first(R, ptab, lc,
#ifndef KV_G_JOINT_LADDER
                   KV_GD(32),
#endif
                   KV_DP1(32), KV_DN1(32), KV_DP2(32), KV_DN2(32));
#if defined(KV_QUAD_WINDOWS)
  /* 8 quad frames (two pairs each) */
#pragma unroll 1
  for (int w = 31; w >= 3; w -= 4) {
    u64 a[8] = {KV_DP1(w), KV_DN1(w), KV_DP2(w), KV_DN2(w),
                KV_DP1(w - 1), KV_DN1(w - 1), KV_DP2(w - 1), KV_DN2(w - 1)};
    u64 b[8] = {KV_DP1(w - 2), KV_DN1(w - 2), KV_DP2(w - 2), KV_DN2(w - 2),
                KV_DP1(w - 3), KV_DN1(w - 3), KV_DP2(w - 3), KV_DN2(w - 3)};
    gej_window_step4(R, ptab, lc, KV_GD(w - 1), KV_GD(w - 3), a, b);
  }
#elif defined(KV_PAIR_WINDOWS)
  /* 16 window pairs */
#pragma unroll 1
  for (int w = 31; w >= 1; w -= 2) {
    gej_window_step2(R, ptab, lc, KV_GD(w - 1),
                     KV_DP1(w), KV_DN1(w), KV_DP2(w), KV_DN2(w),
                     KV_DP1(w - 1), KV_DN1(w - 1), KV_DP2(w - 1), KV_DN2(w - 1));
  }
#else
#pragma unroll 1
  for (int w = 31; w >= 0; w--) {
    u64 g_active = (w & 1) == 0; /* G digits sit at even window positions */
    gej_window_step(R, ptab, lc, g_active, KV_GD(w & ~1),
                    KV_DP1(w), KV_DN1(w), KV_DP2(w), KV_DN2(w));
  }
#endif
#undef KV_GD
#undef KV_DP1
#undef KV_DN1
#undef KV_DP2
#undef KV_DN2
  /* back from the isomorphic curve: (X, Y, Z) there is (X, Y, Z·Zg) on
   * secp256k1 (infinity keeps z == 0) */
  fe26 rz;
  fe26_mul(rz, R.z, zg);
  R.z = rz;
}

/* A BIP-340 verification up to and including the ladder: parses the tuple and
 * computes R = s·G - e·P (Jacobian). Returns 0 when the verdict is still
 * pending on R, else the final KVS_* code of an early exit. rx is r as a field
 * element (canonical limbs), valid when 0 is returned. */
__device__ inline uint8_t schnorr_ladder_one(gej &R, fe26 &rx, const uint8_t *rb,
                                             const uint8_t *sb, const uint8_t *pkb,
                                             const uint8_t *msg) {
  ge P;
  if (!lift_x_even(P, pkb)) return KVS_BAD_PUBKEY;
  fe rxu;
  fe_from_be(rxu, rb);
  if (fe_gte_p_full(rxu)) return KVS_INVALID;
  fe26_from_fe(rx, rxu);
  sc s;
  if (sc_from_be(s, sb)) return KVS_INVALID;
  uint8_t eh[32];
  sha256_tagged96(BIP340_CHALLENGE_MID, rb, pkb, msg, eh);
  sc e, ne;
  sc_from_be(e, eh);
  sc_neg(ne, e);
  ecmult_double(R, s, ne, P);
  return 0;
}

/* The verdict from R's affine coordinates, given zi = 1/R.z: x == r and even
 * y. Five field operations. */
__device__ __forceinline__ uint8_t schnorr_affine_verdict(const gej &R,
                                                          const fe26 &zi,
                                                          const fe26 &rx) {
  fe26 zi2, zi3, xa, ya;
  fe26_sqr(zi2, zi);
  fe26_mul(zi3, zi2, zi);
  fe26_mul(xa, R.x, zi2);
  fe26_mul(ya, R.y, zi3);
  fe26_normalize(ya);
  if (ya.l[0] & 1) return KVS_INVALID;
  return fe26_eq(xa, rx) ? KVS_VALID : KVS_INVALID;
}

/* One BIP-340 verification; returns KVS_* */
__device__ inline uint8_t schnorr_verify_one(const uint8_t *rb, const uint8_t *sb,
                                             const uint8_t *pkb, const uint8_t *msg) {
  gej R;
  fe26 rx;
  uint8_t pre = schnorr_ladder_one(R, rx, rb, sb, pkb, msg);
  if (pre) return pre;
  if (gej_is_infinity(R)) return KVS_INVALID;
  /* affine via one inversion */
  fe26 zi;
  fe26_inv(zi, R.z);
  return schnorr_affine_verdict(R, zi, rx);
}

/* ---------------- split verify: ladder kernel + batched finish ----------------
 * The Fermat inversion above (255 squarings + 15 multiplies) serves one parity
 * bit per signature. Large batches run the ladder and the finish as two
 * kernels: the ladder kernel leaves R in HBM, and the finish kernel inverts K
 * signatures' R.z per LANE with Montgomery's trick (one inversion plus three
 * multiplies per value). Batching has to be per lane: a wave pays for the
 * chain whether one lane or 64 run it.
 *
 * Intermediate buffer, 121 B per signature: 30 u32 limbs (R.x, R.y, R.z) as
 * structure-of-arrays, limb j of signature i at limbs[j*n + i], then n
 * pre-status bytes (0 = pending, else the final KVS_* code). Limbs of a
 * non-pending entry are never written and never enter arithmetic. */
#ifndef KV_FINISH_K
#define KV_FINISH_K 16
#endif

__device__ __forceinline__ void fin_load26(fe26 &v, const u32 *__restrict__ limbs,
                                           unsigned long long n, int coord,
                                           unsigned long long i) {
#pragma unroll
  for (int j = 0; j < 10; j++) v.l[j] = limbs[(unsigned long long)(10 * coord + j) * n + i];
}

/* z of entry i for the batch product: R.z, or 1 where no inversion is wanted
 * (code != 0). Branch-free. */
__device__ __forceinline__ void fin_load_z(fe26 &z, const u32 *__restrict__ limbs,
                                           unsigned long long n,
                                           unsigned long long i, uint8_t code) {
  fe26 one;
  fe26_set_int(one, 1);
  fin_load26(z, limbs, n, 2, i);
  fe26_cmov(z, one, (u32)(code != 0));
}

/* The finish of one lane: entries i = first + m*step, m < KV_FINISH_K. st[m]
 * receives the final KVS_* code of entry m (KVS_INVALID for i >= n, which the
 * caller does not publish). Entries that are not pending, out of range or at
 * infinity (z == 0 mod p, verdict KVS_INVALID) enter the product as 1, so
 * their neighbours' inverses are untouched. */
__device__ inline void schnorr_finish_lane(uint8_t st[KV_FINISH_K],
                                           const u32 *__restrict__ limbs,
                                           const uint8_t *__restrict__ pre,
                                           const uint8_t *__restrict__ tuples,
                                           unsigned long long n,
                                           unsigned long long first,
                                           unsigned long long step) {
  fe26 pref[KV_FINISH_K]; /* pref[m] = z_0 · … · z_{m-1} */
  fe26 acc, one;
  fe26_set_int(acc, 1);
  fe26_set_int(one, 1);
#pragma unroll 1
  for (int m = 0; m < KV_FINISH_K; m++) {
    unsigned long long i = first + (unsigned long long)m * step;
    u32 inr = i < n;
    unsigned long long ii = inr ? i : n - 1; /* clamped: loads stay in bounds */
    uint8_t code = inr ? pre[ii] : (uint8_t)KVS_INVALID;
    fe26 z;
    fin_load_z(z, limbs, n, ii, code);
    u32 inf = (u32)fe26_normalizes_to_zero(z); /* z is a mul output: <= 2 */
    fe26_cmov(z, one, inf);
    st[m] = inf ? (uint8_t)KVS_INVALID : code;
    pref[m] = acc;
    fe26_mul(acc, acc, z);
  }
  fe26 inv;
  fe26_inv(inv, acc); /* acc != 0: every factor is a non-zero residue */
#pragma unroll 1
  for (int m = KV_FINISH_K - 1; m >= 0; m--) {
    unsigned long long i = first + (unsigned long long)m * step;
    unsigned long long ii = i < n ? i : n - 1;
    uint8_t code = st[m];
    fe26 z, zi;
    fin_load_z(z, limbs, n, ii, code);
    fe26_mul(zi, inv, pref[m]); /* 1/z_m */
    fe26_mul(inv, inv, z);      /* 1/(z_0 · … · z_{m-1}) */
    if (code == 0) {
      gej R;
      fin_load26(R.x, limbs, n, 0, ii);
      fin_load26(R.y, limbs, n, 1, ii);
      fe rxu;
      fe_from_be(rxu, tuples + ii * 128); /* r < p: the ladder checked it */
      fe26 rx;
      fe26_from_fe(rx, rxu);
      st[m] = schnorr_affine_verdict(R, zi, rx);
    }
  }
}

#ifndef KV_LB
/* default: 3 blocks/CU minimum. The window-fused ladder fits ~124 VGPRs, so
 * 3 waves/SIMD hide more of the residual stalls — measured 36.2M vs 34.7M
 * (2 blocks) and 32.1M (4 blocks) schnorr verifies/s at 1M tuples. */
#define KV_LB __launch_bounds__(256, 3)
#endif
extern "C" __global__ void KV_LB kv_schnorr_verify_kernel(const uint8_t *__restrict__ tuples,
                                                    unsigned long long n,
                                                    unsigned long long *__restrict__ bitmap,
                                                    uint8_t *__restrict__ status) {
  unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  int valid = 0;
  if (i < n) {
    const uint8_t *t = tuples + i * 128;
    uint8_t st = schnorr_verify_one(t, t + 32, t + 64, t + 96);
    if (status) status[i] = st;
    valid = (st == KVS_VALID);
  }
  unsigned long long mask = __ballot(valid);
  if ((threadIdx.x & 63) == 0) {
    unsigned long long word = i / 64; /* lane0's index is 64-aligned */
    if (i < n) bitmap[word] = mask;
  }
}

#ifndef KV_HOST_TEST
extern "C" __global__ void KV_LB kv_schnorr_ladder_kernel(const uint8_t *__restrict__ tuples,
                                                    unsigned long long n,
                                                    u32 *__restrict__ limbs,
                                                    uint8_t *__restrict__ pre) {
  unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint8_t *t = tuples + i * 128;
  gej R;
  fe26 rx;
  uint8_t st = schnorr_ladder_one(R, rx, t, t + 32, t + 64, t + 96);
  pre[i] = st;
  if (st) return;
#pragma unroll
  for (int j = 0; j < 10; j++) {
    limbs[(unsigned long long)j * n + i] = R.x.l[j];
    limbs[(unsigned long long)(10 + j) * n + i] = R.y.l[j];
    limbs[(unsigned long long)(20 + j) * n + i] = R.z.l[j];
  }
}

/* Lane t of T lanes (T a multiple of 64, T*KV_FINISH_K >= n, grid = T/64
 * blocks of 64) finishes signatures m*T + t: for each m the 64 lanes of a wave
 * hold 64 consecutive signatures, so one ballot is one whole bitmap word. */
extern "C" __global__ void __launch_bounds__(64)
kv_schnorr_finish_kernel(const uint8_t *__restrict__ tuples, unsigned long long n,
                         const u32 *__restrict__ limbs,
                         const uint8_t *__restrict__ pre, unsigned long long T,
                         unsigned long long *__restrict__ bitmap,
                         uint8_t *__restrict__ status) {
  unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  uint8_t st[KV_FINISH_K];
  schnorr_finish_lane(st, limbs, pre, tuples, n, t, T);
#pragma unroll 1
  for (int m = 0; m < KV_FINISH_K; m++) {
    unsigned long long i = (unsigned long long)m * T + t;
    int valid = 0;
    if (i < n) {
      if (status) status[i] = st[m];
      valid = (st[m] == KVS_VALID);
    }
    unsigned long long mask = __ballot(valid);
    /* lane 0's index is 64-aligned; i < n keeps the store below `words` */
    if ((threadIdx.x & 63) == 0 && i < n) bitmap[i / 64] = mask;
  }
}
#endif /* !KV_HOST_TEST */

/* ---------------- ECDSA ---------------- */

__device__ inline uint8_t ecdsa_verify_one(const uint8_t *rb, const uint8_t *sb,
                                           const uint8_t *pk33, const uint8_t *msg) {
  ge P;
  if (!parse_compressed(P, pk33)) return KVS_BAD_PUBKEY;
  sc r, s;
  if (sc_from_be(r, rb)) return KVS_BAD_SIG;  /* parse_compact overflow */
  if (sc_from_be(s, sb)) return KVS_BAD_SIG;
  if (sc_is_zero(r) || sc_is_zero(s)) return KVS_INVALID;
  /* libsecp256k1 secp256k1_ecdsa_verify rejects high-S */
  static const u64 NHALF[4] = {0xDFE92F46681B20A0ULL, 0x5D576E7357A4501DULL,
                               0xFFFFFFFFFFFFFFFFULL, 0x7FFFFFFFFFFFFFFFULL};
  int high = 0;
  for (int i = 3; i >= 0; i--) {
    if (s.d[i] > NHALF[i]) { high = 1; break; }
    if (s.d[i] < NHALF[i]) break;
  }
  if (high) return KVS_INVALID;
  sc z;
  sc_from_be(z, msg); /* reduced mod n like secp256k1_scalar_set_b32 */
  sc w, u1, u2;
  sc_inv(w, s);
  sc_mul(u1, z, w);
  sc_mul(u2, r, w);
  gej R;
  ecmult_double(R, u1, u2, P);
  if (gej_is_infinity(R)) return KVS_INVALID;
  /* x(R) ≡ r (mod n): X == (r + k·n)·Z² for k ∈ {0,1} with r+n < p */
  fe26 z2;
  fe26_sqr(z2, R.z);
  fe rf;
  rf.n[0] = r.d[0];
  rf.n[1] = r.d[1];
  rf.n[2] = r.d[2];
  rf.n[3] = r.d[3];
  fe26 rf26, t;
  fe26_from_fe(rf26, rf);
  fe26_mul(t, rf26, z2);
  if (fe26_eq(t, R.x)) return KVS_VALID;
  /* r + n */
  u64 carry = 0;
  fe rn;
  rn.n[0] = addc(rf.n[0], KV_N0, carry);
  rn.n[1] = addc(rf.n[1], KV_N1, carry);
  rn.n[2] = addc(rf.n[2], KV_N2, carry);
  rn.n[3] = addc(rf.n[3], KV_N3, carry);
  if (!carry && !fe_gte_p_full(rn)) {
    fe26 rn26;
    fe26_from_fe(rn26, rn);
    fe26_mul(t, rn26, z2);
    if (fe26_eq(t, R.x)) return KVS_VALID;
  }
  return KVS_INVALID;
}

extern "C" __global__ void KV_LB kv_ecdsa_verify_kernel(const uint8_t *__restrict__ tuples,
                                                  unsigned long long n,
                                                  unsigned long long *__restrict__ bitmap,
                                                  uint8_t *__restrict__ status) {
  unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  int valid = 0;
  if (i < n) {
    const uint8_t *t = tuples + i * 132; /* r32‖s32‖pk33‖msg32‖pad3 */
    uint8_t st = ecdsa_verify_one(t, t + 32, t + 64, t + 97);
    if (status) status[i] = st;
    valid = (st == KVS_VALID);
  }
  unsigned long long mask = __ballot(valid);
  if ((threadIdx.x & 63) == 0 && i < n) bitmap[i / 64] = mask;
}

} // namespace kv
