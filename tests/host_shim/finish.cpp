/* Host shim for the field reduction and the batched Schnorr finish
 * (test_fe26_reduce_host.py, test_schnorr_finish_host.py). It sits on top of
 * main.cpp the way ladder.cpp does, so the device sources compile exactly as
 * they do there (KV_HOST_TEST on: magnitude and reduction asserts live);
 * host_fe26_mul / host_fe26_sqr come from main.cpp and return raw limbs. */
#include "main.cpp"

extern "C" int host_finish_k(void) { return KV_FINISH_K; }

/* One lane of the finish kernel: entries first + m*step, m < KV_FINISH_K, of
 * an n-signature intermediate buffer (limbs: 30*n u32, structure-of-arrays;
 * pre: n bytes; tuples: n*128 bytes, only r is read). st_out: KV_FINISH_K
 * final codes. */
extern "C" void host_schnorr_finish_lane(const uint32_t *limbs, const uint8_t *pre,
                                         const uint8_t *tuples,
                                         unsigned long long n,
                                         unsigned long long first,
                                         unsigned long long step,
                                         uint8_t *st_out) {
  kv::schnorr_finish_lane(st_out, limbs, pre, tuples, n, first, step);
}
