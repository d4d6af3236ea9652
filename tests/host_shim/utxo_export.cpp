/* Host shim for the table value → export record function
 * (test_utxo_export_host.py): compiles utxo_value_export from
 * kv_utxo_rehash_kernels.hip with g++ (KV_HOST_TEST drops the kernels, which
 * need wave intrinsics and the table's slot type). */
#include "shim.h"
#include "kv_utxo_rehash_kernels.hip"

/* converts val64 in place; returns 1 for an arena value, else 0 */
extern "C" int host_utxo_value_export(uint8_t *val64, uint32_t *spk_len,
                                      uint32_t *arena_off) {
  return kv::utxo_value_export(val64, spk_len, arena_off);
}
