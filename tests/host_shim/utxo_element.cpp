/* Host shim for the UTXO-entry → U3072 element function
 * (test_utxo_element_host.py): compiles utxo_entry_element from
 * kv_utxo_commit_kernels.hip with g++ (KV_HOST_TEST drops the kernels, which
 * need wave intrinsics and the table's slot type). */
#include "shim.h"
#include "kv_utxo_commit_kernels.hip"

extern "C" void host_utxo_entry_element(const uint8_t *op36, const uint8_t *val64,
                                        const uint8_t *arena, uint64_t *out48) {
  kv::utxo_entry_element(op36, val64, arena, out48);
}

extern "C" int host_utxo_value_spk_ok(const uint8_t *val64, uint64_t arena_len) {
  return kv::utxo_value_spk_ok(val64, arena_len);
}
