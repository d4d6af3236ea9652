/* Host shim for the undo journal's value-rewriting rule
 * (test_utxo_journal_host.py): compiles utxo_value_journal_rewrite from
 * kv_utxo_journal_kernels.hip with g++ (KV_HOST_TEST drops the kernels, which
 * need wave intrinsics and the table's slot type). */
#include "shim.h"
#include "kv_utxo_journal_kernels.hip"

/* rewrites val64 in place; returns 0 inline / 1 arena / -1 refused, as the
 * device function does. mode 0 = set (capture), 1 = rebase (revert). */
extern "C" int host_utxo_value_journal_rewrite(uint8_t *val64, int mode, uint64_t add,
                                               uint64_t src_len, uint64_t dst_len,
                                               uint32_t *old_off, uint32_t *spk_len) {
  return kv::utxo_value_journal_rewrite(val64, mode, add, src_len, dst_len, old_off,
                                        spk_len);
}

/* the capture kernel's use of the rule on one value: the fail word is set, and
 * the value left alone, exactly when the rule refuses */
extern "C" void host_journal_capture_value(uint8_t *val64, uint64_t blob_cursor,
                                           uint64_t arena_len, uint32_t *fail_word) {
  uint32_t off, len;
  if (kv::utxo_value_journal_rewrite(val64, KV_JOURNAL_SET, blob_cursor, arena_len,
                                     0xffffffffULL, &off, &len) < 0)
    *fail_word = 1;
}
