/* Host shim for the covenant-binding check of phase 1
 * (test_covenants_host.py): compiles kvh_check_covenant_info from
 * kv_validate_host.inc with g++ and runs it on one transaction of a blob —
 * test infrastructure only. */
#include <stdint.h>
#include <string.h>

#include "kaspa_engine_abi.h"
#include "kv_validate_host.inc"

/* the code of transaction tx_index (0, KV_ERR_COVENANT_AUTH_INPUT or
 * KV_ERR_COVENANT_GENESIS_ID); -1 for a blob that does not parse */
extern "C" int host_check_covenant_info(const uint8_t *blob, size_t blob_len,
                                        uint32_t tx_index) {
  std::vector<kvhost::HTx> txs;
  int n = kvhost::parse_blob_host(blob, blob_len, txs);
  if (n < 0 || tx_index >= (uint32_t)n) return -1;
  return kvhost::kvh_check_covenant_info(txs[tx_index]);
}

/* is output out_index of that transaction a continuation output? */
extern "C" int host_cov_is_continuation(const uint8_t *blob, size_t blob_len,
                                        uint32_t tx_index, uint32_t out_index) {
  std::vector<kvhost::HTx> txs;
  int n = kvhost::parse_blob_host(blob, blob_len, txs);
  if (n < 0 || tx_index >= (uint32_t)n) return -1;
  if (out_index >= txs[tx_index].outputs.size()) return -1;
  return kvhost::h_cov_is_continuation(txs[tx_index], txs[tx_index].outputs[out_index]);
}
