"""Probe: what the per-script changes of a journaled diff cost on one GPU, against
what a host has to do without them.

Builds utxo_commit_probe's table (4M slots, 1M inline entries plus 1,000 arena
entries) and utxo_reorg_probe's diffs: 3,000 and 30,000 outpoints per side, 1%
of each side in the arena. Per diff and round, on the same table:
  - baseline:  what a host must do today to know a diff's UtxoChanges:
               kv_utxo_lookup_spk of the removed outpoints BEFORE the apply,
               plus kv_utxo_lookup of the added ones after it (wall time of
               the two calls; filtering by script would come on top);
  - changes:   kv_utxo_changes_by_spk on the record kv_utxo_apply_diff pushed,
               one call with max_entries above the answer, for 1, 1,000 and
               65,536 queries (half of them, as far as the diff has that many,
               scripts the diff touches) and for KV_UTXO_CHANGES_ALL with
               scripts: wall time of the call and the kernel_ms it reports.
The diff is reverted after every round. Query arrays are packed once, outside
the timed calls. Every call ends in a stream synchronisation, so wall times are
of finished work. It prints one JSON line with the best and the median of the
rounds, and checks the totals of every call against the diff and that
kv_utxo_commitment after all rounds equals the one before, mod P. There is no
pass threshold on the times.
"""
import ctypes
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

from utxo_commit_probe import (CAPACITY, N_ARENA, N_INLINE, P,  # noqa: E402
                               make_entries, num)
from utxo_rehash_probe import upsert  # noqa: E402
from utxo_reorg_probe import DIFFS, make_diff, summary, timed  # noqa: E402

QUERY_COUNTS = (1, 1000, 65536)
ROUNDS = 7  # after one warm-up round


def amounts(ents):
    return int(np.ascontiguousarray(ents[:, 0:8]).view("<u8").sum(dtype=np.uint64))


def make_queries(rs, diff, n_q):
    """n_q distinct 34-byte scripts, packed: up to half of them inline scripts
    of the diff, alternating between its sides, the rest random"""
    from rusty_kaspa_amd.engine import KvSpkQuery
    rem_ents, add_ents = diff[1], diff[4]
    inline = lambda e: e[e[:, 20] == 34][:, 24:58]
    sides = [inline(rem_ents), inline(add_ents)]
    n_hit = min((n_q + 1) // 2, len(sides[0]), len(sides[1]))
    scripts = np.empty((n_q, 34), dtype=np.uint8)
    scripts[:] = rs.randint(0, 256, size=(n_q, 34), dtype=np.uint8)
    for i in range(n_hit):
        scripts[i] = sides[i % 2][i // 2]
    heads = (KvSpkQuery * n_q)()
    for i in range(n_q):
        heads[i] = KvSpkQuery(34, 0, 0)
    return heads, scripts.tobytes(), n_q, n_hit


def run_diff(eng, rs, diff):
    from rusty_kaspa_amd.engine import (KV_UTXO_CHANGES_ALL, KV_UTXO_MAX_SPK,
                                        KvUtxoChangesResult)
    rem_ops, rem_ents, rem_spk, add_ops, add_ents, add_spk = diff
    d = len(rem_ops)
    ctx = ctypes.c_void_p(eng.ctx)
    rem_b, add_b = rem_ops.tobytes(), add_ops.tobytes()
    add_e, add_s = add_ents.tobytes(), add_spk.tobytes()
    ent_out = (ctypes.c_uint8 * (64 * d))()
    bm = (ctypes.c_uint64 * ((d + 63) // 64))()
    spk = (ctypes.c_uint8 * max(1, rem_spk.size))()
    used = ctypes.c_size_t()
    end = 3 * d
    rec_out = (ctypes.c_uint8 * (96 * end))()
    spk_cap = KV_UTXO_MAX_SPK + 34 * 2 * d + rem_spk.size + add_spk.size
    spk_out = (ctypes.c_uint8 * spk_cap)()
    want = (end, amounts(add_ents), amounts(rem_ents), d, d, 0)

    def check(rc):
        if rc:
            raise RuntimeError(eng.lib.kv_last_error().decode())

    def lookup_removed():
        check(eng.lib.kv_utxo_lookup_spk(ctx, rem_b, ctypes.c_size_t(d), ent_out, bm, spk,
                                         ctypes.c_size_t(len(spk)), ctypes.byref(used)))

    def lookup_added():
        check(eng.lib.kv_utxo_lookup(ctx, add_b, ctypes.c_size_t(d), ent_out, bm, None))

    def changes(token, flags, heads, blob, n_q, scripts):
        cur, n, s_used = ctypes.c_uint64(0), ctypes.c_size_t(), ctypes.c_size_t()
        res = KvUtxoChangesResult()
        check(eng.lib.kv_utxo_changes_by_spk(
            ctx, ctypes.c_uint64(token), ctypes.c_uint32(flags), ctypes.byref(cur),
            heads, ctypes.c_size_t(n_q), blob, ctypes.c_size_t(len(blob)),
            ctypes.c_size_t(end), rec_out, spk_out if scripts else None,
            ctypes.c_size_t(spk_cap), ctypes.byref(s_used), ctypes.byref(n),
            ctypes.byref(res)))
        got = (res.cursor_end, res.added_amount, res.removed_amount, res.n_added,
               res.n_removed, res.n_added_gone)
        return res.kernel_ms, n.value, got == want and cur.value == end

    sets = {str(n_q): make_queries(rs, diff, n_q) for n_q in QUERY_COUNTS}
    names = list(sets) + ["all_with_scripts"]
    t = {"baseline_wall": [], "baseline_lookup_removed_wall": []}
    for name in names:
        t[name + "_wall"], t[name + "_kernel"] = [], []
    matches, clean = {}, True
    for r in range(ROUNDS + 1):
        ms_rem, _ = timed(lookup_removed)
        token, res = eng.utxo_apply_diff(rem_b, add_b, add_e, add_s)
        clean = clean and res["n_removed_missing"] == res["n_added_overwrote"] == 0
        ms_add, _ = timed(lookup_added)
        row = {}
        for name in names:
            if name in sets:
                heads, blob, n_q, n_hit = sets[name]
                wall, (kernel, n, ok) = timed(
                    lambda: changes(token, 0, heads, blob, n_q, False))
                ok = ok and n == n_hit
            else:
                wall, (kernel, n, ok) = timed(
                    lambda: changes(token, KV_UTXO_CHANGES_ALL, None, b"", 0, True))
                ok = ok and n == 2 * d
            row[name] = (wall, kernel)
            matches[name] = n
            clean = clean and ok
        eng.utxo_revert(token)
        if r == 0:
            continue  # warm-up: first launches, buffer growth
        t["baseline_lookup_removed_wall"].append(ms_rem)
        t["baseline_wall"].append(ms_rem + ms_add)
        for name, (wall, kernel) in row.items():
            t[name + "_wall"].append(wall)
            t[name + "_kernel"].append(kernel)
    return {
        "outpoints_per_side": d,
        "arena_per_side": int(rem_spk.shape[0]),
        "cursor_end": end,
        "baseline": summary(t["baseline_wall"]),
        "baseline_lookup_removed": summary(t["baseline_lookup_removed_wall"]),
        "changes": {name: {"records": matches[name],
                           "wall": summary(t[name + "_wall"]),
                           "kernel": summary(t[name + "_kernel"])}
                    for name in names},
    }, clean


def main():
    from rusty_kaspa_amd.engine import Engine  # needs __graft_entry__.build()

    ops, ents, spks = make_entries()
    eng = Engine()
    ctx = ctypes.c_void_p(eng.ctx)
    assert eng.lib.kv_utxo_reset(ctx, ctypes.c_uint64(CAPACITY)) == 0
    upsert(eng, ops[:N_INLINE], ents[:N_INLINE])
    upsert(eng, ops[N_INLINE:], ents[N_INLINE:], spks.tobytes())
    c0, n0, _ = eng.utxo_commitment()
    rs = np.random.RandomState(8)
    results, ok = [], True
    for d in DIFFS:
        res, clean = run_diff(eng, rs, make_diff(rs, ops, ents, spks, d))
        results.append(res)
        ok = ok and clean
    c1, n1, _ = eng.utxo_commitment()
    journal = eng.utxo_journal_stats()
    eng.close()
    ok = bool(ok and n0 == n1 == N_INLINE + N_ARENA and num(c0) % P == num(c1) % P
              and journal["n_records"] == 0)
    print(json.dumps({
        "probe": "utxo_changes",
        "entries": n1, "arena_entries": N_ARENA, "rounds": ROUNDS,
        "diffs": results,
        "consistent": ok,
    }), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
