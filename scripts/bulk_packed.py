"""Bulk path: the packed verdict form (kw_validate_host_packed) against the full-word form
(kw_validate_host), same process, same box (profiles/r09_bulk_packed.txt).

  python scripts/bulk_packed.py [rows] [config]   on the GPU box: C4 1M by default. For staged columns,
      page-locked columns (kw_batch_pin_host) — both into page-locked outputs — and pageable outputs:
      three alternations of (full words best of 3, packed best of 3). KW_BULK_DEBUG=1 adds the host
      stage times of every pass on stderr.
  python scripts/bulk_packed.py --shares [rows]   no GPU: each bench config's exception share and
      packed bytes per request, from the reference host encoder over host-walk rows (100k by default).
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "policy-server_amd"), os.path.join(ROOT, "tests")]
import kwgpu as K  # noqa: E402
from helpers import config  # noqa: E402

CONFIGS = {"c1_namespace": 1, "c2_trusted": 2, "c3_group": 3, "c4_64": 4, "c5_mixed": 5, "c6_256": 6}
NS = "kubewarden"


def shares(rows):
    for name, scfg in CONFIGS.items():
        env = K.EvaluationEnvironment(config(name), continue_on_errors=True, always_accept_namespace=NS)
        ids = env.policy_ids()
        words = K.SynthBatch(scfg, rows, seed=scfg).batch().debug_host_walk(env, ids)
        p = K.PackedVerdicts.from_words(env, ids, words)
        per_row = p.G * 16 + 4 + 4.0 * p.exc_count / rows
        print(f"{name}: {len(ids)} columns, {rows} rows: exceptions {p.exc_count / words.size:.4f} of the words; "
              f"packed {per_row:.1f} B per request (planes {p.G * 16}, offset 4, exceptions {4.0 * p.exc_count / rows:.1f}) "
              f"against {4 * len(ids)} B of full words", flush=True)


def timed(fn, reps=3):
    best = 1e9
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--shares":
        return shares(int(sys.argv[2]) if len(sys.argv) > 2 else 100_000)
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    name = sys.argv[2] if len(sys.argv) > 2 else "c4_64"
    env = K.EvaluationEnvironment(config(name), continue_on_errors=True, always_accept_namespace=NS, device=0)
    ids = env.policy_ids()
    npol = len(ids)
    syn = K.SynthBatch(CONFIGS[name], n, seed=4)
    first = syn.batch().validate_host_packed(env, ids)  # (also warms the pools; sizes the exception arrays)
    need = first.exc_count
    print(f"{name}: {n} rows x {npol} policies; exceptions {need} words = {need / (n * npol):.4f} of the words; read back "
          f"{(need * 4 + n * (first.G * 16 + 4)) / 1e6:.1f} MB packed against {n * npol * 4 / 1e6:.1f} MB of full words", flush=True)
    del first
    for mode in ("staged columns, page-locked output", "page-locked columns, page-locked output", "staged columns, pageable output"):
        pageable = "pageable output" in mode
        b = syn.batch()
        if mode.startswith("page-locked columns"):
            b.pin_host(0)
        if pageable:
            import numpy as np
            full_out = np.empty(n * npol, dtype=np.uint32)
            pk_out = K.PackedVerdicts(n, npol, exc_cap=need)
        else:
            full_out = K.PinnedWords(n * npol).array
            pk_out = K.PackedVerdicts.page_locked(n, npol, exc_cap=need)
        b.validate_host(env, ids, out=full_out)  # untimed: first touch of the outputs
        b.validate_host_packed(env, ids, out=pk_out)
        for alt in range(3):
            tf = timed(lambda: b.validate_host(env, ids, out=full_out))
            tp = timed(lambda: b.validate_host_packed(env, ids, out=pk_out))
            print(f"{mode}, alternation {alt}: full words {tf * 1e3:.2f} ms = {n / tf / 1e6:.1f} M req/s; "
                  f"packed {tp * 1e3:.2f} ms = {n / tp / 1e6:.1f} M req/s; packed / full time {tp / tf:.3f}", flush=True)
        b.close()
        del full_out, pk_out


if __name__ == "__main__":
    main()
