"""The summary form (kw_batch_summary, kw_validate_host_summary) against the calls it stands beside,
same process, same box (profiles/r10_summary.txt).

  python scripts/summary_bench.py [rows] [config]   on the GPU box: C4 1M by default.
      Resident: three alternations of validate + verdicts, validate + summary with planes and
      validate + summary without (wall time from Python, best of 3 each; the page-locked forms of the
      outputs as well). Bulk: three alternations of validate_host_packed and validate_host_summary
      into page-locked outputs, with planes and without.
  python scripts/summary_bench.py --kernels [rows] [config]   the run to put under
      rocprofv3 --kernel-trace --stats: four bulk passes of each of the packed and the summary form
      over the same chunks, so pack_codes_kernel and summary_kernel have the same calls; prints the
      bytes each moves per pass. --kernels-one: the same in one chunk of all rows (KW_BULK_RAMP=0),
      where a call's time gives the kernel's bytes per second.
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "policy-server_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

import kwgpu as K  # noqa: E402
from helpers import config  # noqa: E402

CONFIGS = {"c1_namespace": 1, "c2_trusted": 2, "c3_group": 3, "c4_64": 4, "c5_mixed": 5, "c6_256": 6}
NS = "kubewarden"


def timed(fn, reps=3):
    best = 1e9
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best


def setup(argv):
    n = int(argv[0]) if argv else 1_000_000
    name = argv[1] if len(argv) > 1 else "c4_64"
    env = K.EvaluationEnvironment(config(name), continue_on_errors=True, always_accept_namespace=NS, device=0)
    return n, name, env, env.policy_ids(), K.SynthBatch(CONFIGS[name], n, seed=4)


def kernels(argv, one_chunk):
    if one_chunk:  # (read once per process: no ramp of small first chunks; each pass's line on stderr says "chunks 1")
        os.environ["KW_BULK_RAMP"], os.environ["KW_BULK_DEBUG"] = "0", "1"
    n, name, env, ids, syn = setup(argv)
    chunk = n if one_chunk else 0
    npol, G = len(ids), (len(ids) + 63) // 64
    # the same passes for both forms, so the two kernels' calls and totals compare one to one
    first = syn.batch().validate_host_packed(env, ids, out=K.PackedVerdicts(n, npol, exc_cap=n * npol), chunk_rows=chunk)
    pk = K.PackedVerdicts.page_locked(n, npol, exc_cap=first.exc_count)
    sm = K.Summary(n, npol, pinned=True)
    b = syn.batch()
    b.validate_host_summary(env, ids, chunk_rows=chunk)
    for _ in range(3):
        b.validate_host_packed(env, ids, out=pk, chunk_rows=chunk)
    for _ in range(3):
        b.validate_host_summary(env, ids, out=sm, chunk_rows=chunk)
    mb = (n * npol * 4 + n * G * 16) / 1e6
    print(f"{name}: {n} rows x {npol} policies. Per pass, pack_codes_kernel and summary_kernel each read "
          f"{n * npol * 4 / 1e6:.1f} MB of words and write {n * G * 16 / 1e6:.1f} MB of planes = {mb:.1f} MB "
          f"(pack_codes also {n * G * 4 / 1e6:.1f} MB of counts). Four passes of each form in "
          f"{'one chunk of all rows: a call moves the whole ' + format(mb, '.1f') + ' MB' if one_chunk else 'the default chunks'}",
          flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] in ("--kernels", "--kernels-one"):
        return kernels(sys.argv[2:], sys.argv[1] == "--kernels-one")
    n, name, env, ids, syn = setup(sys.argv[1:])
    npol = len(ids)
    print(f"{name}: {n} rows x {npol} policies; full words {n * npol * 4 / 1e6:.1f} MB, planes "
          f"{n * ((npol + 63) // 64) * 16 / 1e6:.1f} MB, counters {npol * K._native.KW_SUM_N * 8 / 1e3:.1f} kB", flush=True)

    # resident: the batch is on the device; each timed call is a pass and what comes back from it
    b = syn.batch().to_device(0)
    words = np.empty(n * npol, dtype=np.uint32)
    words_pin = K.PinnedWords(n * npol).array
    s_planes, s_pin, s_count = K.Summary(n, npol), K.Summary(n, npol, pinned=True), K.Summary(n, npol, planes=False)

    def pass_and(fn):
        def run():
            b.validate(env, ids)
            fn()
        return run
    forms = [("verdicts", pass_and(lambda: b.verdicts(out=words))),
             ("verdicts, page-locked", pass_and(lambda: b.verdicts(out=words_pin))),
             ("summary with planes", pass_and(lambda: b.summary(out=s_planes))),
             ("summary with planes, page-locked", pass_and(lambda: b.summary(out=s_pin))),
             ("summary, counters only", pass_and(lambda: b.summary(out=s_count)))]
    for _, fn in forms:
        fn()  # untimed: first touch of the outputs, the pools
    assert np.array_equal(s_planes.col, K.Summary.from_words(words, npol, planes=False).col)
    for alt in range(3):
        ts = [(label, timed(fn)) for label, fn in forms]
        base = ts[0][1]
        print(f"resident validate + ..., alternation {alt}: " +
              "; ".join(f"{label} {t * 1e3:.3f} ms ({t / base:.3f})" for label, t in ts), flush=True)
    b.close()
    del words, words_pin

    # bulk: host columns in, page-locked outputs
    first = syn.batch().validate_host_packed(env, ids)
    pk = K.PackedVerdicts.page_locked(n, npol, exc_cap=first.exc_count)
    del first
    hb = syn.batch()
    bulk = [("packed", lambda: hb.validate_host_packed(env, ids, out=pk)),
            ("summary with planes", lambda: hb.validate_host_summary(env, ids, out=s_pin)),
            ("summary, counters only", lambda: hb.validate_host_summary(env, ids, out=s_count))]
    for _, fn in bulk:
        fn()
    for alt in range(3):
        ts = [(label, timed(fn)) for label, fn in bulk]
        base = ts[0][1]
        print(f"bulk, staged columns, page-locked output, alternation {alt}: " +
              "; ".join(f"{label} {t * 1e3:.2f} ms = {n / t / 1e6:.1f} M req/s ({t / base:.3f})" for label, t in ts), flush=True)
    hb.close()


if __name__ == "__main__":
    main()
