"""The metrics of a pass on the device (kw_batch_outcomes, kw_metrics_record_pass) against the calls
they stand beside, same process, same box (profiles/r12_metrics_pass.txt).

  python scripts/metrics_pass_bench.py [rows] [config] [rows_c]   on the GPU box: C4, 1M and 100k rows.
    (a) the device time of kw_batch_outcomes over the synthetic stream's own attribute groups and of
        kw_batch_summary without planes on the same resident pass: HIP events inside the two calls
        (KW_BULK_DEBUG makes them print their lines, which this script passes through), five
        alternations; the calls' wall time beside them.
    (b) the wall time of record_pass at `rows`, and of its three steps called one by one: dictionary
        (the first call builds it, later calls copy it), device count, fold.
    (c) at rows_c rows: kw_metrics_record over all pairs, with the read-back of the words, against
        record_pass on the same batch; the two renders must be equal.
  python scripts/metrics_pass_bench.py --kernels [rows] [config]   the run to put under
    rocprofv3 --kernel-trace --stats: five summaries without planes and five outcome counts of one pass.
"""
import os
import sys
import time

os.environ.setdefault("KW_BULK_DEBUG", "1")  # (read once per process)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "policy-server_amd"), os.path.join(ROOT, "tests")]
import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402

import kwgpu as K  # noqa: E402
from helpers import config  # noqa: E402
from kwgpu import _native as N  # noqa: E402

CONFIGS = {"c1_namespace": 1, "c2_trusted": 2, "c3_group": 3, "c4_64": 4, "c5_mixed": 5, "c6_256": 6}
NS = "kubewarden"


def wall(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def say(text):
    sys.stderr.flush()
    print(text, flush=True)


def record_all_pairs(m, env, batch, ids, words, latency_ms, origin):
    npol = len(ids)
    n = words.size
    rows = np.repeat(np.arange(n // npol, dtype=np.uint64), npol)
    pols = np.tile(np.array([env._idx(p) for p in ids], dtype=np.int32), n // npol)
    lat = np.full(n, latency_ms, dtype=np.uint64)
    t0 = time.perf_counter()
    rc = N.lib().kw_metrics_record(m._h, env._h, batch._h, rows.ctypes.data_as(C.POINTER(C.c_uint64)),
                                   pols.ctypes.data_as(C.POINTER(C.c_int32)), words.ctypes.data_as(C.POINTER(C.c_uint32)),
                                   lat.ctypes.data_as(C.POINTER(C.c_uint64)), n, origin)
    assert rc == N.KW_OK
    return (time.perf_counter() - t0) * 1e3


def main():
    argv = sys.argv[1:]
    kernels = bool(argv) and argv[0] == "--kernels"
    if kernels:
        argv = argv[1:]
    n = int(argv[0]) if argv else 1_000_000
    name = argv[1] if len(argv) > 1 else "c4_64"
    n_c = int(argv[2]) if len(argv) > 2 else 100_000
    env = K.EvaluationEnvironment(config(name), continue_on_errors=True, always_accept_namespace=NS, device=0)
    ids = env.policy_ids()
    npol = len(ids)
    b = K.SynthBatch(CONFIGS[name], n, seed=4).batch().to_device(0)
    b.validate(env, ids)
    t_dict, (rg, first) = wall(b.attribute_groups)
    ng = first.size
    say(f"{name}: {n} rows x {npol} policies = {n * npol / 1e6:.1f} M pairs, words {n * npol * 4 / 1e6:.1f} MB; "
        f"{ng} attribute groups, table {ng * N.KW_OUT_N * npol * 8 / 1e3:.1f} kB, row list {n * 4 / 1e6:.1f} MB")
    count = K.Summary(n, npol, planes=False)
    b.summary(out=count)
    table = b.outcomes(rg, ng)  # untimed: first touch, the pools
    assert (table.sum(axis=(0, 1)) == n).all()
    assert np.array_equal(table[:, N.KW_OUT_INIT_ERROR, :].sum(axis=0), count.col[:, N.KW_SUM_FST_INIT_ERROR])
    if kernels:
        for _ in range(4):
            b.summary(out=count)
            b.outcomes(rg, ng)
        return
    say("(a) device time, HIP events inside the calls ([kw summary] / [kw outcomes] lines), and the calls' wall time")
    for alt in range(5):
        t_s, _ = wall(lambda: b.summary(out=count))
        t_o, _ = wall(lambda: b.outcomes(rg, ng))
        say(f"    alternation {alt}: wall summary without planes {t_s:.3f} ms, outcomes {t_o:.3f} ms")
    say("(a') the same with every row in one group, and with the rows' groups drawn at random from 4096")
    b.outcomes(None, 1)
    b.outcomes(np.random.default_rng(1).integers(0, 4096, n).astype(np.uint32), 4096)

    say(f"(b) record_pass at {n} rows; its steps one by one (dictionary first call {t_dict:.3f} ms: built)")
    for alt in range(3):
        m = K.Metrics()
        t_all, _ = wall(lambda: m.record_pass(env, b, ids, 7))
        m2 = K.Metrics()
        t_d, (rg2, first2) = wall(b.attribute_groups)
        t_o, tab = wall(lambda: b.outcomes(rg2, first2.size))
        t_f, _ = wall(lambda: m2.add_outcomes(env, b, ids, tab, first2, 7))
        say(f"    alternation {alt}: record_pass {t_all:.3f} ms; dictionary (kept: copied out) {t_d:.3f} ms, "
            f"device count {t_o:.3f} ms, fold {t_f:.3f} ms")
        assert m.render() == m2.render()
    fresh = K.SynthBatch(CONFIGS[name], n, seed=4).batch()
    t_build, _ = wall(fresh.attribute_groups)
    say(f"    dictionary built on a fresh batch of {n} rows: {t_build:.3f} ms")
    fresh.close()
    b.close()

    say(f"(c) at {n_c} rows: kw_metrics_record over all {n_c * npol / 1e6:.1f} M pairs against record_pass, same batch")
    c = K.SynthBatch(CONFIGS[name], n_c, seed=4).batch().to_device(0)
    c.validate(env, ids)
    for alt in range(2):
        mp, md = K.Metrics(), K.Metrics()
        t_read, words = wall(c.verdicts)
        t_rec = record_all_pairs(mp, env, c, ids, words, 7, K.VALIDATE)
        c2 = K.SynthBatch(CONFIGS[name], n_c, seed=4).batch().to_device(0)  # a batch whose dictionary is not built yet
        c2.validate(env, ids)
        t_first, _ = wall(lambda: md.record_pass(env, c2, ids, 7))
        same = mp.render() == md.render()
        md2 = K.Metrics()
        t_again, _ = wall(lambda: md2.record_pass(env, c2, ids, 7))
        say(f"    alternation {alt}: read-back {t_read:.3f} ms + kw_metrics_record {t_rec:.1f} ms = {t_read + t_rec:.1f} ms; "
            f"record_pass {t_first:.3f} ms with the dictionary built in it, {t_again:.3f} ms with it kept "
            f"({(t_read + t_rec) / t_first:.0f}x / {(t_read + t_rec) / t_again:.0f}x); renders equal: {same}")
        assert same and md2.render() == mp.render()
        c2.close()


if __name__ == "__main__":
    main()
