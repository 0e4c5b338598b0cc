"""The digest's drill-down on the device (kw_batch_digest_members) beside the digest it follows and
against what a caller had to do before it: read every verdict word back (kw_batch_verdicts) and pick
the members on the host (kw_debug_digest_members_words, the exact reducer), same process, same box
(profiles/r15_members.txt).

  python scripts/members_bench.py [rows] [config]   on the GPU box: C4 at 1M rows, AUDIT.
    One resident kw_validate_batch pass and its digest; then three selections: the largest group, the
    32 groups with the most findings, every group. Per selection: kw_batch_digest_members once untimed
    (first touch, the pools), then five alternations of kw_batch_digest and kw_batch_digest_members on
    the same pass into arrays sized once, by the host clock around each call (both end in a stream
    synchronise). KW_BULK_DEBUG makes the library print its [kw members] line, which this script passes
    through: the table and the staging on the host, check and walk on the device by HIP events inside
    the call, read-back, and the ordering on the host, each apart. Then the host path once, and the
    two results compared byte for byte.
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


def run(name, n):
    env = K.EvaluationEnvironment(config(name), continue_on_errors=True, always_accept_namespace=NS, device=0)
    ids = env.policy_ids()
    npol = len(ids)
    b = K.SynthBatch(CONFIGS[name], n, seed=4).batch().to_device(0)
    b.validate(env, ids, K.AUDIT)
    say(f"{name}: {n} rows x {npol} policies = {n * npol / 1e6:.1f} M pairs, words {n * npol * 4 / 1e6:.1f} MB, AUDIT")
    d = b.digest()  # untimed: first touch, the pools, the sizes
    say(f"    {d.findings} findings, {d.recs.size} groups, {d.wide.size} wide")
    drecs = np.zeros(max(d.recs.size, 1), dtype=np.dtype(K.DIGEST_REC))
    dwide = np.zeros(max(d.wide.size, 1), dtype=np.uint64)
    dst = N.KwDigest(drecs.ctypes.data_as(C.POINTER(N.KwDigestRec)), drecs.size, 0,
                     dwide.ctypes.data_as(C.POINTER(C.c_uint64)), dwide.size, 0, 0)
    t_read, words = wall(b.verdicts)
    say(f"    kw_batch_verdicts alone on this pass: {t_read:.1f} ms")
    by_count = d.recs[np.argsort(-d.recs["count"].astype(np.int64), kind="stable")]
    for label, recs in (("the largest group", by_count[:1]), ("the 32 groups with the most findings", by_count[:32]),
                        ("every group", d.recs)):
        recs = np.ascontiguousarray(recs)
        total = int(recs["count"].sum())
        say(f"  {label}: {recs.size} groups, {total} members ({total * 12 / 1e6:.2f} MB of rows and words)")
        first = b.digest_members(recs)  # untimed
        assert first.rows.size == total
        off = np.zeros(recs.size + 1, dtype=np.uint64)
        rows = np.zeros(max(total, 1), dtype=np.uint64)
        wd = np.zeros(max(total, 1), dtype=np.uint32)
        st = N.KwMembers(off.ctypes.data_as(C.POINTER(C.c_uint64)), rows.ctypes.data_as(C.POINTER(C.c_uint64)),
                         wd.ctypes.data_as(C.POINTER(C.c_uint32)), total, 0)
        rp = recs.ctypes.data_as(C.POINTER(N.KwDigestRec))
        walls = []
        for alt in range(5):
            t_d, rc = wall(lambda: N.lib().kw_batch_digest(b._h, C.byref(dst)))
            assert rc == N.KW_OK and dst.n == d.recs.size
            t_m, rc = wall(lambda: N.lib().kw_batch_digest_members(b._h, rp, recs.size, C.byref(st)))
            assert rc == N.KW_OK and st.n == total
            walls.append(t_m)
            say(f"    alternation {alt}: wall digest {t_d:.3f} ms, members {t_m:.3f} ms")
        assert rows[:total].tobytes() == first.rows.tobytes() and wd[:total].tobytes() == first.words.tobytes()
        t_read, words = wall(lambda: b.verdicts(out=words))
        t_red, ref = wall(lambda: b.digest_members_from_words(words, npol, recs))
        same = (np.array_equal(ref.off, first.off) and ref.rows.tobytes() == first.rows.tobytes() and
                ref.words.tobytes() == first.words.tobytes())
        best = min(walls)
        say(f"    the host path: kw_batch_verdicts {t_read:.1f} ms + kw_debug_digest_members_words {t_red:.1f} ms = "
            f"{t_read + t_red:.1f} ms; kw_batch_digest_members {best:.3f} ms (best of 5): {(t_read + t_red) / best:.1f}x; "
            f"{'below' if best < t_read else 'NOT below'} kw_batch_verdicts alone; members equal: {same}")
        assert same
    b.close()


def main():
    argv = sys.argv[1:]
    n = int(argv[0]) if argv else 1_000_000
    for name in (argv[1:] or ["c4_64"]):
        run(name, n)


if __name__ == "__main__":
    main()
