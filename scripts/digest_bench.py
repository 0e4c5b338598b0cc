"""The violation digest on the device (kw_batch_digest) against what a caller had to do before it:
read every verdict word back (kw_batch_verdicts) and group the findings on the host
(kw_debug_digest_words, the exact reducer), same process, same box (profiles/r14_digest.txt).

  python scripts/digest_bench.py [rows] [config ...]   on the GPU box: C4, C2 and C3 at 1M rows, AUDIT.
    Per workload: one resident kw_validate_batch pass; kw_batch_digest five times into arrays sized
    once (KW_BULK_DEBUG makes the library print its [kw digest] line, which this script passes
    through: host preparation, device count / verify / gather by HIP events, read-back, and the
    findings, groups and leftovers); the summary without planes beside it, which reads the same
    words; then the host path once, and the two results compared byte for byte.
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
    first = b.digest()  # untimed: first touch, the pools, the sizes
    stats = b.debug_digest_stats()
    say(f"    {first.findings} findings ({100.0 * first.findings / (n * npol):.1f} % of the pairs), {first.recs.size} groups, "
        f"{first.wide.size} wide, {stats['leftovers']} leftovers, {stats['ranges']} ranges ({stats['cuts']} cut), {stats['slots']} slots")
    recs = np.zeros(max(first.recs.size, 1), dtype=np.dtype(K.DIGEST_REC))
    wide = np.zeros(max(first.wide.size, 1), dtype=np.uint64)
    st = N.KwDigest(recs.ctypes.data_as(C.POINTER(N.KwDigestRec)), recs.size, 0,
                    wide.ctypes.data_as(C.POINTER(C.c_uint64)), wide.size, 0, 0)
    count = K.Summary(n, npol, planes=False)
    b.summary(out=count)
    walls = []
    for alt in range(5):
        t_s, _ = wall(lambda: b.summary(out=count))
        t_d, rc = wall(lambda: N.lib().kw_batch_digest(b._h, C.byref(st)))
        assert rc == N.KW_OK and st.n == first.recs.size
        walls.append(t_d)
        say(f"    alternation {alt}: wall summary without planes {t_s:.3f} ms, digest {t_d:.3f} ms "
            f"({st.n * 24 / 1e3:.1f} kB of records back)")
    assert recs[:st.n].tobytes() == first.recs.tobytes()
    t_read, words = wall(b.verdicts)
    t_red, ref = wall(lambda: b.digest_from_words(words, npol, cap=recs.size, wide_cap=wide.size))
    same = (ref.findings == first.findings and ref.recs.tobytes() == first.recs.tobytes() and np.array_equal(ref.wide, first.wide))
    best = min(walls)
    say(f"    the host path: kw_batch_verdicts {t_read:.1f} ms + kw_debug_digest_words {t_red:.1f} ms = {t_read + t_red:.1f} ms; "
        f"kw_batch_digest {best:.3f} ms (best of 5): {(t_read + t_red) / best:.0f}x; records equal: {same}")
    assert same
    b.close()


def main():
    argv = sys.argv[1:]
    n = int(argv[0]) if argv else 1_000_000
    for name in (argv[1:] or ["c4_64", "c2_trusted", "c3_group"]):
        run(name, n)


if __name__ == "__main__":
    main()
