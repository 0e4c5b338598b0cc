"""The AdmissionResponse bodies of chosen pairs on the device (kw_batch_responses) against what a
caller had to do before it: one format_response per item on the host (kw_debug_responses_words
how=0), on one thread and spread over 16, same process, same box (profiles/r19_responses.txt).

  python scripts/responses_bench.py [rows] [config]   on the GPU box: C4 at 1M rows, AUDIT.
    The item sets of scripts/messages_bench.py: one resident kw_validate_batch pass, its digest and
    the members of the largest group and of the 32 groups with the most findings. Per selection:
    kw_batch_responses once untimed (first touch, the pools, the uid column and the container names),
    then three calls into a page-locked text buffer (kw_host_alloc) and three into a pageable one, by
    the host clock around each call (it ends in a stream synchronise). KW_BULK_DEBUG makes the library
    print its [kw responses] line, which this script passes through: the three steps by HIP events
    inside the call, the offsets' read-back, the text's read-back. Then kw_batch_messages over the same
    items into the page-locked buffer (its [kw messages] lines: the device steps side by side, and the
    message bytes an item beside the response bytes). Then the host reference on one thread and over
    16 threads (each a slice of the items into its own arrays, made and touched before the timing):
    once untimed, three times timed, and the results compared byte for byte.
"""
import os
import sys
import threading
import time

os.environ.setdefault("KW_BULK_DEBUG", "1")  # (read once per process)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "policy-server_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]
import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402

import kwgpu as K  # noqa: E402
from helpers import config  # noqa: E402
from kwgpu import _native as N  # noqa: E402
from messages_bench import CONFIGS, NS, THREADS, p32, p64, say, span, wall  # noqa: E402


class HostFormatter:
    """how=0 over the items in `threads` slices, each into its own arrays (sized from the device's
    offsets). The arrays are made and touched once, outside the timed region; render() times the calls
    alone (thread start and join included for more than one thread)."""

    def __init__(self, env, arr, npol, b, words, rows, cols, off, threads):
        self.env, self.arr, self.npol, self.b, self.words, self.threads = env, arr, npol, b, words, threads
        n = rows.size
        cuts = [n * t // threads for t in range(threads + 1)]
        self.parts = []
        for t in range(threads):
            r, c = np.ascontiguousarray(rows[cuts[t]:cuts[t + 1]]), np.ascontiguousarray(cols[cuts[t]:cuts[t + 1]])
            m = r.size
            o = np.zeros(m + 1, dtype=np.uint64)
            host = np.zeros(max(m, 1), dtype=np.uint64)
            text = np.ones(max(int(off[cuts[t + 1]] - off[cuts[t]]), 1), dtype=np.uint8)  # (ones: every page is touched)
            st = N.KwResponses(p64(o), text.ctypes.data, text.size, 0, None, p64(host), host.size, 0)
            self.parts.append((r, c, m, o, host, text, st))

    def _work(self, t):
        r, c, m, o, host, text, st = self.parts[t]
        rc = N.lib().kw_debug_responses_words(self.env._h, self.b._h, self.arr, self.npol, p32(self.words), self.words.size // self.npol,
                                              p64(r), p32(c), m, 0, C.byref(st))
        assert rc == N.KW_OK, rc

    def render(self):
        t0 = time.perf_counter()
        if self.threads == 1:
            self._work(0)
        else:
            ts = [threading.Thread(target=self._work, args=(t,)) for t in range(self.threads)]
            for t in ts:
                t.start()
            for t in ts:
                t.join()
        return (time.perf_counter() - t0) * 1e3

    def result(self):
        """(lengths, text) of the last render, outside any timing."""
        return (np.concatenate([np.diff(p[3].astype(np.int64)) for p in self.parts]),
                np.concatenate([p[5][:p[6].bytes] for p in self.parts]))


def run(name, n):
    env = K.EvaluationEnvironment(config(name), continue_on_errors=True, always_accept_namespace=NS, device=0)
    ids = env.policy_ids()
    npol = len(ids)
    arr = env._array(ids)
    b = K.SynthBatch(CONFIGS[name], n, seed=4).batch().to_device(0)
    b.validate(env, ids, K.AUDIT)
    say(f"{name}: {n} rows x {npol} policies = {n * npol / 1e6:.1f} M pairs, words {n * npol * 4 / 1e6:.1f} MB, AUDIT")
    d = b.digest()
    say(f"    {d.findings} findings, {d.recs.size} groups, {d.wide.size} wide")
    words = b.verdicts()
    by_count = d.recs[np.argsort(-d.recs["count"].astype(np.int64), kind="stable")]
    sets = (("the largest group", by_count[:1]), ("the 32 groups with the most findings", by_count[:32]))
    for label, recs in sets:
        recs = np.ascontiguousarray(recs)
        m = b.digest_members(recs, words=False)
        rows = np.ascontiguousarray(m.rows)
        cols = np.repeat(recs["col"].astype(np.uint32), np.diff(m.off.astype(np.int64)))
        ni = rows.size
        first = b.responses(env, ids, rows, cols)  # untimed
        nbytes = first.text.size
        say(f"  {label}: {recs.size} groups, {ni} items, {nbytes} response bytes ({nbytes / 1e6:.2f} MB, {nbytes / max(ni, 1):.1f} a response), "
            f"{first.host.size} for the host, stats {b.debug_responses_stats()}; PCIe at 55-57 GB/s: {nbytes / 56e6:.2f} ms")
        off = np.zeros(ni + 1, dtype=np.uint64)
        host = np.zeros(max(first.host.size, 1), dtype=np.uint64)
        pinned = C.c_void_p()
        assert N.lib().kw_host_alloc(0, max(nbytes, 1), C.byref(pinned)) == N.KW_OK
        pageable = np.zeros(max(nbytes, 1), dtype=np.uint8)
        for kind, ptr in (("page-locked", pinned.value), ("pageable", pageable.ctypes.data)):
            st = N.KwResponses(p64(off), ptr, nbytes, 0, None, p64(host), host.size, 0)
            walls = []
            for rep in range(3):
                t, rc = wall(lambda: N.lib().kw_batch_responses(b._h, env._h, arr, npol, p64(rows), p32(cols), ni, C.byref(st)))
                assert rc == N.KW_OK and st.bytes == nbytes
                walls.append(t)
            got = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(max(nbytes, 1),))[:nbytes]
            assert got.tobytes() == first.text.tobytes() and np.array_equal(off, first.off)
            say(f"    kw_batch_responses into a {kind} text buffer, the call by the host clock: {span(walls)} "
                f"({nbytes / 1e6 / min(walls):.2f} GB/s of text at best)")
            dev_walls = walls if kind == "page-locked" else dev_walls
        # the messages call over the same items, for the device steps side by side
        msgs = b.messages(env, ids, rows, cols)  # untimed
        moff = np.zeros(ni + 1, dtype=np.uint64)
        st = N.KwMessages(p64(moff), pinned.value, nbytes, 0, None, p64(host), host.size, 0)  # (a message is shorter than its response)
        walls = []
        for rep in range(3):
            t, rc = wall(lambda: N.lib().kw_batch_messages(b._h, env._h, arr, npol, p64(rows), p32(cols), ni, C.byref(st)))
            assert rc == N.KW_OK and st.bytes == msgs.text.size
            walls.append(t)
        say(f"    kw_batch_messages over the same items, page-locked: {span(walls)}; {msgs.text.size / max(ni, 1):.1f} bytes a message "
            f"against {nbytes / max(ni, 1):.1f} a response")
        N.lib().kw_host_free(pinned)
        lens = np.diff(first.off.astype(np.int64))
        for threads in (1, THREADS):
            hf = HostFormatter(env, arr, npol, b, words, rows, cols, first.off, threads)
            hf.render()  # untimed
            walls = [hf.render() for rep in range(3)]
            hl, ht = hf.result()
            del hf
            same = np.array_equal(hl, lens) and ht.tobytes() == first.text.tobytes()
            say(f"    kw_debug_responses_words how=0 on {threads} host thread(s): {span(walls)} ({min(walls) * 1e3 / max(ni, 1):.3f} us an item at best); "
                f"bytes equal to the device's: {same}")
            assert same
            if threads == THREADS:
                say(f"    device (page-locked) {span(dev_walls)} against {THREADS} host threads {span(walls)}: "
                    f"{'the ranges do not overlap, the device call is ' + format(min(walls) / max(dev_walls), '.1f') + 'x faster at the least' if max(dev_walls) < min(walls) else 'the host threads are ' + format(min(dev_walls) / max(walls), '.1f') + 'x faster at the least' if max(walls) < min(dev_walls) else 'THE RANGES OVERLAP'}")
    b.close()


def main():
    argv = sys.argv[1:]
    n = int(argv[0]) if argv else 1_000_000
    for name in (argv[1:] or ["c4_64"]):
        run(name, n)


if __name__ == "__main__":
    main()
