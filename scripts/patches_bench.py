"""The JSONPatch of accepted mutations on the device (kw_batch_patches) against the only way a caller
had before it: one kw_format_response_doc per pair on the host, which parses the pair's whole
document again, on one thread and spread over 16, same process, same box (profiles/r21_patches.txt).

  python scripts/patches_bench.py [rows] [config]   on the GPU box: C4 at 1M rows, AUDIT.
    One resident kw_validate_batch pass over a batch made from columns (SynthBatch), its shape columns
    set with kw_batch_set_patch_shape: the synthetic documents always carry
    securityContext.capabilities.add and drop arrays under /spec or /spec/template/spec, so the shapes
    are known without JSON. The items are every pair whose word has KW_F_PATCH. Per form:
    kw_batch_patches once untimed (first touch, the pools, the shape columns and the uids), then three
    calls into a page-locked text buffer (kw_host_alloc) and three into a pageable one, by the host
    clock around each call (it ends in a stream synchronise). KW_BULK_DEBUG makes the library print
    its [kw patches] line, which this script passes through. Then the host: a sample of the pairs
    (every k-th, their documents from SynthBatch.json made before the timing), one
    kw_format_response_doc each through ctypes, on one thread and over 16 threads (a slice each),
    once untimed, three times timed, scaled to all pairs; the same loop over calls that return at
    their argument check gives the share of the calling overhead. The sample's bytes are compared
    with the device's. The 16 threads are Python threads: between calls of a few microseconds they
    queue for the interpreter's lock, so read the 16-thread line beside its marshalling share
    (profiles/r21_patches.txt found it slower than one thread).
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

SAMPLE = 40000


def synthetic_shapes(b):
    """The shape columns of a SynthBatch batch from its columns alone."""
    v = b.view()
    n = int(v.n_requests)
    ctr_off = np.ctypeslib.as_array(v.ctr_off, shape=(n + 1,)).astype(np.int64)
    nc = int(ctr_off[n])
    flags = np.ctypeslib.as_array(v.ctr_flags, shape=(max(nc, 1),))[:nc]
    req = np.ctypeslib.as_array(v.req_flags, shape=(n,))
    koff = np.ctypeslib.as_array(v.kind.off, shape=(n + 1,)).astype(np.int64)
    kbytes = np.ctypeslib.as_array(v.kind.bytes, shape=(int(koff[n]),))
    is_pod = (np.diff(koff) == 3) & (kbytes[np.minimum(koff[:-1], max(kbytes.size - 1, 0))] == ord("P"))
    pointer = np.where((req & N.KW_REQ_HAS_PODSPEC) == 0, N.KW_PP_NONE, np.where(is_pod, N.KW_PP_POD, N.KW_PP_TEMPLATE)).astype(np.uint8)
    # a container's index in its own list: its place in the run of its kind within the row
    kind = (flags & 6).astype(np.int64)
    row_of = np.repeat(np.arange(n), np.diff(ctr_off))
    key = row_of * 8 + kind
    start = np.r_[True, key[1:] != key[:-1]] if nc else np.zeros(0, dtype=bool)
    first = np.maximum.accumulate(np.where(start, np.arange(nc), 0)) if nc else np.zeros(0, dtype=np.int64)
    index = np.arange(nc) - first
    place = (np.uint32((N.KW_PS_CAPS + N.KW_PS_ADD_ARRAY + N.KW_PS_DROP_ARRAY) << N.KW_PS_SHIFT) | index.astype(np.uint32)).astype(np.uint32)
    return place, pointer


class HostDocs:
    """kw_format_response_doc per sampled pair in `threads` slices; the documents and the argument
    tuples are made before the timing."""

    def __init__(self, env, b, ids, words, rows, cols, docs, threads):
        npol = len(ids)
        idx = [env._idx(i) for i in ids]
        self.f = N.lib().kw_format_response_doc
        self.b, self.env, self.threads = b, env, threads
        args = [(env._h, b._h, int(r), idx[int(c)], int(words[int(r) * npol + int(c)]), None, docs[int(r)], len(docs[int(r)]),
                 N.KW_DOC_ADMISSION_REVIEW) for r, c in zip(rows.tolist(), cols.tolist())]
        cuts = [len(args) * t // threads for t in range(threads + 1)]
        self.parts = [args[cuts[t]:cuts[t + 1]] for t in range(threads)]
        self.out = [[] for _ in range(threads)]

    def _work(self, t, keep, skip_rows):
        f, buf, need = self.f, C.create_string_buffer(1 << 16), C.c_size_t()
        out = []
        for a in self.parts[t]:
            if skip_rows:  # the same marshalling, a return at the argument check
                f(a[0], a[1], 1 << 62, *a[3:], buf, len(buf), C.byref(need))
                continue
            rc = f(*a, buf, len(buf), C.byref(need))
            assert rc == N.KW_OK, rc
            if keep:
                out.append(buf.value)
        self.out[t] = out

    def render(self, keep=False, skip_rows=False):
        t0 = time.perf_counter()
        if self.threads == 1:
            self._work(0, keep, skip_rows)
        else:
            ts = [threading.Thread(target=self._work, args=(t, keep, skip_rows)) for t in range(self.threads)]
            for t in ts:
                t.start()
            for t in ts:
                t.join()
        return (time.perf_counter() - t0) * 1e3


def run(name, n):
    policies = config(name)
    env = K.EvaluationEnvironment(policies, continue_on_errors=True, always_accept_namespace=NS, device=0)
    ids = env.policy_ids()
    npol = len(ids)
    arr = env._array(ids)
    syn = K.SynthBatch(CONFIGS[name], n, seed=4)
    b = syn.batch()
    t, _ = wall(lambda: b.set_patch_shape(*synthetic_shapes(b)))
    say(f"{name}: {n} rows x {npol} policies = {n * npol / 1e6:.1f} M pairs, AUDIT; the shape columns from the columns: {t:.1f} ms")
    b.to_device(0)
    b.validate(env, ids, K.AUDIT)
    words = b.verdicts()
    w2 = words.reshape(n, npol)
    r, c = np.nonzero(w2 & np.uint32(N.KW_F_PATCH))
    rows, cols = np.ascontiguousarray(r.astype(np.uint64)), np.ascontiguousarray(c.astype(np.uint32))
    ni = rows.size
    say(f"  {ni} pairs carry KW_F_PATCH ({100.0 * ni / (n * npol):.2f} % of all), in {np.unique(cols).size} columns, on {np.unique(rows).size} rows")
    pick = np.arange(0, ni, max(1, ni // SAMPLE))
    docs = {int(x): syn.json(int(x)).encode() for x in np.unique(rows[pick])}
    say(f"  the host sample: {pick.size} pairs, {len(docs)} documents of {sum(map(len, docs.values())) / max(len(docs), 1):.0f} bytes on average")
    results = {}
    for form, fname in ((N.KW_PATCH_OPS, "KW_PATCH_OPS"), (N.KW_PATCH_RESPONSE, "KW_PATCH_RESPONSE")):
        first = b.patches(env, ids, rows, cols, form=form)  # untimed
        nbytes = first.text.size
        assert first.host.size == 0
        say(f"  {fname}: {ni} items, {nbytes} bytes ({nbytes / 1e6:.2f} MB, {nbytes / max(ni, 1):.1f} an item), stats {b.debug_patches_stats()}; "
            f"PCIe at 55-57 GB/s: {nbytes / 56e6:.2f} ms")
        off = np.zeros(ni + 1, dtype=np.uint64)
        host = np.zeros(1, dtype=np.uint64)
        pinned = C.c_void_p()
        assert N.lib().kw_host_alloc(0, max(nbytes, 1), C.byref(pinned)) == N.KW_OK
        pageable = np.zeros(max(nbytes, 1), dtype=np.uint8)
        for kind, ptr in (("page-locked", pinned.value), ("pageable", pageable.ctypes.data)):
            st = N.KwResponses(p64(off), ptr, nbytes, 0, None, p64(host), host.size, 0)
            walls = []
            for rep in range(3):
                t, rc = wall(lambda: N.lib().kw_batch_patches(b._h, env._h, arr, npol, p64(rows), p32(cols), ni, form, C.byref(st)))
                assert rc == N.KW_OK and st.bytes == nbytes
                walls.append(t)
            got = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(max(nbytes, 1),))[:nbytes]
            assert got.tobytes() == first.text.tobytes() and np.array_equal(off, first.off)
            say(f"    kw_batch_patches into a {kind} text buffer, the call by the host clock: {span(walls)} "
                f"({nbytes / 1e6 / min(walls):.2f} GB/s of text at best)")
            if kind == "page-locked":
                results[form] = walls
        N.lib().kw_host_free(pinned)
        if form == N.KW_PATCH_RESPONSE:
            device_sample = [first.get(int(i)) for i in pick]
    scale = ni / pick.size
    for threads in (1, THREADS):
        hd = HostDocs(env, b, ids, words, rows[pick], cols[pick], docs, threads)
        hd.render(keep=True)  # untimed
        same = [x for part in hd.out for x in part] == device_sample
        walls = [hd.render() for rep in range(3)]
        over = [hd.render(skip_rows=True) for rep in range(3)]
        scaled = [w * scale for w in walls]
        say(f"  kw_format_response_doc per pair on {threads} host thread(s), {pick.size} pairs: {span(walls)} "
            f"({min(walls) * 1e3 / pick.size:.2f} us a pair at best, of which the call's marshalling alone {min(over) * 1e3 / pick.size:.2f} us); "
            f"scaled to {ni} pairs: {span(scaled)}; bytes equal to the device's: {same}")
        assert same
        for form, fname in ((N.KW_PATCH_OPS, "KW_PATCH_OPS"), (N.KW_PATCH_RESPONSE, "KW_PATCH_RESPONSE")):
            d = results[form]
            verdict = (f"the device call is {min(scaled) / max(d):.1f}x faster at the least" if max(d) < min(scaled)
                       else f"the host threads are {min(d) / max(scaled):.1f}x faster at the least" if max(scaled) < min(d) else "THE RANGES OVERLAP")
            say(f"    device {fname} (page-locked) {span(d)} against {threads} host thread(s) {span(scaled)}: {verdict}")
    b.close()


def main():
    argv = sys.argv[1:]
    n = int(argv[0]) if argv else 1_000_000
    for name in (argv[1:] or ["c4_64"]):
        run(name, n)


if __name__ == "__main__":
    main()
