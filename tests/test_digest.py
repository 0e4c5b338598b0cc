"""The violation digest (include/kwgpu.h kw_batch_digest; policy-server_amd/csrc/digest.hpp) on the
host: the words of the host walk (pinned to the oracle elsewhere) go through the reference reducer
(kw_debug_digest_words) and must equal a restatement in Python (tests/digest_cases.py: a dict keyed by
(col, reason, allowed, key) with the keys cut from Batch.view() by the header's table, not through
kw_batch_finding_key); kw_batch_finding_key against the same cuts; the totals; the key tied to the
messages kw_format_response gives; the argument errors and both KW_E_NOSPACE forms.
tests/digest_check.cpp runs digest.hpp alone (key rules, order, capacity arithmetic, range halving,
the leftover list's overflow) as a plain executable under AddressSanitizer and UBSan (no Python in
that process)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import digest_cases as DC
import kwgpu as K
import outcomes_cases as OC
from helpers import config, many_policies_config, wide_docs, wide_entity_case
from kwgpu import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "policy-server_amd")
CXX = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
NS = "kubewarden"
ROWS = 300
WORKLOADS = ["c2", "c3", "c4", "c5", "c6", "parity", "wide_docs", "wide_entity"]
_memo = {}


def workload(name):
    """(env, ids, batch, origin, words of the host walk, Columns), made once."""
    if name in _memo:
        return _memo[name]
    origin = K.AUDIT
    if name in ("c2", "c3", "c4", "c5"):
        cfg = {"c2": "c2_trusted", "c3": "c3_group", "c4": "c4_64", "c5": "c5_mixed"}[name]
        env = K.EvaluationEnvironment(config(cfg), continue_on_errors=True, always_accept_namespace=NS)
        batch = K.SynthBatch(int(name[1]), ROWS, seed=700 + int(name[1])).batch()
    elif name == "c6":  # a 40-member group: its causes do not fit the word (wide findings)
        env = K.EvaluationEnvironment(many_policies_config(), continue_on_errors=True, always_accept_namespace=NS)
        batch = K.SynthBatch(6, 150, seed=706).batch()
    elif name == "parity":  # privileged containers, namespaces, monitor mode, an initialisation error
        env = K.EvaluationEnvironment(OC.policies(), continue_on_errors=True, always_accept_namespace=NS)
        batch, origin = K.Batch.from_json(OC.docs(ROWS)), K.VALIDATE
    elif name == "wide_docs":
        env = K.EvaluationEnvironment(config("c4_64"), continue_on_errors=True, always_accept_namespace=NS)
        batch = K.Batch.from_json(wide_docs())
    else:
        doc, pols = wide_entity_case()
        env = K.EvaluationEnvironment(pols, continue_on_errors=True)
        batch, origin = K.Batch.from_json([doc]), K.VALIDATE
    ids = env.policy_ids()
    _memo[name] = (env, ids, batch, origin, batch.debug_host_walk(env, ids, origin), DC.Columns(batch))
    return _memo[name]


def reference(name):
    """(Digest of the reference reducer, (groups, wide, findings) of the restatement), made once."""
    key = ("ref", name)
    if key not in _memo:
        env, ids, batch, origin, w, cols = workload(name)
        _memo[key] = (batch.digest_from_words(w, len(ids)), DC.expected(cols, w, len(ids)))
    return _memo[key]


def test_fixture_is_not_vacuous():
    """What the other tests rely on: every reason 1-13 but the ones no workload can reach occurs, so
    do findings that were let through, two-string keys, wide findings and groups of many members."""
    reasons, allowed, wide, biggest, kv = set(), 0, 0, 0, 0
    for name in WORKLOADS:
        d, (groups, w, findings) = reference(name)
        assert findings > 0, name
        reasons |= {k[1] for k in groups}
        allowed += sum(1 for k in groups if k[2])
        kv += sum(1 for k in groups if k[1] == 11)
        wide += len(w)
        biggest = max([biggest] + [g[2] for g in groups.values()])
    assert {1, 2, 3, 5, 6, 8, 9, 10, 11, 12, 13, 15} <= reasons, sorted(reasons)
    assert allowed > 0 and wide > 0 and kv > 1 and biggest > 50
    assert len(reference("wide_entity")[1][0]) == 4 and len(reference("c6")[1][1]) > 0


@pytest.mark.parametrize("name", WORKLOADS)
def test_reducer_matches_the_restatement(name):
    env, ids, batch, origin, w, cols = workload(name)
    d, (groups, wide, findings) = reference(name)
    want = DC.as_records(groups)
    assert d.recs.size == want.size
    assert d.recs.tobytes() == want.tobytes(), np.nonzero(d.recs != want)[0][:8]
    assert d.wide.tolist() == wide and d.wide.dtype == np.uint64
    # the totals: every word with a reason is in one group or in the wide list
    assert d.findings == findings == int(np.count_nonzero((w >> np.uint32(8)) & np.uint32(0xFF)))
    assert int(d.recs["count"].sum()) + d.wide.size == d.findings
    # ordered by (col, reason, first_row), which is total: no two groups of a column share a first row
    order = [(int(r["col"]), (int(r["word"]) >> 8) & 0xFF, int(r["first_row"])) for r in d.recs]
    assert order == sorted(order)
    assert len({(c, f) for c, _, f in order}) == len(order)
    # word is the word of (first_row, col)
    w2 = w.reshape(-1, len(ids))
    assert all(int(w2[int(r["first_row"]), int(r["col"])]) == int(r["word"]) for r in d.recs)
    again = batch.digest_from_words(w, len(ids))
    assert DC.same(d, again)  # the same input, the same bytes


@pytest.mark.parametrize("name", WORKLOADS)
def test_finding_key_matches_the_cuts(name):
    env, ids, batch, origin, w, cols = workload(name)
    w2 = w.reshape(-1, len(ids))
    rr, cc = np.nonzero((w2 >> np.uint32(8)) & np.uint32(0xFF))
    step = max(1, rr.size // 1500)
    for r, c in list(zip(rr.tolist(), cc.tolist()))[::step]:
        word = int(w2[r, c])
        reason = (word >> 8) & 0xFF
        if (word >> 16) == N.KW_ARG_WIDE and reason in DC.WIDE_REASONS:
            continue
        want = cols.key(r, word)
        got = batch.finding_key(r, word)
        if isinstance(want, int) or want == ():
            assert got == (b"", None), (r, c, hex(word))
        elif len(want) == 2:
            assert got == want, (r, c, hex(word))
        else:
            assert got == (want[0], None), (r, c, hex(word))


def test_two_strings_keep_their_lengths_apart():
    """("ab", "c") and ("a", "bc") under one constraint policy are two groups; equal pairs one."""
    mod = "registry://ghcr.io/kubewarden/policies/safe-labels:v0.1.14"
    pols = {"labels": {"module": mod, "settings": {"constrained_labels": {"ab": "^x$", "a": "^x$"}}}}
    docs = []
    for i, labels in enumerate(({"ab": "c"}, {"a": "bc"}, {"ab": "c"}, {"a": "bc"}, {"a": "x"})):
        docs.append({"request": {"uid": str(i), "kind": {"group": "", "version": "v1", "kind": "Pod"},
                                 "resource": {"group": "", "version": "v1", "resource": "pods"}, "operation": "CREATE",
                                 "userInfo": {}, "object": {"kind": "Pod", "metadata": {"labels": labels},
                                                            "spec": {"containers": [{"name": "c", "image": "nginx"}]}}}})
    env = K.EvaluationEnvironment(pols, continue_on_errors=True)
    b = K.Batch.from_json(docs)
    w = b.debug_host_walk(env, env.policy_ids())
    d = b.digest_from_words(w, 1)
    assert [(int(r["first_row"]), int(r["count"])) for r in d.recs] == [(0, 2), (1, 2)] and d.findings == 4
    assert b.finding_key(0, int(d.recs[0]["word"])) == (b"ab", b"c")
    assert b.finding_key(1, int(d.recs[1]["word"])) == (b"a", b"bc")


def _message(env, batch, ids, row, col, word):
    resp = batch.format_response(env, row, ids[col], word)
    return (resp.get("status") or {}).get("message")


@pytest.mark.parametrize("name", ["c4", "c2", "parity", "wide_entity"])
def test_the_key_is_what_the_message_quotes(name):
    """All pairs of a group format to the same status message (for the reasons that name a container,
    after the leading container '<name>' is cut), two groups of one (col, reason, allowed) to
    different ones."""
    env, ids, batch, origin, w, cols = workload(name)
    w2 = w.reshape(-1, len(ids))
    members = {}
    rr, cc = np.nonzero((w2 >> np.uint32(8)) & np.uint32(0xFF))
    for r, c in zip(rr.tolist(), cc.tolist()):
        word = int(w2[r, c])
        reason = (word >> 8) & 0xFF
        if not 1 <= reason <= 12 or env.is_group(env._idx(ids[c])):
            continue
        members.setdefault((c, reason, bool(word & N.KW_F_ALLOWED), cols.key(r, word)), []).append((r, word))
    assert members
    by_class = {}
    checked = 0
    for k, pairs in members.items():
        msgs = set()
        for r, word in pairs:
            m = _message(env, batch, ids, r, k[0], word)
            if m is not None and 3 <= k[1] <= 9:
                cut = re.sub(r"^container '[^']*' ", "", m)
                assert cut != m, m
                m = cut
            msgs.add(m)
        assert len(msgs) == 1, (k, msgs)
        checked += len(pairs)
        by_class.setdefault(k[:3], []).append(msgs.pop())
    assert checked > 0
    for cls, msgs in by_class.items():
        said = [m for m in msgs if m is not None]
        assert len(set(said)) == len(said), (cls, said[:4])


def _call_words(batch, words, rows, npol, cap, wide_cap, recs=True, wide=True):
    r = np.zeros(max(cap, 1), dtype=np.dtype(K.DIGEST_REC))
    wd = np.zeros(max(wide_cap, 1), dtype=np.uint64)
    st = N.KwDigest(r.ctypes.data_as(C.POINTER(N.KwDigestRec)) if recs else None, cap, 0,
                    wd.ctypes.data_as(C.POINTER(C.c_uint64)) if wide else None, wide_cap, 0, 0)
    rc = N.lib().kw_debug_digest_words(batch._h, None if words is None else words.ctypes.data_as(C.POINTER(C.c_uint32)),
                                       rows, npol, C.byref(st))
    return rc, st


def test_nospace_forms_and_argument_errors():
    env, ids, batch, origin, w, cols = workload("c6")
    d, _ = reference("c6")
    npol, rows = len(ids), batch.n
    assert d.recs.size > 1 and d.wide.size > 1
    # a record array one too small, a wide list one too small: KW_E_NOSPACE with the exact needs
    for cap, wide_cap in ((d.recs.size - 1, d.wide.size), (d.recs.size, d.wide.size - 1), (0, 0)):
        rc, st = _call_words(batch, w, rows, npol, cap, wide_cap)
        assert rc == N.KW_E_NOSPACE and (st.n, st.nwide, st.findings) == (d.recs.size, d.wide.size, d.findings)
        with pytest.raises(K.DigestNoSpace) as e:
            batch.digest_from_words(w, npol, cap=cap, wide_cap=wide_cap)
        assert (e.value.need, e.value.need_wide) == (d.recs.size, d.wide.size)
    rc, st = _call_words(batch, w, rows, npol, d.recs.size, d.wide.size)  # exactly enough
    assert rc == N.KW_OK and st.n == d.recs.size
    assert DC.same(batch.digest_from_words(w, npol, cap=d.recs.size, wide_cap=d.wide.size), d)
    # fewer rows than the batch holds are a prefix; more are an error
    half = batch.digest_from_words(w[:(rows // 2) * npol], npol)
    assert half.findings == int(np.count_nonzero((w[:(rows // 2) * npol] >> np.uint32(8)) & np.uint32(0xFF)))
    assert _call_words(batch, np.zeros((rows + 1) * npol, dtype=np.uint32), rows + 1, npol, 8, 8)[0] == N.KW_E_ARG
    assert _call_words(batch, w, rows, 0, 8, 8)[0] == N.KW_E_ARG
    assert _call_words(batch, None, rows, npol, 8, 8)[0] == N.KW_E_ARG
    assert _call_words(batch, w, rows, npol, 8, 8, recs=False)[0] == N.KW_E_ARG
    assert _call_words(batch, w, rows, npol, 8, 8, wide=False)[0] == N.KW_E_ARG
    assert N.lib().kw_debug_digest_words(batch._h, w.ctypes.data_as(C.POINTER(C.c_uint32)), rows, npol, None) == N.KW_E_ARG
    # no words at all: an empty digest
    none = batch.digest_from_words(np.zeros(rows * npol, dtype=np.uint32), npol)
    assert none.recs.size == 0 and none.wide.size == 0 and none.findings == 0
    assert batch.digest_from_words(np.zeros(0, dtype=np.uint32), npol).findings == 0


def test_finding_key_errors():
    env, ids, batch, origin, w, cols = workload("c4")
    d, _ = reference("c4")
    r = next(r for r in d.recs if (int(r["word"]) >> 8) & 0xFF == 11)
    row, word = int(r["first_row"]), int(r["word"])
    key, val = batch.finding_key(row, word)
    L = N.lib()
    need, split = C.c_size_t(), C.c_size_t()
    buf = C.create_string_buffer(64)

    def call(row, word, cap):
        return L.kw_batch_finding_key(batch._h, row, word, buf, cap, C.byref(need), C.byref(split))
    assert call(row, word, len(key) + len(val) - 1) == N.KW_E_NOSPACE
    assert (need.value, split.value) == (len(key) + len(val), len(key))
    assert call(row, word, len(key) + len(val)) == N.KW_OK and buf.raw[:need.value] == key + val
    assert call(batch.n, word, 64) == N.KW_E_ARG           # a row outside the batch
    assert call(row, word & 0xFF, 64) == N.KW_E_ARG        # not a finding
    assert call(row, (8 << 8) | (0xFFFF << 16), 64) == N.KW_E_ARG  # a wide finding has no key here
    assert call(row, (12 << 8) | (0xFFFF << 16), 0) == N.KW_OK and need.value == 0  # a number, whatever it is
    assert call(row, 0xA5A5A5A5, 0) == N.KW_OK and need.value == 0  # the poison sentinel's reason: a number
    assert L.kw_batch_finding_key(batch._h, row, word, buf, 64, None, C.byref(split)) == N.KW_E_ARG


def test_device_entry_needs_a_pass():
    env, ids, batch, origin, w, cols = workload("c4")
    with pytest.raises(K.EvaluationError) as e:
        batch.digest()  # never on a device
    assert e.value.code == N.KW_E_ARG
    with pytest.raises(K.EvaluationError) as e:
        batch.debug_digest_stats()
    assert e.value.code == N.KW_E_ARG


def test_digest_check_under_sanitizers(tmp_path):
    exe = tmp_path / "digest_check"
    subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(PKG, "csrc"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "digest_check.cpp")], check=True)
    # (out-of-bounds accesses and undefined behaviour are the point; the leak check at exit needs
    # ptrace rights a test runner may lack)
    out = subprocess.run([str(exe)], check=False, capture_output=True, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "failures 0" in out.stdout
