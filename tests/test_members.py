"""The digest's drill-down (include/kwgpu.h kw_batch_digest_members; policy-server_amd/csrc/members.hpp)
on the host: the words of the host walk go through the reference reducer
(kw_debug_digest_members_words) and must equal a restatement in Python (tests/members_cases.py: the
findings bucketed by (col, reason, allowed, key) with the keys cut from Batch.view()); the properties
the header promises for the records of a digest; a group named by any of its members; the members'
messages; hand cases; every argument error that needs no device and KW_E_NOSPACE.
tests/members_check.cpp runs members.hpp alone (table geometry, all-equal tags, duplicate detection,
the order, the capacity arithmetic) as a plain executable under AddressSanitizer and UBSan (no Python
in that process)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import kwgpu as K
import members_cases as MC
from kwgpu import _native as N
from test_digest import reference, workload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "policy-server_amd")
CXX = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
WORKLOADS = ["c2", "c3", "c4", "c5", "c6", "parity", "wide_docs", "wide_entity"]
SELECTIONS = ["all", "third_reversed", "largest", "singletons", "none"]


@pytest.mark.parametrize("name", WORKLOADS)
def test_reducer_matches_the_restatement(name):
    env, ids, batch, origin, w, cols = workload(name)
    d, _ = reference(name)
    npol = len(ids)
    sel = MC.selections(d.recs)
    assert sel["all"].size > 0 and sel["largest"].size == 1
    for s in SELECTIONS:
        recs = sel[s]
        got = batch.digest_members_from_words(w, npol, recs)
        off, rows, words = MC.expected(cols, w, npol, recs)
        assert got.off.dtype == np.uint64 and got.rows.dtype == np.uint64 and got.words.dtype == np.uint32
        assert np.array_equal(got.off, off), (name, s)
        assert np.array_equal(got.rows, rows) and np.array_equal(got.words, words), (name, s)
        assert got.rows.size == int(recs["count"].sum())  # n is the sum of the counts
        if recs.size:
            MC.check_properties(got, recs, w, npol)
        assert MC.same(got, batch.digest_members_from_words(w, npol, recs))  # the same input, the same bytes
        rows_only = batch.digest_members_from_words(w, npol, recs, with_words=False)  # words = NULL
        assert rows_only.words is None and np.array_equal(rows_only.rows, rows) and np.array_equal(rows_only.off, off)


def test_fixture_is_not_vacuous():
    singles = many = 0
    for name in WORKLOADS:
        d, _ = reference(name)
        singles += int((d.recs["count"] == 1).sum())
        many += int((d.recs["count"] > 1).sum())
    assert singles > 10 and many > 10
    d, _ = reference("c4")
    assert d.recs[::3][::-1].size > 10 and int(d.recs["count"].max()) > 50


@pytest.mark.parametrize("name", ["c4", "c3", "parity"])
def test_a_record_need_not_be_the_lowest_row(name):
    """Naming a group by its last member, with that member's word, gives the same members."""
    env, ids, batch, origin, w, cols = workload(name)
    d, _ = reference(name)
    npol = len(ids)
    first = batch.digest_members_from_words(w, npol, d.recs)
    last = d.recs.copy()
    for g in range(d.recs.size):
        e = int(first.off[g + 1]) - 1
        last[g]["first_row"], last[g]["word"], last[g]["count"] = first.rows[e], first.words[e], 0  # (count is ignored)
    assert (last["first_row"] != d.recs["first_row"]).any()
    assert MC.same(batch.digest_members_from_words(w, npol, last), first)


@pytest.mark.parametrize("name", ["c4", "parity"])
def test_members_format_to_one_message(name):
    """Every member of a sampled group formats, from the returned (row, word) alone, to the same status
    message once the leading container '<name>' is cut (tests/test_digest.py's check on the pairs this
    entry returns)."""
    env, ids, batch, origin, w, cols = workload(name)
    d, _ = reference(name)
    recs = d.recs[[(int(x) >> 8) & 0xFF in range(1, 13) and not env.is_group(env._idx(ids[int(c)]))
                   for x, c in zip(d.recs["word"], d.recs["col"])]]
    recs = recs[recs["count"] > 1][::5]
    assert recs.size > 3
    m = batch.digest_members_from_words(w, len(ids), recs)
    checked = 0
    for g, r in enumerate(recs):
        msgs = set()
        reason = (int(r["word"]) >> 8) & 0xFF
        for i in range(int(m.off[g]), int(m.off[g + 1])):
            resp = batch.format_response(env, int(m.rows[i]), ids[int(r["col"])], int(m.words[i]))
            msg = (resp.get("status") or {}).get("message")
            if msg is not None and 3 <= reason <= 9:
                cut = re.sub(r"^container '[^']*' ", "", msg)
                assert cut != msg, msg
                msg = cut
            msgs.add(msg)
            checked += 1
        assert len(msgs) == 1, (r, msgs)
    assert checked > recs.size


def _pod(i, labels=None, image="nginx"):
    return {"request": {"uid": str(i), "kind": {"group": "", "version": "v1", "kind": "Pod"},
                        "resource": {"group": "", "version": "v1", "resource": "pods"}, "operation": "CREATE",
                        "userInfo": {}, "object": {"kind": "Pod", "metadata": {"labels": labels or {}},
                                                   "spec": {"containers": [{"name": "c", "image": image}]}}}}


def test_two_strings_keep_their_lengths_apart():
    """("ab", "c") and ("a", "bc") under one constraint policy: members [0, 2] and [1, 3]."""
    mod = "registry://ghcr.io/kubewarden/policies/safe-labels:v0.1.14"
    pols = {"labels": {"module": mod, "settings": {"constrained_labels": {"ab": "^x$", "a": "^x$"}}}}
    docs = [_pod(i, l) for i, l in enumerate(({"ab": "c"}, {"a": "bc"}, {"ab": "c"}, {"a": "bc"}, {"a": "x"}))]
    env = K.EvaluationEnvironment(pols, continue_on_errors=True)
    b = K.Batch.from_json(docs)
    w = b.debug_host_walk(env, env.policy_ids())
    d = b.digest_from_words(w, 1)
    m = b.digest_members_from_words(w, 1, d.recs)
    assert m.off.tolist() == [0, 2, 4] and m.rows.tolist() == [0, 2, 1, 3]
    assert m.words.tolist() == [int(w[0]), int(w[2]), int(w[1]), int(w[3])]
    back = b.digest_members_from_words(w, 1, d.recs[::-1])  # the caller's order
    assert back.rows.tolist() == [1, 3, 0, 2]


def test_one_image_in_two_columns_is_two_groups():
    mod = "registry://ghcr.io/kubewarden/policies/trusted-repos:v0.1.12"
    pols = {"a": {"module": mod, "settings": {"images": {"reject": ["evil.io/x:1"]}}},
            "b": {"module": mod, "settings": {"images": {"reject": ["evil.io/x:1", "evil.io/y:2"]}}}}
    imgs = ["evil.io/x:1", "nginx", "evil.io/y:2", "evil.io/x:1", "evil.io/y:2"]
    env = K.EvaluationEnvironment(pols, continue_on_errors=True)
    ids = env.policy_ids()
    b = K.Batch.from_json([_pod(i, image=im) for i, im in enumerate(imgs)])
    w = b.debug_host_walk(env, ids)
    d = b.digest_from_words(w, 2)
    ca, cb = ids.index("a"), ids.index("b")
    got = {}
    m = b.digest_members_from_words(w, 2, d.recs)
    for g, r in enumerate(d.recs):
        got[(int(r["col"]), b.finding_key(int(r["first_row"]), int(r["word"]))[0])] = m.rows[int(m.off[g]):int(m.off[g + 1])].tolist()
    assert got == {(ca, b"evil.io/x:1"): [0, 3], (cb, b"evil.io/x:1"): [0, 3], (cb, b"evil.io/y:2"): [2, 4]}


def _call(batch, words, rows, npol, recs, cap, off=True, out_rows=True, out_words=True, groups=True):
    recs = np.ascontiguousarray(recs, dtype=np.dtype(K.DIGEST_REC))
    o = np.full(recs.size + 1, 0xDEAD, dtype=np.uint64)
    r = np.zeros(max(cap, 1), dtype=np.uint64)
    wd = np.zeros(max(cap, 1), dtype=np.uint32)
    st = N.KwMembers(o.ctypes.data_as(C.POINTER(C.c_uint64)) if off else None,
                     r.ctypes.data_as(C.POINTER(C.c_uint64)) if out_rows else None,
                     wd.ctypes.data_as(C.POINTER(C.c_uint32)) if out_words else None, cap, 12345)
    rc = N.lib().kw_debug_digest_members_words(batch._h, None if words is None else words.ctypes.data_as(C.POINTER(C.c_uint32)),
                                               rows, npol, recs.ctypes.data_as(C.POINTER(N.KwDigestRec)) if groups else None,
                                               recs.size, C.byref(st))
    return rc, st, o


def test_argument_errors():
    env, ids, batch, origin, w, cols = workload("c6")
    d, _ = reference("c6")
    npol, rows = len(ids), batch.n
    w2 = w.reshape(rows, npol)
    recs = d.recs[:8]
    n = int(recs["count"].sum())
    assert _call(batch, w, rows, npol, recs, n)[0] == N.KW_OK

    def bad(change):
        r = recs.copy()
        change(r)
        return _call(batch, w, rows, npol, r, n + 8)[0]

    def setf(i, field, value):
        def f(r):
            r[i][field] = value
        return f

    assert bad(setf(3, "col", npol)) == N.KW_E_ARG                    # col >= npol
    assert bad(setf(3, "first_row", rows)) == N.KW_E_ARG              # first_row >= rows
    assert bad(setf(3, "word", int(recs[3]["word"]) & 0xFFFF00FF)) == N.KW_E_ARG  # not a finding
    assert bad(setf(3, "word", int(recs[3]["word"]) ^ (1 << 16))) == N.KW_E_ARG   # not the pass's word there
    assert d.wide.size > 0
    pair = int(d.wide[0])  # a wide finding belongs to kw_digest.wide, not to a group
    wr, wc = pair // npol, pair % npol

    def wide(r):
        r[3] = (wc, int(w2[wr, wc]), wr, 1)
    assert bad(wide) == N.KW_E_ARG
    # two records that name the same group: the same record twice, and another member of the group
    many = d.recs[d.recs["count"] > 1][:1]
    m = batch.digest_members_from_words(w, npol, many)
    other = many.copy()
    other[0]["first_row"], other[0]["word"] = m.rows[-1], m.words[-1]
    assert int(other[0]["first_row"]) != int(many[0]["first_row"])
    assert _call(batch, w, rows, npol, np.concatenate([many, many]), 4 * n)[0] == N.KW_E_ARG
    assert _call(batch, w, rows, npol, np.concatenate([recs[recs["first_row"] != many[0]["first_row"]], many, other]),
                 4 * n + int(many[0]["count"]) * 2)[0] == N.KW_E_ARG
    # the caller's arrays
    assert _call(batch, w, rows, npol, recs, n, off=False)[0] == N.KW_E_ARG
    assert _call(batch, w, rows, npol, recs, n, out_rows=False)[0] == N.KW_E_ARG
    assert _call(batch, w, rows, npol, recs, n, groups=False)[0] == N.KW_E_ARG
    assert _call(batch, w, rows + 1, npol, recs, n)[0] == N.KW_E_ARG
    assert _call(batch, w, rows, 0, recs, n)[0] == N.KW_E_ARG
    assert _call(batch, None, rows, npol, recs, n)[0] == N.KW_E_ARG
    assert N.lib().kw_debug_digest_members_words(batch._h, w.ctypes.data_as(C.POINTER(C.c_uint32)), rows, npol, None, 0, None) == N.KW_E_ARG
    with pytest.raises(K.EvaluationError) as e:
        batch.digest_members_from_words(w, npol, np.concatenate([many, many]))
    assert e.value.code == N.KW_E_ARG
    # no group named: KW_OK with n = 0, whatever the arrays
    rc, st, o = _call(batch, w, rows, npol, recs[:0], 0, out_rows=False, out_words=False)
    assert rc == N.KW_OK and st.n == 0 and int(o[0]) == 0
    rc, st, _ = _call(batch, w, rows, npol, recs[:0], 0, off=False, out_rows=False, out_words=False, groups=False)
    assert rc == N.KW_OK and st.n == 0


def test_nospace_keeps_n_and_off_exact():
    env, ids, batch, origin, w, cols = workload("c4")
    d, _ = reference("c4")
    npol, rows = len(ids), batch.n
    recs = d.recs[::2]
    want = batch.digest_members_from_words(w, npol, recs)
    n = want.rows.size
    assert n > 100
    for cap, give in ((n - 1, True), (0, True), (0, False)):
        rc, st, off = _call(batch, w, rows, npol, recs, cap, out_rows=give, out_words=give)
        assert rc == N.KW_E_NOSPACE and st.n == n and np.array_equal(off, want.off)
        with pytest.raises(K.MembersNoSpace) as e:
            batch.digest_members_from_words(w, npol, recs, cap=cap)
        assert e.value.need == n and np.array_equal(e.value.off, want.off)
    rc, st, off = _call(batch, w, rows, npol, recs, n)  # exactly enough
    assert rc == N.KW_OK and st.n == n
    # records kept without their counts: the wrapper grows once to the reported need
    bare = recs.copy()
    bare["count"] = 0
    assert MC.same(batch.digest_members_from_words(w, npol, bare), want)
    assert MC.same(batch.digest_members_from_words(w, npol, recs, cap=n + 5), want)


def test_device_entry_needs_a_pass():
    env, ids, batch, origin, w, cols = workload("c4")
    d, _ = reference("c4")
    with pytest.raises(K.EvaluationError) as e:
        batch.digest_members(d.recs[:4])  # never on a device
    assert e.value.code == N.KW_E_ARG


def test_members_check_under_sanitizers(tmp_path):
    exe = tmp_path / "members_check"
    subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(PKG, "csrc"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "members_check.cpp")], check=True)
    # (out-of-bounds accesses and undefined behaviour are the point; the leak check at exit needs
    # ptrace rights a test runner may lack)
    out = subprocess.run([str(exe)], check=False, capture_output=True, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "failures 0" in out.stdout
