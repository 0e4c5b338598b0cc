"""The AdmissionResponse bodies of chosen pairs (include/kwgpu.h kw_batch_responses;
policy-server_amd/csrc/responses.hpp) on the host: the part and piece renderer the device runs
(kw_debug_responses_words how=1) must equal, byte for byte, one format_response per item (how=0) and
the bytes kw_format_response itself writes, the members' words taken from the same word matrix: over
the hand documents of tests/test_messages.py, the every-reason fixture, configs/c3_group.yml, C4
synthetic rows, and a hand fixture whose every string needs escaping (with a 15-member group that
rejects with all its causes, a 16-member group, a group with a member left out of the policy list and
a mutated member inside a group). The host list is what a predicate over the words and the policy
list, written here from the header's rules, predicts. KW_E_NOSPACE and every argument error that
needs no device. tests/responses_check.cpp runs responses.hpp alone as a plain executable under
AddressSanitizer and UBSan (no Python in that process)."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import kwgpu as K
import outcomes_cases as OC
from kwgpu import _native as N
from test_digest import workload
from test_messages import _pod, arg_of, hand_case, reason_of, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "policy-server_amd")
CXX = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
WIDE = 0xFFFF
ODD = "q\"b\\c\td\x01é"   # a quote, a backslash, a tab, 0x01 and a non-ASCII character
_memo = {}


# ---- the host list, from the rules of the header -----------------------------------------------------

def member_columns(env, ids):
    """Per column: None for a plain policy, else the members' columns (the first column that holds
    member s, or None), settings order."""
    idx = [env._idx(i) for i in ids]
    out = []
    for p in idx:
        if not env.is_group(p):
            out.append(None)
            continue
        out.append([idx.index(m) if m in idx else None for m in env.group_members(p)])
    return out


def unregistered_columns(env, ids):
    """The columns whose policy the mode lookup does not know (the bypass path answers PolicyNotFound)."""
    out = set()
    for c, i in enumerate(ids):
        try:
            env.get_policy_mode(i)
        except K.PolicyNotFound:
            out.add(c)
    return out


def predicted_host(env, ids, words, rows, cols, broken=()):
    """The items the header leaves to the host, from the words [rows][npol] and the policy list alone
    (no string is looked at: no product word names an argument the request does not hold). `broken`:
    the columns of groups with a member that failed to initialise."""
    npol = len(ids)
    unregistered = unregistered_columns(env, ids)
    w2 = np.asarray(words, dtype=np.uint32).reshape(-1, npol)
    mem = member_columns(env, ids)
    host = []
    for i, (r, c) in enumerate(zip(np.asarray(rows).tolist(), np.asarray(cols).tolist())):
        w = int(w2[r, c])
        reason, arg, fst = (w >> 8) & 0xFF, w >> 16, (w >> 3) & 3
        if w & 0x20:  # bypass: only an unregistered policy is the host's
            if c in unregistered:
                host.append(i)
            continue
        if c in broken or (w & 0x40):
            host.append(i)
            continue
        if fst != 1:
            continue
        if reason == 14 or (1 <= reason <= 13 and arg == WIDE):  # (no product word has another reason with a wide ARG)
            host.append(i)
            continue
        if reason != 13:
            continue
        m = mem[c] or []
        if any(x is None for x in m):
            host.append(i)
            continue
        for s, mc in enumerate(m[:16]):
            if not (arg >> s) & 1:
                continue
            mv = int(w2[r, mc])
            if (mv & 1) and (mv & 2):
                continue
            mr = (mv >> 8) & 0xFF
            if mr == 14 or (1 <= mr <= 12 and (mv >> 16) == WIDE):  # the cause's own message is the host's
                host.append(i)
                break
    return np.array(host, dtype=np.uint64)


def causes_of(env, ids, words, rows, cols):
    """Per item the number of causes of a group rejection that carries details (0 otherwise)."""
    npol = len(ids)
    w2 = np.asarray(words, dtype=np.uint32).reshape(-1, npol)
    mem = member_columns(env, ids)
    w = w2[np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)]
    out = np.zeros(w.size, dtype=np.int64)
    for i in np.nonzero((reason_of(w) == 13) & (((w >> np.uint32(3)) & np.uint32(3)) == 1) & ((w & np.uint32(0x60)) == 0)
                        & (arg_of(w) != WIDE))[0].tolist():
        n = len(mem[int(cols[i])] or [])
        out[i] = bin(int(w[i]) >> 16 & ((1 << min(n, 16)) - 1)).count("1")
    return out


def raw_format_response(env, batch, ids, words, row, col):
    """The bytes kw_format_response writes for (row, col) with the members' words of the same row, or
    None when it answers an error."""
    npol = len(ids)
    w2 = np.asarray(words, dtype=np.uint32).reshape(-1, npol)
    mem = member_columns(env, ids)[col]
    mv = None
    if mem is not None:
        mv = (C.c_uint32 * max(len(mem), 1))(*[0 if mc is None else int(w2[row, mc]) for mc in mem])
    need = C.c_size_t()
    buf = C.create_string_buffer(1 << 16)
    rc = N.lib().kw_format_response(env._h, batch._h, int(row), env._idx(ids[col]), int(w2[row, col]), mv, buf, len(buf), C.byref(need))
    return buf.value if rc == N.KW_OK else None  # (a response holds no NUL byte: 0x00 is escaped)


def all_pairs(nrows, npol, limit=None, seed=3):
    """Every pair of the pass (or a sample of `limit`), findings or not."""
    rows = np.repeat(np.arange(nrows, dtype=np.uint64), npol)
    cols = np.tile(np.arange(npol, dtype=np.uint32), nrows)
    if limit is not None and rows.size > limit:
        pick = np.sort(np.random.default_rng(seed).choice(rows.size, size=limit, replace=False))
        rows, cols = rows[pick], cols[pick]
    return rows, cols


def check_case(env, ids, batch, words, rows, cols, formatter=400, **flags):
    """how=1 == how=0 == kw_format_response; the host list is the predicate's. Returns the reference."""
    ref = batch.responses_from_words(env, ids, words, rows, cols, how=0, with_words=True)
    got = batch.responses_from_words(env, ids, words, rows, cols, how=1, with_words=True)
    assert np.array_equal(got.off, ref.off), np.nonzero(got.off != ref.off)[0][:8]
    assert got.text.tobytes() == ref.text.tobytes(), np.nonzero(got.text != ref.text)[0][:8]
    assert np.array_equal(got.words, ref.words) and np.array_equal(got.host, ref.host)
    assert int(ref.off[-1]) == ref.text.size
    w2 = np.asarray(words, dtype=np.uint32).reshape(-1, len(ids))
    assert np.array_equal(ref.words, w2[rows.astype(np.int64), cols.astype(np.int64)])
    assert np.array_equal(ref.host, predicted_host(env, ids, words, rows, cols, **flags))
    lens = np.diff(ref.off.astype(np.int64))
    listed = np.zeros(rows.size, dtype=bool)
    listed[ref.host.astype(np.int64)] = True
    assert (lens[listed] == 0).all() and (lens[~listed] > 0).all()
    assert 2 * int(listed.sum()) <= rows.size  # at least half of the items are rendered
    step = max(1, rows.size // formatter)
    for i in range(0, rows.size, step):
        want = raw_format_response(env, batch, ids, words, int(rows[i]), int(cols[i]))
        if listed[i]:
            continue  # (the predicate above says why; a wide argument the side data holds formats on the host)
        assert want is not None and ref.get(i) == want, (i, hex(int(ref.words[i])))
        json.loads(want.decode("utf-8", errors="surrogateescape"))
    assert same(got, batch.responses_from_words(env, ids, words, rows, cols, how=1, with_words=True))
    return ref


# ---- the fixtures -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["c3", "c4", "parity"])
def test_part_renderer_equals_format_response(name):
    env, ids, batch, origin, w, cols_ = workload(name)
    rows, cols = all_pairs(batch.n, len(ids), limit=20000)
    ref = check_case(env, ids, batch, w, rows, cols)
    causes = causes_of(env, ids, w, rows, cols)
    listed = np.isin(np.arange(rows.size), ref.host)
    print(name, "items", rows.size, "host", ref.host.size, "with two causes or more", int(((causes >= 2) & ~listed).sum()))
    if name == "c3":  # the group case
        assert int(((causes >= 2) & ~listed).sum()) >= 100
    if name == "parity":  # every form: bypass, plain allowed, the three statuses, the host's
        words = ref.words
        assert set(np.unique(reason_of(words)).tolist()) >= set(range(16))
        assert ((words & np.uint32(0x20)) != 0).any() and (((words >> np.uint32(3)) & np.uint32(3)) == 2).any()
        assert (((words >> np.uint32(3)) & np.uint32(3)) == 3).any() and ref.host.size > 100
        texts = [ref.get(i) for i in range(0, rows.size, 7)]
        assert any(t.endswith(b'"allowed":true}') for t in texts) and any(b'"code":500}}' in t for t in texts)
    # any order and repeats
    order = np.random.default_rng(5).integers(0, rows.size, size=700)
    for how in (0, 1):
        sh = batch.responses_from_words(env, ids, w, rows[order], cols[order], how=how)
        assert [sh.get(i) for i in range(order.size)] == [ref.get(int(j)) for j in order]


def test_hand_documents():
    env, ids, batch, w = hand_case()
    rows, cols = all_pairs(batch.n, len(ids))
    ref = check_case(env, ids, batch, w, rows, cols, formatter=rows.size)
    assert ref.host.size == 0
    texts = [ref.get(i) for i in range(rows.size)]
    assert any(b"container 'c\\u0027" in t for t in texts) is False  # (the apostrophe is not escaped)
    assert any(b"container 'c'\\\"\\\\\xc3\xa9' uses image 'bad'" in t for t in texts)
    assert any(len(t) > 5000 for t in texts)


def odd_case(device=None, leave_out=True):
    """(env, ids, batch, words of the host walk): every string a response quotes carries ODD. Groups:
    g15 (15 members that all reject: 15 causes, more than the pieces of one plan), g16 (16 members:
    the causes do not fit the word), gmut (a member that mutates inside a group), gleft (a group one
    of whose members is left out of `ids`)."""
    key = ("odd", device, leave_out)
    if key in _memo:
        return _memo[key]
    tr = "registry://ghcr.io/kubewarden/policies/trusted-repos:v0.1.12"
    sl = "registry://ghcr.io/kubewarden/policies/safe-labels:v0.1.14"
    caps = "registry://ghcr.io/kubewarden/policies/psp-capabilities:v0.1.9"
    regex = "^\"\\\\\t\x01é$"  # matches the five characters " \ tab 0x01 e-acute
    labels = {"module": sl, "settings": {"denied_labels": ["no" + ODD], "mandatory_labels": ["must" + ODD],
                                         "constrained_labels": {"k" + ODD: regex}}}
    imgrej = {"module": tr, "settings": {"images": {"reject": ["*bad*"]}}}
    regrej = {"module": tr, "settings": {"registries": {"reject": ["evil.io"]}}}
    tagrej = {"module": tr, "settings": {"tags": {"reject": ["t*"]}}}

    def group(n, msg):
        return {"policies": {f"m{i}": (labels if i % 3 == 0 else imgrej if i % 3 == 1 else regrej) for i in range(n)},
                "expression": " || ".join(f"m{i}()" for i in range(n)), "message": msg}

    pols = {
        "labels " + ODD: labels,
        "imgrej": imgrej, "regrej": regrej, "tagrej": tagrej,
        "ns": {"module": "registry://ghcr.io/kubewarden/policies/namespace-validate:v0.1.0", "settings": {"valid_namespace": "only" + ODD}},
        "aa": {"module": "registry://ghcr.io/kubewarden/policies/psp-apparmor:v0.1.7", "settings": {"allowed_profiles": ["runtime/default"]}},
        "caps": {"module": caps, "settings": {"allowed_capabilities": ["CHOWN"]}},
        "g15": group(15, "fifteen " + ODD),
        "g16": group(16, "sixteen " + ODD),
        "gmut": {"policies": {"plain": imgrej, "mut": {"module": caps,
                                                       "settings": {"allowed_capabilities": ["*"], "required_drop_capabilities": ["NET_RAW"]}}},
                 "expression": "plain() || mut()", "message": "mutating " + ODD},
        "gleft": {"policies": {"a": imgrej, "b": tagrej}, "expression": "a() || b()", "message": "left " + ODD},
    }
    docs = []
    for i in range(120):
        name = "c" + ODD if i % 2 else "c"
        image = ("evil.io/bad" + ODD + ":t" + ODD) if i % 3 else "quay.io/ok:1"
        lab = {}
        if i % 4 != 3:
            lab["must" + ODD] = "1"
        if i % 4 == 1:
            lab["k" + ODD] = "v" + ODD
        if i % 5 == 2:
            lab["no" + ODD] = ODD
        ctr = {"name": name, "image": image}
        if i % 6 == 1:
            ctr["securityContext"] = {"capabilities": {"add": ["CAP" + ODD]}}
        ann = {}
        if i % 7 == 3:
            ann["container.apparmor.security.beta.kubernetes.io/" + name] = "localhost/" + ODD
        d = _pod(i, lab, [ctr], ns=("ns" + ODD) if i % 2 == 0 else "only" + ODD, annotations=ann)
        d["request"]["uid"] = f"uid-{i}-" + ODD
        docs.append(d)
    env = K.EvaluationEnvironment(pols, continue_on_errors=True, **({} if device is None else {"device": device}))
    ids = env.policy_ids()
    if leave_out:
        ids = [i for i in ids if i != "gleft/b"]
    batch = K.Batch.from_json(docs)
    _memo[key] = (env, ids, batch, batch.debug_host_walk(env, ids))
    return _memo[key]


def test_escaped_fixture():
    env, ids, batch, w = odd_case()
    npol = len(ids)
    rows, cols = all_pairs(batch.n, npol)
    ref = check_case(env, ids, batch, w, rows, cols, formatter=rows.size)
    w2 = w.reshape(-1, npol)
    col = {name: ids.index(name) for name in ("g15", "g16", "gmut", "gleft")}
    causes = causes_of(env, ids, w, rows, cols)
    listed = np.isin(np.arange(rows.size), ref.host)
    # the 15-member group rejects with all 15 causes, rendered; the 16-member group's causes are wide
    assert ((causes == 15) & ~listed & (cols == col["g15"])).sum() > 20
    g16 = w2[:, col["g16"]]
    assert ((reason_of(g16) == 13) & (arg_of(g16) == WIDE)).sum() > 20
    assert listed[(cols == col["g16"]) & (reason_of(ref.words) == 13)].all()
    # the group with a member that is no column: every rejection is the host's
    left = (cols == col["gleft"]) & (reason_of(ref.words) == 13)
    assert left.sum() > 20 and listed[left].all()
    # a mutated member inside a group
    texts = [ref.get(i) for i in range(rows.size)]
    mut = [t for t, c in zip(texts, cols.tolist()) if c == col["gmut"] and b"mutation is not allowed inside of policy group" in t]
    assert len(mut) > 20
    # every kind of string arrives escaped, and the JSON reads back as the strings that went in
    seen = set()
    for t in texts:
        if not t:
            continue
        doc = json.loads(t.decode("utf-8"))
        assert doc["uid"].endswith(ODD)
        msgs = [doc.get("status", {}).get("message", "")] + [c["message"] for c in doc.get("status", {}).get("details", {}).get("causes", [])]
        for m in msgs:
            for what, needle in (("ns", "namespace 'ns" + ODD), ("valid ns", "only 'only" + ODD), ("name", "container 'c" + ODD),
                                 ("image", "uses image 'evil.io/bad" + ODD), ("cap", "adds capability 'CAP" + ODD),
                                 ("aa", "AppArmor profile 'localhost/" + ODD), ("key", "label 'k" + ODD), ("value", "value 'v" + ODD),
                                 ("constraint", "constraint '^\""), ("denied", "label 'no" + ODD), ("mandatory", "mandatory label 'must" + ODD),
                                 ("group message", "fifteen " + ODD), ("tag", "tag 't" + ODD)):
                if needle in m:
                    seen.add(what)
        for c in doc.get("status", {}).get("details", {}).get("causes", []):
            assert c["field"].startswith("spec.policies.")
    assert seen == {"ns", "valid ns", "name", "image", "cap", "aa", "key", "value", "constraint", "denied", "mandatory", "group message",
                    "tag"}, seen
    assert any("é" in i and '"' in i for i in ids)  # a policy name that needs escaping
    assert (causes[~listed] >= 2).sum() >= 100


def _call(env, ids, batch, w, nrows, rows, cols, cap, host_cap, how=1, off=True, text=True, host=True, npol=None, pols=None):
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    cols = np.ascontiguousarray(cols, dtype=np.uint32)
    n = rows.size
    o = np.full(n + 1, 0xDEAD, dtype=np.uint64)
    t = np.zeros(max(cap, 1), dtype=np.uint8)
    h = np.zeros(max(host_cap, 1), dtype=np.uint64)
    st = N.KwResponses(o.ctypes.data_as(C.POINTER(C.c_uint64)) if off else None, t.ctypes.data if text else None, cap, 12345, None,
                       h.ctypes.data_as(C.POINTER(C.c_uint64)) if host else None, host_cap, 12345)
    arr = env._array(ids) if pols is None else (C.c_int32 * len(pols))(*pols)
    rc = N.lib().kw_debug_responses_words(env._h, batch._h, arr, len(ids) if npol is None else npol,
                                          None if w is None else w.ctypes.data_as(C.POINTER(C.c_uint32)), nrows,
                                          rows.ctypes.data_as(C.POINTER(C.c_uint64)), cols.ctypes.data_as(C.POINTER(C.c_uint32)), n, how,
                                          C.byref(st))
    return rc, st, o, t, h


def test_nospace_keeps_the_counts_exact():
    env, ids, batch, w = odd_case()
    rows, cols = all_pairs(batch.n, len(ids))
    ref = batch.responses_from_words(env, ids, w, rows, cols, how=0, with_words=True)
    nbytes, nhost = ref.text.size, ref.host.size
    assert nbytes > 1000 and nhost > 1
    for how in (0, 1):
        for cap, hcap in ((nbytes - 1, nhost), (0, nhost), (nbytes, nhost - 1), (0, 0)):
            rc, st, off, _, _ = _call(env, ids, batch, w, batch.n, rows, cols, cap, hcap, how=how, text=cap > 0, host=hcap > 0)
            assert rc == N.KW_E_NOSPACE and st.bytes == nbytes and st.nhost == nhost and np.array_equal(off, ref.off)
        rc, st, off, text, host = _call(env, ids, batch, w, batch.n, rows, cols, nbytes, nhost, how=how)  # exactly enough
        assert rc == N.KW_OK and text[:nbytes].tobytes() == ref.text.tobytes() and np.array_equal(host[:nhost], ref.host)
    with pytest.raises(K.MessagesNoSpace) as e:
        batch.responses_from_words(env, ids, w, rows, cols, how=1, cap=nbytes - 1)
    assert e.value.need == nbytes and e.value.nhost == nhost and np.array_equal(e.value.off, ref.off)
    with pytest.raises(K.MessagesNoSpace):
        batch.responses_from_words(env, ids, w, rows, cols, how=0, host_cap=nhost - 1)
    assert same(batch.responses_from_words(env, ids, w, rows, cols, how=1, with_words=True, cap=nbytes + 7), ref)


def test_argument_errors():
    env, ids, batch, origin, w, cols_ = workload("c4")
    npol, nrows = len(ids), batch.n
    r, c = all_pairs(nrows, npol, limit=50)
    ref = batch.responses_from_words(env, ids, w, r, c, how=0)
    cap = ref.text.size

    def good():
        rc, st, off, text, _ = _call(env, ids, batch, w, nrows, r, c, cap, 50)
        assert rc == N.KW_OK and text[:cap].tobytes() == ref.text.tobytes() and np.array_equal(off, ref.off)

    def bad(rc):
        assert rc == N.KW_E_ARG
        good()

    def with_item(i, row, col):
        rr, kk = r.copy(), c.copy()
        rr[i], kk[i] = row, col
        return _call(env, ids, batch, w, nrows, rr, kk, cap + 500, 50)[0]

    good()
    bad(with_item(7, nrows, 0))               # a row outside the pass
    bad(with_item(7, 0, npol))                # a col outside the pass
    bad(_call(env, ids, batch, w, nrows + 1, r, c, cap, 50)[0])   # more rows than the batch's
    bad(_call(env, ids, batch, w, nrows, r, c, cap, 50, npol=0)[0])
    bad(_call(env, ids, batch, None, nrows, r, c, cap, 50)[0])
    bad(_call(env, ids, batch, w, nrows, r, c, cap, 50, how=2)[0])
    bad(_call(env, ids, batch, w, nrows, r, c, cap, 50, off=False)[0])
    bad(_call(env, ids, batch, w, nrows, r, c, cap, 50, text=False)[0])
    bad(_call(env, ids, batch, w, nrows, r, c, cap, 50, host=False)[0])
    pols = [env._idx(i) for i in ids]
    pols[3] = 1 << 20
    bad(_call(env, ids, batch, w, nrows, r, c, cap, 50, pols=pols)[0])  # a policy index outside the env
    pols[3] = -1
    bad(_call(env, ids, batch, w, nrows, r, c, cap, 50, pols=pols)[0])
    arr = env._array(ids)
    bad(N.lib().kw_debug_responses_words(env._h, batch._h, arr, npol, w.ctypes.data_as(C.POINTER(C.c_uint32)), nrows, None, None, 0, 0, None))
    # n = 0 is KW_OK, whatever the arrays
    rc, st, o, _, _ = _call(env, ids, batch, w, nrows, r[:0], c[:0], 0, 0, text=False, host=False)
    assert rc == N.KW_OK and st.bytes == 0 and st.nhost == 0 and int(o[0]) == 0
    assert _call(env, ids, batch, w, nrows, r[:0], c[:0], 0, 0, off=False, text=False, host=False)[0] == N.KW_OK
    with pytest.raises(ValueError):
        batch.responses_from_words(env, ids, w, r, c[:10])
    with pytest.raises(K.EvaluationError) as e:
        batch.responses_from_words(env, ids, w, [nrows], [0])
    assert e.value.code == N.KW_E_ARG
    good()


def test_device_entry_needs_a_pass():
    env, ids, batch, origin, w, cols_ = workload("c4")
    with pytest.raises(K.EvaluationError) as e:
        batch.responses(env, ids, [0], [0])  # never on a device
    assert e.value.code == N.KW_E_ARG
    with pytest.raises(K.EvaluationError) as e:
        batch.debug_responses_stats()
    assert e.value.code == N.KW_E_ARG


def test_responses_check_under_sanitizers(tmp_path):
    exe = tmp_path / "responses_check"
    subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(PKG, "csrc"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "responses_check.cpp")], check=True)
    # (out-of-bounds accesses and undefined behaviour are the point; the leak check at exit needs
    # ptrace rights a test runner may lack)
    out = subprocess.run([str(exe)], check=False, capture_output=True, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "failures 0" in out.stdout
