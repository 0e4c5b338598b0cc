"""The messages of chosen findings (include/kwgpu.h kw_batch_messages; policy-server_amd/csrc/messages.hpp)
on the host: the piece renderer the device runs (kw_debug_messages_words how=1) must equal, byte for
byte, one policy_message call per item (how=0), over every finding of the digest's workloads and a
sample of pairs without one; the text is tied to the pinned formatter (format_response's
status.message); the host list is exactly the items the header names; hand documents with long, empty
and odd strings and every image form; KW_E_NOSPACE and every argument error that needs no device.
tests/messages_check.cpp runs messages.hpp alone (every reason's pieces, the image forms, arguments
the request does not hold, the offsets past 2^32, the window clipping, the settings search) as a plain
executable under AddressSanitizer and UBSan (no Python in that process)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import kwgpu as K
from kwgpu import _native as N
from test_digest import workload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "policy-server_amd")
CXX = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
WORKLOADS = ["c2", "c3", "c4", "c5", "c6", "parity", "wide_docs", "wide_entity"]
WIDE = 0xFFFF
_memo = {}


def reason_of(w):
    return (np.asarray(w, dtype=np.uint32) >> np.uint32(8)) & np.uint32(0xFF)


def arg_of(w):
    return np.asarray(w, dtype=np.uint32) >> np.uint32(16)


def host_items(words):
    """The items the header leaves to the host: reason 14, or reason 1-12 with ARG KW_ARG_WIDE."""
    r, a = reason_of(words), arg_of(words)
    return np.nonzero((r == 14) | ((r >= 1) & (r <= 12) & (a == WIDE)))[0]


def items_of(words, npol, extra=400, seed=1):
    """(rows, cols) of every finding of words [rows][npol], then `extra` pairs without one."""
    w2 = np.asarray(words, dtype=np.uint32).reshape(-1, npol)
    rr, cc = np.nonzero(reason_of(w2))
    zr, zc = np.nonzero(reason_of(w2) == 0)
    rng = np.random.default_rng(seed)
    pick = rng.choice(zr.size, size=min(extra, zr.size), replace=False) if zr.size else np.zeros(0, dtype=np.int64)
    return (np.concatenate([rr, zr[pick]]).astype(np.uint64), np.concatenate([cc, zc[pick]]).astype(np.uint32), rr.size)


def same(a, b):
    return (np.array_equal(a.off, b.off) and a.text.tobytes() == b.text.tobytes() and np.array_equal(a.host, b.host)
            and ((a.words is None and b.words is None) or np.array_equal(a.words, b.words)))


def rendered(name):
    """(rows, cols, findings, how=0 result with words), made once."""
    if name not in _memo:
        env, ids, batch, origin, w, cols = workload(name)
        rows, cc, nf = items_of(w, len(ids))
        _memo[name] = (rows, cc, nf, batch.messages_from_words(env, ids, w, rows, cc, how=0, with_words=True))
    return _memo[name]


@pytest.mark.parametrize("name", WORKLOADS)
def test_piece_renderer_equals_policy_message(name):
    env, ids, batch, origin, w, cols = workload(name)
    rows, cc, nf, ref = rendered(name)
    assert nf > 0 and rows.size >= nf
    got = batch.messages_from_words(env, ids, w, rows, cc, how=1, with_words=True)
    assert got.off.dtype == np.uint64 and got.host.dtype == np.uint64 and got.text.dtype == np.uint8
    assert np.array_equal(got.off, ref.off), np.nonzero(got.off != ref.off)[0][:8]
    assert got.text.tobytes() == ref.text.tobytes()
    assert np.array_equal(got.words, ref.words) and np.array_equal(got.host, ref.host)
    assert int(got.off[-1]) == got.text.size == ref.text.size
    w2 = w.reshape(-1, len(ids))
    assert np.array_equal(ref.words, w2[rows.astype(np.int64), cc.astype(np.int64)])
    # the host list is exactly the items the header names
    assert np.array_equal(ref.host, host_items(ref.words).astype(np.uint64))
    lens = np.diff(ref.off.astype(np.int64))
    assert (lens[ref.host.astype(np.int64)] == 0).all()
    assert (lens[nf:] == 0).all()  # pairs without a finding: the empty message, not listed
    assert not np.isin(np.arange(nf, rows.size), ref.host).any()
    assert same(got, batch.messages_from_words(env, ids, w, rows, cc, how=1, with_words=True))  # the same input, the same bytes
    bare = batch.messages_from_words(env, ids, w, rows, cc, how=1)
    assert bare.words is None and bare.text.tobytes() == ref.text.tobytes()
    # any order and repeats
    rng = np.random.default_rng(5)
    order = rng.integers(0, rows.size, size=min(rows.size, 700))
    for how in (0, 1):
        sh = batch.messages_from_words(env, ids, w, rows[order], cc[order], how=how)
        assert [sh.get(i) for i in range(order.size)] == [ref.get(int(j)) for j in order]


def test_fixture_is_not_vacuous():
    env, ids, batch, origin, w, cols = workload("parity")
    rows, cc, nf, ref = rendered("parity")
    reasons = reason_of(ref.words[:nf])
    counts = np.bincount(reasons.astype(np.int64), minlength=16)
    assert nf == 4600 and (counts[1:16] > 0).all(), counts
    assert counts[4] == 87 and counts[7] == 19 and counts[14] == 727
    rows6, cc6, nf6, ref6 = rendered("c6")
    wide = (reason_of(ref6.words[:nf6]) == 13) & (arg_of(ref6.words[:nf6]) == WIDE)
    assert int(wide.sum()) == 118
    assert (np.diff(ref6.off.astype(np.int64))[:nf6][wide] > 0).all()  # reason 13 renders whatever its ARG
    means, most = [], 0
    for name in WORKLOADS:
        rows, cc, nf, ref = rendered(name)
        lens = np.diff(ref.off.astype(np.int64))[:nf]
        lens = lens[lens > 0]
        means.append(float(lens.mean()))
        most = max(most, int(lens.max()))
    assert 50 < min(means) and max(means) < 125 and most == 226, (means, most)


@pytest.mark.parametrize("name", WORKLOADS)
def test_text_is_the_formatters_message(name):
    """Every item whose word has the vanilla status, is neither bypassed nor a patch, is not listed in
    `host` and whose column is not a group (a group response needs the members' words): the text is
    the UTF-8 of format_response's status.message. Every such finding of the workload is compared,
    and their number is what the four filters leave."""
    env, ids, batch, origin, w, cols = workload(name)
    rows, cc, nf, ref = rendered(name)
    group = np.array([env.is_group(env._idx(i)) for i in ids])
    words = ref.words[:nf]
    listed = np.zeros(nf, dtype=bool)
    listed[ref.host[ref.host < nf].astype(np.int64)] = True
    eligible = ((((words >> np.uint32(3)) & np.uint32(3)) == 1) & ((words & np.uint32(0x20)) == 0) & ((words & np.uint32(0x40)) == 0)
                & ~listed & ~group[cc[:nf].astype(np.int64)])
    checked = 0
    for i in np.nonzero(eligible)[0].tolist():
        resp = batch.format_response(env, int(rows[i]), ids[int(cc[i])], int(words[i]))
        assert ref.get(i) == resp["status"]["message"].encode("utf-8"), (i, hex(int(words[i])))
        checked += 1
    assert checked == int(eligible.sum())
    print(name, "findings", nf, "compared with the formatter", checked)
    # what the filters leave, as counted here on the CPU with this tree
    assert checked == {"c2": 252, "c3": 633, "c4": 8994, "c5": 10395, "c6": 27041, "parity": 2491, "wide_docs": 2677,
                       "wide_entity": 4}[name], (name, nf)


def _pod(i, labels=None, containers=None, ns=None, annotations=None):
    obj = {"kind": "Pod", "metadata": {"labels": labels or {}, "annotations": annotations or {}}, "spec": {"containers": containers or [{"name": "c", "image": "nginx"}]}}
    req = {"uid": str(i), "kind": {"group": "", "version": "v1", "kind": "Pod"},
           "resource": {"group": "", "version": "v1", "resource": "pods"}, "operation": "CREATE", "userInfo": {}, "object": obj}
    if ns is not None:
        req["namespace"] = ns
        obj["metadata"]["namespace"] = ns
    return {"request": req}


IMAGES = ["nginx", "a/b", "evil.io/x:1", "localhost:5000/a/b@sha256:" + "ab" * 32, "localhost/x", "reg:5000/x",
          "evil.io/x@sha256:" + "cd" * 32, "", "bad", "evil.io/y:2"]
ODD_NAME = "c'\"\\é"
LONG_VALUE = "v" * 5000
LONG_NAME = "n" * 300


def hand_case(device=None):
    """(env, ids, batch, words of the host walk): hand documents under trusted-repos policies of every
    list kind, label policies, a namespace policy and an AppArmor policy. `device`: an environment
    for that device and a batch of its own."""
    if ("hand", device) in _memo:
        return _memo[("hand", device)]
    tr = "registry://ghcr.io/kubewarden/policies/trusted-repos:v0.1.12"
    sl = "registry://ghcr.io/kubewarden/policies/safe-labels:v0.1.14"
    pols = {
        "regallow": {"module": tr, "settings": {"registries": {"allow": ["quay.io"]}}},
        "regrej": {"module": tr, "settings": {"registries": {"reject": ["docker.io", "evil.io", "localhost", "localhost:5000", "reg:5000"]}}},
        "tagrej": {"module": tr, "settings": {"tags": {"reject": ["latest", "1", "2", ""]}}},
        "imgallow": {"module": tr, "settings": {"images": {"allow": ["quay.io/ok:1"]}}},
        "imgrej": {"module": tr, "settings": {"images": {"reject": ["*bad*", "*nginx*", "evil.io/x:1"]}}},
        "labels": {"module": sl, "settings": {"denied_labels": ["no"], "mandatory_labels": ["must"],
                                              "constrained_labels": {"k": "^x$", "kk": "^y+$", "": "^z$"}}},
        "ns": {"module": "registry://ghcr.io/kubewarden/policies/namespace-validate:v0.1.0", "settings": {"valid_namespace": "only"}},
        "aa": {"module": "registry://ghcr.io/kubewarden/policies/psp-apparmor:v0.1.7", "settings": {"allowed_profiles": ["runtime/default"]}},
    }
    docs = []
    for i, im in enumerate(IMAGES):
        docs.append(_pod(i, {"must": "1"}, [{"name": "c", "image": im}]))
    docs.append(_pod(20, {"must": "1"}, [{"name": ODD_NAME, "image": "bad"}]))
    docs.append(_pod(21, {"must": "1"}, [{"name": "", "image": "bad"}]))
    docs.append(_pod(22, {"must": "1", "k": LONG_VALUE}))
    docs.append(_pod(23, {"must": "1", "kk": ""}))
    docs.append(_pod(24, {"must": "1", "": "q"}))
    docs.append(_pod(25, {"no": "1"}))
    docs.append(_pod(26, {}, ns=""))
    docs.append(_pod(27, {"must": "1"}, ns="other"))
    docs.append(_pod(29, {"must": "1"}, [{"name": "ok", "image": "quay.io/ok:1"}, {"name": LONG_NAME, "image": "evil.io/x:1"}]))
    docs.append(_pod(28, {"must": "1"}, annotations={"container.apparmor.security.beta.kubernetes.io/c": "localhost/evil"}))
    env = K.EvaluationEnvironment(pols, continue_on_errors=True, **({} if device is None else {"device": device}))
    ids = env.policy_ids()
    batch = K.Batch.from_json(docs)
    _memo[("hand", device)] = (env, ids, batch, batch.debug_host_walk(env, ids))
    return _memo[("hand", device)]


def test_hand_documents():
    env, ids, batch, w = hand_case()
    npol = len(ids)
    rows, cc, nf = items_of(w, npol, extra=20)
    ref = batch.messages_from_words(env, ids, w, rows, cc, how=0, with_words=True)
    got = batch.messages_from_words(env, ids, w, rows, cc, how=1, with_words=True)
    assert same(got, ref) and ref.host.size == 0
    msgs = {(int(r), ids[int(c)]): ref.get(i) for i, (r, c) in enumerate(zip(rows[:nf], cc[:nf]))}
    # the image forms: the registry and the tag are image_parts' answers
    # (tag None: a digest reference without a tag has no tag, image_parts' has_tag is false, so the
    # tags reject list, which holds "latest", "1", "2" and "", does not fire on it)
    for i, (reg, tag) in enumerate([("docker.io", "latest"), ("docker.io", "latest"), ("evil.io", "1"), ("localhost:5000", None),
                                    ("localhost", "latest"), ("reg:5000", "latest"), ("evil.io", None), ("docker.io", "latest")]):
        head = f"container 'c' uses image '{IMAGES[i]}'"
        assert msgs[(i, "regallow")] == f"{head}: registry '{reg}' is not in the allowed registries".encode(), i
        assert msgs[(i, "regrej")] == f"{head}: registry '{reg}' is rejected".encode(), i
        if tag is None:
            assert (i, "tagrej") not in msgs, i
        else:
            assert msgs[(i, "tagrej")] == f"{head}: tag '{tag}' is rejected".encode(), i
        assert msgs[(i, "imgallow")] == f"{head}, which is not in the allowed images".encode(), i
    assert msgs[(9, "tagrej")] == b"container 'c' uses image 'evil.io/y:2': tag '2' is rejected"
    assert msgs[(0, "imgrej")] == b"container 'c' uses image 'nginx', which is rejected"
    # odd bytes pass through raw; empty and long names
    assert msgs[(10, "imgrej")] == ("container '" + ODD_NAME + "' uses image 'bad', which is rejected").encode("utf-8")
    assert msgs[(11, "imgrej")] == b"container '' uses image 'bad', which is rejected"
    assert msgs[(18, "regrej")] == ("container '" + LONG_NAME + "' uses image 'evil.io/x:1': registry 'evil.io' is rejected").encode()
    assert msgs[(12, "labels")] == ("label 'k' value '" + LONG_VALUE + "' does not match the constraint '^x$'").encode()
    assert msgs[(13, "labels")] == b"label 'kk' value '' does not match the constraint '^y+$'"
    assert msgs[(15, "labels")] == b"label 'no' is denied"
    assert msgs[(16, "labels")] == b"mandatory label 'must' is missing"
    assert msgs[(16, "ns")] == b"namespace '' is not accepted: only 'only' is allowed"
    assert msgs[(17, "ns")] == b"namespace 'other' is not accepted: only 'only' is allowed"
    assert msgs[(19, "aa")] == b"container 'c' uses AppArmor profile 'localhost/evil', which is not allowed"
    assert any(len(m) > 5000 for m in msgs.values()) and any(300 < len(m) < 400 for m in msgs.values())


def _call(env, ids, batch, w, nrows, rows, cols, cap, host_cap, how=1, off=True, text=True, host=True, npol=None, pols=None):
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    cols = np.ascontiguousarray(cols, dtype=np.uint32)
    n = rows.size
    o = np.full(n + 1, 0xDEAD, dtype=np.uint64)
    t = np.zeros(max(cap, 1), dtype=np.uint8)
    h = np.zeros(max(host_cap, 1), dtype=np.uint64)
    st = N.KwMessages(o.ctypes.data_as(C.POINTER(C.c_uint64)) if off else None, t.ctypes.data if text else None, cap, 12345, None,
                      h.ctypes.data_as(C.POINTER(C.c_uint64)) if host else None, host_cap, 12345)
    arr = env._array(ids) if pols is None else (C.c_int32 * len(pols))(*pols)
    rc = N.lib().kw_debug_messages_words(env._h, batch._h, arr, len(ids) if npol is None else npol,
                                         None if w is None else w.ctypes.data_as(C.POINTER(C.c_uint32)), nrows,
                                         rows.ctypes.data_as(C.POINTER(C.c_uint64)), cols.ctypes.data_as(C.POINTER(C.c_uint32)), n, how,
                                         C.byref(st))
    return rc, st, o, t, h


def test_nospace_keeps_the_counts_exact():
    env, ids, batch, origin, w, cols = workload("parity")
    rows, cc, nf, ref = rendered("parity")
    nbytes, nhost = ref.text.size, ref.host.size
    assert nbytes > 1000 and nhost > 1
    for how in (0, 1):
        for cap, hcap in ((nbytes - 1, nhost), (0, nhost), (nbytes, nhost - 1), (0, 0)):
            rc, st, off, _, _ = _call(env, ids, batch, w, batch.n, rows, cc, cap, hcap, how=how, text=cap > 0, host=hcap > 0)
            assert rc == N.KW_E_NOSPACE and st.bytes == nbytes and st.nhost == nhost and np.array_equal(off, ref.off)
        rc, st, off, text, host = _call(env, ids, batch, w, batch.n, rows, cc, nbytes, nhost, how=how)  # exactly enough
        assert rc == N.KW_OK and text[:nbytes].tobytes() == ref.text.tobytes() and np.array_equal(host[:nhost], ref.host)
    with pytest.raises(K.MessagesNoSpace) as e:
        batch.messages_from_words(env, ids, w, rows, cc, how=1, cap=nbytes - 1)
    assert e.value.need == nbytes and e.value.nhost == nhost and np.array_equal(e.value.off, ref.off)
    with pytest.raises(K.MessagesNoSpace):
        batch.messages_from_words(env, ids, w, rows, cc, how=0, host_cap=nhost - 1)
    assert same(batch.messages_from_words(env, ids, w, rows, cc, how=1, with_words=True, cap=nbytes + 7), ref)


def test_argument_errors():
    env, ids, batch, origin, w, cols = workload("c4")
    rows, cc, nf, ref = rendered("c4")
    npol, nrows = len(ids), batch.n
    r, c = rows[:50], cc[:50]
    cap = int(ref.off[50])
    assert _call(env, ids, batch, w, nrows, r, c, cap, 50)[0] == N.KW_OK

    def with_item(i, row, col):
        rr, kk = r.copy(), c.copy()
        rr[i], kk[i] = row, col
        return _call(env, ids, batch, w, nrows, rr, kk, cap + 500, 50)[0]

    assert with_item(7, nrows, 0) == N.KW_E_ARG               # a row outside the pass
    assert with_item(7, 0, npol) == N.KW_E_ARG                # a col outside the pass
    assert _call(env, ids, batch, w, nrows + 1, r, c, cap, 50)[0] == N.KW_E_ARG   # more rows than the batch's
    assert _call(env, ids, batch, w, nrows, r, c, cap, 50, npol=0)[0] == N.KW_E_ARG
    assert _call(env, ids, batch, None, nrows, r, c, cap, 50)[0] == N.KW_E_ARG
    assert _call(env, ids, batch, w, nrows, r, c, cap, 50, how=2)[0] == N.KW_E_ARG
    assert _call(env, ids, batch, w, nrows, r, c, cap, 50, off=False)[0] == N.KW_E_ARG
    assert _call(env, ids, batch, w, nrows, r, c, cap, 50, text=False)[0] == N.KW_E_ARG
    assert _call(env, ids, batch, w, nrows, r, c, cap, 50, host=False)[0] == N.KW_E_ARG
    bad = [env._idx(i) for i in ids]
    bad[3] = 1 << 20
    assert _call(env, ids, batch, w, nrows, r, c, cap, 50, pols=bad)[0] == N.KW_E_ARG  # a policy index outside the env
    bad[3] = -1
    assert _call(env, ids, batch, w, nrows, r, c, cap, 50, pols=bad)[0] == N.KW_E_ARG
    arr = env._array(ids)
    assert N.lib().kw_debug_messages_words(env._h, batch._h, arr, npol, w.ctypes.data_as(C.POINTER(C.c_uint32)), nrows, None, None, 0, 0,
                                           None) == N.KW_E_ARG
    # n = 0 is KW_OK, whatever the arrays
    rc, st, o, _, _ = _call(env, ids, batch, w, nrows, r[:0], c[:0], 0, 0, text=False, host=False)
    assert rc == N.KW_OK and st.bytes == 0 and st.nhost == 0 and int(o[0]) == 0
    assert _call(env, ids, batch, w, nrows, r[:0], c[:0], 0, 0, off=False, text=False, host=False)[0] == N.KW_OK
    with pytest.raises(ValueError):
        batch.messages_from_words(env, ids, w, r, c[:10])
    with pytest.raises(K.EvaluationError) as e:
        batch.messages_from_words(env, ids, w, [nrows], [0])
    assert e.value.code == N.KW_E_ARG


def test_device_entry_needs_a_pass():
    env, ids, batch, origin, w, cols = workload("c4")
    with pytest.raises(K.EvaluationError) as e:
        batch.messages(env, ids, [0], [0])  # never on a device
    assert e.value.code == N.KW_E_ARG
    with pytest.raises(K.EvaluationError) as e:
        batch.debug_messages_stats()
    assert e.value.code == N.KW_E_ARG


def test_messages_check_under_sanitizers(tmp_path):
    exe = tmp_path / "messages_check"
    subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(PKG, "csrc"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "messages_check.cpp")], check=True)
    # (out-of-bounds accesses and undefined behaviour are the point; the leak check at exit needs
    # ptrace rights a test runner may lack)
    out = subprocess.run([str(exe)], check=False, capture_output=True, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "failures 0" in out.stdout
