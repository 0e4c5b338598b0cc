"""The JSONPatch of accepted mutations from columns (include/kwgpu.h kw_batch_patches, kw_format_patch;
policy-server_amd/csrc/patches.hpp) on the host: for every pair whose host-walk word has KW_F_PATCH,
the response kw_format_patch writes from the columns, the two renderers of the diagnostic (how=0: one
format_patch per item; how=1: the walk the device runs, in its rounds and windows) and the response
kw_format_response_doc cuts from the document must be the same bytes; the ops form must be the decoded
patch, and the oracle's capabilities_patch as parsed JSON. Over the documents of
tests/test_mutation.py and shapes of this file's own (securityContext a string, capabilities an
array, drop an object, non-strings inside add, repeated members, an object kind that differs from the
request's, a Pod spec without containers, a container index past 100, a policy of 70 required drops
that the loader splits), random documents of tests/test_flatten_fuzz.py's generator and synthetic C4
and C5 rows. The shape columns through the ABI, the host list by the header's rules, and
tests/patches_check.cpp, which runs patches.hpp alone as a plain executable under AddressSanitizer
and UBSan (no Python in that process)."""
import base64
import ctypes as C
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import kwgpu as K
import oracle as O
import test_flatten_fuzz as FZ
import test_mutation as TM
from helpers import config
from kwgpu import _native as N
from test_messages import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "policy-server_amd")
CXX = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
OPS, RESPONSE = N.KW_PATCH_OPS, N.KW_PATCH_RESPONSE
_memo = {}


# ---- the fixture: every shape ---------------------------------------------------------------------------

def fixture_policies():
    p = dict(TM.POLICIES)
    p["caps-70"] = {"module": TM.CAPS, "allowedToMutate": True,
                    "settings": {"allowed_capabilities": ["*"], "required_drop_capabilities": [f"CAP_{k:02d}" for k in range(70)],
                                 "default_add_capabilities": ["CHOWN", "q\"uote"]}}
    p["labels"] = {"module": "registry://ghcr.io/kubewarden/policies/safe-labels:v0.1.14",
                   "settings": {"mandatory_labels": ["team"]}}
    return p


def fixture_documents():
    docs = TM.documents()
    own = [
        {"name": "sc-string", "image": "nginx", "securityContext": "restricted"},
        {"name": "caps-array", "image": "nginx", "securityContext": {"capabilities": ["KILL"]}},
        {"name": "drop-object", "image": "nginx", "securityContext": {"capabilities": {"drop": {"KILL": 1}, "add": ["CHOWN"]}}},
        {"name": "add-mixed", "image": "nginx", "securityContext": {"capabilities": {"add": [5, None, "SETUID", {"CHOWN": 1}], "drop": []}}},
        {"name": "caps-null", "image": "nginx", "securityContext": {"capabilities": None}},
    ]
    for i, c in enumerate(own):
        docs.append(TM.review(f"own{i}", {"kind": "Pod", "spec": {"containers": [c]}}))
    # the object's kind wins over request.kind.kind, both ways
    spec = {"containers": [TM.CONTAINERS[0], TM.CONTAINERS[3]]}
    docs.append(TM.review("kind-a", {"kind": "Deployment", "spec": {"template": {"spec": spec}}}, kind="Pod"))
    docs.append(TM.review("kind-b", {"kind": "Pod", "spec": spec}, kind="CronJob"))
    docs.append(TM.review("kind-c", {"spec": {"jobTemplate": {"spec": {"template": {"spec": spec}}}}}, kind="CronJob"))
    docs.append(TM.review("no-containers", {"kind": "Pod", "spec": {"restartPolicy": "Always"}}))
    docs.append(TM.review("no-spec", {"kind": "Pod", "metadata": {"name": "x"}}))
    docs.append(TM.review("alone", {"kind": "Pod", "spec": {"containers": ["not-an-object"], "initContainers": [7, TM.CONTAINERS[2]]}}))
    many = ["x"] * 99 + [TM.CONTAINERS[5]] * 3 + [TM.CONTAINERS[0], 4, TM.CONTAINERS[6]]  # indices 99 to 104
    docs.append(TM.review("hundred", {"kind": "Deployment", "spec": {"template": {"spec": {"ephemeralContainers": many}}}},
                          kind="Deployment"))
    docs.append(TM.review('uid "quoted"\\\n\x01é', {"kind": "Pod", "spec": {"containers": [TM.CONTAINERS[1]]}}))
    # repeated members: the last one counts, for the shape as for the columns
    base = TM.review("dup", {"kind": "Pod", "spec": {"containers": [TM.CONTAINERS[3]]}})
    assert '"securityContext": {"capabilities": {"drop": ["KILL"]}}' in base
    for k, (old, new) in enumerate([
            ('"securityContext": {', '"securityContext": 5, "securityContext": {'),
            ('"securityContext": {"capabilities": {"drop": ["KILL"]}}',
             '"securityContext": {"capabilities": {"drop": ["KILL"]}}, "securityContext": null'),
            ('"capabilities": {"drop": ["KILL"]}', '"capabilities": [], "capabilities": {"drop": ["KILL"]}'),
            ('"capabilities": {"drop": ["KILL"]}', '"capabilities": {"drop": ["KILL"]}, "capabilities": "x"'),
            ('"drop": ["KILL"]', '"drop": ["KILL"], "drop": {}'),
            ('"drop": ["KILL"]', '"drop": 1, "add": ["CHOWN"], "drop": ["NET_RAW"], "add": null'),
            ('"containers": [', '"containers": [{"name": "first"}], "containers": [')]):
        assert old in base
        docs.append(base.replace(old, new, 1).replace('"uid": "dup"', f'"uid": "dup{k}"'))
    return docs


def fixture():
    if "fixture" not in _memo:
        _memo["fixture"] = (fixture_policies(), fixture_documents())
    return _memo["fixture"]


# ---- helpers ------------------------------------------------------------------------------------------------

def raw_response_doc(env, batch, ids, row, col, word, doc):
    """The bytes kw_format_response_doc writes, as the library returns them."""
    d = doc.encode() if isinstance(doc, str) else doc
    need = C.c_size_t()
    buf = C.create_string_buffer(1 << 16)
    for _ in (0, 1):
        rc = N.lib().kw_format_response_doc(env._h, batch._h, int(row), env._idx(ids[col]), int(word), None, d, len(d),
                                            N.KW_DOC_ADMISSION_REVIEW, buf, len(buf), C.byref(need))
        if rc != N.KW_E_NOSPACE:
            break
        buf = C.create_string_buffer(need.value + 1)
    assert rc == N.KW_OK, (rc, buf.value)
    return buf.value


def patched_items(words, npol):
    """The (rows, cols) of the pairs whose word has KW_F_PATCH, row-major."""
    w2 = np.asarray(words, dtype=np.uint32).reshape(-1, npol)
    r, c = np.nonzero(w2 & np.uint32(N.KW_F_PATCH))
    return r.astype(np.uint64), c.astype(np.uint32)


def capabilities_columns(policies, ids):
    return {c for c, i in enumerate(ids) if "psp-capabilities" in policies[i]["module"]}


def predicted_host(batch, policies, ids, words, rows, cols):
    """The items the header of kw_batch_patches leaves to the host, from the words, the policy list
    and the shape columns."""
    npol = len(ids)
    w2 = np.asarray(words, dtype=np.uint32).reshape(-1, npol)
    caps = capabilities_columns(policies, ids)
    place, pointer = batch.patch_shape()
    v = batch.view()
    host = []
    for i, (r, c) in enumerate(zip(np.asarray(rows, dtype=np.int64).tolist(), np.asarray(cols, dtype=np.int64).tolist())):
        shapes = place[v.ctr_off[r]:v.ctr_off[r + 1]] >> N.KW_PS_SHIFT
        if not (int(w2[r, c]) & N.KW_F_PATCH) or c not in caps or pointer[r] == N.KW_PP_UNKNOWN or (shapes == N.KW_PS_UNKNOWN).any():
            host.append(i)
    return np.array(host, dtype=np.uint64)


def columns_equal_documents(env, policies, ids, batch, docs, words, seen=None):
    """The four renderings of every patched pair are the same bytes; the ops are the decoded patch
    and the oracle's. Returns the number of patched pairs."""
    npol = len(ids)
    rows, cols = patched_items(words, npol)
    w2 = np.asarray(words, dtype=np.uint32).reshape(-1, npol)
    assert predicted_host(batch, policies, ids, words, rows, cols).size == 0
    out = {}
    for form in (OPS, RESPONSE):
        a0 = batch.patches_from_words(env, ids, words, rows, cols, form=form, how=0, with_words=True)
        a1 = batch.patches_from_words(env, ids, words, rows, cols, form=form, how=1, with_words=True)
        assert a0.host.size == 0 and same(a0, a1), form
        assert np.array_equal(a0.words, w2[rows.astype(np.int64), cols.astype(np.int64)])
        out[form] = a0
    place, pointer = batch.patch_shape()
    v = batch.view()
    for i, (r, c) in enumerate(zip(rows.tolist(), cols.tolist())):
        w = int(w2[r, c])
        want = raw_response_doc(env, batch, ids, r, c, w, docs[r])
        assert batch.format_patch(env, r, ids[c], w, form=RESPONSE) == want, (r, ids[c])
        assert out[RESPONSE].get(i) == want, (r, ids[c])
        ops = base64.b64decode(json.loads(want)["patch"])
        assert out[OPS].get(i) == ops and batch.format_patch(env, r, ids[c], w, form=OPS) == ops
        s = policies[ids[c]]["settings"]
        assert json.loads(ops) == O.capabilities_patch(s.get("required_drop_capabilities", []), s.get("default_add_capabilities", []),
                                                       docs[r]), (r, ids[c])
        if seen is not None:
            seen["mod"].add(len(ops) % 3)
            seen["pointer"].add(int(pointer[r]))
            seen["shape"].update((place[v.ctr_off[r]:v.ctr_off[r + 1]] >> N.KW_PS_SHIFT).tolist())
            seen["longest"] = max(seen["longest"], len(want))
    return rows.size


# ---- 1. columns equal the document -----------------------------------------------------------------------------

@pytest.mark.parametrize("origin", [K.VALIDATE, K.AUDIT])
def test_columns_equal_the_document(origin):
    policies, docs = fixture()
    env = K.EvaluationEnvironment(policies)
    ids = env.policy_ids()
    batch = K.Batch.from_json(docs)
    words = batch.debug_host_walk(env, ids, origin)
    seen = {"mod": set(), "pointer": set(), "shape": set(), "longest": 0}
    n = columns_equal_documents(env, policies, ids, batch, docs, words, seen)
    assert n >= 10
    assert seen["shape"] >= set(range(N.KW_PS_NO_SC, N.KW_PS_MAX + 1)), seen
    assert seen["pointer"] >= {N.KW_PP_POD, N.KW_PP_TEMPLATE, N.KW_PP_CRONJOB}, seen
    assert seen["mod"] == {0, 1, 2} and seen["longest"] > 1000, seen
    place, pointer = batch.patch_shape()
    assert N.KW_PP_NONE in pointer.tolist() and (place & N.KW_PS_INDEX_MASK).max() == 104
    assert ((place >> N.KW_PS_SHIFT) != N.KW_PS_UNKNOWN).all() and (pointer != N.KW_PP_UNKNOWN).all()


# ---- 2. random documents ---------------------------------------------------------------------------------------------

def test_random_documents():
    policies = {"caps": {"module": TM.CAPS, "settings": {"allowed_capabilities": ["*"],
                                                         "required_drop_capabilities": ["KILL", "SYS_TIME", "NET_RAW"],
                                                         "default_add_capabilities": ["CHOWN", "NET_ADMIN", "SETUID"]}}}
    env = K.EvaluationEnvironment(policies)
    ids = env.policy_ids()
    rng = random.Random(2100)
    docs = []
    while len(docs) < 1200:
        d = FZ._doc(rng, False)
        if rng.random() < 0.2 and '"securityContext": {' in d:  # a repeated member: the last one counts
            d = d.replace('"securityContext": {', rng.choice(['"securityContext": 5, "securityContext": {',
                                                             '"securityContext": {"capabilities": {"drop": ["ALL"]}}, "securityContext": {']), 1)
        if rng.random() < 0.2 and '"drop": [' in d:
            d = d.replace('"drop": [', rng.choice(['"drop": null, "drop": [', '"drop": ["KILL"], "add": 3, "drop": [']), 1)
        try:
            K.Batch.from_json([d])
        except K.EvaluationError:
            continue  # (a 422 in the product as in the reference: no row)
        docs.append(d)
    batch = K.Batch.from_json(docs)
    words = batch.debug_host_walk(env, ids, K.AUDIT)
    assert columns_equal_documents(env, policies, ids, batch, docs, words) >= 200


@pytest.mark.parametrize("kind,cfg,least", [(4, "c4_64", 1000), (5, "c5_mixed", 1000)])
def test_synthetic_rows(kind, cfg, least):
    # (counted on the parent's host walk: 1,701 patched pairs of C4 and 1,148 of C5 at 600 rows, seed 4100)
    env, policies, ids, batch, docs, words = synthetic(kind, cfg)
    seen = {"mod": set(), "pointer": set(), "shape": set(), "longest": 0}
    assert columns_equal_documents(env, policies, ids, batch, docs, words, seen) >= least
    assert seen["longest"] > 256


def synthetic(kind, cfg, rows=600, seed=4100):
    key = ("synthetic", kind, rows, seed)
    if key not in _memo:
        policies = config(cfg)
        env = K.EvaluationEnvironment(policies, continue_on_errors=True, always_accept_namespace="kubewarden")
        ids = env.policy_ids()
        syn = K.SynthBatch(kind, rows, seed=seed)
        docs = [syn.json(r) for r in range(rows)]
        batch = K.Batch.from_json(docs)
        _memo[key] = (env, policies, ids, batch, docs, batch.debug_host_walk(env, ids, K.AUDIT), syn)
    return _memo[key][:6]


# ---- 3. windows --------------------------------------------------------------------------------------------------------

def test_windows_and_rounds(monkeypatch):
    env, policies, ids, batch, docs, words = synthetic(5, "c5_mixed")
    rows, cols = patched_items(words, len(ids))
    whole = {f: batch.patches_from_words(env, ids, words, rows, cols, form=f, how=1) for f in (OPS, RESPONSE)}
    assert np.diff(whole[RESPONSE].off.astype(np.int64)).max() > 1024 and np.diff(whole[OPS].off.astype(np.int64)).max() > 256
    monkeypatch.setenv("KW_MESSAGES_WINDOW", "256")
    for f in (OPS, RESPONSE):
        assert same(batch.patches_from_words(env, ids, words, rows, cols, form=f, how=1), whole[f])
    monkeypatch.setenv("KW_MESSAGES_CHUNK", "100")
    for f in (OPS, RESPONSE):
        assert same(batch.patches_from_words(env, ids, words, rows, cols, form=f, how=1), whole[f])
        assert same(batch.patches_from_words(env, ids, words, rows, cols, form=f, how=0), whole[f])


# ---- 4. shapes through the ABI ----------------------------------------------------------------------------------------------

def _arg_error(call):
    with pytest.raises(K.EvaluationError) as e:
        call()
    assert e.value.code == N.KW_E_ARG
    return str(e.value)


def test_shapes_through_the_abi():
    env, policies, ids, jb, docs, words = synthetic(4, "c4_64")
    syn = _memo[("synthetic", 4, 600, 4100)][6]
    sb = syn.batch()
    assert np.array_equal(sb.debug_host_walk(env, ids, K.AUDIT), words)
    rows, cols = patched_items(words, len(ids))
    place, pointer = sb.patch_shape()
    assert (place == 0).all() and (pointer == N.KW_PP_UNKNOWN).all()
    for how in (0, 1):  # every patched item is the host's
        got = sb.patches_from_words(env, ids, words, rows, cols, how=how)
        assert got.text.size == 0 and np.array_equal(got.host, np.arange(rows.size, dtype=np.uint64))
    assert np.array_equal(predicted_host(sb, policies, ids, words, rows, cols), np.arange(rows.size, dtype=np.uint64))
    assert "pointer" in _arg_error(lambda: sb.format_patch(env, int(rows[0]), ids[int(cols[0])], int(words.reshape(-1, len(ids))[rows[0], cols[0]])))
    jplace, jpointer = jb.patch_shape()
    # wrong sizes and codes: KW_E_ARG, nothing changes
    _arg_error(lambda: sb.set_patch_shape(jplace[:-1], jpointer))
    _arg_error(lambda: sb.set_patch_shape(jplace, jpointer[:-1]))
    bad = jplace.copy()
    bad[3] = (N.KW_PS_MAX + 1) << N.KW_PS_SHIFT
    _arg_error(lambda: sb.set_patch_shape(bad, jpointer))
    bad = jpointer.copy()
    bad[5] = N.KW_PP_CRONJOB + 1
    _arg_error(lambda: sb.set_patch_shape(jplace, bad))
    assert (sb.patch_shape()[0] == 0).all()
    # a known pointer and one unknown shape: the message names the container
    half = jplace.copy()
    r0 = int(rows[0])
    c0 = int(sb.view().ctr_off[r0])
    half[c0] = 0
    sb.set_patch_shape(half, jpointer)
    assert "shape of container 0" in _arg_error(lambda: sb.format_patch(env, r0, ids[int(cols[0])], int(words.reshape(-1, len(ids))[r0, cols[0]])))
    sb.set_patch_shape(jplace, jpointer)
    assert np.array_equal(sb.patch_shape()[0], jplace) and np.array_equal(sb.patch_shape()[1], jpointer)
    for f in (OPS, RESPONSE):
        want = jb.patches_from_words(env, ids, words, rows, cols, form=f, how=0)
        for how in (0, 1):
            assert same(sb.patches_from_words(env, ids, words, rows, cols, form=f, how=how), want)
    # a word without KW_F_PATCH, and a patched word under a column of another family: listed, not rendered
    npol = len(ids)
    caps = capabilities_columns(policies, ids)
    other = next(c for c in range(npol) if c not in caps)
    w2 = words.reshape(-1, npol).copy()
    plain = np.nonzero((w2[:, int(cols[0])] & N.KW_F_PATCH) == 0)[0]
    assert plain.size
    w2[r0, other] |= N.KW_F_PATCH
    rr = np.array([r0, plain[0], r0], dtype=np.uint64)
    cc = np.array([cols[0], cols[0], other], dtype=np.uint32)
    for how in (0, 1):
        got = jb.patches_from_words(env, ids, w2, rr, cc, how=how)
        assert got.host.tolist() == [1, 2] and got.off.tolist()[1:] == [got.text.size] * 3 and got.text.size > 0
    assert np.array_equal(predicted_host(jb, policies, ids, w2, rr, cc), [1, 2])
    _arg_error(lambda: jb.format_patch(env, int(plain[0]), ids[int(cols[0])], int(w2[plain[0], cols[0]])))
    assert "family" in _arg_error(lambda: jb.format_patch(env, r0, ids[other], int(w2[r0, other])))
    # the capacity contract, as kw_batch_responses has it
    whole = jb.patches_from_words(env, ids, words, rows, cols, how=1)
    with pytest.raises(K.MessagesNoSpace) as e:
        jb.patches_from_words(env, ids, words, rows, cols, how=1, cap=whole.text.size - 1)
    assert e.value.need == whole.text.size and np.array_equal(e.value.off, whole.off)
    _arg_error(lambda: jb.patches_from_words(env, ids, words, rows, cols, form=2))


# ---- 5. the stand-alone check under sanitizers -------------------------------------------------------------------------------

def test_patches_check_under_sanitizers(tmp_path):
    exe = tmp_path / "patches_check"
    subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(PKG, "csrc"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "patches_check.cpp")], check=True)
    # (out-of-bounds accesses and undefined behaviour are the point; the leak check at exit needs
    # ptrace rights a test runner may lack)
    out = subprocess.run([str(exe)], check=False, capture_output=True, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "failures 0" in out.stdout
