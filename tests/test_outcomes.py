"""The grouped outcome count (include/kwgpu.h kw_batch_outcomes; policy-server_amd/csrc/outcomes.hpp)
on the host: the words of the host walk go through the attribute dictionary
(kw_batch_attribute_groups), the reference reducer (kw_debug_outcome_words) and the fold
(kw_metrics_add_outcomes), and the rendered metrics must be byte-equal to those of every pair fed
through kw_metrics_record; the dictionary against a Python dict; the reducer against np.add.at.
tests/outcomes_check.cpp runs the sort, the unit table, the range cut and the kernel's lane geometry
as a plain executable under AddressSanitizer and UBSan (no Python in that process)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import kwgpu as K
import outcomes_cases as OC
from kwgpu import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "policy-server_amd")
CXX = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
ROWS = 1500
_memo = {}


def fixture():
    """(env, ids, documents, admission batch, raw batch, mixed batch), made once."""
    if "fx" not in _memo:
        env = K.EvaluationEnvironment(OC.policies(), continue_on_errors=True, always_accept_namespace=OC.NS)
        docs = OC.docs(ROWS)
        adm = K.Batch.from_json(docs)
        raw = K.Batch.from_json(OC.raw_docs(docs[:120]), raw=True)
        _memo["fx"] = (env, env.policy_ids(), docs, adm, raw, OC.mixed_batch(adm))
    return _memo["fx"]


def walk(batch, origin):
    env, ids = fixture()[:2]
    key = (id(batch), origin)
    if key not in _memo:
        _memo[key] = batch.debug_host_walk(env, ids, origin)
    return _memo[key]


def expected_groups(batch, rkinds):
    """The dictionary restated over the batch's view: (row_group, first_row) with ids by first
    appearance of (raw) or (requestKind.kind, operation, has namespace, namespace)."""
    v = batch.view()
    flags = np.ctypeslib.as_array(v.req_flags, shape=(v.n_requests,))
    ns, op = OC.strings(v.ns), OC.strings(v.op)
    ids, row_group, first = {}, [], []
    for r in range(v.n_requests):
        if flags[r] & N.KW_REQ_RAW:
            key = ("raw",)
        else:
            has = bool(flags[r] & N.KW_REQ_HAS_NAMESPACE)
            key = (rkinds[r], op[r], has, ns[r] if has else b"")
        if key not in ids:
            ids[key] = len(ids)
            first.append(r)
        row_group.append(ids[key])
    return np.array(row_group, dtype=np.uint32), np.array(first, dtype=np.uint64), ids


def request_kinds(docs):
    return [((d["request"].get("requestKind") or {}).get("kind", "")).encode() for d in docs]


def test_fixture_is_not_vacuous():
    """What the other tests rely on: the outcome codes 0, 1, 3, 4 and 8 occur, the groups are many,
    and bypassed, namespace-less, empty-namespace and raw rows exist."""
    env, ids, docs, adm, raw, mixed = fixture()
    w = walk(adm, K.VALIDATE)
    seen = np.bincount(OC.outcome_code(w), minlength=N.KW_OUT_N)
    for code in (0, 1, 3, 4, 8):
        assert seen[code] > 0, (code, seen)
    assert (w & np.uint32(N.KW_BYPASS)).any()
    row_group, first_row = adm.attribute_groups()
    assert first_row.size >= 50
    v = adm.view()
    flags = np.ctypeslib.as_array(v.req_flags, shape=(v.n_requests,))
    assert ((flags & N.KW_REQ_HAS_NAMESPACE) == 0).any()
    ns = OC.strings(v.ns)
    assert any((flags[r] & N.KW_REQ_HAS_NAMESPACE) and ns[r] == b"" for r in range(ROWS))
    rflags = np.ctypeslib.as_array(raw.view().req_flags, shape=(raw.n,))
    assert (rflags & N.KW_REQ_RAW).all()
    mflags = np.ctypeslib.as_array(mixed.view().req_flags, shape=(mixed.n,))
    assert (mflags & N.KW_REQ_RAW).any() and not (mflags & N.KW_REQ_RAW).all()
    # the run-time error group and the mutating policy are what reach codes 4 and 3
    code = OC.outcome_code(w).reshape(ROWS, len(ids))
    assert (code[:, ids.index("group-runtime-error")] == 4).any() and (code[:, ids.index("group-runtime-error")] == 1).any()
    assert (code[:, ids.index("psp-capabilities-mutating")] == 3).any()
    bypassed = (w.reshape(ROWS, len(ids))[:, 0] & np.uint32(N.KW_BYPASS)) != 0  # (the bypass comes first: service.rs:40-71)
    assert (code[~bypassed, ids.index("namespace-empty")] == 8).all() and (code[bypassed] == 1).all()


def test_fold_equals_per_pair_recording():
    """Both origins over the admission batch, then the raw and the mixed batch, all accumulating in
    one kw_metrics: byte-equal to every pair through kw_metrics_record."""
    env, ids, docs, adm, raw, mixed = fixture()
    fold, pairs = K.Metrics(), K.Metrics()
    for batch, origin, latency in ((adm, K.VALIDATE, 7), (adm, K.AUDIT, 260), (raw, K.VALIDATE, 0), (mixed, K.AUDIT, 20000),
                                   (adm, K.VALIDATE, 7)):
        w = walk(batch, origin)
        row_group, first_row = batch.attribute_groups()
        counts = K.Batch.outcomes_from_words(w, len(ids), row_group, first_row.size)
        assert int(counts.sum()) == w.size
        fold.add_outcomes(env, batch, ids, counts, first_row, latency, origin)
        OC.record_all_pairs(pairs, env, batch, ids, w, latency, origin)
        assert fold.render() == pairs.render()
    text = fold.render()
    for s in ('request_origin="audit"', 'request_origin="validate"', 'error_code="500"', "initialization_error=",
              'mutated="true"', 'resource_kind="Deployment"', 'resource_kind=""', 'resource_namespace=""', 'le="+Inf"'):
        assert s in text, s


def test_fold_skips_policies_outside_the_environment():
    env, ids, docs, adm, raw, mixed = fixture()
    w = walk(raw, K.VALIDATE)
    row_group, first_row = raw.attribute_groups()
    counts = K.Batch.outcomes_from_words(w, len(ids), row_group, first_row.size)
    some, none = K.Metrics(), K.Metrics()
    u64p = C.POINTER(C.c_uint64)
    pols = np.array([env._idx(p) for p in ids], dtype=np.int32)
    bad = pols.copy()
    bad[1::2] = -1
    bad[0] = 10 ** 6
    L = N.lib()

    def add(m, p, first):
        return L.kw_metrics_add_outcomes(m._h, env._h, raw._h, p.ctypes.data_as(C.POINTER(C.c_int32)), len(ids), K.VALIDATE, 3,
                                         first.ctypes.data_as(u64p), first.size, counts.ctypes.data_as(u64p))
    assert add(some, bad, first_row) == N.KW_OK
    keep = [j for j in range(len(ids)) if bad[j] == pols[j]]
    w2 = w.reshape(-1, len(ids))[:, keep]
    OC.record_all_pairs(none, env, raw, [ids[j] for j in keep], w2, 3, K.VALIDATE)
    assert some.render() == none.render() and some.samples()
    # a first_row outside the batch: KW_E_ARG, nothing added
    empty = K.Metrics()
    assert add(empty, pols, np.array([raw.n], dtype=np.uint64)) == N.KW_E_ARG and not empty.samples()


def test_dictionary_matches_a_python_dict():
    env, ids, docs, adm, raw, mixed = fixture()
    kinds = request_kinds(docs)
    for batch, rk in ((adm, kinds), (raw, [b""] * raw.n), (mixed, [b""] * mixed.n)):
        row_group, first_row = batch.attribute_groups()
        want_rg, want_first, keys = expected_groups(batch, rk)
        assert np.array_equal(row_group, want_rg) and np.array_equal(first_row, want_first)
        assert np.array_equal(np.unique(row_group), np.arange(first_row.size))  # ids 0..n-1, each used
        again = batch.attribute_groups()  # kept on the batch
        assert np.array_equal(again[0], row_group) and np.array_equal(again[1], first_row)
    assert raw.attribute_groups()[1].tolist() == [0]  # all raw rows: one group
    assert ("raw",) in expected_groups(mixed, [b""] * mixed.n)[2]
    # a row without a namespace and one whose namespace is "" are different groups
    v = adm.view()
    flags = np.ctypeslib.as_array(v.req_flags, shape=(ROWS,))
    ns = OC.strings(v.ns)
    rg = adm.attribute_groups()[0]
    none_rows = [r for r in range(ROWS) if not flags[r] & N.KW_REQ_HAS_NAMESPACE]
    empty_rows = [r for r in range(ROWS) if flags[r] & N.KW_REQ_HAS_NAMESPACE and ns[r] == b""]
    assert not set(rg[none_rows].tolist()) & set(rg[empty_rows].tolist())


def test_dictionary_nospace_and_synth_batch():
    env, ids, docs, adm, raw, mixed = fixture()
    L = N.lib()
    n = C.c_uint32()
    want = adm.attribute_groups()[1].size
    first = np.zeros(want, dtype=np.uint64)
    u64p = C.POINTER(C.c_uint64)
    assert L.kw_batch_attribute_groups(adm._h, None, first.ctypes.data_as(u64p), want - 1, C.byref(n)) == N.KW_E_NOSPACE
    assert n.value == want  # the need
    assert L.kw_batch_attribute_groups(adm._h, None, None, 0, C.byref(n)) == N.KW_E_NOSPACE and n.value == want
    assert L.kw_batch_attribute_groups(adm._h, None, first.ctypes.data_as(u64p), want, C.byref(n)) == N.KW_OK
    assert L.kw_batch_attribute_groups(None, None, None, 0, C.byref(n)) == N.KW_E_ARG
    syn = K.SynthBatch(4, 3000, seed=5).batch()  # from_soa: no requestKind column
    row_group, first_row = syn.attribute_groups()
    want_rg, want_first, _ = expected_groups(syn, [b""] * 3000)
    assert np.array_equal(row_group, want_rg) and np.array_equal(first_row, want_first) and first_row.size > 1
    # more rows than one host-worker range: the ranges' dictionaries merge in order
    big = K.SynthBatch(0, 40000, seed=6).batch()
    row_group, first_row = big.attribute_groups()
    want_rg, want_first, _ = expected_groups(big, [b""] * 40000)
    assert np.array_equal(row_group, want_rg) and np.array_equal(first_row, want_first)


@pytest.mark.parametrize("npol", [1, 31, 64, 65])
def test_reducer_matches_numpy(npol):
    env, ids, docs, adm, raw, mixed = fixture()
    w = walk(adm, K.VALIDATE).reshape(ROWS, len(ids))
    w = np.ascontiguousarray(np.tile(w, (1, 3))[:, :npol])
    rng = np.random.default_rng(npol)
    for ngroups, rg in ((1, None), (7, rng.integers(0, 7, ROWS)), (ROWS, rng.permutation(ROWS)),
                        (40, rng.integers(0, 20, ROWS) * 2)):  # (every odd group empty)
        got = K.Batch.outcomes_from_words(w, npol, rg, ngroups)
        assert np.array_equal(got, OC.numpy_outcomes(w, npol, rg, ngroups))
        assert int(got.sum()) == ROWS * npol


def test_reducer_hand_made_words():
    ge = 14 << 8
    init = N.KW_FST_INIT_ERROR << N.KW_F_STATUS_SHIFT
    words = np.array([0, 1, 2, 3, ge, ge | 1, ge | 2, ge | 3, init, init | 3 | N.KW_BYPASS,  # all nine codes, init error first
                      N.KW_BYPASS | N.KW_V_MUTATED, N.KW_BYPASS | ge, 0xA5A5A5A5], dtype=np.uint32)
    want = [0, 1, 2, 3, 4, 5, 6, 7, 8, 8, 1, 1, 1]  # a bypass is accepted, not mutated, no error; so reads the poison word
    assert OC.outcome_code(words).tolist() == want
    got = K.Batch.outcomes_from_words(words, 1, np.arange(words.size), words.size)
    assert got.shape == (words.size, N.KW_OUT_N, 1)
    assert np.array_equal(got[:, :, 0].argmax(axis=1), want) and (got.sum(axis=(1, 2)) == 1).all()
    row = K.Batch.outcomes_from_words(words, words.size)  # one row, one group
    assert np.array_equal(row[0].argmax(axis=0), want) and int(row.sum()) == words.size
    assert not K.Batch.outcomes_from_words(np.zeros(0, dtype=np.uint32), 5, None, 3).any()  # 0 rows
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    out = np.zeros(2 * N.KW_OUT_N, dtype=np.uint64)
    L = N.lib()
    ids = np.array([0, 2], dtype=np.uint32)
    assert L.kw_debug_outcome_words(words.ctypes.data_as(u32p), 2, 1, ids.ctypes.data_as(u32p), 2, out.ctypes.data_as(u64p)) == N.KW_E_ARG
    assert L.kw_debug_outcome_words(words.ctypes.data_as(u32p), 2, 1, None, 0, out.ctypes.data_as(u64p)) == N.KW_E_ARG
    assert L.kw_debug_outcome_words(words.ctypes.data_as(u32p), 2, 0, None, 1, out.ctypes.data_as(u64p)) == N.KW_E_ARG


def test_device_entries_need_a_pass():
    env, ids, docs, adm, raw, mixed = fixture()
    b = K.SynthBatch(0, 4, seed=1).batch()  # never on a device
    out = np.zeros(N.KW_OUT_N * len(ids), dtype=np.uint64)
    assert N.lib().kw_batch_outcomes(b._h, None, 1, out.ctypes.data_as(C.POINTER(C.c_uint64))) == N.KW_E_ARG
    with pytest.raises(K.EvaluationError) as e:
        K.Metrics().record_pass(env, b, ids)
    assert e.value.code == N.KW_E_ARG


def test_outcomes_check_under_sanitizers(tmp_path):
    exe = tmp_path / "outcomes_check"
    subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(PKG, "csrc"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "outcomes_check.cpp")], check=True)
    # (out-of-bounds accesses and undefined behaviour are the point; the leak check at exit needs
    # ptrace rights a test runner may lack)
    out = subprocess.run([str(exe)], check=False, capture_output=True, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "failures 0" in out.stdout
