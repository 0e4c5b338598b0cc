"""The JSONPatch of accepted mutations on the device (kw_batch_patches). Every case starts from
poisoned verdict words and requires the device's result in both forms to equal, byte for byte (off,
text, words, host), the reference renderer's (kw_debug_patches_words how=0: one kw_format_patch per
item) over the words read back from the same pass, and again on a second call; the host list must be
the one the predicate of tests/test_patches.py predicts from the words, the policy list and the
shape columns, and on a batch made from JSON every KW_F_PATCH item must be rendered. Item counts
around the wave's 64 items, the shape fixture in both origins, the minimum window and rounds of 100
items over C5 rows (kw_debug_patches_stats proves the paths were taken), a split batch, a bulk pass
with a kw_batch_responses call beside it whose host list is handed on, a batch made from columns
before and after kw_batch_set_patch_shape, and the capacity and argument errors, each followed by a
correct call."""
import numpy as np
import pytest

import kwgpu as K
from helpers import config
from kwgpu import _native as N
from test_messages import same
from test_patches import fixture, patched_items, predicted_host

pytestmark = pytest.mark.gpu
NS = "kubewarden"
POISON = 0xA5A5A5A5
FORMS = (N.KW_PATCH_OPS, N.KW_PATCH_RESPONSE)
_memo = {}


@pytest.fixture(autouse=True)
def _poisoned_verdicts(monkeypatch):
    monkeypatch.setenv("KW_POISON_VERDICTS", "1")


def _words(b):
    rows, rw = b.last_pass()
    words = b.verdicts(rows * rw)
    assert not (words == POISON).any(), "words the pass never wrote"
    return words, rw


def _check(b, env, policies, ids, words, rows, cols, from_json=True):
    """The device's patches of the items over b's last pass against the reference over `words`, in
    both forms; {form: result}."""
    out = {}
    want_host = predicted_host(b, policies, ids, words, rows, cols)
    w = np.asarray(words, dtype=np.uint32).reshape(-1, len(ids))[rows.astype(np.int64), cols.astype(np.int64)]
    if from_json:  # every KW_F_PATCH item is rendered
        assert np.array_equal(want_host, np.nonzero((w & N.KW_F_PATCH) == 0)[0])
    for form in FORMS:
        got = b.patches(env, ids, rows, cols, form=form, words=True)
        ref = b.patches_from_words(env, ids, words, rows, cols, form=form, how=0, with_words=True)
        assert np.array_equal(got.off, ref.off), (form, np.nonzero(got.off != ref.off)[0][:8])
        assert got.text.tobytes() == ref.text.tobytes(), (form, np.nonzero(got.text != ref.text)[0][:8])
        assert np.array_equal(got.words, ref.words) and np.array_equal(got.host, ref.host)
        assert np.array_equal(got.host, want_host)
        lens = np.diff(got.off.astype(np.int64))
        listed = np.isin(np.arange(rows.size), got.host)
        assert (lens[listed] == 0).all() and (lens[~listed] > 0).all()
        assert same(b.patches(env, ids, rows, cols, form=form, words=True), got)  # the same input, the same bytes
        assert b.debug_patches_stats()["host"] == got.host.size
        out[form] = got
    return out


def _is_arg_error(call):
    with pytest.raises(K.EvaluationError) as e:
        call()
    assert e.value.code == N.KW_E_ARG


def _synth(cfg, kind, rows, seed):
    """(env, policies, ids, the batch made from the rows' JSON after an AUDIT pass, its words, the generator)."""
    key = (cfg, rows)
    if key not in _memo:
        policies = config(cfg)
        env = K.EvaluationEnvironment(policies, continue_on_errors=True, always_accept_namespace=NS, device=0)
        ids = env.policy_ids()
        syn = K.SynthBatch(kind, rows, seed=seed)
        b = K.Batch.from_json([syn.json(r) for r in range(rows)]).to_device(0)
        b.validate(env, ids, K.AUDIT)
        words, rw = _words(b)
        _memo[key] = (env, policies, ids, b, words, syn)
    env, policies, ids, b, words, syn = _memo[key]
    if b.last_pass() != (rows, len(ids)):
        b.validate(env, ids, K.AUDIT)
    return _memo[key]


@pytest.mark.parametrize("count", [1, 63, 64, 65, 257, 4096, 4097, "shuffled", "mixed"])
def test_item_counts(count):  # (4096: the scan's tile of lengths exactly full; 4097: one length into a second tile)
    env, policies, ids, b, words, _ = _synth("c4_64", 4, 3000, 4100)
    rows, cols = patched_items(words, len(ids))
    assert rows.size > 4097
    rng = np.random.default_rng(9)
    if count == "shuffled":  # any order, with repeats
        pick = rng.integers(0, rows.size, size=5000)
        rows, cols = rows[pick], cols[pick]
    elif count == "mixed":  # with pairs that carry no patch
        rows = np.concatenate([rows[:2000], rng.integers(0, 3000, size=2000).astype(np.uint64)])
        cols = np.concatenate([cols[:2000], rng.integers(0, len(ids), size=2000).astype(np.uint32)])
        pick = rng.permutation(rows.size)
        rows, cols = rows[pick], cols[pick]
    else:
        rows, cols = rows[1000:1000 + count], cols[1000:1000 + count]
    got = _check(b, env, policies, ids, words, rows, cols)
    if count == "mixed":
        assert 500 < got[N.KW_PATCH_OPS].host.size < 2500
    else:
        assert got[N.KW_PATCH_OPS].host.size == 0 and got[N.KW_PATCH_OPS].text.size > 50 * rows.size
    st = b.debug_patches_stats()
    assert st["rounds"] == 1 and st["windows"] >= (rows.size + 63) // 64


@pytest.mark.parametrize("origin", [K.VALIDATE, K.AUDIT])
def test_shape_fixture(origin):
    policies, docs = fixture()
    env = K.EvaluationEnvironment(policies, device=0)
    ids = env.policy_ids()
    b = K.Batch.from_json(docs).to_device(0)
    b.validate(env, ids, origin)
    words, rw = _words(b)
    rows, cols = patched_items(words, rw)
    assert rows.size >= 10
    got = _check(b, env, policies, ids, words, rows, cols)
    assert got[N.KW_PATCH_RESPONSE].host.size == 0
    # all pairs: the unpatched ones are listed
    ar = np.repeat(np.arange(len(docs), dtype=np.uint64), rw)
    ac = np.tile(np.arange(rw, dtype=np.uint32), len(docs))
    _check(b, env, policies, ids, words, ar, ac)


def test_minimum_window_and_rounds(monkeypatch):
    env, policies, ids, b, words, _ = _synth("c5_mixed", 5, 3000, 4100)
    rows, cols = patched_items(words, len(ids))
    rows, cols = rows[:1000], cols[:1000]
    whole = _check(b, env, policies, ids, words, rows, cols)
    assert np.diff(whole[N.KW_PATCH_OPS].off.astype(np.int64)).max() > 1024
    assert b.debug_patches_stats()["rounds"] == 1
    monkeypatch.setenv("KW_MESSAGES_WINDOW", "256")
    got = _check(b, env, policies, ids, words, rows, cols)
    st = b.debug_patches_stats()
    assert st["spanning"] > 100 and st["windows"] > 4 * ((rows.size + 63) // 64)
    assert all(same(got[f], whole[f]) for f in FORMS)
    monkeypatch.setenv("KW_MESSAGES_CHUNK", "100")
    got = _check(b, env, policies, ids, words, rows, cols)
    assert b.debug_patches_stats()["rounds"] == 10
    assert all(same(got[f], whole[f]) for f in FORMS)
    monkeypatch.delenv("KW_MESSAGES_WINDOW")
    got = _check(b, env, policies, ids, words, rows, cols)
    assert all(same(got[f], whole[f]) for f in FORMS)


def test_split_batch_takes_batch_rows(monkeypatch):
    monkeypatch.setenv("KW_SPLIT", "1")
    policies = config("c5_mixed")
    env = K.EvaluationEnvironment(policies, continue_on_errors=True, always_accept_namespace=NS, device=0)
    ids = env.policy_ids()
    syn = K.SynthBatch(5, 4000, seed=55)
    docs = [syn.json(r) for r in range(4000)]
    b = K.Batch.from_json(docs).to_device(0)
    b.validate(env, ids, K.AUDIT)
    words, rw = _words(b)
    rows, cols = patched_items(words, rw)
    assert rows.size > 3000
    got = _check(b, env, policies, ids, words, rows, cols)
    monkeypatch.setenv("KW_SPLIT", "0")
    flat = K.Batch.from_json(docs).to_device(0)
    flat.validate(env, ids, K.AUDIT)
    for f in FORMS:
        assert same(flat.patches(env, ids, rows, cols, form=f, words=True), got[f])


def test_after_a_bulk_pass():
    policies = config("c4_64")
    env = K.EvaluationEnvironment(policies, continue_on_errors=True, always_accept_namespace=NS, device=0)
    ids = env.policy_ids()
    nrows = 3000
    syn = K.SynthBatch(4, nrows, seed=4200)
    b = K.Batch.from_json([syn.json(r) for r in range(nrows)])
    b.validate_host(env, ids, origin=K.AUDIT, chunk_rows=512)
    assert b.last_pass() == (nrows, len(ids))
    words, rw = _words(b)
    rows, cols = patched_items(words, rw)
    first = b.patches(env, ids, rows, cols, form=N.KW_PATCH_OPS, words=True, cap=2000 * rows.size)
    assert b.debug_patches_stats()["uploaded_side"] == 1  # no pass reads the shape columns
    again = b.patches(env, ids, rows, cols, form=N.KW_PATCH_OPS, words=True, cap=2000 * rows.size)
    assert b.debug_patches_stats()["uploaded_side"] == 0 and same(first, again)
    got = _check(b, env, policies, ids, words, rows, cols)
    assert same(first, got[N.KW_PATCH_OPS])
    # a responses call beside it keeps its own bytes, and its host list goes straight to patches()
    pick = np.random.default_rng(5).choice(nrows * rw, size=20000, replace=False)
    ar, ac = (pick // rw).astype(np.uint64), (pick % rw).astype(np.uint32)
    rsp = b.responses(env, ids, ar, ac, words=True)
    assert same(rsp, b.responses_from_words(env, ids, words, ar, ac, how=0, with_words=True))
    hr, hc = ar[rsp.host.astype(np.int64)], ac[rsp.host.astype(np.int64)]
    assert hr.size > 100
    handed = _check(b, env, policies, ids, words, hr, hc)[N.KW_PATCH_RESPONSE]
    carried = (handed.words & N.KW_F_PATCH) != 0
    assert carried.sum() > 100 and np.array_equal(np.nonzero(~carried)[0], handed.host)
    assert same(b.responses(env, ids, ar, ac, words=True), rsp)


def test_from_soa_with_set_patch_shape():
    env, policies, ids, jb, words, syn = _synth("c4_64", 4, 3000, 4100)
    sb = syn.batch().to_device(0)
    sb.validate(env, ids, K.AUDIT)
    sw, rw = _words(sb)
    assert np.array_equal(sw, words)
    rows, cols = patched_items(words, rw)
    rows, cols = rows[:3000], cols[:3000]
    before = _check(sb, env, policies, ids, sw, rows, cols, from_json=False)
    assert before[N.KW_PATCH_OPS].host.size == rows.size and before[N.KW_PATCH_OPS].text.size == 0
    sb.set_patch_shape(*jb.patch_shape())  # on a device batch: the device copy of the shapes is dropped
    after = _check(sb, env, policies, ids, sw, rows, cols, from_json=False)
    assert sb.debug_patches_stats()["uploaded_side"] == 0
    want = _check(jb, env, policies, ids, words, rows, cols)
    assert all(same(after[f], want[f]) for f in FORMS) and after[N.KW_PATCH_OPS].host.size == 0
    # shapes set again: uploaded again
    place, pointer = jb.patch_shape()
    place = place.copy()
    place[int(sb.view().ctr_off[int(rows[0])])] = 0
    sb.set_patch_shape(place, pointer)
    got = sb.patches(env, ids, rows, cols, cap=want[N.KW_PATCH_RESPONSE].text.size)  # (a cap: one call of the library, not two)
    assert sb.debug_patches_stats()["uploaded_side"] == 1 and got.host.size >= 1 and got.host[0] == 0
    assert np.array_equal(got.host, predicted_host(sb, policies, ids, sw, rows, cols))


def test_errors_on_the_device():
    env, policies, ids, b, words, _ = _synth("c4_64", 4, 3000, 4100)
    npol = len(ids)
    rows, cols = patched_items(words, npol)
    # (two pairs under the last column, which is no psp-capabilities policy: listed for the host)
    rows = np.append(rows[:4000], np.array([0, 1], dtype=np.uint64))
    cols = np.append(cols[:4000], np.array([npol - 1, npol - 1], dtype=np.uint32))
    assert rows.dtype == np.uint64 and cols.dtype == np.uint32
    for form in FORMS:
        whole = _check(b, env, policies, ids, words, rows, cols)[form]
        nbytes, nhost = whole.text.size, whole.host.size
        assert nhost >= 1

        def good():
            assert same(b.patches(env, ids, rows, cols, form=form, words=True), whole)

        for cap in (nbytes - 1, 0):  # KW_E_NOSPACE: bytes, nhost and all of off exact
            with pytest.raises(K.MessagesNoSpace) as e:
                b.patches(env, ids, rows, cols, form=form, cap=cap)
            assert e.value.need == nbytes and e.value.nhost == nhost and np.array_equal(e.value.off, whole.off)
            good()
        assert same(b.patches(env, ids, rows, cols, form=form, words=True, cap=nbytes), whole)
        with pytest.raises(K.MessagesNoSpace) as e:
            b.patches(env, ids, rows, cols, form=form, host_cap=nhost - 1)
        assert e.value.nhost == nhost and e.value.need == nbytes and np.array_equal(e.value.off, whole.off)
        good()
        _is_arg_error(lambda: b.patches(env, ids, np.append(rows, 3000), np.append(cols, 0), form=form))  # a row outside the pass
        good()
        _is_arg_error(lambda: b.patches(env, ids, np.append(rows, 0), np.append(cols, npol), form=form))  # a col outside the pass
        good()
        _is_arg_error(lambda: b.patches(env, ids[:7], rows[:10], cols[:10] % 7, form=form))  # a policy list of another length
        good()
    _is_arg_error(lambda: b.patches(env, ids, rows, cols, form=2))
    b.validate_rows(env, [ids[r % npol] for r in range(3000)])  # a rows-mode pass has a policy per row
    _is_arg_error(lambda: b.patches(env, ids, rows, cols))
    b.validate(env, ids, K.AUDIT)
    assert same(b.patches(env, ids, rows, cols, words=True), whole)
    empty = b.patches(env, ids, rows[:0], cols[:0])
    assert empty.text.size == 0 and empty.off.tolist() == [0]
