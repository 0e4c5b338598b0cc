"""The AdmissionResponse bodies of chosen pairs on the device (kw_batch_responses). Every case starts
from poisoned verdict words and requires the device's result to equal, byte for byte (off, text,
words, host), the reference renderer's (kw_debug_responses_words how=0: one format_response per item,
the members' words from the same matrix) over the words read back from the same pass, and again on a
second call; the host list must be the one the predicate of tests/test_responses.py predicts from
the words and the policy list, and at least half of the items must be rendered. Item counts around
the wave's 64 items, every reason, groups with several causes, the fixture whose every string needs
escaping at the default and the minimum window (kw_debug_responses_stats proves the paths were
taken), rounds of 100 items, a split batch, a bulk pass, the members of a digest group, items drawn
from all pairs, and the capacity and argument errors, each followed by a correct call."""
import numpy as np
import pytest

import kwgpu as K
import outcomes_cases as OC
from helpers import config
from kwgpu import _native as N
from test_messages import items_of, reason_of, same
from test_responses import all_pairs, causes_of, odd_case, predicted_host

pytestmark = pytest.mark.gpu
NS = "kubewarden"
POISON = 0xA5A5A5A5
_memo = {}


@pytest.fixture(autouse=True)
def _poisoned_verdicts(monkeypatch):
    monkeypatch.setenv("KW_POISON_VERDICTS", "1")


def _env(name):
    if name not in _memo:
        _memo[name] = K.EvaluationEnvironment(config(name), continue_on_errors=True, always_accept_namespace=NS, device=0)
    return _memo[name]


def _words(b):
    rows, rw = b.last_pass()
    words = b.verdicts(rows * rw)
    assert not (words == POISON).any(), "words the pass never wrote"
    return words, rw


def _check(b, env, ids, words, rows, cols):
    """The device's responses of the items over b's last pass against the reference over `words`."""
    got = b.responses(env, ids, rows, cols, words=True)
    ref = b.responses_from_words(env, ids, words, rows, cols, how=0, with_words=True)
    assert np.array_equal(got.off, ref.off), np.nonzero(got.off != ref.off)[0][:8]
    assert got.text.tobytes() == ref.text.tobytes(), np.nonzero(got.text != ref.text)[0][:8]
    assert np.array_equal(got.words, ref.words) and np.array_equal(got.host, ref.host)
    assert np.array_equal(got.host, predicted_host(env, ids, words, rows, cols))
    assert 2 * got.host.size <= rows.size  # at least half of the items are rendered on the device
    lens = np.diff(got.off.astype(np.int64))
    listed = np.isin(np.arange(rows.size), got.host)
    assert (lens[listed] == 0).all() and (lens[~listed] > 0).all()
    assert same(b.responses(env, ids, rows, cols, words=True), got)  # the same input, the same bytes
    bare = b.responses(env, ids, rows, cols)
    assert bare.words is None and bare.text.tobytes() == got.text.tobytes()
    assert b.debug_responses_stats()["host"] == got.host.size
    return got


def _is_arg_error(call):
    with pytest.raises(K.EvaluationError) as e:
        call()
    assert e.value.code == N.KW_E_ARG


def _synth(cfg, kind, rows, seed):
    key = (cfg, rows)
    if key not in _memo:
        env = _env(cfg)
        ids = env.policy_ids()
        b = K.SynthBatch(kind, rows, seed=seed).batch().to_device(0)
        b.validate(env, ids, K.AUDIT)
        words, rw = _words(b)
        _memo[key] = (env, ids, b, words)
    env, ids, b, words = _memo[key]
    if b.last_pass() != (rows, len(ids)):
        b.validate(env, ids, K.AUDIT)
    return env, ids, b, words


def _c4(rows):
    return _synth("c4_64", 4, rows, 4100)


@pytest.mark.parametrize("count", [1, 63, 64, 65, 257, 4096, 4097, "all", "shuffled"])
def test_item_counts(count):  # (4096: the scan's tile of lengths exactly full; 4097: one length into a second tile)
    env, ids, b, words = _c4(3000)
    rows, cols, nf = items_of(words, len(ids), extra=0)
    assert nf > 20000
    if count == "shuffled":  # any order, with repeats
        pick = np.random.default_rng(9).integers(0, nf, size=5000)
        rows, cols = rows[pick], cols[pick]
    elif count != "all":
        rows, cols = rows[1000:1000 + count], cols[1000:1000 + count]
    got = _check(b, env, ids, words, rows, cols)
    assert got.text.size > 100 * rows.size  # (the envelope and a uid alone pass 60 bytes)
    st = b.debug_responses_stats()
    assert st["rounds"] == 1 and st["windows"] >= (rows.size + 63) // 64


def test_all_pairs_render_plain_and_bypass_responses():
    env, ids, b, words = _c4(3000)
    rows, cols = all_pairs(3000, len(ids), limit=30000)
    got = _check(b, env, ids, words, rows, cols)
    texts = [got.get(i) for i in range(0, rows.size, 11)]
    assert sum(t.endswith(b'"allowed":true}') for t in texts) > 100 and sum(b'"status"' in t for t in texts) > 100
    # the always-accepted namespace: bypass words, rendered
    bypass = (got.words & np.uint32(0x20)) != 0
    assert bypass.sum() > 0 and (np.diff(got.off.astype(np.int64))[bypass] > 0).all()


def test_every_reason():
    env = K.EvaluationEnvironment(OC.policies(), continue_on_errors=True, always_accept_namespace=NS, device=0)
    ids = env.policy_ids()
    b = K.Batch.from_json(OC.docs(300)).to_device(0)
    b.validate(env, ids, K.VALIDATE)
    words, rw = _words(b)
    assert set(np.unique(reason_of(words)).tolist()) >= set(range(16))
    rows, cols = all_pairs(300, rw)
    got = _check(b, env, ids, words, rows, cols)
    fst = (got.words >> np.uint32(3)) & np.uint32(3)
    assert got.host.size > 700 and (fst == 2).any() and (fst == 3).any() and ((got.words & np.uint32(0x20)) != 0).any()


def test_groups_with_several_causes():
    env, ids, b, words = _synth("c3_group", 3, 2000, 3100)
    rows, cols = all_pairs(2000, len(ids))
    got = _check(b, env, ids, words, rows, cols)
    causes = causes_of(env, ids, words, rows, cols)
    listed = np.isin(np.arange(rows.size), got.host)
    assert int(((causes >= 2) & ~listed).sum()) >= 100
    assert sum(got.get(int(i)).count(b'{"field":"spec.policies.') >= 2 for i in np.nonzero((causes >= 2) & ~listed)[0][:200]) >= 100


def _odd():
    env, ids, batch, w = odd_case(device=0)
    if batch.device != 0:
        batch.to_device(0)
    batch.validate(env, ids, K.VALIDATE)
    words, rw = _words(batch)
    rows, cols = all_pairs(batch.n, rw)
    return env, ids, batch, words, rows, cols


def test_escaped_fixture_and_minimum_window(monkeypatch):
    env, ids, batch, words, rows, cols = _odd()
    whole = _check(batch, env, ids, words, rows, cols)
    st = batch.debug_responses_stats()
    assert st["spanning"] > 0 and st["escaped"] > rows.size  # (every uid grows by escaping)
    causes = causes_of(env, ids, words, rows, cols)
    listed = np.isin(np.arange(rows.size), whole.host)
    assert ((causes == 15) & ~listed).sum() > 20 and ((causes >= 2) & ~listed).sum() >= 100
    assert any(b"mutation is not allowed inside of policy group" in whole.get(i) for i in range(rows.size))
    monkeypatch.setenv("KW_MESSAGES_WINDOW", "256")
    got = _check(batch, env, ids, words, rows, cols)
    st = batch.debug_responses_stats()
    waves = (rows.size + 63) // 64
    assert st["spanning"] > 100 and st["windows"] > waves and st["windows"] >= got.text.size // 256 and st["escaped"] > rows.size
    assert same(got, whole)


def test_rounds_of_a_hundred(monkeypatch):
    env, ids, b, words = _c4(3000)
    rows, cols = all_pairs(3000, len(ids), limit=1000, seed=8)
    whole = _check(b, env, ids, words, rows, cols)
    assert b.debug_responses_stats()["rounds"] == 1
    monkeypatch.setenv("KW_MESSAGES_CHUNK", "100")
    got = _check(b, env, ids, words, rows, cols)
    assert b.debug_responses_stats()["rounds"] == 10
    assert same(got, whole)
    monkeypatch.setenv("KW_MESSAGES_WINDOW", "256")
    assert same(_check(b, env, ids, words, rows, cols), whole)


def test_split_batch_takes_batch_rows(monkeypatch):
    monkeypatch.setenv("KW_SPLIT", "1")
    env = _env("c5_mixed")
    ids = env.policy_ids()
    syn = K.SynthBatch(5, 4000, seed=55)
    b = syn.batch().to_device(0)
    b.validate(env, ids, K.AUDIT)
    words, rw = _words(b)
    rows, cols = all_pairs(4000, rw, limit=20000)
    got = _check(b, env, ids, words, rows, cols)
    assert set(np.unique(reason_of(got.words)).tolist()) & {1, 3, 4, 5, 6, 7, 8, 9}  # messages that quote a container's name
    monkeypatch.setenv("KW_SPLIT", "0")
    flat = syn.batch().to_device(0)
    flat.validate(env, ids, K.AUDIT)
    assert same(flat.responses(env, ids, rows, cols, words=True), got)


def test_after_a_bulk_pass():
    env = _env("c4_64")
    ids = env.policy_ids()
    nrows = 5000
    b = K.SynthBatch(4, nrows, seed=4200).batch()
    b.validate_host(env, ids, origin=K.AUDIT, chunk_rows=512)
    assert b.last_pass() == (nrows, len(ids))
    words, rw = _words(b)
    rows, cols = all_pairs(nrows, rw, limit=20000)
    first = b.responses(env, ids, rows, cols, words=True, cap=400 * rows.size)  # (a cap: one call of the library, not two)
    assert b.debug_responses_stats()["uploaded_side"] == 1  # no pass reads the uid column
    got = _check(b, env, ids, words, rows, cols)
    assert b.debug_responses_stats()["uploaded_side"] == 0 and same(first, got)
    # the messages call beside it: its bytes are its own
    msgs = b.messages(env, ids, rows[:500], cols[:500])
    assert same(msgs, b.messages_from_words(env, ids, words, rows[:500], cols[:500], how=0))


def test_members_of_a_digest_group():
    env, ids, b, words = _c4(300)
    d = b.digest()
    recs = d.recs[::2]
    assert recs.size > 100
    m = b.digest_members(recs)
    cols = np.repeat(recs["col"].astype(np.uint32), np.diff(m.off.astype(np.int64)))
    got = _check(b, env, ids, words, m.rows, cols)
    assert np.array_equal(got.words, m.words) and got.text.size > 100 * m.rows.size


def test_errors_on_the_device():
    env, ids, b, words = _c4(3000)
    npol = len(ids)
    rows, cols = all_pairs(3000, npol, limit=5000, seed=4)
    whole = _check(b, env, ids, words, rows, cols)
    nbytes, nhost = whole.text.size, whole.host.size

    def good():
        assert same(b.responses(env, ids, rows, cols, words=True), whole)

    for cap in (nbytes - 1, 0):  # KW_E_NOSPACE: bytes, nhost and all of off exact
        with pytest.raises(K.MessagesNoSpace) as e:
            b.responses(env, ids, rows, cols, cap=cap)
        assert e.value.need == nbytes and e.value.nhost == nhost and np.array_equal(e.value.off, whole.off)
        good()
    assert same(b.responses(env, ids, rows, cols, words=True, cap=nbytes), whole)
    _is_arg_error(lambda: b.responses(env, ids, np.append(rows, 3000), np.append(cols, 0)))  # a row outside the pass
    good()
    _is_arg_error(lambda: b.responses(env, ids, np.append(rows, 0), np.append(cols, npol)))  # a col outside the pass
    good()
    _is_arg_error(lambda: b.responses(env, ids[:7], rows[:10], cols[:10] % 7))  # a policy list of another length
    good()
    b.validate_rows(env, [ids[r % npol] for r in range(3000)])  # a rows-mode pass has a policy per row
    _is_arg_error(lambda: b.responses(env, ids, rows, cols))
    b.validate(env, ids, K.AUDIT)
    good()
    empty = b.responses(env, ids, rows[:0], cols[:0])
    assert empty.text.size == 0 and empty.off.tolist() == [0]


def test_host_capacity_on_the_device():
    env, ids, batch, words, rows, cols = _odd()
    whole = _check(batch, env, ids, words, rows, cols)
    assert whole.host.size > 1
    with pytest.raises(K.MessagesNoSpace) as e:
        batch.responses(env, ids, rows, cols, host_cap=whole.host.size - 1)
    assert e.value.nhost == whole.host.size and e.value.need == whole.text.size and np.array_equal(e.value.off, whole.off)
    assert same(batch.responses(env, ids, rows, cols, words=True), whole)
