"""The messages of chosen findings on the device (kw_batch_messages). Every case starts from poisoned
verdict words and requires the device's result to equal, byte for byte (off, text, words, host), the
reference renderer's (kw_debug_messages_words how=0: one policy_message call per item) over the words
read back from the same pass, and again on a second call. Item counts around the wave's 64 items,
every reason, the hand documents of tests/test_messages.py, windows at their minimum and rounds of
100 items (kw_debug_messages_stats proves the path was taken), column shapes around the 64-column
groups, a split batch, every kind of pass that leaves all-pairs words in the verdict buffer, the
members of digest groups, and the capacity and argument errors, each followed by a correct call."""
import numpy as np
import pytest

import kwgpu as K
import outcomes_cases as OC
from helpers import config, many_policies_config
from kwgpu import _native as N
from test_messages import LONG_VALUE, hand_case, host_items, items_of, reason_of, same

pytestmark = pytest.mark.gpu
NS = "kubewarden"
POISON = 0xA5A5A5A5
_memo = {}


@pytest.fixture(autouse=True)
def _poisoned_verdicts(monkeypatch):
    monkeypatch.setenv("KW_POISON_VERDICTS", "1")


def _env(name):
    if name not in _memo:
        doc = many_policies_config() if name == "c6_256" else config(name)
        _memo[name] = K.EvaluationEnvironment(doc, continue_on_errors=True, always_accept_namespace=NS, device=0)
    return _memo[name]


def _words(b):
    rows, rw = b.last_pass()
    words = b.verdicts(rows * rw)
    assert not (words == POISON).any(), "words the pass never wrote"
    return words, rw


def _check(b, env, ids, words, rows, cols):
    """The device's messages of the items over b's last pass against the reference over `words`."""
    got = b.messages(env, ids, rows, cols, words=True)
    ref = b.messages_from_words(env, ids, words, rows, cols, how=0, with_words=True)
    assert np.array_equal(got.off, ref.off), np.nonzero(got.off != ref.off)[0][:8]
    assert got.text.tobytes() == ref.text.tobytes(), np.nonzero(got.text != ref.text)[0][:8]
    assert np.array_equal(got.words, ref.words) and np.array_equal(got.host, ref.host)
    assert same(b.messages(env, ids, rows, cols, words=True), got)  # the same input, the same bytes
    bare = b.messages(env, ids, rows, cols)
    assert bare.words is None and bare.text.tobytes() == got.text.tobytes()
    return got


def _is_arg_error(call):
    with pytest.raises(K.EvaluationError) as e:
        call()
    assert e.value.code == N.KW_E_ARG


def _c4(rows):
    key = ("c4", rows)
    if key not in _memo:
        env = _env("c4_64")
        ids = env.policy_ids()
        b = K.SynthBatch(4, rows, seed=4100).batch().to_device(0)
        b.validate(env, ids, K.AUDIT)
        words, rw = _words(b)
        _memo[key] = (env, ids, b, words)
    env, ids, b, words = _memo[key]
    if b.last_pass() != (rows, len(ids)):
        b.validate(env, ids, K.AUDIT)
    return env, ids, b, words


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
    assert got.text.size > (30 * rows.size if rows.size >= 63 else 0)  # (the workloads' messages average 54 bytes and more)
    st = b.debug_messages_stats()
    assert st["rounds"] == 1 and st["windows"] >= (rows.size + 63) // 64 and st["host"] == got.host.size


def test_every_reason():
    env = K.EvaluationEnvironment(OC.policies(), continue_on_errors=True, always_accept_namespace=NS, device=0)
    ids = env.policy_ids()
    b = K.Batch.from_json(OC.docs(300)).to_device(0)
    b.validate(env, ids, K.VALIDATE)
    words, rw = _words(b)
    rows, cols, nf = items_of(words, rw, extra=500)
    assert nf == 4600 and set(np.unique(reason_of(words)).tolist()) >= set(range(16))
    got = _check(b, env, ids, words, rows, cols)
    lens = np.diff(got.off.astype(np.int64))
    assert (lens[nf:] == 0).all() and not np.isin(np.arange(nf, rows.size), got.host).any()
    assert np.array_equal(got.host, host_items(got.words).astype(np.uint64)) and got.host.size >= 727


def _hand():
    env, ids, batch, w = hand_case(device=0)
    if batch.device != 0:
        batch.to_device(0)
    batch.validate(env, ids, K.VALIDATE)
    words, rw = _words(batch)
    rows, cols, nf = items_of(words, rw, extra=20)
    return env, ids, batch, words, rows, cols, nf


def test_hand_documents():
    env, ids, batch, words, rows, cols, nf = _hand()
    got = _check(batch, env, ids, words, rows, cols)
    texts = [got.get(i) for i in range(nf)]
    assert ("label 'k' value '" + LONG_VALUE + "' does not match the constraint '^x$'").encode() in texts
    assert ("container 'c'\"\\é' uses image 'bad', which is rejected").encode("utf-8") in texts
    assert b"container '' uses image 'bad', which is rejected" in texts
    assert b"label 'kk' value '' does not match the constraint '^y+$'" in texts
    assert b"namespace '' is not accepted: only 'only' is allowed" in texts
    assert b"container 'c' uses image 'localhost/x': registry 'localhost' is rejected" in texts
    assert b"container 'c' uses image '': tag 'latest' is rejected" in texts


def test_minimum_window_spans_messages(monkeypatch):
    env, ids, batch, words, rows, cols, nf = _hand()
    whole = _check(batch, env, ids, words, rows, cols)
    assert batch.debug_messages_stats()["spanning"] > 0  # (5,000 bytes pass the default window too)
    monkeypatch.setenv("KW_MESSAGES_WINDOW", "256")
    got = _check(batch, env, ids, words, rows, cols)
    st = batch.debug_messages_stats()
    waves = (rows.size + 63) // 64
    assert st["spanning"] > 1 and st["windows"] > waves and st["windows"] >= got.text.size // 256
    assert same(got, whole)


def test_rounds_of_a_hundred(monkeypatch):
    env, ids, b, words = _c4(3000)
    rows, cols, nf = items_of(words, len(ids), extra=0)
    rows, cols = rows[500:1500], cols[500:1500]
    whole = _check(b, env, ids, words, rows, cols)
    assert b.debug_messages_stats()["rounds"] == 1
    monkeypatch.setenv("KW_MESSAGES_CHUNK", "100")
    got = _check(b, env, ids, words, rows, cols)
    assert b.debug_messages_stats()["rounds"] == 10
    assert same(got, whole)
    monkeypatch.setenv("KW_MESSAGES_WINDOW", "256")
    assert same(_check(b, env, ids, words, rows, cols), whole)


@pytest.mark.parametrize("npol", [1, 63, 64, 65, 128])
def test_column_shapes(npol):
    env = _env("c6_256")
    ids = env.policy_ids()[:npol]
    nrows = 1500
    if "c6" not in _memo:
        _memo["c6"] = K.SynthBatch(6, nrows, seed=6).batch().to_device(0)
    b = _memo["c6"]
    b.validate(env, ids, K.AUDIT)
    assert b.last_pass() == (nrows, npol)
    words, rw = _words(b)
    rows, cols, nf = items_of(words, rw, extra=50)
    keep = np.zeros(rows.size, dtype=bool)
    keep[nf:] = True
    for c in range(npol):  # a sample of the findings of every column
        at = np.nonzero(cols[:nf] == c)[0]
        keep[at[::max(1, at.size // 25)]] = True
    rows, cols = rows[keep], cols[keep]
    assert np.unique(cols).size == npol or npol == 1
    _check(b, env, ids, words, rows, cols)


def test_split_batch_takes_batch_rows(monkeypatch):
    monkeypatch.setenv("KW_SPLIT", "1")
    env = _env("c5_mixed")
    ids = env.policy_ids()
    syn = K.SynthBatch(5, 4000, seed=55)
    b = syn.batch().to_device(0)
    b.validate(env, ids, K.AUDIT)
    words, rw = _words(b)
    rows, cols, nf = items_of(words, rw, extra=100)
    rows, cols = rows[::3], cols[::3]
    got = _check(b, env, ids, words, rows, cols)
    assert set(np.unique(reason_of(got.words)).tolist()) & {1, 3, 4, 5, 6, 7, 8, 9}  # messages that quote a container's name
    monkeypatch.setenv("KW_SPLIT", "0")
    flat = syn.batch().to_device(0)
    flat.validate(env, ids, K.AUDIT)
    assert same(flat.messages(env, ids, rows, cols, words=True), got)


@pytest.mark.parametrize("form", ["validate_batch", "host", "host_packed", "host_summary"])
def test_after_every_kind_of_pass(form):
    env = _env("c4_64")
    ids = env.policy_ids()
    nrows = 5000
    b = K.SynthBatch(4, nrows, seed=4200).batch()
    if form == "validate_batch":
        b.to_device(0).validate(env, ids, K.AUDIT)
    elif form == "host":
        b.validate_host(env, ids, origin=K.AUDIT, chunk_rows=512)
    elif form == "host_packed":
        b.validate_host_packed(env, ids, origin=K.AUDIT, chunk_rows=512)
    else:
        b.validate_host_summary(env, ids, origin=K.AUDIT, chunk_rows=512, planes=False)
    assert b.last_pass() == (nrows, len(ids))
    words, rw = _words(b)
    rows, cols, nf = items_of(words, rw, extra=100)
    rows, cols = rows[::4], cols[::4]
    first = b.messages(env, ids, rows, cols, words=True, cap=300 * rows.size)  # (a cap: one call of the library, not two)
    assert b.debug_messages_stats()["uploaded_names"] == 1  # no pass reads the container names
    got = _check(b, env, ids, words, rows, cols)
    assert b.debug_messages_stats()["uploaded_names"] == 0 and same(first, got)
    key = ("forms", "messages")
    if key in _memo:
        assert same(_memo[key], got)  # every form leaves the same words
    _memo[key] = got


def test_member_messages():
    env, ids, b, words = _c4(300)
    d = b.digest()
    recs = d.recs[::2]
    assert recs.size > 100
    m = b.digest_members(recs)
    got = b.member_messages(env, ids, recs, m, words=True)
    cols = np.repeat(recs["col"].astype(np.uint32), np.diff(m.off.astype(np.int64)))
    ref = b.messages_from_words(env, ids, words, m.rows, cols, how=0, with_words=True)
    assert same(got, ref) and np.array_equal(got.words, m.words) and got.text.size > 30 * m.rows.size


def test_errors_on_the_device():
    env, ids, b, words = _c4(3000)
    npol = len(ids)
    rows, cols, nf = items_of(words, npol, extra=50)
    rows, cols = rows[::5], cols[::5]
    whole = _check(b, env, ids, words, rows, cols)
    nbytes, nhost = whole.text.size, whole.host.size

    def good():
        assert same(b.messages(env, ids, rows, cols, words=True), whole)

    for cap in (nbytes - 1, 0):  # KW_E_NOSPACE: bytes, nhost and all of off exact
        with pytest.raises(K.MessagesNoSpace) as e:
            b.messages(env, ids, rows, cols, cap=cap)
        assert e.value.need == nbytes and e.value.nhost == nhost and np.array_equal(e.value.off, whole.off)
        good()
    assert same(b.messages(env, ids, rows, cols, words=True, cap=nbytes), whole)
    _is_arg_error(lambda: b.messages(env, ids, np.append(rows, 3000), np.append(cols, 0)))  # a row outside the pass
    good()
    _is_arg_error(lambda: b.messages(env, ids, np.append(rows, 0), np.append(cols, npol)))  # a col outside the pass
    good()
    _is_arg_error(lambda: b.messages(env, ids[:7], rows[:10], cols[:10] % 7))  # a policy list of another length
    good()
    b.validate_rows(env, [ids[r % npol] for r in range(3000)])  # a rows-mode pass has a policy per row
    _is_arg_error(lambda: b.messages(env, ids, rows, cols))
    b.validate(env, ids, K.AUDIT)
    good()
    empty = b.messages(env, ids, rows[:0], cols[:0])
    assert empty.text.size == 0 and empty.off.tolist() == [0]


def test_host_items_on_the_device():
    """c6's group of 40 members: reason 13 renders whatever its ARG; the parity workload above holds
    the items left to the host. Here a pass whose host list is not empty and whose host_cap is one
    short answers KW_E_NOSPACE with the exact count."""
    env = K.EvaluationEnvironment(OC.policies(), continue_on_errors=True, always_accept_namespace=NS, device=0)
    ids = env.policy_ids()
    b = K.Batch.from_json(OC.docs(300)).to_device(0)
    b.validate(env, ids, K.VALIDATE)
    words, rw = _words(b)
    rows, cols, nf = items_of(words, rw, extra=0)
    whole = _check(b, env, ids, words, rows, cols)
    assert whole.host.size > 1
    with pytest.raises(K.MessagesNoSpace) as e:
        b.messages(env, ids, rows, cols, host_cap=whole.host.size - 1)
    assert e.value.nhost == whole.host.size and e.value.need == whole.text.size and np.array_equal(e.value.off, whole.off)
    assert same(b.messages(env, ids, rows, cols, words=True), whole)
