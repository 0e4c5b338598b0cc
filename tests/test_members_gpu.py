"""The digest's drill-down on the device (kw_batch_digest_members). Every case starts from poisoned
verdict words and requires the device's result to equal, byte for byte (off, rows, words, n), the
reference host reducer's (kw_debug_digest_members_words) over the words read back from the same pass,
and again on a second call. Row shapes around the wave's unit, column shapes around the 64-column
groups and the narrow-row geometry, selections of one group, of 64, of all, of one column and of one
reason class, tags cut to 4 and to 0 bits (every probe collides), a split batch, every kind of pass
that leaves all-pairs words in the verdict buffer, image keys and group columns, and the argument
and capacity errors, each followed by a correct call on the same batch."""
import numpy as np
import pytest

import kwgpu as K
import members_cases as MC
from helpers import config, many_policies_config
from kwgpu import _native as N

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


def _check(b, recs, words, rw, both_kinds=False):
    """The device's members of `recs` over b's last pass against the host reducer over `words`."""
    got = b.digest_members(recs)
    ref = b.digest_members_from_words(words, rw, recs)
    assert got.rows.size == ref.rows.size > 0
    assert np.array_equal(got.off, ref.off), np.nonzero(got.off != ref.off)[0][:8]
    assert got.rows.tobytes() == ref.rows.tobytes(), np.nonzero(got.rows != ref.rows)[0][:8]
    assert got.words.tobytes() == ref.words.tobytes()
    assert MC.same(b.digest_members(recs), got)  # the same input, the same bytes
    sizes = np.diff(got.off.astype(np.int64))
    if both_kinds:  # not vacuous: a group of two or more members and a singleton
        assert (sizes >= 2).any() and (sizes == 1).any(), (int((sizes >= 2).sum()), int((sizes == 1).sum()))
    return got


def _is_arg_error(call):
    with pytest.raises(K.EvaluationError) as e:
        call()
    assert e.value.code == N.KW_E_ARG


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 3000])
def test_row_shapes(rows):
    env = _env("c4_64")
    ids = env.policy_ids()
    b = K.SynthBatch(4, rows, seed=4100).batch().to_device(0)
    b.validate(env, ids, K.AUDIT)
    words, rw = _words(b)
    d = b.digest_from_words(words, rw)
    assert d.recs.size == {1: 24, 63: 476, 64: 476, 65: 483, 3000: 2403}[rows]
    got = _check(b, d.recs, words, rw, both_kinds=rows >= 63)
    MC.check_properties(got, d.recs, words, rw)
    if rows == 3000:
        assert int((d.recs["count"] >= 64).sum()) == 245 and int(d.recs["count"].max()) == 2031
    # without kw_batch_digest before; after it, the same bytes
    b.digest()
    assert MC.same(b.digest_members(d.recs), got)
    rows_only = b.digest_members(d.recs, words=False)
    assert rows_only.words is None and np.array_equal(rows_only.rows, got.rows) and np.array_equal(rows_only.off, got.off)


@pytest.mark.parametrize("npol", [1, 31, 63, 64, 65, 128])
def test_column_shapes(npol):
    env = _env("c6_256")
    ids = env.policy_ids()[:npol]
    rows = 1500
    if "c6" not in _memo:
        _memo["c6"] = K.SynthBatch(6, rows, seed=6).batch().to_device(0)
    b = _memo["c6"]
    b.validate(env, ids, K.AUDIT)
    assert b.last_pass() == (rows, npol)
    words, rw = _words(b)
    d = b.digest_from_words(words, rw)
    recs = d.recs
    if npol == 1:
        assert recs.size == 1448 and (recs["count"] == 1).all()  # the shape: every group a singleton
    if npol == 128:
        assert recs.size == 92186 and int((recs["count"] >= 2).sum()) == 488
        keep = recs["count"] >= 2
        keep[::7] = True
        recs = recs[keep]
    # (up to 64 columns every group of this input is a singleton; the 65th brings the first larger ones)
    got = _check(b, recs, words, rw, both_kinds=npol >= 65)
    MC.check_properties(got, recs, words, rw)


def _c4_300():
    if "c4_300" not in _memo:
        env = _env("c4_64")
        ids = env.policy_ids()
        b = K.SynthBatch(4, 300, seed=4300).batch().to_device(0)
        b.validate(env, ids, K.AUDIT)
        words, rw = _words(b)
        d = b.digest_from_words(words, rw)
        assert d.recs.size == 831 and int((d.recs["count"] >= 2).sum()) == 548 and int(d.recs["count"].max()) == 205
        _memo["c4_300"] = (env, ids, b, words, rw, d)
    env, ids, b, words, rw, d = _memo["c4_300"]
    if b.last_pass() != (300, len(ids)):
        b.validate(env, ids, K.AUDIT)
    return env, ids, b, words, rw, d


def _sixty_four(d):
    """64 groups of the 300-row pass, both kinds among them, in an order that is not the digest's."""
    many, single = d.recs[d.recs["count"] >= 2], d.recs[d.recs["count"] == 1]
    recs = np.concatenate([single[::9][:24], many[::11][:40]])
    assert recs.size == 64
    return recs


@pytest.mark.parametrize("selection", ["one", "sixty_four", "all", "one_column", "one_class"])
def test_selection_shapes(selection):
    env, ids, b, words, rw, d = _c4_300()
    both = True
    if selection == "one":
        recs, both = d.recs[np.argmax(d.recs["count"]):][:1], False
    elif selection == "sixty_four":
        recs = _sixty_four(d)
    elif selection == "all":
        recs = d.recs
    elif selection == "one_column":
        per_col = np.bincount(d.recs["col"].astype(np.int64))
        recs = d.recs[d.recs["col"] == int(np.argmax(per_col))]
    else:  # one reason class: the class mask rejects most findings before their key bytes
        reasons = (d.recs["word"] >> np.uint32(8)) & np.uint32(0xFF)
        pick = [int(r) for r in np.unique(reasons)
                if ((d.recs["count"] >= 2) & (reasons == r)).any() and ((d.recs["count"] == 1) & (reasons == r)).any()]
        assert pick
        sel = reasons == pick[0]
        assert int(d.recs["count"][sel].sum()) < int(d.recs["count"].sum()) // 2
        recs = d.recs[sel]
    got = _check(b, recs, words, rw, both_kinds=both)
    MC.check_properties(got, recs, words, rw)
    if selection == "one":
        assert got.rows.size == 205


@pytest.mark.parametrize("bits", [4, 0])
def test_colliding_tags(monkeypatch, bits):
    env, ids, b, words, rw, d = _c4_300()
    recs = _sixty_four(d)
    whole = _check(b, recs, words, rw, both_kinds=True)
    monkeypatch.setenv("KW_DIGEST_HASH_BITS", str(bits))
    got = _check(b, recs, words, rw, both_kinds=True)
    assert MC.same(got, whole)
    # records of a digest computed under the lowered bits (its leftover path) select the same members
    low = b.digest()
    assert b.debug_digest_stats()["leftovers"] > 0 and low.recs.tobytes() == d.recs.tobytes()
    assert MC.same(b.digest_members(_sixty_four(low)), whole)


def test_split_batch_reports_batch_rows(monkeypatch):
    monkeypatch.setenv("KW_SPLIT", "1")
    env = _env("c5_mixed")
    ids = env.policy_ids()
    rows = 4000
    syn = K.SynthBatch(5, rows, seed=55)
    b = syn.batch().to_device(0)
    b.validate(env, ids, K.AUDIT)
    words, rw = _words(b)
    d = b.digest_from_words(words, rw)
    assert d.recs.size == 2882 and int((d.recs["count"] >= 2).sum()) == 793
    got = _check(b, d.recs, words, rw, both_kinds=True)
    MC.check_properties(got, d.recs, words, rw)  # batch rows, ascending
    monkeypatch.setenv("KW_SPLIT", "0")
    flat = syn.batch().to_device(0)
    flat.validate(env, ids, K.AUDIT)
    assert MC.same(flat.digest_members(d.recs), got)


@pytest.mark.parametrize("form", ["validate_batch", "host", "host_packed", "host_summary"])
def test_after_every_kind_of_pass(form):
    env = _env("c4_64")
    ids = env.policy_ids()
    rows = 5000
    b = K.SynthBatch(4, rows, seed=4200).batch()
    if form == "validate_batch":
        b.to_device(0).validate(env, ids, K.AUDIT)
    elif form == "host":
        b.validate_host(env, ids, origin=K.AUDIT, chunk_rows=512)
    elif form == "host_packed":
        b.validate_host_packed(env, ids, origin=K.AUDIT, chunk_rows=512)
    else:
        b.validate_host_summary(env, ids, origin=K.AUDIT, chunk_rows=512, planes=False)
    assert b.last_pass() == (rows, len(ids))
    words, rw = _words(b)
    recs = b.digest_from_words(words, rw).recs[::2]
    got = _check(b, recs, words, rw, both_kinds=True)
    key = ("forms", "members")
    if key in _memo:
        assert MC.same(_memo[key], got)  # every form leaves the same words
    _memo[key] = got


@pytest.mark.parametrize("cfg,name", [(2, "c2_trusted"), (3, "c3_group")])
def test_image_keys_and_group_columns(cfg, name):
    env = _env(name)
    ids = env.policy_ids()
    b = K.SynthBatch(cfg, 3000, seed=300 + cfg).batch().to_device(0)
    b.validate(env, ids, K.AUDIT)
    words, rw = _words(b)
    d = b.digest_from_words(words, rw)
    if cfg == 3:  # two large groups beside the singletons
        assert int((d.recs["count"] >= 2).sum()) == 2 and int(d.recs["count"].max()) > 2000
        assert int((d.recs["count"] == 1).sum()) == 6320
    got = _check(b, d.recs, words, rw, both_kinds=cfg == 3)  # (every image group of the c2 input is a singleton)
    MC.check_properties(got, d.recs, words, rw)


def test_errors_on_the_device():
    env = _env("c4_64")
    ids = env.policy_ids()
    rows = 3000
    b = K.SynthBatch(4, rows, seed=4100).batch().to_device(0)
    b.validate(env, ids, K.AUDIT)
    words, rw = _words(b)
    d = b.digest_from_words(words, rw)
    recs = d.recs[::3]
    whole = _check(b, recs, words, rw, both_kinds=True)
    n = whole.rows.size

    def good():
        assert MC.same(b.digest_members(recs), whole)

    # KW_E_NOSPACE: n and all of off exact
    for cap in (n - 1, 0):
        with pytest.raises(K.MembersNoSpace) as e:
            b.digest_members(recs, cap=cap)
        assert e.value.need == n and np.array_equal(e.value.off, whole.off)
        good()
    assert MC.same(b.digest_members(recs, cap=n), whole)
    bare = recs.copy()
    bare["count"] = 0  # records kept without their counts: grown once to the reported need
    assert MC.same(b.digest_members(bare), whole)
    # a duplicate group named by two different members
    g = int(np.argmax(np.diff(whole.off.astype(np.int64))))
    other = recs[g:g + 1].copy()
    other[0]["first_row"], other[0]["word"] = whole.rows[int(whole.off[g + 1]) - 1], whole.words[int(whole.off[g + 1]) - 1]
    assert int(other[0]["first_row"]) != int(recs[g]["first_row"])
    assert MC.same(b.digest_members(other), K.Members(np.array([0, whole.off[g + 1] - whole.off[g]], dtype=np.uint64),
                                                       whole.rows[int(whole.off[g]):int(whole.off[g + 1])],
                                                       whole.words[int(whole.off[g]):int(whole.off[g + 1])]))
    _is_arg_error(lambda: b.digest_members(np.concatenate([recs, other])))
    good()
    # records of an earlier pass. After a pass over ids[:7] the 64-column pass's records of columns 7
    # and up are outside the pass; those of the first seven columns still name groups, for the same
    # policies give the same words there. With the seven in reversed order a column holds another
    # policy, and a record of the 64-column pass whose word differs at its pair is refused.
    b.validate(env, ids[:7], K.AUDIT)
    w7, rw7 = _words(b)
    assert rw7 == 7
    _is_arg_error(lambda: b.digest_members(d.recs[d.recs["col"] >= 7][:3]))
    _check(b, d.recs[d.recs["col"] < 7], w7, 7)
    b.validate(env, ids[6::-1], K.AUDIT)
    w7, rw7 = _words(b)
    w7 = w7.reshape(rows, 7)
    stale = next(r for r in d.recs if int(r["col"]) < 7 and int(w7[int(r["first_row"]), int(r["col"])]) != int(r["word"]))
    d7 = b.digest_from_words(w7, 7)
    _is_arg_error(lambda: b.digest_members(np.concatenate([d7.recs[:5], MC.recs_of([tuple(stale)])])))
    _check(b, d7.recs, w7, 7)
    # a rows-mode pass has a policy per row
    b.validate_rows(env, [ids[r % len(ids)] for r in range(rows)])
    _is_arg_error(lambda: b.digest_members(recs))
    b.validate(env, ids, K.AUDIT)
    good()
    assert b.digest_members(recs[:0]).rows.size == 0  # no group named


def test_a_wide_record_names_no_group():
    env = _env("c6_256")
    ids = env.policy_ids()
    rows = 300
    b = K.SynthBatch(6, rows, seed=66).batch().to_device(0)
    b.validate(env, ids, K.AUDIT)
    words, rw = _words(b)
    d = b.digest_from_words(words, rw)
    assert d.wide.size > 0
    pair = int(d.wide[0])
    wide = MC.recs_of([(pair % rw, int(words[pair]), pair // rw, 1)])
    recs = d.recs[::50]
    _is_arg_error(lambda: b.digest_members(np.concatenate([recs, wide])))
    _check(b, recs, words, rw)
