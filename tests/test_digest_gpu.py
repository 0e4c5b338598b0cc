"""The violation digest on the device (kw_batch_digest). Every case starts from poisoned verdict
words and requires the device's digest to equal the reference host reducer's (kw_debug_digest_words)
over the words read back from the same pass: records, wide list and findings, exactly, and the same
bytes on a second call. Row shapes around the wave's unit, column shapes around the 64-column groups
and the narrow-row geometry, a split batch, every kind of pass that leaves all-pairs words in the
verdict buffer, image keys and group cause masks, wide findings, entity indices past 255, a pass
without findings, a hash cut to 4 and to 0 bits (every probe collides: the leftover path carries the
result), a table budget that forces column ranges, the capacity and argument errors."""
import numpy as np
import pytest

import digest_cases as DC
import kwgpu as K
from helpers import config, many_policies_config, wide_entity_case
from kwgpu import _native as N

pytestmark = pytest.mark.gpu
NS = "kubewarden"
POISON = 0xA5A5A5A5
LABELS = "registry://ghcr.io/kubewarden/policies/safe-labels:v0.1.14"
_memo = {}


@pytest.fixture(autouse=True)
def _poisoned_verdicts(monkeypatch):
    monkeypatch.setenv("KW_POISON_VERDICTS", "1")


def _env(name):
    if name not in _memo:
        doc = many_policies_config() if name == "c6_256" else config(name)
        _memo[name] = K.EvaluationEnvironment(doc, continue_on_errors=True, always_accept_namespace=NS, device=0)
    return _memo[name]


def _check(b):
    """The device's digest of b's last pass against the host reducer over the words read back."""
    rows, rw = b.last_pass()
    got = b.digest()
    words = b.verdicts(rows * rw)
    assert not (words == POISON).any(), "words the pass never wrote"
    ref = b.digest_from_words(words, rw)
    assert got.findings == ref.findings == int(np.count_nonzero((words >> np.uint32(8)) & np.uint32(0xFF)))
    assert got.recs.size == ref.recs.size, (got.recs.size, ref.recs.size, b.debug_digest_stats())
    assert got.recs.tobytes() == ref.recs.tobytes(), np.nonzero(got.recs != ref.recs)[0][:8]
    assert np.array_equal(got.wide, ref.wide)
    assert int(got.recs["count"].sum()) + got.wide.size == got.findings
    assert DC.same(b.digest(), got)  # the same input, the same bytes
    return got, words


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 3000])
def test_row_shapes(rows):
    env = _env("c4_64")
    ids = env.policy_ids()
    b = K.SynthBatch(4, rows, seed=4100).batch().to_device(0)
    b.validate(env, ids, K.AUDIT)
    got, _ = _check(b)
    assert got.findings > 0 and b.debug_digest_stats()["ranges"] == 1


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
    _check(b)


def test_split_batch_reports_batch_rows(monkeypatch):
    monkeypatch.setenv("KW_SPLIT", "1")
    env = _env("c5_mixed")
    ids = env.policy_ids()
    rows = 4000
    syn = K.SynthBatch(5, rows, seed=55)
    reordered, perm, split = syn.batch().debug_reorder()
    assert 0 < split < rows and not np.array_equal(perm, np.arange(rows, dtype=np.uint64))  # the rows do move
    b = syn.batch().to_device(0)
    b.validate(env, ids, K.AUDIT)
    got, words = _check(b)
    # against the digest in device rows, which is what a missing row map would report
    dev_words = words.reshape(rows, -1)[perm.astype(np.int64)]
    wrong = reordered.digest_from_words(dev_words, len(ids))
    assert wrong.recs.size == got.recs.size and int(wrong.recs["count"].sum()) == int(got.recs["count"].sum())
    assert sorted(wrong.recs["first_row"].tolist()) != sorted(got.recs["first_row"].tolist())
    monkeypatch.setenv("KW_SPLIT", "0")
    flat = syn.batch().to_device(0)
    flat.validate(env, ids, K.AUDIT)
    assert DC.same(flat.digest(), got)


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
    got, _ = _check(b)
    key = ("forms", "digest")
    if key in _memo:
        assert DC.same(_memo[key], got)  # every form leaves the same words
    _memo[key] = got


@pytest.mark.parametrize("cfg,name", [(2, "c2_trusted"), (3, "c3_group")])
def test_image_keys_and_group_cause_masks(cfg, name):
    env = _env(name)
    ids = env.policy_ids()
    b = K.SynthBatch(cfg, 3000, seed=300 + cfg).batch().to_device(0)
    b.validate(env, ids, K.AUDIT)
    got, _ = _check(b)
    reasons = {(int(w) >> 8) & 0xFF for w in got.recs["word"]}
    assert reasons & {3, 4, 5, 6, 7}
    if cfg == 3:
        assert 13 in reasons


def test_wide_group_rejections_are_listed():
    env = _env("c6_256")
    ids = env.policy_ids()
    rows = 300
    b = K.SynthBatch(6, rows, seed=66).batch().to_device(0)
    b.validate(env, ids, K.AUDIT)
    got, words = _check(b)
    assert got.wide.size > 0
    w = words[got.wide.astype(np.int64)]
    assert (((w >> np.uint32(8)) & np.uint32(0xFF)) == 13).all() and ((w >> np.uint32(16)) == N.KW_ARG_WIDE).all()
    assert got.wide.tolist() == sorted(got.wide.tolist())


def test_entity_indices_past_255():
    doc, pols = wide_entity_case()
    env = K.EvaluationEnvironment(pols, continue_on_errors=True, device=0)
    ids = env.policy_ids()
    b = K.Batch.from_json([doc] * 3).to_device(0)
    b.validate(env, ids)
    got, _ = _check(b)
    assert got.recs.size == 4 and (got.recs["count"] == 3).all() and (got.recs["first_row"] == 0).all()
    keys = {b.finding_key(0, int(r["word"])) for r in got.recs}
    assert keys == {(b"NET_ADMIN", None), (b"k299", b"bad"), (b"k280", None), (b"localhost/evil", None)}
    assert all((int(r["word"]) >> 16) > 255 for r in got.recs)


def test_a_pass_without_findings():
    env = K.EvaluationEnvironment({"none": {"module": LABELS, "settings": {"denied_labels": ["no-request-has-this-label"]}}},
                                  continue_on_errors=True, device=0)
    b = K.SynthBatch(4, 700, seed=9).batch().to_device(0)
    b.validate(env, env.policy_ids())
    got, _ = _check(b)
    assert got.recs.size == 0 and got.wide.size == 0 and got.findings == 0


@pytest.mark.parametrize("bits", [4, 0])
def test_colliding_hashes_take_the_leftover_path(monkeypatch, bits):
    env = _env("c4_64")
    ids = env.policy_ids()
    b = K.SynthBatch(4, 300, seed=4300).batch().to_device(0)
    b.validate(env, ids, K.AUDIT)
    whole, _ = _check(b)
    assert b.debug_digest_stats()["leftovers"] == 0 and whole.recs.size > 100
    monkeypatch.setenv("KW_DIGEST_HASH_BITS", str(bits))
    got, _ = _check(b)
    stats = b.debug_digest_stats()
    # at most 2^bits tags: all other groups reach the result through the leftover list
    assert stats["leftovers"] >= whole.recs.size - (1 << bits) * stats["ranges"] > 0, stats
    assert DC.same(got, whole)


def test_table_budget_forces_column_ranges(monkeypatch):
    env = _env("c6_256")
    ids = env.policy_ids()[:128]
    b = K.SynthBatch(6, 1500, seed=6).batch().to_device(0)
    b.validate(env, ids, K.AUDIT)
    whole, _ = _check(b)
    assert b.debug_digest_stats()["ranges"] == 1
    per_col = np.bincount(whole.recs["col"].astype(np.int64), minlength=128)
    slots = 64  # digest.hpp kDigestMinSlots; a table takes slots / 2 groups
    while slots // 2 < 2 * int(per_col.max()):
        slots *= 2
    assert whole.recs.size > 3 * (slots // 2), (whole.recs.size, slots)  # so no two ranges can hold the pass
    monkeypatch.setenv("KW_DIGEST_TABLE", str(slots * 24))
    got, _ = _check(b)
    stats = b.debug_digest_stats()
    assert stats["ranges"] >= 3 and stats["cuts"] >= 2 and stats["slots"] == slots, stats
    assert DC.same(got, whole)


def test_nospace_and_argument_errors(monkeypatch):
    env = _env("c4_64")
    ids = env.policy_ids()
    rows = 3000
    b = K.SynthBatch(4, rows, seed=4100).batch().to_device(0)

    def is_arg_error(call):
        with pytest.raises(K.EvaluationError) as e:
            call()
        assert e.value.code == N.KW_E_ARG

    is_arg_error(b.digest)  # a batch without a pass
    b.validate(env, ids, K.AUDIT)
    whole, _ = _check(b)
    with pytest.raises(K.DigestNoSpace) as e:  # one record too few: the exact need
        b.digest(cap=whole.recs.size - 1, wide_cap=8)
    assert (e.value.need, e.value.need_wide) == (whole.recs.size, whole.wide.size)
    assert DC.same(b.digest(cap=whole.recs.size, wide_cap=whole.wide.size), whole)
    # a single column with more groups than the smallest table takes: KW_E_NOSPACE with n = 0
    per_col = np.bincount(whole.recs["col"].astype(np.int64))
    assert per_col.max() > 32
    monkeypatch.setenv("KW_DIGEST_TABLE", "1")
    with pytest.raises(K.DigestNoSpace) as e:
        b.digest()
    assert (e.value.need, e.value.need_wide) == (0, 0)
    monkeypatch.delenv("KW_DIGEST_TABLE")
    assert DC.same(b.digest(), whole)  # the batch is still good
    b.validate_rows(env, [ids[r % len(ids)] for r in range(rows)])
    is_arg_error(b.digest)  # a rows-mode pass has a policy per row
    b.validate(env, ids[:7], K.AUDIT)
    got, _ = _check(b)  # and a later all-pairs pass is digested again
    assert got.recs["col"].max() < 7
