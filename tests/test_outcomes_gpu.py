"""The grouped outcome count on the device (kw_batch_outcomes) and the metrics of a pass
(kw_metrics_record_pass). Every case starts from poisoned verdict words and requires the device's
table to equal the reference host reducer's (kw_debug_outcome_words) over the words read back from
the same pass: exactly, every counter. Row shapes around the unit size R, column shapes around the
64-column groups and the narrow-row geometry, a split batch, every kind of pass that leaves words in
the verdict buffer, a table budget that forces several group ranges, a second pass, the cross-checks
against kw_batch_summary, the rendered metrics against per-pair recording, the argument errors."""
import numpy as np
import pytest

import kwgpu as K
import outcomes_cases as OC
from helpers import config, many_policies_config
from kwgpu import _native as N

pytestmark = pytest.mark.gpu
NS = "kubewarden"
R = 256  # outcomes.hpp kOutUnitRows
POISON = 0xA5A5A5A5
_memo = {}


@pytest.fixture(autouse=True)
def _poisoned_verdicts(monkeypatch):
    monkeypatch.setenv("KW_POISON_VERDICTS", "1")


def _env(name):
    if name not in _memo:
        doc = OC.policies() if name == "outcomes" else many_policies_config() if name == "c6_256" else config(name)
        _memo[name] = K.EvaluationEnvironment(doc, continue_on_errors=True, always_accept_namespace=NS, device=0)
    return _memo[name]


def _check(b, row_group=None, ngroups=None):
    """The device's table of b's last pass against the host reducer over the words read back."""
    rows, rw = b.last_pass()
    got = b.outcomes(row_group, ngroups)
    words = b.verdicts(rows * rw)
    assert not (words == POISON).any(), "words the pass never wrote"
    ref = K.Batch.outcomes_from_words(words, rw, row_group, ngroups)
    assert got.shape == ref.shape
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:8]
    assert int(got.sum()) == rows * rw
    return got, words


def _sized_groups(rows, sizes, seed):
    """Group ids in an order unrelated to the rows: group k has sizes[k] rows, the last group the rest."""
    assert sum(sizes) < rows
    ids = np.concatenate([np.full(n, k, dtype=np.uint32) for k, n in enumerate(sizes)] +
                         [np.full(rows - sum(sizes), len(sizes), dtype=np.uint32)])
    return np.random.default_rng(seed).permutation(ids), len(sizes) + 1


def test_row_shapes_around_the_unit_size():
    env = _env("c4_64")
    ids = env.policy_ids()
    rows = 3000
    b = K.SynthBatch(4, rows, seed=4100).batch().to_device(0)
    b.validate(env, ids)
    rg, ng = _sized_groups(rows, [1, R - 1, R, R + 1, 2 * R + 1], 1)
    got, _ = _check(b, rg, ng)
    assert got.sum(axis=(1, 2)).tolist() == [n * len(ids) for n in (1, R - 1, R, R + 1, 2 * R + 1, rows - 5 * R - 2)]
    one, _ = _check(b)                                             # all rows in one group (NULL)
    again, _ = _check(b, np.zeros(rows, dtype=np.uint32), 1)        # and as ids
    assert np.array_equal(one, again) and np.array_equal(one[0], got.sum(axis=0))
    _check(b, np.random.default_rng(2).permutation(rows).astype(np.uint32), rows)  # every row its own group
    _check(b, np.random.default_rng(3).integers(0, 40, rows).astype(np.uint32) * 3, 130)  # empty groups between and after
    assert np.array_equal(b.outcomes(rg, ng), got)  # the same input, the same bytes


@pytest.mark.parametrize("npol", [1, 31, 33, 63, 64, 65, 128])
def test_column_shapes(npol):
    env = _env("c6_256")
    ids = env.policy_ids()[:npol]
    rows = 1500
    if "c6" not in _memo:
        _memo["c6"] = K.SynthBatch(6, rows, seed=6).batch().to_device(0)
    b = _memo["c6"]
    b.validate(env, ids)
    assert b.last_pass() == (rows, npol)
    rg, ng = _sized_groups(rows, [1, R - 1, R, R + 1, 7, 64 // max(1, min(npol, 32)) + 1], npol)
    _check(b, rg, ng)
    _check(b)


def test_split_batch_takes_ids_in_batch_order(monkeypatch):
    monkeypatch.setenv("KW_SPLIT", "1")
    env = _env("c5_mixed")
    ids = env.policy_ids()
    rows = 4000
    syn = K.SynthBatch(5, rows, seed=55)
    _, perm, split = syn.batch().debug_reorder()
    assert 0 < split < rows and not np.array_equal(perm, np.arange(rows, dtype=np.uint64))  # the rows do move
    b = syn.batch().to_device(0)
    b.validate(env, ids)
    rg = (np.arange(rows) // 300).astype(np.uint32)  # runs of batch rows: light and heavy rows in every group
    got, words = _check(b, rg, 14)
    # against the same ids taken as device rows, which is what a missing row map would count
    wrong = K.Batch.outcomes_from_words(words.reshape(rows, -1)[perm.astype(np.int64)], len(ids), rg, 14)
    assert not np.array_equal(got, wrong)
    monkeypatch.setenv("KW_SPLIT", "0")
    flat = syn.batch().to_device(0)
    flat.validate(env, ids)
    assert np.array_equal(flat.outcomes(rg, 14), got)


@pytest.mark.parametrize("form", ["validate_batch", "host", "host_packed", "host_summary", "validate_rows"])
def test_after_every_kind_of_pass(form):
    env = _env("c4_64")
    ids = env.policy_ids()
    rows = 5000
    syn = K.SynthBatch(4, rows, seed=4200)
    b = syn.batch()
    rg, first = b.attribute_groups()
    assert first.size > 1
    if form == "validate_batch":
        b.to_device(0).validate(env, ids, K.AUDIT)
    elif form == "host":
        b.validate_host(env, ids, chunk_rows=512)
    elif form == "host_packed":
        b.validate_host_packed(env, ids, chunk_rows=512)
    elif form == "host_summary":
        b.validate_host_summary(env, ids, chunk_rows=512, planes=False)
    else:
        b.to_device(0).validate_rows(env, [ids[r % len(ids)] for r in range(rows)])
    assert b.last_pass() == (rows, 1 if form == "validate_rows" else len(ids))
    _check(b, rg, first.size)


def test_table_budget_forces_ranges(monkeypatch):
    env = _env("c4_64")
    ids = env.policy_ids()
    rows = 3000
    b = K.SynthBatch(4, rows, seed=4100).batch().to_device(0)
    b.validate(env, ids)
    rg, ng = _sized_groups(rows, [1, R + 1, 3, R, 40, 40, 40, 40, 40, 2 * R + 1], 9)
    whole, _ = _check(b, rg, ng)
    per_group = N.KW_OUT_N * len(ids) * 8
    for groups_per_range in (4, 3, 1):  # 3, 4 and 11 ranges of the 11 groups, the last one partial
        monkeypatch.setenv("KW_OUTCOME_TABLE", str(groups_per_range * per_group + 8))
        assert -(-ng // groups_per_range) >= 3
        got, _ = _check(b, rg, ng)
        assert np.array_equal(got, whole)
    monkeypatch.setenv("KW_OUTCOME_TABLE", "1")  # below one group's counters: a group a range
    assert np.array_equal(b.outcomes(rg, ng), whole)


def test_second_pass_counts_do_not_carry_over():
    env = _env("c4_64")
    ids = env.policy_ids()
    rows = 3000
    b = K.SynthBatch(4, rows, seed=4100).batch().to_device(0)
    rg, first = b.attribute_groups()
    b.validate(env, ids)
    a, _ = _check(b, rg, first.size)
    b.validate(env, ids[5:28], K.AUDIT)
    c, _ = _check(b, rg, first.size)
    assert c.shape[2] == 23 and int(c.sum()) == rows * 23
    assert np.array_equal(b.outcomes(rg, first.size), c)  # nor from one call to the next


@pytest.mark.parametrize("origin", [K.VALIDATE, K.AUDIT])
def test_summary_cross_checks_and_record_pass(origin):
    """The fixture of tests/test_outcomes.py on the device: the table against the summary of the same
    pass, and the metrics after record_pass byte-equal to kw_metrics_record over all pairs of the
    read-back words, accumulating over two calls."""
    env = _env("outcomes")
    ids = env.policy_ids()
    if "adm" not in _memo:
        _memo["adm"] = K.Batch.from_json(OC.docs(1500)).to_device(0)
    b = _memo["adm"]
    rows = b.n
    b.validate(env, ids, origin)
    rg, first = b.attribute_groups()
    assert first.size >= 50
    got, words = _check(b, rg, first.size)
    for code in (0, 1, 3, 4, 8):
        assert got[:, code, :].any(), code
    s = b.summary(planes=False)
    assert (got.sum(axis=(0, 1)) == rows).all()
    assert np.array_equal(got[:, N.KW_OUT_INIT_ERROR, :].sum(axis=0), s.col[:, N.KW_SUM_FST_INIT_ERROR])
    assert s.col[:, N.KW_SUM_FST_INIT_ERROR].any()
    dev, pairs = K.Metrics(), K.Metrics()
    for latency in (7, 20000):
        dev.record_pass(env, b, ids, latency, origin)
        OC.record_all_pairs(pairs, env, b, ids, words, latency, origin)
        assert dev.render() == pairs.render()
    assert np.array_equal(b.verdicts(), words)  # the words are untouched


def test_argument_errors():
    env = _env("c4_64")
    ids = env.policy_ids()
    rows = 600
    b = K.SynthBatch(4, rows, seed=1).batch().to_device(0)

    def is_arg_error(call):
        with pytest.raises(K.EvaluationError) as e:
            call()
        assert e.value.code == N.KW_E_ARG

    m = K.Metrics()
    is_arg_error(lambda: b.outcomes(ngroups=1))  # a batch with no pass
    is_arg_error(lambda: m.record_pass(env, b, ids))
    b.validate(env, ids)
    rg = np.zeros(rows, dtype=np.uint32)
    rg[rows // 2] = 3
    is_arg_error(lambda: b.outcomes(rg, 3))  # an id >= ngroups
    is_arg_error(lambda: b.outcomes(rg, 0))
    is_arg_error(lambda: m.record_pass(env, b, ids[:-1]))  # npol differs from the pass's words per row
    assert b.outcomes(rg, 4)[3].sum() == len(ids)  # the batch is still good
    m.record_pass(env, b, ids)
    total = sum(int(line.rsplit(" ", 1)[1]) for line in m.render().splitlines()
                if line.startswith("kubewarden_policy_evaluations_total{"))
    assert total == rows * len(ids)
    b.validate_rows(env, [ids[0]] * rows)
    is_arg_error(lambda: m.record_pass(env, b, ids[:1]))  # a rows-mode pass has a policy per row
    assert b.outcomes().sum() == rows  # while the count itself takes it as one column
