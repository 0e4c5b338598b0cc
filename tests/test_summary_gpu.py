"""The summary form on the device (kw_batch_summary, kw_validate_host_summary) and the row fetch
(kw_batch_verdict_rows). Every case compares the counters and the planes with numpy over the oracle's
words (tests/test_summary.py numpy_summary) and with the reference host reducer
(Summary.from_words), byte for byte. Chunked bulk passes (the totals crossing chunks, one column with
64 rows a wave round, partial and several column groups, a row count off every workgroup's span),
the unchunked forms, pageable and page-locked planes, counters only, the resident path in both
origins, a split batch, a rows-mode pass, the audit flow's row fetch and the argument errors. The
verdict buffer is poisoned before every pass: a pair that was never evaluated lands in
KW_SUM_REASON_OTHER, which every case asserts to be empty."""
import numpy as np
import pytest

import kwgpu as K
import oracle as O
from helpers import config, diff_verdicts, many_policies_config
from kwgpu import _native as N
from test_summary import check_invariants, numpy_summary

pytestmark = pytest.mark.gpu
NS = "kubewarden"
_memo = {}


@pytest.fixture(autouse=True)
def _poisoned_verdicts(monkeypatch):
    monkeypatch.setenv("KW_POISON_VERDICTS", "1")


def _envs(name):
    if name not in _memo:
        doc = many_policies_config() if name == "c6_256" else config(name)
        _memo[name] = (K.EvaluationEnvironment(doc, continue_on_errors=True, always_accept_namespace=NS, device=0),
                       O.OracleEnv(doc, continue_on_errors=True, always_accept_namespace=NS))
    return _memo[name]


def _oracle(name, scfg, rows, seed, ids, origin=K.VALIDATE):
    """(synthetic batch, the oracle's words, their numpy summary, the host reducer's), computed once."""
    key = (name, scfg, rows, seed, len(ids), origin)
    if key not in _memo:
        _, oe = _envs(name)
        syn = K.SynthBatch(scfg, rows, seed=seed)
        ora = oe.eval(syn.soa(), ids, origin)
        col, planes = numpy_summary(ora, len(ids))
        assert (col[:, N.KW_SUM_REASON_OTHER] == 0).all()  # the oracle's words are product words
        ref = K.Summary.from_words(ora, len(ids))
        assert np.array_equal(ref.col, col) and np.array_equal(ref.planes, planes)
        _memo[key] = (syn, ora, ref)
    return _memo[key]


def _same(got, ref, planes=True):
    assert (got.col[:, N.KW_SUM_REASON_OTHER] == 0).all(), "words the pass never wrote"
    assert np.array_equal(got.col, ref.col), np.argwhere(got.col != ref.col)[:8]
    if planes:
        assert np.array_equal(got.planes, ref.planes), np.argwhere(got.planes != ref.planes)[:8]
        check_invariants(got.col, got.planes, ref.rows, ref.npol)
    else:
        assert got.planes is None


def _all_outputs(name, scfg, rows, seed, ids, chunk, origin=K.VALIDATE):
    """Pageable planes, page-locked planes (prefilled), counters only."""
    env, _ = _envs(name)
    syn, ora, ref = _oracle(name, scfg, rows, seed, ids, origin)
    _same(syn.batch().validate_host_summary(env, ids, origin=origin, chunk_rows=chunk), ref)
    pin = K.Summary(rows, len(ids), pinned=True)
    pin.planes.fill(0xA5A5A5A5A5A5A5A5)
    pin.col.fill(0xA5A5A5A5A5A5A5A5)
    assert syn.batch().validate_host_summary(env, ids, out=pin, origin=origin, chunk_rows=chunk) is pin
    _same(pin, ref)
    _same(syn.batch().validate_host_summary(env, ids, origin=origin, chunk_rows=chunk, planes=False), ref, planes=False)


@pytest.mark.parametrize("name,scfg,rows,chunk", [
    ("c4_64", 4, 30000, 2048),      # 15 chunks: the totals cross chunks
    ("c4_64", 4, 30000, 0),         # the default chunk size: one chunk
    ("c4_64", 4, 30011, 2048),      # rows off every wave's and workgroup's span
    ("c2_trusted", 2, 50000, 777),  # one column: 64 rows per wave round
    ("c3_group", 3, 20000, 4096),   # 4 columns: 16 rows per wave round
    ("parity", 0, 20000, 1500),
])
def test_summary_chunked_matches_oracle_and_host_reducer(name, scfg, rows, chunk):
    env, _ = _envs(name)
    _all_outputs(name, scfg, rows, 4400 + scfg, env.policy_ids(), chunk)


def _c6_without_wide_groups(env):
    ids = env.policy_ids()
    return [p for j, p in enumerate(ids) if not (env.is_group(j) and len(env.group_members(j)) > 15)]


@pytest.mark.parametrize("ncol", [63, 65, 128])
def test_summary_column_groups(ncol):
    """C6 prefixes without the 40-member group, so the pass stays chunked: a partial last group,
    one column past a group, two full groups."""
    env, _ = _envs("c6_256")
    ids = _c6_without_wide_groups(env)[:ncol]
    assert len(ids) == ncol
    _all_outputs("c6_256", 6, 3000, 6, ids, 512)


def test_summary_unchunked_forms():
    """C6 whole (five column groups, the 40-member group's side data: unchunked, summarised in row
    slabs after the pass); C5's requests beyond the tile capacities on the overflow kernels inside
    chunks."""
    env, _ = _envs("c6_256")
    ids = env.policy_ids()
    assert (len(ids) + 63) // 64 == 5
    _all_outputs("c6_256", 6, 3000, 6, ids, 512)
    env5, _ = _envs("c5_mixed")
    _all_outputs("c5_mixed", 5, 4000, 55, env5.policy_ids(), 256)


def test_summary_overflow_tiles(monkeypatch):
    monkeypatch.setenv("KW_TILE_QUANTILE", "0.05")
    env, _ = _envs("c4_64")
    _all_outputs("c4_64", 4, 6000, 4804, env.policy_ids(), 640)


@pytest.mark.parametrize("origin", [K.VALIDATE, K.AUDIT])
def test_resident_summary(origin):
    """validate() then summary(): planes, counters only, a reused page-locked Summary."""
    env, _ = _envs("c4_64")
    ids = env.policy_ids()
    syn, ora, ref = _oracle("c4_64", 4, 9000, 77, ids, origin)
    b = syn.batch().to_device(0)
    b.validate(env, ids, origin)
    _same(b.summary(), ref)
    _same(b.summary(planes=False), ref, planes=False)
    pin = K.Summary(9000, len(ids), pinned=True)
    pin.planes.fill(0xA5A5A5A5A5A5A5A5)
    assert b.summary(out=pin) is pin
    _same(pin, ref)
    assert np.array_equal(b.verdicts(), ora), diff_verdicts(b.verdicts(), ora, len(ids), ids)  # the words are untouched


def test_second_pass_totals_do_not_carry_over():
    env, _ = _envs("c4_64")
    ids = env.policy_ids()
    syn, _, ref = _oracle("c4_64", 4, 9000, 77, ids)
    _, _, ref2 = _oracle("c4_64", 4, 9000, 77, ids[5:28])
    b = syn.batch().to_device(0)
    b.validate(env, ids)
    _same(b.summary(), ref)
    b.validate(env, ids[5:28])
    _same(b.summary(), ref2)
    _same(b.summary(), ref2)  # nor from one summary to the next
    hb = syn.batch()  # the bulk pass likewise
    _same(hb.validate_host_summary(env, ids, chunk_rows=2048), ref)
    _same(hb.validate_host_summary(env, ids[5:28], chunk_rows=2048), ref2)


def test_split_batch_planes_in_batch_order(monkeypatch):
    monkeypatch.setenv("KW_SPLIT", "1")
    env, _ = _envs("c5_mixed")
    ids = env.policy_ids()
    syn, ora, ref = _oracle("c5_mixed", 5, 4000, 55, ids)
    b = syn.batch().to_device(0)
    _, perm, split = syn.batch().debug_reorder()
    assert 0 < split < 4000 and not np.array_equal(perm, np.arange(4000, dtype=np.uint64))  # the rows do move
    b.validate(env, ids)
    _same(b.summary(), ref)
    s = b.summary()
    _same(s, ref)
    pick = _audit_rows(s, 200, 11)
    heavy = perm[split:].astype(np.int64)  # rows the split moved behind the light ones
    assert np.isin(pick.astype(np.int64), heavy).any() and not np.isin(pick.astype(np.int64), heavy).all()
    got = b.verdict_rows(pick)
    assert np.array_equal(got, ora.reshape(4000, -1)[pick.astype(np.int64)])
    # the fetched words with the side data verdict_rows loaded (scattered back to batch rows) format
    # the responses a full read-back of an unsplit batch formats
    monkeypatch.setenv("KW_SPLIT", "0")
    bf = syn.batch().to_device(0)
    bf.validate(env, ids)
    v = bf.verdicts().reshape(4000, len(ids))
    _compare_responses(env, ids, syn, b, got, pick[:40], bf, v)


def _compare_responses(env, ids, syn, b, got, pick, bf, v):
    """Responses (group members and causes included) of rows `pick` from the fetched words got[i] on
    batch b against those from the full words v[row] on batch bf."""
    groups = {j: env.group_members(j) for j in range(len(ids)) if env.is_group(j)}
    for i, r in enumerate(int(x) for x in pick):
        doc = syn.json(r)
        for j in range(len(ids)):
            mv_g = [int(got[i, m]) for m in groups[j]] if j in groups else None
            mv_f = [int(v[r, m]) for m in groups[j]] if j in groups else None
            assert (b.format_response(env, r, j, int(got[i, j]), mv_g, doc=doc) ==
                    bf.format_response(env, r, j, int(v[r, j]), mv_f, doc=doc))
            assert b.wide_arg(r, j) == bf.wide_arg(r, j)
            if j in groups and (int(got[i, j]) >> 8) & 0xFF == O.R_GROUP:
                assert b.group_causes(r, j, int(got[i, j])) == bf.group_causes(r, j, int(v[r, j]))


def test_rows_mode_pass_is_one_column():
    env, oe = _envs("parity")
    ids = env.policy_ids()
    n = 3000
    syn = K.SynthBatch(0, n, seed=31)
    row_policy = [ids[r % len(ids)] for r in range(n)]
    ora = oe.eval(syn.soa(), ids).reshape(n, len(ids))[np.arange(n), np.arange(n) % len(ids)]
    col, planes = numpy_summary(ora, 1)
    assert (col[:, N.KW_SUM_REASON_OTHER] == 0).all()
    b = syn.batch().to_device(0)
    b.validate_rows(env, row_policy)
    got = b.summary()
    assert got.npol == 1 and np.array_equal(got.col, col) and np.array_equal(got.planes, planes)
    assert np.array_equal(got.col, K.Summary.from_words(ora, 1).col)
    assert np.array_equal(b.verdict_rows([5, 2999, 0])[:, 0], ora[[5, 2999, 0]])


def _audit_rows(summary, n, seed):
    """n rows for the audit flow: drawn from plane 1, some clean rows, shuffled, one repeated."""
    rng = np.random.default_rng(seed)
    hit = summary.flagged_rows(1)
    clean = np.setdiff1d(np.arange(summary.rows), hit)
    assert hit.size >= n - 20 and clean.size >= 20
    pick = np.concatenate([rng.choice(hit, n - 21, replace=False), rng.choice(clean, 20, replace=False)])
    rng.shuffle(pick)
    return np.append(pick, pick[3]).astype(np.uint64)


@pytest.mark.parametrize("name,scfg", [("c3_group", 3), ("c4_64", 4)])
def test_verdict_rows_after_bulk_summary_format_the_same_responses(name, scfg):
    """The audit flow without any full read-back: validate_host_summary, 200 rows from plane 1 and
    some clean ones, their words, messages. The words equal the oracle's rows; the responses (group
    members and causes included) equal those formatted from verdicts() of a second batch."""
    env, _ = _envs(name)
    ids = env.policy_ids()
    rows = 6000
    syn, ora, ref = _oracle(name, scfg, rows, 8800 + scfg, ids)
    ora2 = ora.reshape(rows, len(ids))
    b = syn.batch()
    s = b.validate_host_summary(env, ids, chunk_rows=1024)
    _same(s, ref)
    pick = _audit_rows(s, 200, 5)
    got = b.verdict_rows(pick)
    assert np.array_equal(got, ora2[pick.astype(np.int64)])
    bf = syn.batch().to_device(0)
    bf.validate(env, ids)
    v = bf.verdicts().reshape(rows, len(ids))
    _compare_responses(env, ids, syn, b, got, pick[:60], bf, v)


def test_verdict_rows_on_a_resident_pass():
    env, _ = _envs("c4_64")
    ids = env.policy_ids()
    syn, ora, ref = _oracle("c4_64", 4, 9000, 77, ids)
    b = syn.batch().to_device(0)
    b.validate(env, ids)
    pick = _audit_rows(b.summary(), 200, 9)
    assert np.array_equal(b.verdict_rows(pick), ora.reshape(9000, -1)[pick.astype(np.int64)])
    assert b.verdict_rows([]).shape == (0, len(ids))  # n = 0 is KW_OK


def test_verdict_rows_after_a_packed_pass_that_reported_nospace():
    """kw_validate_host_packed runs to its end when the exceptions do not fit, so the batch's last pass
    is that one although the call raised: verdict_rows sizes its output by the library's record of the
    pass (kw_batch_last_pass), on a fresh batch and after a pass of another width."""
    env, _ = _envs("c4_64")
    ids = env.policy_ids()
    syn, ora, _ = _oracle("c4_64", 4, 9000, 77, ids)
    ora2 = ora.reshape(9000, len(ids))
    pick = np.array([8999, 0, 4321, 0], dtype=np.uint64)
    for before in (None, ids[:3]):
        b = syn.batch()
        if before:
            assert b.validate_host(env, before).size == 9000 * 3 and b.last_pass() == (9000, 3)
        with pytest.raises(K.NoSpace):
            b.validate_host_packed(env, ids, out=K.PackedVerdicts(9000, len(ids), exc_cap=16), chunk_rows=2048)
        assert b.last_pass() == (9000, len(ids))
        got = b.verdict_rows(pick)
        assert got.shape == (4, len(ids)) and np.array_equal(got, ora2[pick.astype(np.int64)])
        assert np.array_equal(b.verdicts(), ora)


_DIRECT_OFF = """
import sys
import numpy as np
sys.path[:0] = [{pkg!r}, {tests!r}]
import kwgpu as K
from helpers import config
env = K.EvaluationEnvironment(config("c3_group"), continue_on_errors=True, always_accept_namespace="kubewarden", device=0)
ids = env.policy_ids()
syn = K.SynthBatch(3, 5000, seed=12)
ref = K.Summary.from_words(syn.batch().validate_host(env, ids, chunk_rows=512), len(ids))
for chunk, pinned in ((512, False), (512, True), (0, True)):
    count = syn.batch().validate_host_summary(env, ids, chunk_rows=chunk, planes=False)
    assert count.planes is None and np.array_equal(count.col, ref.col)
    full = syn.batch().validate_host_summary(env, ids, out=K.Summary(5000, len(ids), pinned=pinned), chunk_rows=chunk)
    assert np.array_equal(full.col, ref.col) and np.array_equal(full.planes, ref.planes)
print("direct off ok")
"""


def test_counters_only_with_direct_read_back_off():
    """KW_BULK_DIRECT=0 (an A/B setting read once per process, hence the child process) sends every
    read-back through the bounce blocks; a counters-only summary has nothing to copy out of them."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = _DIRECT_OFF.format(pkg=os.path.join(root, "policy-server_amd"), tests=os.path.join(root, "tests"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, KW_BULK_DIRECT="0", KW_POISON_VERDICTS="1"))
    assert out.returncode == 0 and "direct off ok" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


def test_argument_errors():
    env, _ = _envs("c4_64")
    ids = env.policy_ids()
    syn, _, _ = _oracle("c4_64", 4, 9000, 77, ids)
    b = syn.batch().to_device(0)

    def is_arg_error(call):
        with pytest.raises(K.EvaluationError) as e:
            call()
        assert e.value.code == N.KW_E_ARG

    is_arg_error(lambda: b.summary(out=K.Summary(9000, len(ids))))  # before any pass
    is_arg_error(lambda: b.verdict_rows([0]))
    b.validate(env, ids)
    is_arg_error(lambda: b.summary(out=K.Summary(8999, len(ids))))
    is_arg_error(lambda: b.summary(out=K.Summary(9000, len(ids) - 1)))
    is_arg_error(lambda: b.verdict_rows([0, 9000]))
    is_arg_error(lambda: syn.batch().validate_host_summary(env, ids, out=K.Summary(9001, len(ids))))
    is_arg_error(lambda: syn.batch().validate_host_summary(env, ids, out=K.Summary(9000, len(ids) + 1)))
    assert b.summary().rows == 9000  # the batch is still good
