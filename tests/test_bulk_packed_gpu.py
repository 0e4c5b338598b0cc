"""Bulk path, packed output (kw_validate_host_packed): the device packs each chunk's verdict words
into bit-planes, per-row offsets and exception words (include/kwgpu.h kw_packed) and only those are
read back. Every case checks the whole pass twice: unpack() equals the oracle's words on every
(row, policy) pair, and planes / exc_off / exc / dict equal the reference host encoder's output over
the oracle's words byte for byte, which pins format, order and dictionary on the device. Chunked
passes (the running total crossing chunks, one column with many rows per wave, partial and several
column groups, a row count off every workgroup span), the unchunked forms, pageable and page-locked
outputs, both origins, the capacity error (chunked and in the slabs of an unchunked pass), a batch
without rows through all three bulk forms, and the responses formatted from word(r, c)."""
import numpy as np
import pytest

import kwgpu as K
import oracle as O
from helpers import config, diff_verdicts, many_policies_config

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
    """(synthetic batch, the oracle's words, the host encoder's packing of them), computed once."""
    key = (name, scfg, rows, seed, len(ids), origin)
    if key not in _memo:
        env, oe = _envs(name)
        syn = K.SynthBatch(scfg, rows, seed=seed)
        ora = oe.eval(syn.soa(), ids, origin)
        _memo[key] = (syn, ora, K.PackedVerdicts.from_words(env, ids, ora, origin))
    return _memo[key]


def _same(got, ora, ref, ids):
    """Total: every word, and every byte of the packed arrays against the host encoder's."""
    words = got.unpack()
    assert np.array_equal(words, ora), diff_verdicts(words, ora, len(ids), ids)
    assert got.exc_count == ref.exc_count
    assert np.array_equal(got.dict, ref.dict)
    assert np.array_equal(got.planes, ref.planes)
    assert np.array_equal(got.exc_off, ref.exc_off)
    assert np.array_equal(got.exc[:got.exc_count], ref.exc[:ref.exc_count])


def _both_outputs(name, scfg, rows, seed, ids, chunk, origin=K.VALIDATE):
    env, _ = _envs(name)
    syn, ora, ref = _oracle(name, scfg, rows, seed, ids, origin)
    got = syn.batch().validate_host_packed(env, ids, origin=origin, chunk_rows=chunk)  # pageable
    _same(got, ora, ref, ids)
    pin = K.PackedVerdicts.page_locked(rows, len(ids), exc_cap=ref.exc_count)  # direct DMA, exact capacity
    pin.planes.fill(0xA5A5A5A5A5A5A5A5)
    pin.exc_off.fill(0xA5A5A5A5)
    pin.exc.fill(0xA5A5A5A5)
    got2 = syn.batch().validate_host_packed(env, ids, out=pin, origin=origin, chunk_rows=chunk)
    assert got2 is pin
    _same(pin, ora, ref, ids)


@pytest.mark.parametrize("name,scfg,rows,chunk", [
    ("c4_64", 4, 30000, 2048),      # 15 chunks: the running total crosses chunks
    ("c4_64", 4, 30000, 0),         # the default chunk size: one chunk
    ("c2_trusted", 2, 50000, 777),  # one column: 64 rows per wave round
    ("c3_group", 3, 20000, 4096),   # 4 columns: 16 rows per wave round
    ("parity", 0, 20000, 1500),
    ("c4_64", 4, 30011, 2048),      # rows off every wave's and workgroup's span
    # one column, 256 * 1024 + 1 items in one chunk: 257 block sums, so the one-workgroup scan over
    # them takes a second round of 256. The first chunk of a pass is a sixteenth of chunk_rows
    # (bulkplan.hpp chunk_bounds), so 16 times the rows, rounded up to whole tiles, keeps them together
    ("c2_trusted", 2, 262145, 16 * 262208),
])
def test_packed_chunked_matches_oracle_and_host_encoder(name, scfg, rows, chunk):
    env, _ = _envs(name)
    _both_outputs(name, scfg, rows, 4400 + scfg, env.policy_ids(), chunk)


def _c6_without_wide_groups(env):
    ids = env.policy_ids()
    return [p for j, p in enumerate(ids) if not (env.is_group(j) and len(env.group_members(j)) > 15)]


@pytest.mark.parametrize("ncol", [63, 65, 128])
def test_packed_column_groups(ncol):
    """C6 prefixes without the 40-member group, so the pass stays chunked: a partial last group,
    one column past a group, two full groups."""
    env, _ = _envs("c6_256")
    ids = _c6_without_wide_groups(env)[:ncol]
    assert len(ids) == ncol
    _both_outputs("c6_256", 6, 3000, 6, ids, 512)


def test_packed_unchunked_forms():
    """C6 whole (five column groups, the 40-member group's side data: unchunked, packed in row slabs
    after the pass); C5's requests beyond the tile capacities on the overflow kernels inside chunks."""
    env, _ = _envs("c6_256")
    ids = env.policy_ids()
    assert (len(ids) + 63) // 64 == 5
    _both_outputs("c6_256", 6, 3000, 6, ids, 512)
    env5, _ = _envs("c5_mixed")
    _both_outputs("c5_mixed", 5, 4000, 55, env5.policy_ids(), 256)


def test_packed_overflow_tiles(monkeypatch):
    monkeypatch.setenv("KW_TILE_QUANTILE", "0.05")
    env, _ = _envs("c4_64")
    _both_outputs("c4_64", 4, 6000, 4804, env.policy_ids(), 640)


def test_packed_audit_origin_and_same_batch_both_forms():
    """The audit origin; then one batch object through validate_host and validate_host_packed:
    identical words, and the batch stays usable for a device pass."""
    env, oe = _envs("c4_64")
    ids = env.policy_ids()
    _both_outputs("c4_64", 4, 9000, 77, ids, 1024, origin=K.AUDIT)
    syn, ora, ref = _oracle("c4_64", 4, 9000, 77, ids, K.VALIDATE)
    b = syn.batch()
    full = b.validate_host(env, ids, chunk_rows=1024).copy()
    packed = b.validate_host_packed(env, ids, chunk_rows=1024)
    assert np.array_equal(packed.unpack(), full) and np.array_equal(full, ora)
    _same(packed, ora, ref, ids)
    b.validate(env, ids)
    assert np.array_equal(b.verdicts(), ora)


def test_packed_capacity_too_small_reports_the_need():
    """A chunked pass whose exceptions exceed the caller's capacity runs to its end and reports the
    need, which then suffices; without `out` the binding regrows and retries by itself."""
    env, _ = _envs("c4_64")
    ids = env.policy_ids()
    syn, ora, ref = _oracle("c4_64", 4, 30000, 4404, ids)
    for pinned in (False, True):
        small = K.PackedVerdicts(30000, len(ids), exc_cap=ref.exc_count // 3, pinned=pinned)
        with pytest.raises(K.NoSpace) as e:
            syn.batch().validate_host_packed(env, ids, out=small, chunk_rows=2048)
        assert e.value.need == ref.exc_count
        fit = K.PackedVerdicts(30000, len(ids), exc_cap=e.value.need, pinned=pinned)
        _same(syn.batch().validate_host_packed(env, ids, out=fit, chunk_rows=2048), ora, ref, ids)
    assert ref.exc_count > max(1024, 30000 * len(ids) // 4)  # the default capacity is too small here:
    _same(syn.batch().validate_host_packed(env, ids, chunk_rows=2048), ora, ref, ids)  # regrown, retried


def test_packed_capacity_too_small_on_the_unchunked_path():
    """C6 whole runs unchunked and is packed in six row slabs of 512. A capacity of a third of the
    exceptions is exceeded in the second slab (the oracle's offsets say so), so the later slabs run
    on without exception read-backs and count: the call reports the need, which then suffices."""
    env, _ = _envs("c6_256")
    ids = env.policy_ids()
    syn, ora, ref = _oracle("c6_256", 6, 3000, 6, ids)
    cap = ref.exc_count // 3
    assert cap > 0 and ref.exc_count > ref.exc_off[512]  # more than one slab's share
    assert ref.exc_off[512] <= cap < ref.exc_off[5 * 512]  # some words fit; the overflow is not left to the last slab
    for pinned in (False, True):
        small = K.PackedVerdicts(3000, len(ids), exc_cap=cap, pinned=pinned)
        with pytest.raises(K.NoSpace) as e:
            syn.batch().validate_host_packed(env, ids, out=small, chunk_rows=512)
        assert e.value.need == ref.exc_count
        fit = K.PackedVerdicts(3000, len(ids), exc_cap=e.value.need, pinned=pinned)
        _same(syn.batch().validate_host_packed(env, ids, out=fit, chunk_rows=512), ora, ref, ids)


def test_empty_batch_through_all_three_forms():
    """No rows, C4's policies: the words form returns an empty array, the packed form no exceptions
    and the one offset 0, the summary form all-zero counters (prefilled outputs)."""
    env, _ = _envs("c4_64")
    ids = env.policy_ids()
    empty = K.Batch.from_json([])  # (SynthBatch makes no batch without rows)
    assert empty.n == 0
    assert empty.validate_host(env, ids).size == 0
    p = K.PackedVerdicts(0, len(ids))
    p.exc_off.fill(0xA5A5A5A5)
    p.exc_count = 7
    assert empty.validate_host_packed(env, ids, out=p) is p
    assert p.exc_count == 0 and p.exc_off[0] == 0 and p.unpack().size == 0
    for planes in (True, False):
        s = K.Summary(0, len(ids), planes=planes)
        s.col.fill(0xA5A5A5A5A5A5A5A5)
        assert empty.validate_host_summary(env, ids, out=s) is s
        assert not s.col.any()


@pytest.mark.parametrize("name,scfg", [("c3_group", 3), ("c4_64", 4)])
def test_packed_words_format_the_same_responses(name, scfg):
    """200 rows: the response of every (row, policy) formatted from word(r, c) of a packed pass
    equals the one from the full-word pass, group members and causes included."""
    env, _ = _envs(name)
    ids = env.policy_ids()
    n = 200
    syn = K.SynthBatch(scfg, n, seed=8800 + scfg)
    bf, bp = syn.batch(), syn.batch()
    v = bf.validate_host(env, ids).reshape(n, len(ids))
    p = bp.validate_host_packed(env, ids)
    groups = {j: env.group_members(j) for j in range(len(ids)) if env.is_group(j)}
    for r in range(n):
        doc = syn.json(r)
        pw = [p.word(r, c) for c in range(len(ids))]
        assert pw == [int(x) for x in v[r]]
        for j in range(len(ids)):
            mv_p = [pw[m] for m in groups[j]] if j in groups else None
            mv_f = [int(v[r, m]) for m in groups[j]] if j in groups else None
            assert bp.format_response(env, r, j, pw[j], mv_p, doc=doc) == bf.format_response(env, r, j, int(v[r, j]), mv_f, doc=doc)
            if j in groups and (pw[j] >> 8) & 0xFF == O.R_GROUP:
                assert bp.group_causes(r, j, pw[j]) == bf.group_causes(r, j, int(v[r, j]))
