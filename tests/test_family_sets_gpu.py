"""GPU: every family-set instantiation of the tile kernel against the oracle (kernels.hip
evaluate_tiles_kernel<LDST, TIMING, F, PROD>; DESIGN.md §5 lists which test runs which).

The policy lists of tests/family_cases.py, one per family set F of {image, label, container,
group}, run with LDS and with global tables, in both origins, at the verdict-row widths where the
kernel's P3 changes writer, in rows mode, on 8-row tiles that take predecessor ranges, under the
phase clocks, with NFA elements over a narrow layout, and through the bulk path. Every pass starts
from poisoned verdict words, every word must equal the oracle's, and every pass is asked which
variant its launch requested (kw_debug_last_variants), so no case can pass on another instantiation.

The default batch is SynthBatch(0, 197): at 64-row tiles three full tiles and one of five rows.
tests/test_family_sets.py checks on the host that this batch makes every column accept and reject.
"""
import numpy as np
import pytest

import family_cases as F
import kwgpu as K
import oracle as O
from family_cases import ALL, CTR, GRP, IMG, LBL, NFA, RNG
from helpers import diff_verdicts

pytestmark = pytest.mark.gpu
ORIGINS = [pytest.param(K.VALIDATE, id="validate"), pytest.param(K.AUDIT, id="audit")]
TABLES = [pytest.param(True, id="lds"), pytest.param(False, id="global")]
KNOBS = ("KW_TILE_GENERIC", "KW_TILE_DEBUG", "KW_GLOBAL_TABLES", "KW_SPLIT", "KW_SLOT_ROWS", "KW_TILE_QUANTILE", "KW_SCHED",
         "KW_SCHED_TAIL")
_cache = {}


@pytest.fixture(autouse=True)
def _knobs(monkeypatch):
    monkeypatch.setenv("KW_POISON_VERDICTS", "1")
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _tables(monkeypatch, lds):
    if not lds:
        monkeypatch.setenv("KW_GLOBAL_TABLES", "1")


def _envs(which="family"):
    """(device environment, oracle environment, top-level policy ids), built once per module."""
    if which not in _cache:
        doc = F.document() if which == "family" else F.nfa_document()
        env = K.EvaluationEnvironment(doc, continue_on_errors=True, always_accept_namespace=F.NS, device=0)
        oe = O.OracleEnv(doc, continue_on_errors=True, always_accept_namespace=F.NS)
        assert env.policy_ids() == [p["id"] for p in oe.pol]
        _cache[which] = (env, oe, [p for p in env.policy_ids() if "/" not in p])
    return _cache[which]


def _batch(spec):
    """The synthetic batch `spec`, resident on device 0, built once per module."""
    if spec not in _cache:
        syn = K.SynthBatch(spec[0], spec[1], seed=spec[2])
        _cache[spec] = (syn, syn.batch().to_device(0))
    return _cache[spec]


def _oracle(spec, origin, cols, which="family"):
    """The oracle's words [rows][cols]: evaluated once per batch and origin over the document's
    top-level policies (never written again), columns selected per case."""
    env, oe, top = _envs(which)
    key = ("words", which, spec, origin)
    if key not in _cache:
        w = oe.eval(_batch(spec)[0].soa(), top, origin).reshape(spec[1], len(top))
        w.setflags(write=False)
        _cache[key] = w
    return np.ascontiguousarray(_cache[key][:, [top.index(c) for c in cols]])


def _check_pass(b, env, cols, origin, ora, want):
    """One all-pairs pass: the oracle's words, one launch, the variant `want`, and the kernel kind
    kw_debug_last_kernels reports consistent with it."""
    b.validate(env, cols, origin)
    variants, kernels = b.debug_last_variants(), b.debug_last_kernels()
    got = b.verdicts().reshape(ora.shape)
    assert variants == [want], (variants, want, cols)
    assert kernels == [K.KERNEL_PROD if want.prod else K.KERNEL_GENERIC], (kernels, want)
    assert len(b.debug_last_launches()) == 1
    assert np.array_equal(got, ora), f"{want} {cols}: " + diff_verdicts(got.reshape(-1), ora.reshape(-1), len(cols), cols)
    return variants[0]


# ---- the family matrix

@pytest.mark.parametrize("origin", ORIGINS)
@pytest.mark.parametrize("lds", TABLES)
@pytest.mark.parametrize("feat", F.SETS)
def test_family_matrix(monkeypatch, feat, lds, origin):
    _tables(monkeypatch, lds)
    env = _envs()[0]
    b = _batch(F.DEFAULT_BATCH)[1]
    cols = F.selection(feat)
    prod = F.prod_shape(feat, lds, len(cols))
    assert prod == (feat == (LBL | CTR) and lds), "the production shape: the label / container list with LDS tables"
    _check_pass(b, env, cols, origin, _oracle(F.DEFAULT_BATCH, origin, cols), F.variant(feat, lds, prod=prod))


def test_every_family_set_launches_in_both_table_modes(monkeypatch):
    """The variants the launches report back, as a set: all 16 family sets, both table modes."""
    env = _envs()[0]
    b = _batch(F.DEFAULT_BATCH)[1]
    seen = set()
    for lds in (True, False):
        monkeypatch.setenv("KW_GLOBAL_TABLES", "0" if lds else "1")
        for feat in F.SETS:
            cols = F.selection(feat)
            b.validate(env, cols, K.VALIDATE)
            v, = b.debug_last_variants()
            got, ora = b.verdicts(), _oracle(F.DEFAULT_BATCH, K.VALIDATE, cols)
            assert np.array_equal(got, ora.reshape(-1)), (feat, lds, diff_verdicts(got, ora.reshape(-1), len(cols), cols))
            assert not v.timing and v.resolve() == v
            seen.add((v.feat, v.lds_tables))
    assert seen == {(f, lds) for f in range(16) for lds in (True, False)}


# ---- the P3 writers

@pytest.mark.parametrize("width", F.WIDTHS)
@pytest.mark.parametrize("feat", F.SETS)
def test_p3_writers(feat, width):
    """The verdict-word writers by row width: 3 columns (scalar stores, npol % 4 != 0), 4 and 8
    (16-byte stores, a power-of-two number of 4-column groups), 12 (16-byte stores, three groups),
    for every family set, i.e. the group writer and both no-group writers at every column form.
    From width 4 on the row holds a constant column (an init error, an unsupported module or a
    constant-folded group) whose place in its 4-column group moves with the family set."""
    env = _envs()[0]
    b = _batch(F.DEFAULT_BATCH)[1]
    cols = F.padded(feat, width)
    want = F.variant(feat, True, prod=F.prod_shape(feat, True, width))
    _check_pass(b, env, cols, K.VALIDATE, _oracle(F.DEFAULT_BATCH, K.VALIDATE, cols), want)


@pytest.mark.parametrize("feat,width", [(15, 8), (6, 12), (10, 3)])
def test_p3_writers_reversed(feat, width):
    env = _envs()[0]
    b = _batch(F.DEFAULT_BATCH)[1]
    cols = F.padded(feat, width)[::-1]
    want = F.variant(feat, True, prod=F.prod_shape(feat, True, width))
    _check_pass(b, env, cols, K.AUDIT, _oracle(F.DEFAULT_BATCH, K.AUDIT, cols), want)


# ---- rows mode

@pytest.mark.parametrize("lds", TABLES)
@pytest.mark.parametrize("feat", F.SETS)
def test_rows_mode(monkeypatch, feat, lds):
    """A policy per row, cycling through the list (every policy of it occurs): the pass plans for
    the distinct policies of the rows, hence the list's family set; never the production shape."""
    _tables(monkeypatch, lds)
    env = _envs()[0]
    n = F.DEFAULT_BATCH[1]
    b = _batch(F.DEFAULT_BATCH)[1]
    cols = F.selection(feat)
    pick = (np.arange(n) + np.arange(n) // len(cols) + feat) % len(cols)
    assert set(pick.tolist()) == set(range(len(cols)))
    for origin in (K.VALIDATE, K.AUDIT):
        b.validate_rows(env, [cols[int(j)] for j in pick], origin)
        variants, kernels = b.debug_last_variants(), b.debug_last_kernels()
        got = b.verdicts(count=n)
        want = _oracle(F.DEFAULT_BATCH, origin, cols)[np.arange(n), pick]
        assert variants == [F.variant(feat, lds)] and kernels == [K.KERNEL_GENERIC], (variants, kernels)
        bad = (got != want).nonzero()[0]
        assert not len(bad), [(int(r), cols[int(pick[r])], K.decode(got[r]), K.decode(want[r])) for r in bad[:8]]


# ---- small tiles, predecessor ranges

@pytest.mark.parametrize("lds", TABLES)
@pytest.mark.parametrize("feat", F.SMALL_TILE_SETS)
def test_small_tiles_with_predecessor_ranges(monkeypatch, feat, lds):
    """8-row tiles over rows of many containers: cmax > 4 x rows, so P2 ORs predecessor ranges in
    whatever instantiation the list takes; the wave scan only for label / container with LDS tables."""
    _tables(monkeypatch, lds)
    monkeypatch.setenv("KW_SLOT_ROWS", "8")
    env = _envs()[0]
    b = _batch(F.SMALL_TILE_BATCH)[1]
    cols = F.selection(feat)
    plan = b.debug_plan(env, cols)
    assert plan["rows"] == 8 and plan["cmax"] > 4 * plan["rows"], plan
    want = F.want_variant(feat, lds, ranges=True)._replace(prod=F.prod_shape(feat, lds, len(cols)))
    assert bool(want.feat & RNG) == (lds and feat == (LBL | CTR))
    for origin in (K.VALIDATE, K.AUDIT):
        _check_pass(b, env, cols, origin, _oracle(F.SMALL_TILE_BATCH, origin, cols), want)


# ---- phase clocks

@pytest.mark.parametrize("feat,lds", F.TIMING_CASES)
def test_phase_clock_instantiations(monkeypatch, feat, lds):
    """KW_TILE_DEBUG=512: the image, image / group and label / container sets keep an instantiation
    of their own with LDS tables; the label set and every-family one run kFeatAll's, in both table
    modes (the label set: the every-family code over a layout planned for one family)."""
    _tables(monkeypatch, lds)
    monkeypatch.setenv("KW_TILE_DEBUG", "512")
    env = _envs()[0]
    b = _batch(F.DEFAULT_BATCH)[1]
    cols = F.selection(feat)
    for origin in (K.VALIDATE, K.AUDIT):
        v = _check_pass(b, env, cols, origin, _oracle(F.DEFAULT_BATCH, origin, cols), F.variant(feat, lds, timing=True))
        own = lds and feat in (IMG, IMG | GRP, LBL | CTR)
        assert v.resolve() == F.variant(feat if own else ALL, lds, timing=True)


# ---- NFA elements on a narrow layout

@pytest.mark.parametrize("lds", TABLES)
@pytest.mark.parametrize("cols", F.NFA_CASES, ids=["+".join(c) for c in F.NFA_CASES])
def test_nfa_on_a_narrow_layout(monkeypatch, cols, lds):
    """One-family lists whose pattern exceeds the DFA budget: the every-family kernel with NFA
    elements over a tile layout planned for that one family (o_img or o_lk of size 0)."""
    _tables(monkeypatch, lds)
    env = _envs("nfa")[0]
    b = _batch(F.DEFAULT_BATCH)[1]
    for origin in (K.VALIDATE, K.AUDIT):
        ora = _oracle(F.DEFAULT_BATCH, origin, cols, "nfa")
        assert len({int(x) for x in ora[:, cols.index([c for c in cols if c != "ns-0"][0])]}) > 2
        v = _check_pass(b, env, cols, origin, ora, F.variant(ALL | NFA, lds))
        assert v.resolve() == v


# ---- the bulk path

@pytest.mark.parametrize("feat", F.SETS)
def test_bulk_path(feat):
    env = _envs()[0]
    syn = _batch(F.DEFAULT_BATCH)[0]
    cols = F.selection(feat)
    got = syn.batch().validate_host(env, cols, chunk_rows=128)
    ora = _oracle(F.DEFAULT_BATCH, K.VALIDATE, cols).reshape(-1)
    assert np.array_equal(got, ora), diff_verdicts(got, ora, len(cols), cols)
