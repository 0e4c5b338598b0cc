"""CPU: the policy lists of tests/family_cases.py plan to the tile-kernel instantiation each is named
for (kw_debug_plan_variants: the arguments the dispatch would be called with; Variant.resolve: the
instantiation the dispatch maps them to), and the batches the device tests run them over exercise
every column (conditions on the oracle's words). tests/test_family_sets_gpu.py runs the lists.
"""
import numpy as np
import pytest

import family_cases as F
import kwgpu as K
import oracle as O
from family_cases import ALL, CTR, GRP, IMG, LBL, NFA, RNG

KNOBS = ("KW_TILE_GENERIC", "KW_TILE_DEBUG", "KW_GLOBAL_TABLES", "KW_SPLIT", "KW_SLOT_ROWS", "KW_TILE_QUANTILE")
TABLES = [pytest.param(True, id="lds"), pytest.param(False, id="global")]
_cache = {}


@pytest.fixture(autouse=True)
def _clean(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _tables(monkeypatch, lds):
    if not lds:
        monkeypatch.setenv("KW_GLOBAL_TABLES", "1")


def _env():
    if "env" not in _cache:
        _cache["env"] = K.EvaluationEnvironment(F.document(), continue_on_errors=True, always_accept_namespace=F.NS)
    return _cache["env"]


def _oracle():
    if "oe" not in _cache:
        _cache["oe"] = O.OracleEnv(F.document(), continue_on_errors=True, always_accept_namespace=F.NS)
    return _cache["oe"]


def _syn(spec):
    if spec not in _cache:
        _cache[spec] = K.SynthBatch(spec[0], spec[1], seed=spec[2])
    return _cache[spec]


def _top():
    return [p for p in _env().policy_ids() if "/" not in p]


def _words(spec, origin):
    """The oracle's words [rows][top-level policies] of a batch, evaluated once."""
    key = ("words", spec, origin)
    if key not in _cache:
        top = _top()
        _cache[key] = _oracle().eval(_syn(spec).soa(), top, origin).reshape(spec[1], len(top))
        _cache[key].setflags(write=False)
    return _cache[key]


# ---- the document and its lists

def test_document_builds_alike_on_both_sides():
    env, oe = _env(), _oracle()
    assert env.policy_ids() == [p["id"] for p in oe.pol]
    for c in ("c-bad", "c-unsupported"):
        assert env.policy_initialization_error(c)
    for g in F.GROUPS + ["c-folded"]:
        assert env.is_group(env.lookup(g))
    named = {p for f in F.SETS for p in F.selection(f)} | set(F.NS_FILLERS) | set(F.CONSTANTS)
    assert named == set(_top()), "a policy of the document that no list uses, or a list naming none"


def test_sixteen_lists_sixteen_sets():
    b = _syn(F.DEFAULT_BATCH).batch()
    feats = [b.debug_plan_variants(_env(), F.selection(f))[0].feat for f in F.SETS]
    assert sorted(feats) == list(range(16))
    assert F.SETS == list(range(16))


def test_padded_lists_hold_what_they_say():
    seen = set()
    for f in F.SETS:
        assert len(F.core(f)) <= 3
        for w in F.WIDTHS:
            cols = F.padded(f, w)
            assert len(cols) == w == len(set(cols)) and set(F.core(f)) <= set(cols)
            const = [i for i, c in enumerate(cols) if c in F.CONSTANTS]
            assert (len(const) == 1) == (w >= 4), (f, w, cols)
            if const:
                seen.add((w, const[0] % 4))
    assert seen == {(w, p) for w in (4, 8, 12) for p in range(4)}, "a constant column at every position of a 4-column group"


# ---- planned variants

@pytest.mark.parametrize("lds", TABLES)
@pytest.mark.parametrize("feat", F.SETS)
def test_planned_variant(monkeypatch, feat, lds):
    """The full list and every padded one, both origins: the family set the list is named for, one
    launch, and the production shape exactly where the predicate admits it."""
    _tables(monkeypatch, lds)
    env, b = _env(), _syn(F.DEFAULT_BATCH).batch()
    for cols in [F.selection(feat), F.selection(feat)[::-1]] + [F.padded(feat, w) for w in F.WIDTHS]:
        for origin in (K.VALIDATE, K.AUDIT):
            want = F.variant(feat, lds, prod=F.prod_shape(feat, lds, len(cols)))
            assert b.debug_plan_variants(env, cols, origin) == [want], cols
            assert b.debug_plan_kernels(env, cols, origin) == [K.KERNEL_PROD if want.prod else K.KERNEL_GENERIC]
            assert want.resolve() == want, "a family set without clocks or NFA elements has its own instantiation"
    assert F.prod_shape(feat, lds, len(F.selection(feat))) == (feat == (LBL | CTR) and lds)


@pytest.mark.parametrize("lds", TABLES)
@pytest.mark.parametrize("feat", F.SETS)
def test_planned_variant_under_phase_clocks(monkeypatch, feat, lds):
    """KW_TILE_DEBUG=512: the launch asks for its own family set with clocks; the dispatch keeps the
    image, image / group and label / container sets with LDS tables and sends the rest to kFeatAll."""
    _tables(monkeypatch, lds)
    monkeypatch.setenv("KW_TILE_DEBUG", "512")
    b = _syn(F.DEFAULT_BATCH).batch()
    got = b.debug_plan_variants(_env(), F.selection(feat))
    assert got == [F.variant(feat, lds, timing=True)]
    own = lds and feat in (IMG, IMG | GRP, LBL | CTR)
    assert got[0].resolve() == F.variant(feat if own else ALL, lds, timing=True)
    assert b.debug_plan_kernels(_env(), F.selection(feat)) == [K.KERNEL_GENERIC]


@pytest.mark.parametrize("lds", TABLES)
def test_planned_variant_with_an_nfa_element(monkeypatch, lds):
    _tables(monkeypatch, lds)
    env = K.EvaluationEnvironment(F.nfa_document(), continue_on_errors=True, always_accept_namespace=F.NS)
    b = _syn(F.DEFAULT_BATCH).batch()
    for cols in F.NFA_CASES:
        for debug in (None, "512"):
            if debug:
                monkeypatch.setenv("KW_TILE_DEBUG", debug)
            got = b.debug_plan_variants(env, cols)
            assert got == [F.variant(ALL | NFA, lds, timing=bool(debug))], cols
            assert got[0].resolve() == F.variant(ALL | NFA, lds), "clocks or not, the one NFA instantiation"
            monkeypatch.delenv("KW_TILE_DEBUG", raising=False)
    # (the namespace policy alone reads no NFA classifier: its own narrow kernel)
    assert b.debug_plan_variants(env, ["ns-0"]) == [F.variant(0, lds)]


@pytest.mark.parametrize("lds", TABLES)
@pytest.mark.parametrize("feat", F.SETS)
def test_planned_variant_on_small_tiles(monkeypatch, feat, lds):
    """8-row tiles over rows of many containers: every list's tiles take predecessor ranges
    (cmax > 4 x rows), and only the label / container set with LDS tables has the wave scan."""
    _tables(monkeypatch, lds)
    monkeypatch.setenv("KW_SLOT_ROWS", "8")
    env, b = _env(), _syn(F.SMALL_TILE_BATCH).batch()
    cols = F.selection(feat)
    plan = b.debug_plan(env, cols)
    assert plan["rows"] == 8 and plan["cmax"] > 4 * plan["rows"] and plan["chunks"] == 1, plan
    scan = lds and feat == (LBL | CTR)
    want = F.want_variant(feat, lds, ranges=True)
    assert bool(want.feat & RNG) == scan
    want = want._replace(prod=F.prod_shape(feat, lds, len(cols)))
    assert b.debug_plan_variants(env, cols) == [want]
    assert plan["scan_regions"] == (1 if scan else 0), plan
    assert want.resolve() == want
    monkeypatch.setenv("KW_TILE_DEBUG", "512")  # the clocks have no wave-scan instantiation
    got, = b.debug_plan_variants(env, cols)
    assert got == F.variant(want.feat, lds, timing=True)
    assert not got.resolve().feat & RNG and got.resolve().timing


def test_resolve_over_every_request():
    """Variant.resolve over all requests: idempotent, never drops a family the launch carries, and
    lands on one of the instantiations the library compiles (kernels.hip tile_fn's list)."""
    compiled = {F.variant(f, l) for f in range(16) for l in (True, False)}
    compiled |= {F.variant(ALL | NFA, True), F.variant(ALL | NFA, False), F.variant(LBL | CTR | RNG, True)}
    compiled |= {F.variant(f, True, timing=True) for f in (IMG, IMG | GRP, LBL | CTR, ALL)} | {F.variant(ALL, False, timing=True)}
    compiled |= {F.variant(LBL | CTR, True, prod=True), F.variant(LBL | CTR | RNG, True, prod=True)}
    reached = set()
    for word in range(0x800):
        if word & 0xC0:
            continue
        v = K.Variant.from_word(word)
        if v.prod and not ((v.feat & ~RNG) == (LBL | CTR) and v.lds_tables and not v.timing):
            continue  # (not a request: tile_prod_shape admits only these)
        if (v.feat & NFA) and (v.feat & ALL) != ALL:
            continue  # (not a request: the planner sets kFeatNfa with every family)
        r = v.resolve()
        assert r in compiled, (v, r)
        assert r.resolve() == r
        assert (r.feat & ALL) & (v.feat & ALL) == (v.feat & ALL), (v, r)
        assert r.lds_tables == v.lds_tables
        reached.add(r)
    assert reached == compiled and len(compiled) == 42


# ---- the inputs of the device tests

def _accepts(w):
    return (w & K._native.KW_F_ALLOWED) != 0


@pytest.mark.parametrize("origin", [K.VALIDATE, K.AUDIT])
def test_default_batch_exercises_every_column(origin):
    top = _top()
    w = _words(F.DEFAULT_BATCH, origin)
    bypass = (w[:, 0] & K._native.KW_BYPASS) != 0
    assert bypass.any(), "no row in the always-accepted namespace"
    assert ((w & K._native.KW_BYPASS) != 0).all(axis=1).tolist() == bypass.tolist()
    for j, name in enumerate(top):
        col = w[~bypass, j]
        if name in F.CONSTANTS:
            assert len(set(col.tolist())) == 1, name
            continue
        assert len(set(col.tolist())) >= 2, name
        # (a monitor policy's final word always allows: the verdict bit tells its rows apart)
        acc = (col & K._native.KW_V_ALLOWED) != 0
        assert acc.any() and (~acc).any(), (name, "accepts and rejects")
    for g in F.GROUPS:
        assert (~_accepts(w[~bypass, top.index(g)])).any(), g
    if origin == K.VALIDATE:
        assert ((w[:, top.index(F.MUTATING)] & K._native.KW_F_PATCH) != 0).any(), "the mutating column never patches"


def test_small_tile_batch_exercises_its_columns():
    top = _top()
    w = _words(F.SMALL_TILE_BATCH, K.VALIDATE)
    bypass = (w[:, 0] & K._native.KW_BYPASS) != 0
    assert bypass.any()
    for name in sorted({p for f in F.SMALL_TILE_SETS for p in F.selection(f)}):
        acc = (w[~bypass, top.index(name)] & K._native.KW_V_ALLOWED) != 0
        assert acc.any() and (~acc).any(), name


@pytest.mark.parametrize("origin", [K.VALIDATE, K.AUDIT])
def test_oracle_columns_are_independent(origin):
    """The oracle's word for a column in any list equals its word in the full list: the device
    tests evaluate the oracle once per origin and select columns."""
    top = _top()
    full = _words(F.DEFAULT_BATCH, origin)
    soa = _syn(F.DEFAULT_BATCH).soa()
    lists = [F.selection(f) for f in F.SETS] + [F.padded(f, w) for f in (0, 6, 9, 15) for w in F.WIDTHS] + [F.selection(15)[::-1]]
    for cols in lists:
        sub = _oracle().eval(soa, cols, origin).reshape(full.shape[0], len(cols))
        assert np.array_equal(sub, full[:, [top.index(c) for c in cols]]), cols
