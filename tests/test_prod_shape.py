"""CPU: which tile launches take a production-shape kernel (kernels.hpp tile_prod_shape, the one
predicate the launch decides by).

The predicate over a table (kw_debug_prod_shape builds a launch record from the values): the
production shape qualifies for both family sets that have such a kernel, and every defeating
condition, tried alone, disqualifies. Then real plans (kw_debug_plan_kernels: the planner's launch
records, nothing launched): C4's and C5's launches at 5,000 requests qualify, KW_TILE_GENERIC=1
sends every one to the generic kernel, and the settings that change a launch's shape do what the
table says. KW_TILE_GENERIC is a planning knob (it is in the plan cache's key), but no plan word
depends on it.
"""
import pytest

import kwgpu as K
from helpers import config

NS = "kubewarden"
IMG, LBL, CTR, GRP, NFA, RNG = 1, 2, 4, 8, 16, 32
SHAPE = dict(feat=LBL | CTR, lds_tables=1, debug=0, nchunk=1, rows_mode=0, prefetch=0, ncols=64, vec4=1, timing=0)
ORDER = ("feat", "lds_tables", "debug", "nchunk", "rows_mode", "prefetch", "ncols", "vec4", "timing")

DEFEATS = [
    ("debug bit 1", dict(debug=1)), ("debug bit 2", dict(debug=2)), ("debug bit 4", dict(debug=4)),
    ("debug bit 256", dict(debug=256)), ("debug bit 1024", dict(debug=1024)), ("debug bit 2048", dict(debug=2048)),
    ("debug bit 4096", dict(debug=4096)), ("debug bit 8192", dict(debug=8192)), ("debug bit 16384", dict(debug=16384)),
    ("two chunks", dict(nchunk=2)),
    ("rows mode", dict(rows_mode=1)),
    ("prefetch on", dict(prefetch=1)),
    ("6 column groups", dict(ncols=24)),
    ("an NFA element", dict(feat=IMG | LBL | CTR | GRP | NFA)),
    ("global tables", dict(lds_tables=0)),
    # beyond the issue's list: what else the launch must have
    ("phase clocks", dict(timing=1)),
    ("no 16-byte stores", dict(vec4=0)),
    ("no column", dict(ncols=0)),
    ("more groups than threads", dict(ncols=4 * 512)),
    ("image family", dict(feat=IMG)), ("image and group families", dict(feat=IMG | GRP)),
    ("label family alone", dict(feat=LBL)), ("every family", dict(feat=IMG | LBL | CTR | GRP)),
]


def qualifies(**kw):
    v = dict(SHAPE, **kw)
    return K.library().kw_debug_prod_shape(*[v[k] for k in ORDER])


@pytest.mark.parametrize("feat", [LBL | CTR, LBL | CTR | RNG])
@pytest.mark.parametrize("ncols", [4, 8, 64, 256, 1024])
def test_production_shape_qualifies(feat, ncols):
    assert qualifies(feat=feat, ncols=ncols) == 1


@pytest.mark.parametrize("feat", [LBL | CTR, LBL | CTR | RNG])
@pytest.mark.parametrize("what,change", DEFEATS, ids=[d[0] for d in DEFEATS])
def test_each_defeating_condition_disqualifies(feat, what, change):
    if "feat" not in change:
        change = dict(change, feat=feat)
    assert qualifies(**change) == 0, what


def _env(name):
    return K.EvaluationEnvironment(config(name), continue_on_errors=True, always_accept_namespace=NS)


@pytest.fixture(autouse=True)
def _clean(monkeypatch):
    for k in ("KW_TILE_GENERIC", "KW_TILE_DEBUG", "KW_GLOBAL_TABLES", "KW_SPLIT", "KW_SLOT_ROWS"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("name,scfg,knobs", [("c4_64", 4, {}), ("c4_64", 4, {"KW_SLOT_ROWS": "8"}), ("c5_mixed", 5, {}),
                                             ("c5_mixed", 5, {"KW_SPLIT": "1"})])
def test_real_plans_qualify(monkeypatch, name, scfg, knobs):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    env = _env(name)
    ids = env.policy_ids()
    b = K.SynthBatch(scfg, 5_000, seed=1).batch()
    plan = b.debug_plan(env, ids)
    kernels = b.debug_plan_kernels(env, ids)
    assert len(kernels) == plan["regions"] * plan["launches"] and kernels
    assert kernels == [K.KERNEL_PROD] * len(kernels), (plan, kernels)
    if knobs.get("KW_SPLIT") == "1":  # the heavy region's launch is the wave-scan one: the kFeatRng production kernel
        assert plan["regions"] == 2 and plan["scan_regions"] == 2, plan
    monkeypatch.setenv("KW_TILE_GENERIC", "1")
    assert b.debug_plan_kernels(env, ids) == [K.KERNEL_GENERIC] * len(kernels)
    assert b.debug_plan(env, ids) == plan
    monkeypatch.setenv("KW_TILE_GENERIC", "0")
    assert b.debug_plan_kernels(env, ids) == kernels


@pytest.mark.parametrize("name,scfg,knobs", [("c4_64", 4, {"KW_TILE_DEBUG": "16384"}), ("c4_64", 4, {"KW_TILE_DEBUG": "512"}),
                                             ("c4_64", 4, {"KW_GLOBAL_TABLES": "1"}), ("c6_256", 6, {}), ("c2_trusted", 2, {}),
                                             ("c3_group", 3, {}), ("c1_namespace", 1, {}), ("parity", 0, {})])
def test_other_plans_stay_generic(monkeypatch, name, scfg, knobs):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    env = _env(name)
    ids = env.policy_ids()
    b = K.SynthBatch(scfg, 5_000, seed=1).batch()
    kernels = b.debug_plan_kernels(env, ids)
    assert kernels and kernels == [K.KERNEL_GENERIC] * len(kernels), kernels


@pytest.mark.parametrize("name,scfg", [("parity", 0), ("c1_namespace", 1), ("c2_trusted", 2), ("c3_group", 3), ("c4_64", 4),
                                       ("c5_mixed", 5), ("c6_256", 6)])
def test_plan_words_do_not_depend_on_the_knob(monkeypatch, name, scfg):
    env = _env(name)
    ids = env.policy_ids()
    b = K.SynthBatch(scfg, 5_000, seed=1).batch()
    plans = []
    for v in (None, "1", "0"):
        if v is not None:
            monkeypatch.setenv("KW_TILE_GENERIC", v)
        plans.append(b.debug_plan(env, ids))
    assert plans[0] == plans[1] == plans[2], plans
