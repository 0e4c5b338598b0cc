"""CPU: the script string functions over the whole Unicode case tables (tests/script_unicode_cases.py:
2,795 case-mapped code points by value, 113 closure code points alone in four contexts, the
Final_Sigma context of 6,817 code points, White_Space and its look-alikes under trim). Three-way, as
test_rhai_forms.py: what the generator says (CPython's str.upper / lower / strip), the oracle's
interpreter, and the product through the slot compiler's host walk in both device forms: the truth
table the host interpreter fills at load, and (KW_GROUP_FORM=script) the typed bytecode of
groupvm.hpp run_script_prog with its per-script char table."""
import numpy as np
import pytest

import kwgpu as K
from helpers import diff_verdicts
from script_unicode_cases import FAMILIES, VECTORS, chunks, groups_doc, oracle_env, review, scripts
from test_rhai_forms import check_expected

ALLOWED = K._native.KW_F_ALLOWED


@pytest.fixture(params=["table", "script"])
def form(request, monkeypatch):
    if request.param == "script":
        monkeypatch.setenv("KW_GROUP_FORM", "script")
    else:
        monkeypatch.delenv("KW_GROUP_FORM", raising=False)
    return request.param


def test_families_cover_the_tables():
    from script_unicode_cases import closure_code_points, context_code_points, value_code_points
    values = value_code_points()
    assert len(values) == 2795
    assert sum(len(chr(c).upper()) > 1 or len(chr(c).lower()) > 1 for c in values) == 103
    assert any(c >= 0x10000 for c in values)
    closure = closure_code_points()
    assert len(closure) == 113 and {0x3C3, 0xB5, 0x345, 0x3D0, 0x1C80, 0x1C88, 0x1E9B, 0x1F80} <= set(closure)
    seen, sample = context_code_points()
    assert len(seen) == 6217 and sum(c >= 0x80 for c in seen) == 6160 and len(sample) == 600
    assert len(scripts("closure")) == 4 * 113
    for family in FAMILIES:
        assert all(s.endswith("&& a()") for s in scripts(family))


@pytest.mark.parametrize("family", list(FAMILIES))
def test_host_walk_matches_oracle_and_generator(form, family):
    docs = [review(v, f"uid-{v or 'none'}") for v in VECTORS]
    b = K.Batch.from_json(docs)
    for k, rows in enumerate(chunks(family)):
        doc = groups_doc(rows)
        env = K.EvaluationEnvironment(doc, continue_on_errors=True)
        oe = oracle_env(family, k)
        ids = env.policy_ids()
        assert ids == [p["id"] for p in oe.pol]
        for g in range(len(rows)):
            env.validate_settings(f"g{g}")
            assert oe.pol[oe.ids[f"g{g}"]]["valid"], (rows[g], oe.pol[oe.ids[f"g{g}"]]["expr_error"])
        for origin in (K.AUDIT, K.VALIDATE):
            got = b.debug_host_walk(env, ids, origin)
            want = oe.eval(b.view(), ids, origin)
            assert np.array_equal(got, want), diff_verdicts(got, want, len(ids), ids)
        v = got.reshape(len(docs), len(ids))
        for g, expr in enumerate(rows):  # what the generator says: allowed with a, cause a without
            j = ids.index(f"g{g}")
            members = env.group_members(j)
            for r, exp in ((0, ("causes", {"a"})), (1, True)):
                resp = b.format_response(env, r, j, int(v[r, j]), [int(v[r, m]) for m in members], doc=docs[r])
                assert resp == oe.response_doc(b.view(), r, j, K.VALIDATE, doc=docs[r]), (expr, VECTORS[r])
                check_expected(resp, exp, (form, expr, VECTORS[r]))


@pytest.mark.parametrize("family", list(FAMILIES))
def test_generator_is_not_vacuous(form, family):
    """The expected number plus one: product and oracle reject with `a` present (and name no cause:
    the script never reaches a())."""
    import oracle as O
    rows = scripts(family, bump=1)
    picks = sorted({0, 1, len(rows) // 3, len(rows) // 2, len(rows) - 1})
    if family == "closure":  # "a" + σ: the context in which Σ's final form appears
        picks.append(next(k for k, s in enumerate(rows) if s.startswith('let s = "a" + "σ";')))
    rows = [rows[k] for k in picks]
    assert not set(rows) & set(scripts(family))
    doc = groups_doc(rows)
    env = K.EvaluationEnvironment(doc, continue_on_errors=True)
    oe = O.OracleEnv(doc, continue_on_errors=True)
    ids = env.policy_ids()
    docs = [review(v, f"uid-{v or 'none'}") for v in VECTORS]
    b = K.Batch.from_json(docs)
    got = b.debug_host_walk(env, ids, K.VALIDATE)
    want = oe.eval(b.view(), ids, K.VALIDATE)
    assert np.array_equal(got, want), diff_verdicts(got, want, len(ids), ids)
    v = got.reshape(len(docs), len(ids))
    for g, expr in enumerate(rows):
        j = ids.index(f"g{g}")
        members = env.group_members(j)
        assert not int(v[1, j]) & ALLOWED, expr
        resp = b.format_response(env, 1, j, int(v[1, j]), [int(v[1, m]) for m in members], doc=docs[1])
        check_expected(resp, ("causes", set()), (form, expr))
