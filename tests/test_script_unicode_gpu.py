"""GPU: the script string functions over the whole Unicode case tables, run by wide_groups_kernel
(groups.hip) through the typed bytecode of groupvm.hpp and each script's own char table. The
scripts are those of tests/script_unicode_cases.py (expected values from CPython's str.upper /
lower / strip): 2,795 case-mapped code points by value, 113 closure code points alone in four
contexts, the Final_Sigma context of 6,817 code points, White_Space and its look-alikes under trim.
Verdict words are poisoned first, so a skipped pair cannot pass; the device's words must equal the
oracle's word for word in both origins, and responses formatted from them the oracle's.

wide_groups_kernel gives consecutive threads consecutive groups of one row, so a wave runs the
scripts of a pass one after another: an environment holds at most script_unicode_cases.CHUNK groups."""
import numpy as np
import pytest

import kwgpu as K
from helpers import diff_verdicts
from script_unicode_cases import FAMILIES, VECTORS, chunks, groups_doc, oracle_env, review

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("family", list(FAMILIES))
def test_unicode_sweep_on_device(monkeypatch, family):
    monkeypatch.setenv("KW_POISON_VERDICTS", "1")
    monkeypatch.setenv("KW_GROUP_FORM", "script")
    docs = [review(VECTORS[k % len(VECTORS)], f"uid-{k}") for k in range(len(VECTORS) * 8)]
    b = K.Batch.from_json(docs).to_device(0)
    allowed = 0
    for k, rows in enumerate(chunks(family)):
        env = K.EvaluationEnvironment(groups_doc(rows), continue_on_errors=True, device=0)
        oe = oracle_env(family, k)
        ids = env.policy_ids()
        for origin in (K.VALIDATE, K.AUDIT):
            b.validate(env, ids, origin)
            got = b.verdicts()
            want = oe.eval(b.view(), ids, origin)
            assert np.array_equal(got, want), diff_verdicts(got, want, len(ids), ids)
        v = got.reshape(len(docs), len(ids))
        for g, expr in enumerate(rows):
            j = ids.index(f"g{g}")
            members = env.group_members(j)
            allowed += int(v[1, j] & K._native.KW_F_ALLOWED != 0) - int(v[0, j] & K._native.KW_F_ALLOWED != 0)
            for r in range(len(VECTORS)):
                resp = b.format_response(env, r, j, int(v[r, j]), [int(v[r, m]) for m in members], doc=docs[r])
                assert resp == oe.response_doc(b.view(), r, j, K.AUDIT, doc=docs[r]), (expr, VECTORS[r])
    # what the generator says: every group allows the row with label a and rejects the row without
    assert allowed == sum(len(rows) for rows in chunks(family))
