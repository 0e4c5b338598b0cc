"""CPU: the planner (plan.cpp plan_pass, through kw_debug_plan) gives the plans recorded in
tests/golden/plan_words.json: all 16 words, for every configuration at 5,000 and 50,000 requests
(c2_trusted also at 600,000, the taller-tile branch), under each setting of the live planning knobs.
A plan that fails records its return code.

The file holds what the library planned before plan_pass became a file of its own (plan.cpp). The test only
reads it. `PYTHONPATH=policy-server_amd:tests python tests/test_plan_golden.py` rewrites it from the
library KWGPU_LIB names, which must be a build of a commit whose plans are known good (never the
code under test).
"""
import contextlib
import json
import os

import pytest

import kwgpu as K
from helpers import GOLDEN, config

PATH = os.path.join(GOLDEN, "plan_words.json")
CASES = [("parity", 0), ("c1_namespace", 1), ("c2_trusted", 2), ("c3_group", 3), ("c4_64", 4), ("c5_mixed", 5),
         ("c6_256", 6)]
SIZES = {name: (5_000, 50_000) for name, _ in CASES}
SIZES["c2_trusted"] += (600_000,)
KNOBS = [{}, {"KW_SLOT_ROWS": "8"}, {"KW_SLOT_ROWS": "96"}, {"KW_GLOBAL_TABLES": "1"}, {"KW_TILE_QUANTILE": "0.5"},
         {"KW_TILE_SPLIT": "0.2"}, {"KW_ROUND_SPLIT": "0"}, {"KW_SPLIT": "0"}, {"KW_SPLIT": "1"},
         {"KW_SPLIT": "1", "KW_HEAVY_ROWS": "12"}, {"KW_HEAVY_CTR": "3"}, {"KW_GROUP_FORM": "script"}]
LIVE = sorted({k for kn in KNOBS for k in kn})


@contextlib.contextmanager
def knobs(kn):
    saved = {k: os.environ.pop(k, None) for k in LIVE}
    os.environ.update(kn)
    try:
        yield
    finally:
        for k in LIVE:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def label(kn):
    return ",".join(f"{k}={v}" for k, v in kn.items()) or "none"


def plans(name, scfg):
    """{"<rows>/<knobs>": the 16 plan words, or [return code]} of one configuration."""
    out = {}
    batches = {n: K.SynthBatch(scfg, n, seed=1).batch() for n in SIZES[name]}
    for kn in KNOBS:
        with knobs(kn):
            # (a new environment per setting: KW_GROUP_FORM is read when the groups compile)
            env = K.EvaluationEnvironment(config(name), continue_on_errors=True, always_accept_namespace="kubewarden")
            ids = env.policy_ids()
            for n, b in batches.items():
                try:
                    words = [int(w) for w in b.debug_plan(env, ids).values()]
                except K.EvaluationError as e:
                    words = [int(e.code)]
                out[f"{n}/{label(kn)}"] = words
    return out


@pytest.mark.parametrize("name,scfg", CASES)
def test_plan_words(name, scfg):
    with open(PATH) as f:
        want = json.load(f)[name]
    got = plans(name, scfg)
    assert len(got) == len(SIZES[name]) * len(KNOBS) and got.keys() == want.keys()
    diff = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not diff, diff


if __name__ == "__main__":
    import kwgpu._native as N
    print("library:", N.LIB_PATH)
    doc = {name: plans(name, scfg) for name, scfg in CASES}
    with open(PATH, "w") as f:  # one plan per line
        f.write("{\n" + ",\n".join(
            json.dumps(name) + ": {\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(w)}" for k, w in sorted(doc[name].items()))
            + "\n}" for name in sorted(doc)) + "\n}\n")
