"""GPU: passes over block-aware tile cuts (KW_TILE_CUT) give the oracle's verdict words bit for
bit, from poisoned verdict words (rows no tile covered keep the sentinel), with the knob on and
off, and the settings agree. One resident batch runs them in turn, so every switch goes through
the plan cache's key and the descriptor cache's key.
(The balanced static order r08 also built was removed after it measured slower; the file keeps the
name the r08 issue gave it.)
"""
import numpy as np
import pytest

import kwgpu as K
import oracle as O
from helpers import config, diff_verdicts

pytestmark = pytest.mark.gpu

NS = "kubewarden"
SETTINGS = ["1", "0", "1"]  # KW_TILE_CUT
SYNTH = {"c4_64": 4, "c2_trusted": 2, "c5_mixed": 5}

_cache = {}


@pytest.fixture(autouse=True)
def _poisoned_verdicts(monkeypatch):
    monkeypatch.setenv("KW_POISON_VERDICTS", "1")


def _envs(name):
    if name not in _cache:
        doc = config(name)
        _cache[name] = (K.EvaluationEnvironment(doc, continue_on_errors=True, always_accept_namespace=NS, device=0),
                        O.OracleEnv(doc, continue_on_errors=True, always_accept_namespace=NS))
    return _cache[name]


def _case(name, n):
    """(synthetic batch, oracle verdicts per origin) of n rows of config `name`, computed once."""
    key = (name, n)
    if key not in _cache:
        env, oe = _envs(name)
        syn = K.SynthBatch(SYNTH[name], n, seed=8000 + n)
        ids = env.policy_ids()
        _cache[key] = (syn, {o: oe.eval(syn.soa(), ids, o) for o in (K.VALIDATE, K.AUDIT)})
    return _cache[key]


def _settings(monkeypatch, name, n):
    env, _ = _envs(name)
    ids = env.policy_ids()
    syn, ora = _case(name, n)
    b = syn.batch().to_device(0)
    for origin in (K.VALIDATE, K.AUDIT):
        words = []
        for cut in SETTINGS:
            monkeypatch.setenv("KW_TILE_CUT", cut)
            b.validate(env, ids, origin)
            gpu = b.verdicts()
            assert np.array_equal(gpu, ora[origin]), (cut, diff_verdicts(gpu, ora[origin], len(ids), ids))
            words.append(gpu)
        for w in words[1:]:
            assert np.array_equal(w, words[0])
    return b, env, ids


# 200,000 rows: the smallest of these at which 64-row tiles come several to a slot, so that the cuts
# are kept (tests/test_tile_cuts.py)
@pytest.mark.parametrize("n", [1, 65, 5003, 20000, 200000])
def test_c4_default_geometry(monkeypatch, n):
    _settings(monkeypatch, "c4_64", n)


@pytest.mark.parametrize("n", [1, 65, 5003, 20000])
def test_c4_eight_row_tiles(monkeypatch, n):
    monkeypatch.setenv("KW_SLOT_ROWS", "8")
    _settings(monkeypatch, "c4_64", n)


def test_c2_image_instantiation(monkeypatch):
    _settings(monkeypatch, "c2_trusted", 5003)


def test_c5_forced_split(monkeypatch):
    monkeypatch.setenv("KW_SPLIT", "1")
    b, env, ids = _settings(monkeypatch, "c5_mixed", 20000)
    assert b.debug_plan(env, ids)["regions"] == 2


def test_back_to_back_batches_of_different_sizes(monkeypatch):
    """Two resident batches of different sizes take turns on one stream, the knobs switching between
    the passes: each pass must run its own batch's descriptors for its own setting (the descriptor
    cache's key holds the knob and the grid)."""
    import torch
    env, _ = _envs("c4_64")
    ids = env.policy_ids()
    (sa, oa), (sb, ob) = _case("c4_64", 200000), _case("c4_64", 5003)
    a, b = sa.batch().to_device(0), sb.batch().to_device(0)
    s = torch.cuda.Stream(device=0)
    for cut in SETTINGS:
        monkeypatch.setenv("KW_TILE_CUT", cut)
        a.validate(env, ids, K.VALIDATE, stream=s.cuda_stream)
        b.validate(env, ids, K.AUDIT, stream=s.cuda_stream)
        ga, gb = a.verdicts(), b.verdicts()
        assert np.array_equal(ga, oa[K.VALIDATE]), (cut, diff_verdicts(ga, oa[K.VALIDATE], len(ids), ids))
        assert np.array_equal(gb, ob[K.AUDIT]), (cut, diff_verdicts(gb, ob[K.AUDIT], len(ids), ids))
