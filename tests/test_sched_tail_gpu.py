"""GPU parity of the tile schedule with a counter-drawn tail (kernels.hip, the tile loop; plan.cpp
sched_static_rounds): a launch's first rounds strided, its last KW_SCHED_TAIL rounds handed out by
the per-XCD counters. Tiles forced down to 8 requests; back-to-back passes over batches of very
different sizes, policy-list order and origin alternating, every pass from poisoned verdict words (a tile no slot ran keeps the sentinel) and
bit-exact against the oracle. Each pass is asked what it launched (kw_debug_last_launches: the
workgroups, the descriptors, the static rounds S) and the big batches' launches must really have
taken the forced tail, S = their whole rounds - tail, so the cases cannot pass on the strided path.

The planner lays 8-row tiles of these policy sets out at 8 workgroups a CU (a grid of 2048), and
the launch clamps that to what the device holds of the instantiation (4 a CU for the label /
container one: 1024 workgroups), so the rounds are taken from the launch, not from the plan. At 1024
workgroups 49 152 rows are 6 whole rounds (an XCD's tail is exactly the forced rounds, nothing
beyond) and 60 000 rows 7 and a part; 98 304 and 100 003 rows run beside them so that both forced
tails also fit where the device holds the planned 2048 (6 rounds there).
"""
import ctypes as C

import numpy as np
import pytest

import kwgpu as K
import oracle as O
from helpers import config, diff_verdicts

pytestmark = pytest.mark.gpu
NS = "kubewarden"
SIZES = [60_000, 1, 77, 5_003, 49_152, 98_304, 100_003]
TAILED = 98_304  # from here on both forced tails leave two static rounds, at the planned grid too

_cache = {}


def _envs(name):
    if name not in _cache:
        doc = config(name)
        _cache[name] = (K.EvaluationEnvironment(doc, continue_on_errors=True, always_accept_namespace=NS, device=0),
                        O.OracleEnv(doc, continue_on_errors=True, always_accept_namespace=NS))
    return _cache[name]


def _threads():
    import os
    return max(1, min(16, len(os.sched_getaffinity(0))))


def _whole_rounds(ndesc, grid):
    out = (C.c_uint64 * 7)()
    assert K.library().kw_debug_sched_tail(ndesc, grid, 0, 2, out) == 0
    return int(out[6])


def _check_launches(b, tail, must_tail):
    """What the pass just run launched: every launch with two static rounds beside the forced tail
    took it (S = whole rounds - tail, from the launched grid), every other one stayed strided; the
    static rounds per launch. must_tail: every launch has to have taken the tail."""
    launches = b.debug_last_launches()
    assert launches
    for grid, ndesc, S in launches:
        q = _whole_rounds(ndesc, grid)
        assert S == (q - tail if tail and q >= tail + 2 else -1), (grid, ndesc, S, q, tail)
        assert not must_tail or S >= 2, ("the launch took no tail: the case tests nothing", grid, ndesc, q)
    return [S for _, _, S in launches]


@pytest.fixture(autouse=True)
def _knobs(monkeypatch):
    monkeypatch.setenv("KW_POISON_VERDICTS", "1")
    monkeypatch.setenv("KW_SLOT_ROWS", "8")
    monkeypatch.delenv("KW_SCHED", raising=False)


@pytest.mark.parametrize("tail", ["1", "3"])
@pytest.mark.parametrize("name,scfg", [("c4_64", 4), ("c2_trusted", 2)])
def test_tail_schedule_covers_every_tile(monkeypatch, name, scfg, tail):
    monkeypatch.setenv("KW_SCHED_TAIL", tail)
    env, oe = _envs(name)
    ids = env.policy_ids()
    for k, n in enumerate(SIZES):
        syn = K.SynthBatch(scfg, n, seed=1900 + k)
        b = syn.batch().to_device(0)
        for cols, origin in ((ids, K.VALIDATE), (ids[::-1], K.AUDIT)):
            b.validate(env, cols, origin)
            _check_launches(b, int(tail), must_tail=n >= TAILED)
            gpu = b.verdicts()
            ora = oe.eval(syn.soa(), cols, origin, threads=_threads())
            assert np.array_equal(gpu, ora), f"{name} rows {n} tail {tail}: " + diff_verdicts(gpu, ora, len(cols), cols)
        b.close()


def test_tail_setting_switches_between_passes_on_one_batch(monkeypatch):
    """tail -> 0 -> another tail over one resident batch: the counters restart from zero each
    launch, and no S of an earlier pass is kept with the cached plan."""
    env, oe = _envs("c4_64")
    ids = env.policy_ids()
    syn = K.SynthBatch(4, 100_003, seed=1911)
    b = syn.batch().to_device(0)
    ora = oe.eval(syn.soa(), ids, K.VALIDATE, threads=_threads())
    seen = []
    for tail in ("3", "0", "1", "3"):
        monkeypatch.setenv("KW_SCHED_TAIL", tail)
        b.validate(env, ids, K.VALIDATE)
        seen.append(_check_launches(b, int(tail), must_tail=tail != "0"))
        gpu = b.verdicts()
        assert np.array_equal(gpu, ora), f"tail {tail}: " + diff_verdicts(gpu, ora, len(ids), ids)
    assert seen[1] == [-1] and seen[0] == seen[3] and seen[2] == [seen[0][0] + 2], seen
    b.close()


@pytest.mark.parametrize("tail", ["1", "3"])
def test_tail_schedule_on_a_split_batch(monkeypatch, tail):
    """A forced light / heavy split: two launches of different geometry share the counters, one
    after the other, each with its own S."""
    monkeypatch.setenv("KW_SCHED_TAIL", tail)
    monkeypatch.setenv("KW_SPLIT", "1")
    env, oe = _envs("c5_mixed")
    ids = env.policy_ids()
    n = 150_000  # at least 6 and 5 whole rounds of the light and the heavy region's launch
    syn = K.SynthBatch(5, n, seed=1921)
    assert 0 < syn.batch().debug_reorder()[2] < n
    b = syn.batch().to_device(0)
    for cols, origin in ((ids, K.VALIDATE), (ids[::-1], K.AUDIT)):
        b.validate(env, cols, origin)
        assert len(_check_launches(b, int(tail), must_tail=True)) >= 2  # the light and the heavy region
        gpu = b.verdicts()
        ora = oe.eval(syn.soa(), cols, origin, threads=_threads())
        assert np.array_equal(gpu, ora), f"tail {tail}: " + diff_verdicts(gpu, ora, len(cols), cols)
    b.close()
