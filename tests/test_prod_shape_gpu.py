"""GPU parity of the production-shape tile kernels (kernels.hip evaluate_tiles_kernel's PROD;
DESIGN.md §5): the verdict words of a pass that takes them are bit-exact against the oracle and
against the same pass on the generic kernel (KW_TILE_GENERIC=1), and each pass is asked which kernel
its launches took (kw_debug_last_kernels), so no case can pass on the other path. Every pass starts
from poisoned verdict words: a word no tile wrote keeps the sentinel.

Cases: 8-row tiles (many tiles), 64-row tiles one of which holds more than 256 labels (the fifth
label block), bypassed namespaces beside a request beyond the tile capacities (the overflow list
stays on its own kernels), a forced light / heavy split (the heavy region's launch is the kFeatRng
kernel), the counter-drawn tail, and launches that must not qualify (several chunks; an ablation bit).
"""
import ctypes as C
import os

import numpy as np
import pytest

import kwgpu as K
import oracle as O
from helpers import config, diff_verdicts
from test_label_steal import MIXES, steal_docs

pytestmark = pytest.mark.gpu
NS = "kubewarden"
PROD, GENERIC = K.KERNEL_PROD, K.KERNEL_GENERIC

_cache = {}


def _envs(name):
    if name not in _cache:
        doc = config(name)
        _cache[name] = (K.EvaluationEnvironment(doc, continue_on_errors=True, always_accept_namespace=NS, device=0),
                        O.OracleEnv(doc, continue_on_errors=True, always_accept_namespace=NS))
    return _cache[name]


def _threads():
    return max(1, min(16, len(os.sched_getaffinity(0))))


@pytest.fixture(autouse=True)
def _knobs(monkeypatch):
    monkeypatch.setenv("KW_POISON_VERDICTS", "1")
    for k in ("KW_TILE_GENERIC", "KW_TILE_DEBUG", "KW_SLOT_ROWS", "KW_SPLIT", "KW_SCHED", "KW_SCHED_TAIL"):
        monkeypatch.delenv(k, raising=False)


def _both_kernels(monkeypatch, b, env, ids, origin, ora, want):
    """One pass as the settings stand (its launches must have taken the kernels `want`), one on the
    generic kernel; both equal to the oracle's words, hence to each other. Returns the launches."""
    b.validate(env, ids, origin)
    kernels, launches = b.debug_last_kernels(), b.debug_last_launches()
    assert kernels == want and len(launches) == len(kernels), (kernels, want, launches)
    got = b.verdicts()
    assert np.array_equal(got, ora), "production shape: " + diff_verdicts(got, ora, len(ids), ids)
    monkeypatch.setenv("KW_TILE_GENERIC", "1")
    b.validate(env, ids, origin)
    assert b.debug_last_kernels() == [GENERIC] * len(want)
    gen = b.verdicts()
    monkeypatch.delenv("KW_TILE_GENERIC")
    assert np.array_equal(gen, ora), "generic: " + diff_verdicts(gen, ora, len(ids), ids)
    assert np.array_equal(got, gen)
    return launches


@pytest.mark.parametrize("n", [600, 40_000])
def test_c4_short_tiles(monkeypatch, n):
    """8-row tiles. 600 requests: 75 tiles, a tile per slot, the plain kernel; 40,000: 5,000 tiles,
    more than two per slot of the strided schedule at any grid the device may hold (at most 2,048
    workgroups of this layout), and tiles of more than 32 containers, which at 8 rows is the
    planner's threshold for predecessor ranges: the launch is the kFeatRng kernel's."""
    monkeypatch.setenv("KW_SLOT_ROWS", "8")
    env, oe = _envs("c4_64")
    ids = env.policy_ids()
    syn = K.SynthBatch(4, n, seed=1301)
    b = syn.batch().to_device(0)
    for cols, origin in ((ids, K.VALIDATE), (ids[::-1], K.AUDIT)):
        ora = oe.eval(syn.soa(), cols, origin, threads=_threads())
        (grid, ndesc, _), = _both_kernels(monkeypatch, b, env, cols, origin, ora, [PROD])
        assert n < 40_000 or ndesc > 2 * grid, (grid, ndesc)
    b.close()


@pytest.mark.parametrize("origin", [K.VALIDATE, K.AUDIT])
def test_c4_tall_tiles_with_a_fifth_label_block(monkeypatch, origin):
    """600 requests of four or five labels in 64-row tiles: tiles of 256-320 labels."""
    env, oe = _envs("c4_64")
    ids = env.policy_ids()
    b = K.Batch.from_json(steal_docs(MIXES["few"], n=600, seed=23, five=0.8)).to_device(0)
    plan = b.debug_plan(env, ids, origin)
    assert plan["chunks"] == 1 and plan["rows"] == 64 and 256 < plan["lmax"] <= 320, plan
    ora = oe.eval(b.view(), ids, origin)
    _both_kernels(monkeypatch, b, env, ids, origin, ora, [PROD])
    b.close()


def test_c4_bypass_and_overflow(monkeypatch):
    """Every seventh request in the always-accepted namespace, and one request whose labels and
    containers exceed the tile capacities even alone: it runs on the overflow kernels."""
    env, oe = _envs("c4_64")
    ids = env.policy_ids()
    docs = steal_docs(MIXES["few"], n=600, seed=29, five=0.3)
    for r in range(0, 600, 7):
        docs[r]["request"]["namespace"] = NS
    # (its one container keeps the tiles' container capacity low: the launch stays the plain kernel's,
    # not the kFeatRng one's, which the split and the 8-row cases run)
    docs[301]["request"]["object"]["metadata"]["labels"] = {f"k{i}": ("prod" if i % 3 else "x" * 20) for i in range(20_000)}
    b = K.Batch.from_json(docs).to_device(0)
    assert b.debug_tile_descs(env, ids)[1] >= 1, "no request went to the overflow list: the case tests nothing"
    assert b.debug_plan(env, ids)["scan_regions"] == 0
    for origin in (K.VALIDATE, K.AUDIT):
        ora = oe.eval(b.view(), ids, origin)
        _both_kernels(monkeypatch, b, env, ids, origin, ora, [PROD])
    b.close()


def test_c5_split_regions(monkeypatch):
    """A forced light / heavy split: the light region's launch takes the plain production kernel,
    the heavy region's the kFeatRng one."""
    monkeypatch.setenv("KW_SPLIT", "1")
    env, oe = _envs("c5_mixed")
    ids = env.policy_ids()
    syn = K.SynthBatch(5, 600, seed=1305)
    assert 0 < syn.batch().debug_reorder()[2] < 600
    b = syn.batch().to_device(0)
    plan = b.debug_plan(env, ids)
    assert plan["regions"] == 2 and plan["scan_regions"] == 2 and plan["launches"] == 1, plan
    for cols, origin in ((ids, K.VALIDATE), (ids[::-1], K.AUDIT)):
        ora = oe.eval(syn.soa(), cols, origin, threads=_threads())
        _both_kernels(monkeypatch, b, env, cols, origin, ora, [PROD, PROD])
    b.close()


def test_c4_counter_drawn_tail(monkeypatch):
    """The tail forced as tests/test_sched_tail_gpu.py forces it: 8-row tiles, KW_SCHED_TAIL, a
    batch with two static rounds beside the tail at any grid the device may hold."""
    monkeypatch.setenv("KW_SLOT_ROWS", "8")
    monkeypatch.setenv("KW_SCHED_TAIL", "3")
    env, oe = _envs("c4_64")
    ids = env.policy_ids()
    syn = K.SynthBatch(4, 98_304, seed=1307)
    b = syn.batch().to_device(0)
    ora = oe.eval(syn.soa(), ids, K.VALIDATE, threads=_threads())
    (grid, ndesc, S), = _both_kernels(monkeypatch, b, env, ids, K.VALIDATE, ora, [PROD])
    out = (C.c_uint64 * 7)()
    assert K.library().kw_debug_sched_tail(ndesc, grid, 0, 2, out) == 0
    assert S >= 2 and S == int(out[6]) - 3, ("the launch took no tail: the case tests nothing", grid, ndesc, S, int(out[6]))
    b.close()


def test_c6_several_chunks_stay_generic(monkeypatch):
    env, oe = _envs("c6_256")
    ids = env.policy_ids()
    syn = K.SynthBatch(6, 600, seed=1309)
    b = syn.batch().to_device(0)
    assert b.debug_plan(env, ids)["chunks"] > 1
    b.validate(env, ids, K.VALIDATE)
    kernels = b.debug_last_kernels()
    assert kernels and kernels == [GENERIC] * len(kernels), kernels
    got = b.verdicts()
    ora = oe.eval(syn.soa(), ids, K.VALIDATE, threads=_threads())
    assert np.array_equal(got, ora), diff_verdicts(got, ora, len(ids), ids)
    b.close()


def test_c4_ablation_bit_stays_generic(monkeypatch):
    """KW_TILE_DEBUG=16384 (no container / label violation words) disqualifies the launch. An
    ablated pass writes words the oracle does not describe, so the check against the oracle is on
    a second, unablated pass over the same resident batch, which takes the production kernel again
    (the launch that must not qualify and still equals the oracle is C6's, above)."""
    env, oe = _envs("c4_64")
    ids = env.policy_ids()
    syn = K.SynthBatch(4, 600, seed=1311)
    b = syn.batch().to_device(0)
    monkeypatch.setenv("KW_TILE_DEBUG", "16384")
    b.validate(env, ids, K.VALIDATE)
    assert b.debug_last_kernels() == [GENERIC]
    monkeypatch.delenv("KW_TILE_DEBUG")
    ora = oe.eval(syn.soa(), ids, K.VALIDATE, threads=_threads())
    _both_kernels(monkeypatch, b, env, ids, K.VALIDATE, ora, [PROD])
    b.close()
