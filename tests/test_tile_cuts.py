"""Block-aware tile cuts (pass.cpp build_descs, kernels.hpp tile_cost / tile_slot), on the host
through kw_debug_tile_descs.

For C4 batches of several sizes at three tile heights, and a C5 batch with a forced light / heavy
split: the descriptors and the overflow list cover every row once; a tile's rows are contiguous, at
most the geometry's height and within its capacities; the array is in row order; with KW_TILE_CUT=0
it is the fixed cut, word for word (restated here from the batch's offsets); the cuts do not raise
the estimated total cost, nor the tiles of the busiest slot; two builds agree. The cost and slot
helpers are also compared with plain restatements.
(r08 also built a balanced static order of the descriptors; it measured slower on the GPU and was
removed, so there is no permutation to check: DESIGN.md §10.)
"""
import ctypes as C

import numpy as np
import pytest

import kwgpu as K
from helpers import config

NS = "kubewarden"
STR_COLS = ["ns", "ctr_image", "ctr_apparmor", "cap_add", "cap_drop", "lbl_key", "lbl_val"]
W_DESC = 34  # words per descriptor in the record: 32 descriptor words, cost low / high
# kernels.hpp tile_cost_weights, label / container families (C4, C5): fixed, request, label,
# container and capability-string block
C4_WEIGHTS = (47000, 8450, 9960, 10600, 2750)
FEAT_IMG, FEAT_LBL, FEAT_CTR = 1, 2, 4
ALL_STRINGS = 0x7f

_envs = {}


def env_of(name):
    if name not in _envs:
        _envs[name] = K.EvaluationEnvironment(config(name), continue_on_errors=True, always_accept_namespace=NS)
    return _envs[name]


class Cols:
    """The offsets of a batch (in device-row order) as numpy arrays."""

    def __init__(self, b):
        s = b.view()
        self._keep = (b, s)
        n = self.n = int(s.n_requests)
        arr = lambda p, k: np.ctypeslib.as_array(p, (k,)).astype(np.int64) if k else np.zeros(0, np.int64)  # noqa: E731
        self.ctr_off = arr(s.ctr_off, n + 1)
        self.lbl_off = arr(s.lbl_off, n + 1)
        nc = int(self.ctr_off[n])
        self.capadd_off = arr(s.capadd_off, nc + 1)
        self.capdrop_off = arr(s.capdrop_off, nc + 1)
        self.str_off = [arr(getattr(s, c).off, int(getattr(s, c).n) + 1) for c in STR_COLS]

    def str_range(self, m, r0, r1):
        cb, ce = self.ctr_off[r0], self.ctr_off[r1]
        if m == 0:
            return r0, r1
        if m == 3:
            return self.capadd_off[cb], self.capadd_off[ce]
        if m == 4:
            return self.capdrop_off[cb], self.capdrop_off[ce]
        if m in (5, 6):
            return self.lbl_off[r0], self.lbl_off[r1]
        return cb, ce

    def desc(self, g, r0, r1):
        """The 32 descriptor words of requests [r0, r1) under region geometry g (kernels.hpp TileDesc)."""
        d = [0] * 32
        cb, ce = int(self.ctr_off[r0]), int(self.ctr_off[r1])
        d[0:8] = [cb, ce, int(self.lbl_off[r0]), int(self.lbl_off[r1]), int(self.capadd_off[cb]), int(self.capadd_off[ce]),
                  int(self.capdrop_off[cb]), int(self.capdrop_off[ce])]
        fits = d[1] - d[0] <= g["cmax"] and d[5] - d[4] <= g["kmax"] and d[7] - d[6] <= g["kmax"] and d[3] - d[2] <= g["lmax"]
        for m in range(7):
            if not g["staged"][m]:
                continue
            g0, g1 = (int(x) for x in self.str_range(m, r0, r1))
            off = self.str_off[m]
            d[8 + m] = int(off[g0]) & ~15
            d[16 + m] = (((int(off[g1]) + 15) & ~15) - d[8 + m]) // 16
            fits = fits and d[16 + m] * 16 <= g["sb_cap"][m]
        d[23] = 1 if fits else 0
        d[24], d[25], d[26] = r0 & 0xffffffff, r0 >> 32, r1 - r0
        return d

    def fixed_cut(self, g):
        """Descriptors and overflow rows of the fixed cut: tiles of g["rows"] rows from the region's
        first row, a run beyond the capacities halved until its parts fit, single requests that still
        do not fit on the overflow list."""
        out, ovf = [], []
        for t0 in range(g["lo"], g["hi"], g["rows"]):
            todo = [(t0, min(g["hi"], t0 + g["rows"]))]
            while todo:
                r0, r1 = todo.pop()
                d = self.desc(g, r0, r1)
                if d[23]:
                    out.append(d)
                elif r1 - r0 > 1:
                    mid = r0 + (r1 - r0) // 2
                    todo += [(mid, r1), (r0, mid)]
                else:
                    ovf.append(r0)
        return out, ovf


def parse(w):
    """kw_debug_tile_descs' record (include/kwgpu.h) -> (regions, overflow rows)."""
    w = np.asarray(w, dtype=np.int64)
    nreg, novf = int(w[0]), int(w[1])
    at = 2
    regions = []
    for _ in range(nreg):
        g = dict(zip(("rows", "cmax", "kmax", "lmax", "grid", "nx", "dyn", "ndesc", "lo", "hi"), (int(x) for x in w[at:at + 10])))
        g["staged"] = [int(x) for x in w[at + 10:at + 17]]
        g["sb_cap"] = [int(x) for x in w[at + 17:at + 24]]
        at += 24
        g["d"] = w[at:at + W_DESC * g["ndesc"]].reshape(g["ndesc"], W_DESC)
        at += W_DESC * g["ndesc"]
        regions.append(g)
    ovf = [int(x) for x in w[at:at + novf]]
    assert at + novf == len(w)
    return regions, ovf


def r0_of(d):
    return d[:, 24] | (d[:, 25] << 32)


def cost_of(d):
    return d[:, 32] | (d[:, 33] << 32)


# ---- plain restatements of the two shared helpers
def py_blocks(items):
    return (items + 63) // 64


def py_cost(weights, nreq, nlbl, nctr, ncap):
    fixed, req, lbl, ctr, cap = weights
    return fixed + req * py_blocks(nreq) + lbl * py_blocks(nlbl) + ctr * py_blocks(nctr) + cap * py_blocks(ncap)


def py_slot(ndesc, grid, b):
    """(nx, xcd, slot, wpx, t_lo, t_hi): workgroup b runs on XCD b % nx as its slot b // nx; the XCD
    serves the contiguous descriptors [t_lo, t_hi) with wpx workgroups."""
    nx = min(8, grid)
    xcd = b % nx
    wpx = len(range(xcd, grid, nx))
    return nx, xcd, b // nx, wpx, ndesc * xcd // nx, ndesc * (xcd + 1) // nx


def py_tiles(ndesc, grid, b):
    """The descriptors workgroup b runs on the strided schedule, in its order."""
    nx, xcd, slot, wpx, t_lo, t_hi = py_slot(ndesc, grid, b)
    return list(range(t_lo + slot, t_hi, wpx))


def most_tiles(ndesc, grid):
    return max(len(py_tiles(ndesc, grid, b)) for b in range(grid))


# ---- the plans
def record(b, env, ids, monkeypatch, cut):
    monkeypatch.setenv("KW_TILE_CUT", cut)
    return b.debug_tile_descs(env, ids)


def check_plan(b, env, ids, monkeypatch, seen):
    dev, _perm, _split = b.debug_reorder()  # the rows as a resident pass sees them
    cols = Cols(dev)
    with_cuts = record(b, env, ids, monkeypatch, "1")
    assert np.array_equal(with_cuts, record(b, env, ids, monkeypatch, "1")), "two builds of one plan differ"
    fixed = record(b, env, ids, monkeypatch, "0")
    for name, rec in (("cut", with_cuts), ("fixed", fixed)):
        regions, ovf = parse(rec)
        covered = [(r, 1) for r in ovf]
        for g in regions:
            d = g["d"]
            assert (d[:, 23] == 1).all(), "only fitting tiles get a descriptor"
            r0, nr = r0_of(d), d[:, 26]
            assert ((nr >= 1) & (nr <= g["rows"])).all()
            assert ((r0 >= g["lo"]) & (r0 + nr <= g["hi"])).all()
            covered += list(zip(r0.tolist(), nr.tolist()))
            # a tile's words are those of its contiguous rows [r0, r0 + nr), and within the capacities
            for row in d if len(d) <= 400 else d[:: max(1, len(d) // 400)]:
                a = int(row[24] | (row[25] << 32))
                assert row[:32].tolist() == cols.desc(g, a, a + int(row[26]))
            assert (d[:, 1] - d[:, 0] <= g["cmax"]).all() and (d[:, 3] - d[:, 2] <= g["lmax"]).all()
            assert (d[:, 5] - d[:, 4] <= g["kmax"]).all() and (d[:, 7] - d[:, 6] <= g["kmax"]).all()
            for m in range(7):
                if g["staged"][m]:
                    assert (d[:, 16 + m] * 16 <= g["sb_cap"][m]).all()
            # the estimated cost is tile_cost over the tile's item counts
            want = [py_cost(C4_WEIGHTS, int(x[26]), int(x[3] - x[2]), int(x[1] - x[0]), int(x[5] - x[4] + x[7] - x[6])) for x in d]
            assert cost_of(d).tolist() == want
            assert g["nx"] == min(8, g["grid"])
            assert np.array_equal(r0, np.sort(r0)), "row order"
        nxt = 0
        for a, k in sorted(covered):  # every row once
            assert a == nxt
            nxt += k
        assert nxt == cols.n
    rc, _ = parse(with_cuts)
    rn, ovf_n = parse(fixed)
    for gc, gn in zip(rc, rn):
        # KW_TILE_CUT=0: the fixed cut, word for word, in row order
        want, want_ovf = cols.fixed_cut(gn)
        assert gn["d"][:, :32].tolist() == want
        seen["overflow"] += len(want_ovf)
        # the cuts do not raise the estimated total cost, nor the tiles of the launch's busiest slot
        total_cut, total_fixed = int(cost_of(gc["d"]).sum()), int(cost_of(gn["d"]).sum())
        assert total_cut <= total_fixed, (total_cut, total_fixed)
        assert most_tiles(gc["ndesc"], gc["grid"]) <= most_tiles(gn["ndesc"], gn["grid"])
        seen["cut_gain"].append(1.0 - total_cut / total_fixed)
        seen["shorter"] |= gc["ndesc"] > gn["ndesc"]
    assert sorted(ovf_n) == sorted(o for g in rn for o in cols.fixed_cut(g)[1])
    return rc


@pytest.mark.parametrize("height", [None, "8", "24"])
def test_c4_cuts(monkeypatch, height):
    if height:
        monkeypatch.setenv("KW_SLOT_ROWS", height)
    env = env_of("c4_64")
    ids = env.policy_ids()
    seen = {"overflow": 0, "cut_gain": [], "shorter": False}
    # (the cuts are kept only where they do not give the busiest slot a tile more than the fixed cut
    # does: at 64 rows that takes several tiles a slot, so one larger batch at that height)
    for n in (1, 63, 64, 65, 5003, 20000) + (() if height else (200000,)):
        regions = check_plan(K.SynthBatch(4, n, seed=20250509 + n).batch(), env, ids, monkeypatch, seen)
        assert len(regions) == 1 and regions[0]["rows"] == int(height or 64)
    print("estimated gain of the cuts per batch", ["%.4f" % g for g in seen["cut_gain"]])
    if not height:
        assert seen["shorter"], "no batch was cut into more tiles than the fixed height gives"
        assert seen["cut_gain"][-1] > 0.01  # ~2 % of the estimated tile work at 64 rows


def test_c5_forced_split_cuts_each_region(monkeypatch):
    monkeypatch.setenv("KW_SPLIT", "1")
    env = env_of("c5_mixed")
    ids = env.policy_ids()
    seen = {"overflow": 0, "cut_gain": [], "shorter": False}
    regions = check_plan(K.SynthBatch(5, 20000, seed=505).batch(), env, ids, monkeypatch, seen)
    assert len(regions) == 2 and regions[0]["hi"] == regions[1]["lo"]
    assert regions[0]["rows"] != regions[1]["rows"] or regions[0]["cmax"] != regions[1]["cmax"]  # each its own geometry


def test_halved_tiles_and_overflow_survive_the_cuts(monkeypatch):
    """Capacities from the median tile: many tiles are halved, and the cut tiles still fit."""
    monkeypatch.setenv("KW_TILE_QUANTILE", "0.5")
    env = env_of("c4_64")
    seen = {"overflow": 0, "cut_gain": [], "shorter": False}
    check_plan(K.SynthBatch(4, 5003, seed=77).batch(), env, env.policy_ids(), monkeypatch, seen)


def test_cost_helper_matches_a_plain_restatement():
    L = K.library()
    counts = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000)
    both = FEAT_LBL | FEAT_CTR
    for nreq in (1, 56, 64, 65, 128):
        for nlbl in counts:
            for nctr in counts:
                for ncap in (0, 1, 64, 65, 200):
                    assert L.kw_debug_tile_cost(both, ALL_STRINGS, nreq, nlbl, nctr, ncap) == \
                        py_cost(C4_WEIGHTS, nreq, nlbl, nctr, ncap)
    fixed, req, lbl, ctr, cap = C4_WEIGHTS
    # a family the launch does not carry, or a column it does not classify, costs nothing
    assert L.kw_debug_tile_cost(FEAT_LBL, ALL_STRINGS, 64, 130, 130, 130) == py_cost((fixed, req, lbl, 0, 0), 64, 130, 130, 130)
    assert L.kw_debug_tile_cost(FEAT_CTR, ALL_STRINGS, 64, 130, 130, 130) == py_cost((fixed, req, 0, ctr, cap), 64, 130, 130, 130)
    assert L.kw_debug_tile_cost(both, ALL_STRINGS & ~(1 << 3), 64, 130, 130, 130) == py_cost((fixed, req, lbl, ctr, 0), 64, 130, 130, 130)
    assert L.kw_debug_tile_cost(both, ALL_STRINGS & ~(1 << 5), 64, 130, 130, 130) == py_cost((fixed, req, 0, ctr, cap), 64, 130, 130, 130)
    # the image family: a container block also pays its image chains
    assert L.kw_debug_tile_cost(both | FEAT_IMG, ALL_STRINGS, 64, 130, 130, 130) > L.kw_debug_tile_cost(both, ALL_STRINGS, 64, 130, 130, 130)
    # whole blocks: an item more in a full block costs a block, an item fewer saves nothing
    assert L.kw_debug_tile_cost(both, ALL_STRINGS, 64, 128, 128, 192) == L.kw_debug_tile_cost(both, ALL_STRINGS, 64, 65, 65, 129)
    assert L.kw_debug_tile_cost(both, ALL_STRINGS, 64, 129, 128, 192) - L.kw_debug_tile_cost(both, ALL_STRINGS, 64, 128, 128, 192) == lbl


@pytest.mark.parametrize("grid", [1, 7, 8, 9, 1024])
def test_slot_helper_matches_a_plain_restatement(grid):
    L = K.library()
    out = (C.c_uint64 * 7)()
    for ndesc in (0, 1, 5, grid - 1, grid, grid + 1, 3 * grid + 2, 16750, (1 << 33) + 5):
        owner = np.zeros(ndesc if ndesc < (1 << 16) else 0, dtype=np.int64)
        for b in range(grid):
            assert L.kw_debug_tile_slot(ndesc, grid, b, 0, out) == 0
            assert tuple(out[:6]) == py_slot(ndesc, grid, b)
            mine = py_tiles(ndesc, grid, b) if ndesc < (1 << 16) else []
            for k in sorted(set(range(len(mine))) & {0, 1, 2, len(mine) - 1}):
                assert L.kw_debug_tile_slot(ndesc, grid, b, k, out) == 0 and out[6] == mine[k]
            # the tile after a slot's last is outside the XCD's range
            assert L.kw_debug_tile_slot(ndesc, grid, b, len(mine), out) == 0 and (ndesc >= (1 << 16) or out[6] >= out[5])
            owner[mine] += 1
        assert (owner == 1).all(), "every descriptor belongs to exactly one slot"
    assert L.kw_debug_tile_slot(10, grid, grid, 0, out) != 0
