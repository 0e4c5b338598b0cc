"""The counter-drawn tail of the tile schedule, host side (kernels.hpp tile_tail_lo /
tile_whole_rounds, plan.cpp sched_static_rounds) through kw_debug_sched_tail / kw_debug_sched_rounds.

With S static rounds a slot's first S tiles are its strided ones and the XCD's counter hands out
the rest of the XCD's range. Checked against a plain restatement, exhaustively over small and odd
grids and descriptor counts: every descriptor is exactly one slot's static tile or lies in exactly
one XCD's tail, never both or neither; S = q (the launch's whole rounds) leaves less than a round
on the XCD that has fewest rounds; the rule that picks S per launch never gives more than q, gives
no counter below its least round count, and obeys KW_SCHED / KW_SCHED_TAIL.
"""
import ctypes as C

import numpy as np
import pytest

import kwgpu as K

GRIDS = [1, 3, 7, 8, 9, 64, 1000, 1024]
TAIL, MIN_ROUNDS = 2, 7  # plan.cpp kSchedTail, kSchedTailMinRounds


def ndescs(grid):
    return sorted({n for n in (0, 1, grid - 1, grid, grid + 1, 2 * grid - 1, 2 * grid + 1, 15 * grid + 617, 16 * grid) if n >= 0})


def py_ranges(ndesc, grid):
    """Per XCD (t_lo, t_hi, wpx): workgroup b runs on XCD b % nx, the XCD serves [t_lo, t_hi)."""
    nx = min(8, grid)
    return [(ndesc * x // nx, ndesc * (x + 1) // nx, len(range(x, grid, nx))) for x in range(nx)]


def py_rounds(ndesc, grid):
    return min((hi - lo) // wpx for lo, hi, wpx in py_ranges(ndesc, grid))


def sched_tail(L, ndesc, grid, b, S):
    out = (C.c_uint64 * 7)()
    assert L.kw_debug_sched_tail(ndesc, grid, b, S, out) == 0
    return tuple(int(v) for v in out)


def rounds_of(L, ndesc, grid, dyn):
    r = C.c_int(-7)
    assert L.kw_debug_sched_rounds(ndesc, grid, int(dyn), C.byref(r)) == 0
    return r.value


@pytest.mark.parametrize("grid", GRIDS)
def test_static_tiles_and_tails_cover_every_descriptor_once(grid):
    L = K.library()
    nx = min(8, grid)
    for ndesc in ndescs(grid):
        ranges = py_ranges(ndesc, grid)
        q = py_rounds(ndesc, grid)
        for S in sorted({0, 1, 2, max(q - 1, 0), q}):
            static = np.zeros(ndesc, dtype=np.int64)
            tail = np.zeros(ndesc, dtype=np.int64)
            for b in range(grid):
                t_lo, slot, wpx, nstatic, tail_lo, t_hi, rounds = sched_tail(L, ndesc, grid, b, S)
                lo, hi, w = ranges[b % nx]
                assert (t_lo, slot, wpx, t_hi, rounds) == (lo, b // nx, w, hi, q)
                assert tail_lo == min(lo + S * w, hi)
                mine = [lo + slot + k * w for k in range(S) if lo + slot + k * w < hi]
                assert nstatic == len(mine) and all(t < tail_lo for t in mine)
                if S <= q:
                    assert nstatic == S, "within the whole rounds every static tile exists"
                static[mine] += 1
                if b < nx:  # the XCD's tail, once per XCD
                    tail[tail_lo:t_hi] += 1
                    if S == q:
                        assert t_hi - tail_lo < ((hi - lo) // w - q + 1) * w, "S = q: less than a round beyond the XCD's own extra rounds"
            assert ((static + tail) == 1).all(), (grid, ndesc, S)
        if ndesc:
            short = [hi - min(lo + q * w, hi) < w for lo, hi, w in ranges if (hi - lo) // w == q]
            assert short and all(short)
    out = (C.c_uint64 * 7)()
    assert L.kw_debug_sched_tail(10, grid, grid, 2, out) != 0


@pytest.mark.parametrize("grid", GRIDS)
def test_rule_picks_static_rounds_within_the_whole_rounds(monkeypatch, grid):
    L = K.library()
    monkeypatch.delenv("KW_SCHED", raising=False)
    counts = set(ndescs(grid)) | {k * grid + d for k in (3, 4, 5, MIN_ROUNDS - 1, MIN_ROUNDS, 33) for d in (-1, 0, 7)}
    for ndesc in sorted(n for n in counts if n >= 0):
        q = py_rounds(ndesc, grid)
        # the default: a tail for strided launches of enough rounds, today's choice otherwise
        monkeypatch.delenv("KW_SCHED_TAIL", raising=False)
        assert rounds_of(L, ndesc, grid, True) == 2
        S = rounds_of(L, ndesc, grid, False)
        if q < MIN_ROUNDS:
            assert S == -1, "no counter below the least round count"
        else:
            assert S == q - TAIL and 2 <= S <= q
        # 0: today's choice exactly
        monkeypatch.setenv("KW_SCHED_TAIL", "0")
        assert rounds_of(L, ndesc, grid, False) == -1 and rounds_of(L, ndesc, grid, True) == 2
        # forced: T rounds of tail wherever two static rounds are left beside them
        for T in (1, 3, 4):
            monkeypatch.setenv("KW_SCHED_TAIL", str(T))
            for dyn in (False, True):
                S = rounds_of(L, ndesc, grid, dyn)
                if q >= T + 2:
                    assert S == q - T and 2 <= S <= q
                else:
                    assert S == (2 if dyn else -1)
        # KW_SCHED forces its schedule whatever the tail setting
        monkeypatch.setenv("KW_SCHED", "static")
        assert rounds_of(L, ndesc, grid, False) == -1
        monkeypatch.setenv("KW_SCHED", "dynamic")
        assert rounds_of(L, ndesc, grid, True) == 2
        monkeypatch.delenv("KW_SCHED")
    r = C.c_int(0)
    assert L.kw_debug_sched_rounds(10, 0, 0, C.byref(r)) != 0
