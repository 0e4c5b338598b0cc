"""The summary form (include/kwgpu.h kw_summary; policy-server_amd/csrc/summary.hpp) on the host:
verdict words of the host walk go through the reference reducer (kw_debug_summarize_words) and must
equal counters and plane bits worked out here in numpy (shifts, masks, np.add.at); the invariants
that tie counters and planes together hold; hand-made rows pin the poison word's bucket.
tests/summary_check.cpp runs the reducer and the reduction kernel's geometry as a plain executable
under AddressSanitizer and UBSan (no Python in that process)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import kwgpu as K
from helpers import config
from kwgpu import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "policy-server_amd")
CXX = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
NS = "kubewarden"
ROWS = 2000
_cache = {}


def _env(name):
    if name not in _cache:
        _cache[name] = K.EvaluationEnvironment(config(name), continue_on_errors=True, always_accept_namespace=NS)
    return _cache[name]


def _walk(name, scfg, ids, origin, rows=ROWS):
    key = (name, scfg, len(ids), origin, rows)
    if key not in _cache:
        _cache[key] = K.SynthBatch(scfg, rows, seed=7100 + scfg).batch().debug_host_walk(_env(name), ids, origin)
    return _cache[key]


def numpy_summary(words, npol):
    """(col [npol][32], planes [rows][G][2]) of words [rows][npol] by the definitions of kwgpu.h."""
    w = np.asarray(words, dtype=np.uint32).reshape(-1, npol)
    rows, G = w.shape[0], (npol + 63) // 64
    col = np.zeros((npol, N.KW_SUM_N), dtype=np.uint64)
    for k, bit in ((N.KW_SUM_F_ALLOWED, N.KW_F_ALLOWED), (N.KW_SUM_V_ALLOWED, N.KW_V_ALLOWED),
                   (N.KW_SUM_V_MUTATED, N.KW_V_MUTATED), (N.KW_SUM_F_PATCH, N.KW_F_PATCH), (N.KW_SUM_BYPASS, N.KW_BYPASS)):
        col[:, k] = ((w & np.uint32(bit)) != 0).sum(axis=0)
    st = (w & np.uint32(N.KW_F_STATUS_MASK)) >> np.uint32(N.KW_F_STATUS_SHIFT)
    for v, k in ((1, N.KW_SUM_FST_VANILLA), (2, N.KW_SUM_FST_MUTATION_REFUSED), (3, N.KW_SUM_FST_INIT_ERROR)):
        col[:, k] = (st == v).sum(axis=0)
    reason = ((w >> np.uint32(8)) & np.uint32(0xFF)).astype(np.int64)
    bucket = np.where(reason <= 15, N.KW_SUM_REASON + reason, N.KW_SUM_REASON_OTHER)
    cols = np.broadcast_to(np.arange(npol), w.shape)
    np.add.at(col, (cols.reshape(-1), bucket.reshape(-1)), np.uint64(1))
    planes = np.zeros((rows, G, 2), dtype=np.uint64)
    # (a word of the "other" bucket, which no product word is, sets both bits)
    for h, bits in ((0, ((w & np.uint32(N.KW_F_ALLOWED)) == 0) | (reason > 15)), (1, reason != 0)):
        pad = np.zeros((rows, G * 64), dtype=np.uint64)
        pad[:, :npol] = bits
        planes[:, :, h] = (pad.reshape(rows, G, 64) << np.arange(64, dtype=np.uint64)[None, None, :]).sum(axis=2, dtype=np.uint64)
    return col, planes


def popcount(a):
    return np.unpackbits(np.ascontiguousarray(a).view(np.uint8)).reshape(a.shape + (64,)).sum(axis=-1)


def check_invariants(col, planes, rows, npol):
    """What ties the counters and the planes of any pass together."""
    col = col.astype(np.int64)
    assert (col[:, 9:16] == 0).all()
    assert (col[:, N.KW_SUM_REASON:].sum(axis=1) + col[:, N.KW_SUM_REASON_OTHER] == rows).all()
    if planes is None:
        return
    G = (npol + 63) // 64
    assert planes.shape == (rows, G, 2)
    bits = ((planes[:, :, None, :] >> np.arange(64, dtype=np.uint64)[None, None, :, None]) & np.uint64(1)).astype(np.int64)
    per_col = bits.reshape(rows, G * 64, 2).sum(axis=0)  # [column][plane]
    assert (per_col[npol:] == 0).all()  # the padding bits
    product = col[:, N.KW_SUM_REASON_OTHER] == 0  # (an "other" word sets plane 0 whatever its F_ALLOWED bit)
    assert (col[:, N.KW_SUM_F_ALLOWED] + per_col[:npol, 0] == rows)[product].all()
    assert (per_col[:npol, 1] == rows - col[:, N.KW_SUM_REASON]).all()
    assert int(popcount(planes).sum()) == int(per_col.sum())


def _check(words, npol):
    rows = words.size // npol
    s = K.Summary.from_words(words, npol)
    col, planes = numpy_summary(words, npol)
    assert np.array_equal(s.col, col)
    assert np.array_equal(s.planes, planes)
    check_invariants(s.col, s.planes, rows, npol)
    only = K.Summary.from_words(words, npol, planes=False)  # counters only: the same col
    assert only.planes is None and np.array_equal(only.col, s.col)
    assert np.array_equal(K.Summary.from_words(words, npol).planes, s.planes)  # the same input, the same bytes
    return s


@pytest.mark.parametrize("origin", [K.VALIDATE, K.AUDIT])
@pytest.mark.parametrize("name,scfg", [("c4_64", 4), ("parity", 0), ("c3_group", 3), ("c6_256", 6)])
def test_host_walk_words_reduce_as_numpy_does(name, scfg, origin):
    env = _env(name)
    ids = env.policy_ids()
    s = _check(_walk(name, scfg, ids, origin), len(ids))
    assert (s.col[:, N.KW_SUM_REASON_OTHER] == 0).all()  # no product word has another reason
    assert s.col[:, N.KW_SUM_REASON + 1:].any()           # and the walk found something to count


@pytest.mark.parametrize("ncol", [1, 4, 63, 64, 65, 128, 296])
def test_column_counts_as_prefixes_of_c6(ncol):
    env = _env("c6_256")
    ids = env.policy_ids()[:ncol]
    assert len(ids) == ncol
    _check(_walk("c6_256", 6, ids, K.VALIDATE, rows=300), ncol)


def test_hand_made_rows():
    npol = 70
    empty = _check(np.zeros(0, dtype=np.uint32), npol)  # 0 rows
    assert not empty.col.any() and empty.planes.shape == (0, 2, 2)
    ok = np.uint32(N.KW_V_ALLOWED | N.KW_F_ALLOWED)
    one = _check(np.full(npol, ok, dtype=np.uint32), npol)  # 1 row, all accepted
    assert (one.col[:, N.KW_SUM_F_ALLOWED] == 1).all() and (one.col[:, N.KW_SUM_REASON] == 1).all() and not one.planes.any()
    w = np.full((3, npol), ok, dtype=np.uint32)
    w[1] = (np.arange(npol, dtype=np.uint32) % 15 + 1) << 8 | (N.KW_FST_VANILLA << N.KW_F_STATUS_SHIFT)  # a row of all rejects
    w[2, 5] = 0xA5A5A5A5   # the poison word
    w[2, 69] = 0xA5A5A5A5  # and one in the second group
    s = _check(w.reshape(-1), npol)
    assert int(s.planes[1, 0, 0]) == 2**64 - 1 and int(s.planes[1, 1, 0]) == 2**6 - 1
    assert np.array_equal(s.planes[1, :, 0], s.planes[1, :, 1])
    assert (s.col[:, N.KW_SUM_FST_VANILLA] == 1).all()
    for c in (5, 69):
        assert s.col[c, N.KW_SUM_REASON_OTHER] == 1 and s.col[c, N.KW_SUM_REASON:].sum() == 2
        for h in (0, 1):  # both planes, although 0xA5A5A5A5 has the KW_F_ALLOWED bit set
            assert (int(s.planes[2, c // 64, h]) >> (c % 64)) & 1 == 1
    assert s.col[:, N.KW_SUM_REASON_OTHER].sum() == 2


def test_arguments():
    w = np.zeros(8, dtype=np.uint32)
    s = K.Summary(3, 4)
    st = s._struct()
    import ctypes as C
    rc = N.lib().kw_debug_summarize_words(w.ctypes.data_as(C.POINTER(C.c_uint32)), 2, 4, C.byref(st))
    assert rc == N.KW_E_ARG  # rows differ from the summary's
    z = K.Summary(0, 1)
    z.npol = 0
    st = z._struct()
    assert N.lib().kw_debug_summarize_words(None, 0, 0, C.byref(st)) == N.KW_E_ARG
    with pytest.raises(ValueError):  # counters only: no per-row bits to list
        K.Summary(2, 3, planes=False).flagged_rows()
    with pytest.raises(ValueError):  # `planes` against what the reused Summary holds
        K.Batch._summary_out(K.Summary(2, 3, planes=False), 2, 3, True)
    assert K.Batch._summary_out(None, 2, 3, None).planes is not None
    rows, rw = C.c_uint64(), C.c_uint32()  # a batch that never was on a device holds no pass
    b = K.SynthBatch(0, 4, seed=1).batch()
    assert N.lib().kw_batch_last_pass(b._h, C.byref(rows), C.byref(rw)) == N.KW_E_ARG


def test_summary_check_under_sanitizers(tmp_path):
    exe = tmp_path / "summary_check"
    subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(PKG, "csrc"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "summary_check.cpp")], check=True)
    # (out-of-bounds accesses and undefined behaviour are the point; the leak check at exit needs
    # ptrace rights a test runner may lack)
    out = subprocess.run([str(exe)], check=False, capture_output=True, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "failures 0" in out.stdout
