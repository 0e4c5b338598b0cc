"""The packed verdict form (include/kwgpu.h kw_packed; policy-server_amd/csrc/packed.hpp) on the
host: verdict words of the host walk go through the reference encoder (kw_debug_pack_words) under
the dictionary a device pass uses, and must come back word for word from unpack() and word(r, c);
the exception count equals the words outside their column's dictionary, counted here in numpy; the
offsets, the padding bits and the capacity error hold. tests/packed_check.cpp runs the same entries
as a plain executable under AddressSanitizer and UBSan (no Python in that process)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import kwgpu as K
from helpers import config

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


def _check(env, ids, origin, words, reason0_never_escapes=False):
    npol = len(ids)
    rows = words.size // npol
    p = K.PackedVerdicts.from_words(env, ids, words, origin)
    w2 = words.reshape(rows, npol)
    assert np.array_equal(p.unpack(), words)
    got = np.array([p.word(r, c) for r in range(0, rows, max(1, rows // 40)) for c in range(npol)], dtype=np.uint32)
    assert np.array_equal(got, w2[::max(1, rows // 40)].reshape(-1))  # (every pair: packed_check.cpp)
    absent = ~(w2[:, :, None] == p.dict[None, :, :]).any(axis=2)
    assert p.exc_count == int(absent.sum())  # the encoder never escapes a word its dictionary holds
    off = p.exc_off.astype(np.int64)
    assert off[0] == 0 and (np.diff(off) >= 0).all() and off[rows] == p.exc_count
    assert np.array_equal(np.diff(off), absent.sum(axis=1))
    assert np.array_equal(p.exc[:p.exc_count], w2[absent])  # row-major (row, column) order
    if npol % 64:
        assert not (p.planes[:, -1, :] >> np.uint64(npol % 64)).any()  # bits of columns >= npol
    esc = p.planes[:, :, 0] & p.planes[:, :, 1]
    bits = ((esc[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)).reshape(rows, -1)[:, :npol]
    assert np.array_equal(bits.astype(bool), absent)
    if reason0_never_escapes:
        assert ((p.exc[:p.exc_count] >> 8) & 0xff).all()  # follows from finish_word
    if p.exc_count:  # one word short: the exact need
        with pytest.raises(K.NoSpace) as e:
            K.PackedVerdicts.from_words(env, ids, words, origin, exc_cap=p.exc_count - 1)
        assert e.value.need == p.exc_count
        assert K.PackedVerdicts.from_words(env, ids, words, origin, exc_cap=p.exc_count).exc_count == p.exc_count
    return p


@pytest.mark.parametrize("origin", [K.VALIDATE, K.AUDIT])
@pytest.mark.parametrize("name,scfg", [("c4_64", 4), ("parity", 0), ("c3_group", 3), ("c6_256", 6)])
def test_host_walk_words_round_trip(name, scfg, origin):
    env = _env(name)
    ids = env.policy_ids()
    _check(env, ids, origin, _walk(name, scfg, ids, origin), reason0_never_escapes=name == "c4_64")


@pytest.mark.parametrize("ncol", [1, 4, 63, 64, 65, 128, 296])
def test_column_counts_as_prefixes_of_c6(ncol):
    env = _env("c6_256")
    ids = env.policy_ids()[:ncol]
    assert len(ids) == ncol
    _check(env, ids, K.VALIDATE, _walk("c6_256", 6, ids, K.VALIDATE, rows=300))


def test_hand_made_rows():
    env = _env("c4_64")
    ids = env.policy_ids()
    npol = len(ids)
    empty = K.PackedVerdicts.from_words(env, ids, np.zeros(0, dtype=np.uint32))  # 0 rows: the dictionary alone
    assert empty.exc_count == 0 and empty.exc_off[0] == 0 and empty.unpack().size == 0
    d = empty.dict
    assert (d[:, 2] == d[0, 2]).all() and (d[:, 0] != d[:, 2]).all()  # the bypass word; accepted differs from it
    cols = np.arange(npol, dtype=np.uint32)
    w = np.empty((3, npol), dtype=np.uint32)
    w[0] = 0x00010100 + (cols << 16)       # a row of all exceptions,
    w[0, 5] = 0xA5A5A5A5                    # the poison word among them
    w[1] = d[cols, cols % 3]               # a row of none: each dictionary entry in turn
    w[2] = d[:, 0]
    w[2, npol - 1] = 0xA5A5A5A5            # a poisoned word among coded ones
    p = _check(env, ids, K.VALIDATE, w.reshape(-1))
    assert list(p.exc_off) == [0, npol, npol, npol + 1]
    assert p.exc[5] == 0xA5A5A5A5 and p.exc[npol] == 0xA5A5A5A5 and p.word(2, npol - 1) == 0xA5A5A5A5
    # lowest matching index: a column whose accepted and mutated words coincide codes 0
    same = np.nonzero(d[:, 0] == d[:, 1])[0]
    for c in same[:3]:
        assert (int(p.planes[2, c // 64, 0]) >> (c % 64)) & 1 == 0 and (int(p.planes[2, c // 64, 1]) >> (c % 64)) & 1 == 0


def test_dictionary_follows_the_policies():
    """dict[col] is a function of (env, policies, origin): the same column anywhere in a list has
    the same entry, and the audit origin's words differ from the validate origin's for a monitor
    policy only through finish_word."""
    env = _env("parity")
    ids = env.policy_ids()
    z = np.zeros(0, dtype=np.uint32)
    a = K.PackedVerdicts.from_words(env, ids, z).dict
    b = K.PackedVerdicts.from_words(env, ids[::-1], z).dict
    assert np.array_equal(a, b[::-1])
    assert np.array_equal(a, K.PackedVerdicts.from_words(env, ids, z).dict)
    allowed = a[:, 0] & K._native.KW_V_ALLOWED
    assert ((allowed != 0) | (((a[:, 0] >> 8) & 0xff) != 0)).all()  # accepted, or a constant error word


def test_packed_check_under_sanitizers(tmp_path):
    exe = tmp_path / "packed_check"
    subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(PKG, "csrc"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "packed_check.cpp"), "-L", PKG, "-lkwgpu", "-lkwsynth",
                    f"-Wl,-rpath,{PKG}"], check=True)
    # (out-of-bounds accesses and undefined behaviour are the point; the leak check at exit needs
    # ptrace rights a test runner may lack)
    out = subprocess.run([str(exe), ROOT], check=False, capture_output=True, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "failures 0" in out.stdout
