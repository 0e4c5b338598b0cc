"""The tile kernel's staging copy jobs (kernels.hpp CopyJob / copy_span, plan.cpp build_copy_jobs).

CPU: for a pass planned on the host (kw_debug_copy_jobs), every tile descriptor x every job — the
span the kernel's own span function gives (byte offset into the column, pieces, LDS destination)
equals what the batch's offsets give, recomputed here from Batch.view().
GPU: the same hand-made batches, and the label / container instantiations' other shapes, bit-exact
against the oracle from poisoned verdict words.
"""
import json

import numpy as np
import pytest

import kwgpu as K
import oracle as O
from helpers import config, diff_verdicts

NS = "kubewarden"
CAPS = ["NET_ADMIN", "SYS_TIME", "CHOWN", "KILL", "SETUID", "MKNOD", "SYS_PTRACE"]
KEYS = ["app", "tier", "env", "team", "owner", "version", "legacy", "debug", "region", "pci"]
# soa string columns in kernels.hpp Str order (S_NS .. S_LV)
STR_COLS = ["ns", "ctr_image", "ctr_apparmor", "cap_add", "cap_drop", "lbl_key", "lbl_val"]


@pytest.fixture(autouse=True)
def _poisoned_verdicts(monkeypatch):
    monkeypatch.setenv("KW_POISON_VERDICTS", "1")


def edge_docs(n, giant=True):
    """n Pod reviews: requests without a pod spec, without containers, without labels; container
    counts 0..5 (and 9) in a pattern of period 8 x 13, so tiles of any height start at container
    indices of every residue mod 4; strings of every length mod 16; with `giant`, one request of 300
    containers x 3 added capabilities and 200 labels in the middle (alone beyond low capacities)."""
    docs = []
    for r in range(n):
        n_ctr = 9 if r % 13 == 0 else [1, 2, 3, 0, 1, 1, 2, 5][r % 8]
        n_lbl = r % 5
        if giant and n >= 40 and r == n // 2:
            n_ctr, n_lbl = 300, 200
        ctrs = [{"name": f"c{i}", "image": ["nginx", "ghcr.io/x/y:1.0", "docker.io/library/busybox:latest"][(i + r) % 3],
                 "securityContext": {"privileged": (i + r) % 17 == 0,
                                     "capabilities": {"add": [CAPS[(i + j + r) % 7] for j in range(3 if n_ctr == 300 else (i + r) % 3)],
                                                      "drop": ["KILL", "ALL"][: (i + r) % 3]}}}
                for i in range(n_ctr)]
        labels = {(KEYS[(i + r) % 10] if i < 10 else f"k{i}"): "v" * ((i * 7 + r) % 19) for i in range(n_lbl)}
        meta = {"name": f"p{r}", "namespace": NS if r % 29 == 7 else "ns-%d" % (r % 6)}
        if labels:
            meta["labels"] = labels
        if r % 3 == 1:
            meta["annotations"] = {f"container.apparmor.security.beta.kubernetes.io/c{i}":
                                   ("localhost/evil" if (i + r) % 5 == 0 else "runtime/default") for i in range(0, n_ctr, 2)}
        obj = {"kind": "Pod", "metadata": meta}
        if r % 7 != 3:
            obj["spec"] = {"containers": ctrs}
        docs.append(json.dumps({"request": {"uid": str(r), "kind": {"group": "", "version": "v1", "kind": "Pod"},
                                            "resource": {"group": "", "version": "v1", "resource": "pods"},
                                            "operation": "CREATE", "userInfo": {}, "object": obj}}))
    return docs


class Cols:
    """The batch's columns as numpy arrays, from Batch.view()."""

    def __init__(self, b):
        s = b.view()
        self._s = s
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

    def expect(self, col, r0, nr):
        """(byte offset into the column, pieces, bytes per piece) of column `col` for requests [r0, r0 + nr)."""
        r1 = r0 + nr
        cb, ce = int(self.ctr_off[r0]), int(self.ctr_off[r1])
        if col == 0:
            return r0, (nr + 3) // 4, 4
        if col in (1, 2):
            return 4 * r0, nr + 1, 4
        if col == 3:
            return 4 * (cb // 4), (ce + 3) // 4 - cb // 4, 4
        if col in (4, 5):
            return 4 * cb, ce - cb + 1, 4
        m = (col - 6) // 2
        g0, g1 = (int(x) for x in self.str_range(m, r0, r1))
        if col % 2 == 0:
            return 4 * g0, g1 - g0 + 1, 4
        off = self.str_off[m]
        sa = int(off[g0]) & ~15
        return sa, (((int(off[g1]) + 15) & ~15) - sa) // 16, 16


def check_jobs(b, env, ids, seen):
    """Every descriptor x job of the pass planned for `b`; adds what the batch exercised to `seen`."""
    w = [int(x) for x in b.debug_copy_jobs(env, ids)]
    cols = Cols(b)
    at = 1
    assert w[0] == 1  # these batches are not split into regions
    rows, njobs, ndesc, novf, lo, hi, lds_bytes, split = w[at:at + 8]
    at += 8
    assert split == 0 and (lo, hi) == (0, cols.n)
    lay = w[at:at + 20]
    at += 20
    dest = lay[:6] + [lay[6 + m] if c == 0 else lay[13 + m] for m in range(7) for c in (0, 1)]
    staged = [m for m in range(7) if lay[13 + m]]
    jobs = [w[at + 4 * j:at + 4 * j + 4] for j in range(njobs)]
    at += 4 * njobs
    # one job per array the pass stages, none for a column it does not stage
    assert sorted(j[0] for j in jobs) == sorted(list(range(6)) + [6 + 2 * m + c for m in staged for c in (0, 1)])
    for col, lds, piece, _code in jobs:
        assert lds == dest[col] and lds % 16 == 0 and lds < lds_bytes, (col, lds, dest[col])
    covered = []
    for _ in range(ndesc):
        d = w[at:at + 32]
        at += 32
        r0, nr, fits = d[24] | (d[25] << 32), d[26], d[23]
        assert fits == 1 and 0 < nr <= rows
        covered.append((r0, nr))
        cb = int(cols.ctr_off[r0])
        assert d[0] == cb and d[1] == cols.ctr_off[r0 + nr] and d[2] == cols.lbl_off[r0] and d[3] == cols.lbl_off[r0 + nr]
        seen["cb&3"].add(cb & 3)
        seen["r0&3"].add(r0 & 3)
        if nr < rows and r0 + nr < cols.n:
            seen["halved"] = True
        for m in staged:
            g0, g1 = cols.str_range(m, r0, r0 + nr)
            seen["begin&15"].add(int(cols.str_off[m][g0]) & 15)
            seen["end&15"].add(int(cols.str_off[m][g1]) & 15)
        for col, lds, piece, _code in jobs:
            got = (w[at] | (w[at + 1] << 32), w[at + 2], piece)
            at += 3
            assert got == cols.expect(col, r0, nr), (r0, nr, col, got, cols.expect(col, r0, nr))
    ovf = w[at:at + novf]
    at += novf
    assert at == len(w)
    seen["overflow"] += len(ovf)
    # the descriptors and the overflow requests cover every row once, in order
    runs = sorted(covered + [(r, 1) for r in ovf])
    nxt = 0
    for r0, nr in runs:
        assert r0 == nxt
        nxt += nr
    assert nxt == cols.n
    seen["empty"] |= any(cols.ctr_off[r + 1] == cols.ctr_off[r] and cols.lbl_off[r + 1] == cols.lbl_off[r] for r in range(cols.n))
    return rows


def test_spans_match_the_columns_offsets(monkeypatch):
    env = K.EvaluationEnvironment(config("c4_64"), continue_on_errors=True, always_accept_namespace=NS)
    ids = env.policy_ids()
    seen = {"cb&3": set(), "r0&3": set(), "begin&15": set(), "end&15": set(), "halved": False, "overflow": 0, "empty": False}
    b = K.Batch.from_json(edge_docs(300))
    for height in ("8", "24", "64"):
        monkeypatch.setenv("KW_SLOT_ROWS", height)
        assert check_jobs(b, env, ids, seen) == int(height)
    assert seen["overflow"] == 0
    # capacities from the median tile: the giant request overflows alone, its neighbours run as halves
    monkeypatch.setenv("KW_TILE_QUANTILE", "0.5")
    for height in ("24", "64"):
        monkeypatch.setenv("KW_SLOT_ROWS", height)
        before = seen["overflow"]
        check_jobs(b, env, ids, seen)
        assert seen["overflow"] == before + 1
    monkeypatch.delenv("KW_TILE_QUANTILE")
    monkeypatch.delenv("KW_SLOT_ROWS")
    for n in (1, 63, 65):
        check_jobs(K.Batch.from_json(edge_docs(n)), env, ids, seen)
    assert seen["cb&3"] == {0, 1, 2, 3} and seen["halved"] and seen["empty"]
    assert seen["r0&3"] - {0}, "no halved tile starts off a multiple of 4 requests"
    assert len(seen["begin&15"]) > 8 and len(seen["end&15"]) > 8


# ---------------------------------------------------------------------------------------- GPU
_cache = {}


def _envs(name):
    if name not in _cache:
        doc = config(name)
        _cache[name] = (K.EvaluationEnvironment(doc, continue_on_errors=True, always_accept_namespace=NS, device=0),
                        O.OracleEnv(doc, continue_on_errors=True, always_accept_namespace=NS))
    return _cache[name]


def _edge(n):
    """(docs, oracle verdicts per origin) of edge_docs(n) under c4_64, computed once."""
    key = ("edge", n)
    if key not in _cache:
        env, oe = _envs("c4_64")
        docs = edge_docs(n)
        view = K.Batch.from_json(docs)
        ids = env.policy_ids()
        _cache[key] = (docs, {o: oe.eval(view.view(), ids, o) for o in (K.VALIDATE, K.AUDIT)})
    return _cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_edge_batches_all_pairs(n):
    env, _ = _envs("c4_64")
    ids = env.policy_ids()
    docs, ora = _edge(n)
    b = K.Batch.from_json(docs).to_device(0)
    for origin in (K.VALIDATE, K.AUDIT):
        b.validate(env, ids, origin)
        gpu = b.verdicts()
        assert np.array_equal(gpu, ora[origin]), diff_verdicts(gpu, ora[origin], len(ids), ids)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_edge_batches_rows_mode(n):
    env, _ = _envs("c4_64")
    ids = env.policy_ids()
    docs, ora = _edge(n)
    b = K.Batch.from_json(docs).to_device(0)
    pick = np.random.default_rng(n).integers(0, len(ids), n)
    for origin in (K.VALIDATE, K.AUDIT):
        b.validate_rows(env, [ids[int(j)] for j in pick], origin)
        want = ora[origin].reshape(n, len(ids))[np.arange(n), pick]
        assert np.array_equal(b.verdicts(count=n), want)


@pytest.mark.gpu
def test_forced_split_has_a_table_per_region(monkeypatch):
    """KW_SPLIT=1: the requests of more than 5 containers after the others, two regions, each launch
    with its own geometry and job table."""
    monkeypatch.setenv("KW_SPLIT", "1")
    env, _ = _envs("c4_64")
    ids = env.policy_ids()
    docs, ora = _edge(1000)
    b = K.Batch.from_json(docs).to_device(0)
    assert b.debug_plan(env, ids)["regions"] == 2
    for origin in (K.VALIDATE, K.AUDIT):
        b.validate(env, ids, origin)
        gpu = b.verdicts()
        assert np.array_equal(gpu, ora[origin]), diff_verdicts(gpu, ora[origin], len(ids), ids)


@pytest.mark.gpu
def test_low_capacities_halve_tiles_and_overflow(monkeypatch):
    monkeypatch.setenv("KW_TILE_QUANTILE", "0.5")
    env, _ = _envs("c4_64")
    ids = env.policy_ids()
    docs, ora = _edge(1000)
    b = K.Batch.from_json(docs).to_device(0)
    for origin in (K.VALIDATE, K.AUDIT):
        b.validate(env, ids, origin)
        gpu = b.verdicts()
        assert np.array_equal(gpu, ora[origin]), diff_verdicts(gpu, ora[origin], len(ids), ids)


@pytest.mark.gpu
def test_container_scan_instantiation(monkeypatch):
    """C5's skewed container counts in 8-row tiles: the wave-scan instantiation (kFeatRng)."""
    monkeypatch.setenv("KW_SLOT_ROWS", "8")
    env, oe = _envs("c5_mixed")
    ids = env.policy_ids()
    syn = K.SynthBatch(5, 400, seed=507)
    b = syn.batch().to_device(0)
    assert b.debug_plan(env, ids)["scan_regions"] != 0
    for origin in (K.VALIDATE, K.AUDIT):
        b.validate(env, ids, origin)
        gpu = b.verdicts()
        ora = oe.eval(syn.soa(), ids, origin)
        assert np.array_equal(gpu, ora), diff_verdicts(gpu, ora, len(ids), ids)


@pytest.mark.gpu
def test_global_table_multi_chunk_instantiation():
    """c6_256: classifiers read from global memory, several slot chunks per launch."""
    env, oe = _envs("c6_256")
    ids = env.policy_ids()
    syn = K.SynthBatch(6, 500, seed=607)
    b = syn.batch().to_device(0)
    plan = b.debug_plan(env, ids)
    assert plan["lds_tables"] == 0 and plan["chunks"] > 1
    for origin in (K.VALIDATE, K.AUDIT):
        b.validate(env, ids, origin)
        gpu = b.verdicts()
        ora = oe.eval(syn.soa(), ids, origin)
        assert np.array_equal(gpu, ora), diff_verdicts(gpu, ora, len(ids), ids)


@pytest.mark.gpu
def test_bulk_pass_in_two_row_chunks():
    """validate_host over two row chunks: descriptors built per chunk, one job table for the pass."""
    env, _ = _envs("c4_64")
    ids = env.policy_ids()
    docs, ora = _edge(1000)
    for origin in (K.VALIDATE, K.AUDIT):
        got = K.Batch.from_json(docs).validate_host(env, ids, origin=origin, chunk_rows=512)
        assert np.array_equal(got, ora[origin]), diff_verdicts(got, ora[origin], len(ids), ids)
