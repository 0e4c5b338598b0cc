"""The fixture the grouped-outcome tests share (tests/test_outcomes.py on the host walk's words,
tests/test_outcomes_gpu.py on the device's): a policy list that reaches the outcome codes 0, 1, 3, 4
and 8, and AdmissionReview documents whose metrics attributes (requestKind, operation, namespace)
make more than 50 groups, with bypassed rows, rows without a namespace and rows whose namespace is
the empty string. A kw_batch_from_json batch is all admission or all raw, so the raw rows come as a
second batch of the same documents' objects (raw_docs) and, mixed with admission rows in one batch,
as a kw_batch_from_soa copy whose request flags mark every fifth row raw (mixed_batch; such a batch
has no requestKind column)."""
import ctypes as C
import json

import numpy as np

import kwgpu as K
from helpers import config
from kwgpu import _native as N

NS = "kubewarden"  # the always-accept namespace
LABELS = "registry://ghcr.io/kubewarden/policies/safe-labels:v0.1.14"


def policies():
    """Parity's policies with a psp-capabilities policy that may mutate, a namespace policy whose
    valid_namespace is empty (an initialisation error under continue_on_errors) and a group whose
    expression fails at run time for the requests without label "a" (tests/rhai_cases.py, the
    evaluation errors: array index out of bounds)."""
    doc = dict(config("parity"))
    doc["psp-capabilities-mutating"] = dict(doc["psp-capabilities"], allowedToMutate=True)
    doc["namespace-empty"] = {"module": "file:///tmp/namespace-validate-policy.wasm", "settings": {"valid_namespace": ""}}
    doc["group-runtime-error"] = {
        "policies": {"a": {"module": LABELS, "settings": {"mandatory_labels": ["a"]}}},
        "expression": "if a() { true } else { [1][5] == 1 }", "message": "runtime error group"}
    return doc


def docs(n, seed=21):
    """n AdmissionReview dicts from the synthetic workload 0 with the attributes varied."""
    syn = K.SynthBatch(0, n, seed=seed)
    out = []
    for i in range(n):
        d = json.loads(syn.json(i))
        r = d["request"]
        if i % 3:
            r["requestKind"] = {"group": "apps" if i % 2 else "", "version": "v1", "kind": ("Deployment", "Pod", "Job")[i % 5 % 3]}
        r["namespace"] = f"team-{(i * 7) % 13}"
        if i % 7 == 0:
            r["namespace"] = NS  # bypass
        if i % 11 == 0:
            r.pop("namespace", None)
        if i % 13 == 0:
            r["namespace"] = ""  # a namespace that is the empty string: not the same as none
        r["operation"] = ("CREATE", "UPDATE", "DELETE")[(i // 2) % 3]
        if i % 4 == 0:
            r["object"].setdefault("metadata", {}).setdefault("labels", {})["a"] = "x"
        out.append(d)
    return out


def raw_docs(admission_docs):
    return [{"request": d["request"]["object"]} for d in admission_docs]


def mixed_batch(admission_batch):
    """A from_soa copy of the batch with every fifth row flagged raw."""
    v = admission_batch.view()
    flags = np.ctypeslib.as_array(v.req_flags, shape=(v.n_requests,)).copy()
    flags[::5] |= N.KW_REQ_RAW
    v.req_flags = flags.ctypes.data_as(C.POINTER(C.c_uint8))
    b = K.Batch.from_soa(v)  # (copies the columns)
    return b


def strings(col):
    """A kw_strcol of a batch view as a list of bytes."""
    off = np.ctypeslib.as_array(col.off, shape=(col.n + 1,))
    if col.n == 0 or off[-1] == 0:
        return [b""] * col.n
    pool = bytes(np.ctypeslib.as_array(col.bytes, shape=(int(off[-1]),)))
    return [pool[off[i]:off[i + 1]] for i in range(col.n)]


def outcome_code(w):
    """Metrics::record's reading of verdict words (src/metrics.rs:49-140, service.rs:40-150), in numpy."""
    w = np.asarray(w, dtype=np.uint32)
    init = ((w & np.uint32(N.KW_F_STATUS_MASK)) >> np.uint32(N.KW_F_STATUS_SHIFT)) == N.KW_FST_INIT_ERROR
    bypass = (w & np.uint32(N.KW_BYPASS)) != 0
    vanilla = (w & np.uint32(3)) | np.where(((w >> np.uint32(8)) & np.uint32(0xFF)) == 14, np.uint32(4), np.uint32(0))
    return np.where(init, 8, np.where(bypass, 1, vanilla)).astype(np.int64)


def numpy_outcomes(words, npol, row_group, ngroups):
    """out [ngroups][9][npol] by np.add.at."""
    code = outcome_code(words).reshape(-1, npol)
    rows = code.shape[0]
    out = np.zeros((ngroups, N.KW_OUT_N, npol), dtype=np.uint64)
    g = np.zeros(rows, dtype=np.int64) if row_group is None else np.asarray(row_group, dtype=np.int64)
    np.add.at(out, (np.repeat(g, npol), code.reshape(-1), np.tile(np.arange(npol), rows)), np.uint64(1))
    return out


def record_all_pairs(m, env, batch, ids, words, latency_ms, origin):
    """Every (row, policy) pair of words [rows][len(ids)] through kw_metrics_record."""
    npol = len(ids)
    w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
    n = w.size
    rows = np.repeat(np.arange(n // npol, dtype=np.uint64), npol)
    pols = np.tile(np.array([env._idx(p) for p in ids], dtype=np.int32), n // npol)
    lat = np.full(n, latency_ms, dtype=np.uint64)
    rc = N.lib().kw_metrics_record(m._h, env._h, batch._h, rows.ctypes.data_as(C.POINTER(C.c_uint64)),
                                   pols.ctypes.data_as(C.POINTER(C.c_int32)), w.ctypes.data_as(C.POINTER(C.c_uint32)),
                                   lat.ctypes.data_as(C.POINTER(C.c_uint64)), n, origin)
    assert rc == N.KW_OK
