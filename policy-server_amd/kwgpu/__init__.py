"""kwgpu — Python binding of the MI355X admission-evaluation engine (libkwgpu.so).

Plumbing for tests and the benchmark over the C ABI in include/kwgpu.h. Names mirror the
reference so tests read like its own:

  EvaluationEnvironment   src/evaluation/evaluation_environment.rs:86-127 (+ builder :130-366)
  EvaluationError & co    src/evaluation/errors.rs:5-24
  evaluate / RequestOrigin  src/api/service.rs:16-152
  PolicyMode              src/config.rs:287-294

Every evaluation runs on the GPU through the C ABI; nothing here computes a verdict.
"""
import collections
import ctypes as C
import json

from . import _native as N
from ._native import KwSoa, KwTiming  # noqa: F401

PROTECT, MONITOR = N.KW_MODE_PROTECT, N.KW_MODE_MONITOR
VALIDATE, AUDIT = N.KW_ORIGIN_VALIDATE, N.KW_ORIGIN_AUDIT
# the tile kernel a launch took (Batch.debug_last_kernels): the generic one, or the production-shape one
KERNEL_GENERIC, KERNEL_PROD = 0, 1
# family and flag bits of a tile launch (Variant.feat): image, label, container, group families; NFA
# elements; predecessor ranges by wave scan
FEAT_IMG, FEAT_LBL, FEAT_CTR, FEAT_GRP, FEAT_NFA, FEAT_RNG = 1, 2, 4, 8, 16, 32
FEAT_ALL = 15


class Variant(collections.namedtuple("Variant", "feat lds_tables timing prod")):
    """What a tile launch asks the kernel's dispatch for (Batch.debug_last_variants,
    debug_plan_variants): the family and flag bits, LDS or global tables, phase clocks, production
    shape. resolve(): the instantiation of the kernel that request takes (kw_debug_resolve_variant)."""
    __slots__ = ()

    @classmethod
    def from_word(cls, w):
        return cls(w & N.KW_VARIANT_FEAT, bool(w & N.KW_VARIANT_LDS_TABLES), bool(w & N.KW_VARIANT_TIMING),
                   bool(w & N.KW_VARIANT_PROD))

    def word(self):
        return (self.feat | (N.KW_VARIANT_LDS_TABLES if self.lds_tables else 0) | (N.KW_VARIANT_TIMING if self.timing else 0) |
                (N.KW_VARIANT_PROD if self.prod else 0))

    def resolve(self):
        return Variant.from_word(N.lib().kw_debug_resolve_variant(self.word()))


class RequestOrigin:
    Validate = N.KW_ORIGIN_VALIDATE
    Audit = N.KW_ORIGIN_AUDIT


class PolicyMode:
    Protect = N.KW_MODE_PROTECT
    Monitor = N.KW_MODE_MONITOR


class EvaluationError(Exception):
    """errors.rs:5-24; `code` is the KW_E_* status, str() the reference Display string."""

    code = None

    def __init__(self, message, code=None):
        super().__init__(message)
        if code is not None:
            self.code = code


class InvalidPolicyId(EvaluationError):
    code = N.KW_E_INVALID_ID


class PolicyInitialization(EvaluationError):
    code = N.KW_E_INIT


class PolicyNotFound(EvaluationError):
    code = N.KW_E_NOT_FOUND


class BootstrapFailure(EvaluationError):
    code = N.KW_E_BOOTSTRAP


class EngineError(EvaluationError):
    code = N.KW_E_ENGINE


class PayloadError(EvaluationError):
    """HTTP 422 of JsonExtractor (handlers.rs:29-39)."""

    code = N.KW_E_PAYLOAD


class DeviceError(EvaluationError):
    code = N.KW_E_DEVICE


_ERRORS = {c.code: c for c in (InvalidPolicyId, PolicyInitialization, PolicyNotFound, BootstrapFailure,
                               EngineError, PayloadError, DeviceError)}


def raise_for(code, message):
    if code == N.KW_OK:
        return
    cls = _ERRORS.get(code, EvaluationError)
    raise cls(message, code)


def http_status(code):
    """handle_evaluation_error (handlers.rs:321-342) + the 422 of the JSON extractor."""
    if code == N.KW_OK:
        return 200
    if code == N.KW_E_NOT_FOUND:
        return 404
    if code == N.KW_E_PAYLOAD:
        return 422
    return 500


def library():
    return N.lib()


class EvaluationEnvironment:
    """Immutable compiled policy set (EvaluationEnvironmentBuilder::build)."""

    def __init__(self, policies, continue_on_errors=False, always_accept_namespace=None, device=-1, yaml=False):
        """policies: a dict, JSON text, or (yaml=True) the policies.yml text itself."""
        L = N.lib()
        if isinstance(policies, (dict, list)):
            doc = json.dumps(policies).encode()
        elif isinstance(policies, str):
            doc = policies.encode()
        else:
            doc = bytes(policies)
        opts = N.KwEnvOptions(1 if continue_on_errors else 0,
                              always_accept_namespace.encode() if always_accept_namespace is not None else None,
                              device)
        h = C.c_void_p()
        err = C.create_string_buffer(4096)
        build = L.kw_env_build_yaml if yaml else L.kw_env_build
        rc = build(doc, len(doc), C.byref(opts), C.byref(h), err, len(err))
        raise_for(rc, err.value.decode(errors="replace"))
        self._h = h
        self.device = device
        self._L = L

    @classmethod
    def from_serialized(cls, blob, device=-1):
        self = cls.__new__(cls)
        L = N.lib()
        h = C.c_void_p()
        err = C.create_string_buffer(4096)
        buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
        rc = L.kw_env_deserialize(buf, len(blob), device, C.byref(h), err, len(err))
        raise_for(rc, err.value.decode(errors="replace"))
        self._h, self.device, self._L = h, device, L
        return self

    def serialize(self):
        need = C.c_size_t()
        self._L.kw_env_serialize(self._h, None, 0, C.byref(need))
        buf = (C.c_uint8 * need.value)()
        rc = self._L.kw_env_serialize(self._h, buf, need.value, C.byref(need))
        raise_for(rc, "serialize")
        return bytes(buf)

    def close(self):
        if getattr(self, "_h", None):
            self._L.kw_env_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- lookups (evaluation_environment.rs:373-469)
    def lookup(self, policy_id):
        """PolicyID::from_str + map lookup -> policy index; raises InvalidPolicyId / PolicyNotFound."""
        idx = C.c_int32()
        b = policy_id.encode()
        rc = self._L.kw_env_lookup(self._h, b, len(b), C.byref(idx))
        if rc == N.KW_E_INVALID_ID:
            raise InvalidPolicyId(f"Not a valid Policy ID: {policy_id}")
        if rc == N.KW_E_NOT_FOUND:
            raise PolicyNotFound(f"unknown policy: {policy_id}")
        raise_for(rc, policy_id)
        return idx.value

    def policy_count(self):
        return self._L.kw_env_policy_count(self._h)

    def policy_id(self, idx):
        buf = C.create_string_buffer(1024)
        raise_for(self._L.kw_env_policy_id(self._h, idx, buf, len(buf)), "policy_id")
        return buf.value.decode()

    def policy_ids(self):
        return [self.policy_id(i) for i in range(self.policy_count())]

    def is_group(self, idx):
        return self._L.kw_env_is_group(self._h, idx) == 1

    def group_members(self, idx):
        out = (C.c_int32 * 256)()
        n = self._L.kw_env_group_members(self._h, idx, out, 256)
        return list(out[:n])

    def get_policy_mode(self, policy):
        idx = self._idx(policy)
        v = C.c_int()
        rc = self._L.kw_env_get_policy_mode(self._h, idx, C.byref(v))
        if rc == N.KW_E_NOT_FOUND:
            raise PolicyNotFound(f"unknown policy: {self.policy_id(idx)}")
        raise_for(rc, "get_policy_mode")
        return v.value

    def get_policy_allowed_to_mutate(self, policy):
        idx = self._idx(policy)
        v = C.c_int()
        rc = self._L.kw_env_get_policy_allowed_to_mutate(self._h, idx, C.byref(v))
        if rc == N.KW_E_NOT_FOUND:
            raise PolicyNotFound(f"unknown policy: {self.policy_id(idx)}")
        raise_for(rc, "get_policy_allowed_to_mutate")
        return bool(v.value)

    def patterns(self, col):
        """The distinct patterns of request column `col` as (kind, text) (kw_env_pattern)."""
        out = []
        for i in range(self._L.kw_env_pattern_count(self._h, col)):
            kind = C.c_int()
            buf = C.create_string_buffer(1 << 16)
            raise_for(self._L.kw_env_pattern(self._h, col, i, C.byref(kind), buf, len(buf)), "kw_env_pattern")
            out.append((kind.value, buf.value.decode()))
        return out

    def classify(self, col, s, key=b""):
        """Diagnostic (kw_env_classify): the ids of the column patterns `s` matches through the
        compiled classifiers; `key` selects the label key for COL_LV."""
        s = s.encode() if isinstance(s, str) else s
        key = key.encode() if isinstance(key, str) else key
        cap = 4096
        out = (C.c_uint32 * cap)()
        n = self._L.kw_env_classify(self._h, col, key, len(key), s, len(s), out, cap)
        if n < 0:
            raise EngineError("kw_env_classify failed")
        return sorted(out[:min(n, cap)])

    def should_always_accept_requests_made_inside_of_namespace(self, ns):
        b = ns.encode()
        return self._L.kw_env_should_always_accept_requests_made_inside_of_namespace(self._h, b, len(b)) == 1

    def policy_initialization_error(self, policy):
        buf = C.create_string_buffer(4096)
        r = self._L.kw_env_policy_initialization_error(self._h, self._idx(policy), buf, len(buf))
        return buf.value.decode() if r == 1 else None

    def validate_settings(self, policy):
        """Raises like EvaluationEnvironment::validate_settings (evaluation_environment.rs:472-510)."""
        buf = C.create_string_buffer(4096)
        rc = self._L.kw_env_validate_settings(self._h, self._idx(policy), buf, len(buf))
        raise_for(rc, buf.value.decode(errors="replace"))

    def _idx(self, policy):
        return policy if isinstance(policy, int) else self.lookup(policy)

    def _array(self, policies):
        """The policy list as the C ABI's int32 index array, memoised per list: building it costs a
        lookup per policy (~100 us for 64 on the host), more than a small shard's whole pass."""
        key = tuple(policies)
        memo = self.__dict__.setdefault("_arrays", {})
        arr = memo.get(key)
        if arr is None:
            arr = (C.c_int32 * len(policies))(*[self._idx(p) for p in policies])
            if len(memo) > 256:
                memo.clear()
            memo[key] = arr
        return arr

    # --- service::evaluate for one request (service.rs:30-152)
    def evaluate(self, policy_id, document, origin=VALIDATE, raw=False):
        """Returns the AdmissionResponse dict; raises the EvaluationError the handler maps to HTTP."""
        if isinstance(document, (dict, list)):
            document = json.dumps(document)
        doc = document.encode() if isinstance(document, str) else bytes(document)
        need = C.c_size_t()
        buf = C.create_string_buffer(1 << 16)
        rc = self._L.kw_evaluate(self._h, policy_id.encode(), doc, len(doc),
                                 N.KW_DOC_RAW_REVIEW if raw else N.KW_DOC_ADMISSION_REVIEW, origin,
                                 buf, len(buf), C.byref(need))
        if rc == N.KW_E_NOSPACE:
            buf = C.create_string_buffer(need.value)
            rc = self._L.kw_evaluate(self._h, policy_id.encode(), doc, len(doc),
                                     N.KW_DOC_RAW_REVIEW if raw else N.KW_DOC_ADMISSION_REVIEW, origin,
                                     buf, len(buf), C.byref(need))
        raise_for(rc, buf.value.decode(errors="replace"))
        return json.loads(buf.value.decode())


class PinnedWords:
    """A page-locked uint32 host array (kw_host_alloc) for verdict buffers a caller keeps: the bulk
    path reads verdicts back into it by direct DMA. `.array` is the numpy view.

    The allocation lives exactly as long as the ctypes buffer the view wraps (a weakref.finalize on
    it calls kw_host_free): any view or slice of `.array` keeps it alive, whether or not this
    wrapper still exists. close() only drops the wrapper's own reference."""

    def __init__(self, count, device=0):
        import numpy as np
        import weakref
        L = N.lib()
        p = C.c_void_p()
        raise_for(L.kw_host_alloc(device, max(count, 1) * 4, C.byref(p)), "kw_host_alloc failed")
        buf = (C.c_uint32 * max(count, 1)).from_address(p.value)
        self._free = weakref.finalize(buf, L.kw_host_free, C.c_void_p(p.value))
        self.array = np.frombuffer(buf, dtype=np.uint32, count=count)

    @property
    def alive(self):
        """True while the page-locked allocation exists (some view still references it)."""
        return self._free.alive

    def close(self):
        self.array = None


class PackedVerdicts:
    """The packed verdict form of a pass of rows x npol (kw_packed, include/kwgpu.h): `.planes`
    uint64 [rows][G][2] bit-planes of a 2-bit code per column, `.dict` uint32 [npol][3] the words the
    codes 0-2 stand for, `.exc_off` uint32 [rows + 1] and `.exc` the words of code 3 in (row, column)
    order; `.exc_count` of them after a pass. word(row, col) and unpack() give the full words back.

    exc_cap: capacity of `.exc` in words (default: a quarter of rows x npol, at least 1024;
    Batch.validate_host_packed regrows an array it made itself). pinned=True takes the three output
    arrays from page-locked memory (PinnedWords' allocator: direct DMA), which lives as long as any
    view of them."""

    def __init__(self, rows, npol, exc_cap=None, pinned=False, device=0):
        import numpy as np
        self.rows, self.npol = int(rows), int(npol)
        self.G = (self.npol + 63) // 64
        self.pinned, self.device = pinned, device
        self.dict = np.zeros((self.npol, 3), dtype=np.uint32)
        self.planes = self._alloc(self.rows * self.G * 2, np.uint64).reshape(self.rows, self.G, 2)
        self.exc_off = self._alloc(self.rows + 1, np.uint32)
        self.exc_count = 0
        self._grow(max(1024, self.rows * self.npol // 4) if exc_cap is None else int(exc_cap))

    @classmethod
    def page_locked(cls, rows, npol, exc_cap=None, device=0):
        """The output arrays in page-locked memory (kw_host_alloc), beside PinnedWords."""
        return cls(rows, npol, exc_cap=exc_cap, pinned=True, device=device)

    def _alloc(self, count, dtype):
        import numpy as np
        if not self.pinned:
            return np.zeros(count, dtype=dtype)
        words = count * np.dtype(dtype).itemsize // 4
        return PinnedWords(words, self.device).array.view(dtype)[:count]

    def _grow(self, cap):
        import numpy as np
        self.exc = self._alloc(max(cap, 1), np.uint32)[:cap]

    def _struct(self):
        u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
        return N.KwPacked(self.rows, self.npol, self.planes.ctypes.data_as(u64p), self.exc_off.ctypes.data_as(u32p),
                          self.exc.ctypes.data_as(u32p), self.exc.size, self.dict.ctypes.data_as(u32p), self.exc_count)

    @classmethod
    def from_words(cls, env, policies, words, origin=VALIDATE, exc_cap=None):
        """Diagnostic (kw_debug_pack_words): full words [rows][npol] packed on the host by the
        reference encoder, under the dictionary a device pass over these policies uses. On
        KW_E_NOSPACE raises NoSpace with the need in .need."""
        import numpy as np
        npol = len(policies)
        words = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
        rows = words.size // npol
        self = cls(rows, npol, exc_cap=rows * npol if exc_cap is None else exc_cap)
        arr = (C.c_int32 * npol)(*[env._idx(p) for p in policies])
        st = self._struct()
        rc = N.lib().kw_debug_pack_words(env._h, arr, npol, origin, words.ctypes.data_as(C.POINTER(C.c_uint32)), rows,
                                         C.byref(st))
        self.exc_count = st.exc_count
        if rc == N.KW_E_NOSPACE:
            raise NoSpace(st.exc_count)
        raise_for(rc, "kw_debug_pack_words failed")
        return self

    def word(self, row, col):
        """The verdict word of (row, col) (kw_packed_word)."""
        w = C.c_uint32()
        st = self._struct()
        raise_for(N.lib().kw_packed_word(C.byref(st), row, col, C.byref(w)), "kw_packed_word: outside the pass")
        return w.value

    def unpack(self, row0=0, row1=None):
        """Rows [row0, row1) as full words, flat [rows][npol] (kw_packed_unpack)."""
        import numpy as np
        row1 = self.rows if row1 is None else row1
        out = np.empty(max(row1 - row0, 0) * self.npol, dtype=np.uint32)
        st = self._struct()
        raise_for(N.lib().kw_packed_unpack(C.byref(st), row0, row1, out.ctypes.data_as(C.POINTER(C.c_uint32))),
                  "kw_packed_unpack failed")
        return out


class Summary:
    """The summary form of a pass of rows x npol (kw_summary, include/kwgpu.h): `.col` uint64
    [npol][KW_SUM_N] per-column counters (indices: kwgpu._native.KW_SUM_*), `.planes` uint64
    [rows][G][2] with bit c of [r][g][0] set where column 64 g + c rejects and of [r][g][1] where
    its reason is non-zero, or None with planes=False (counters only). pinned=True takes the planes
    from page-locked memory (direct DMA), which lives as long as any view of them."""

    def __init__(self, rows, npol, planes=True, pinned=False, device=0):
        import numpy as np
        self.rows, self.npol = int(rows), int(npol)
        self.G = (self.npol + 63) // 64
        self.pinned, self.device = pinned, device
        self.col = np.zeros((self.npol, N.KW_SUM_N), dtype=np.uint64)
        self.planes = None
        if planes:
            n = self.rows * self.G * 2
            flat = PinnedWords(n * 2, device).array.view(np.uint64)[:n] if pinned else np.zeros(n, dtype=np.uint64)
            self.planes = flat.reshape(self.rows, self.G, 2)

    def _struct(self):
        u64p = C.POINTER(C.c_uint64)
        return N.KwSummary(self.rows, self.npol, self.col.ctypes.data_as(u64p),
                           None if self.planes is None else self.planes.ctypes.data_as(u64p))

    @classmethod
    def from_words(cls, words, npol, planes=True):
        """Diagnostic (kw_debug_summarize_words): full words [rows][npol] reduced on the host by the
        reference reducer."""
        import numpy as np
        words = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
        self = cls(words.size // npol, npol, planes=planes)
        st = self._struct()
        raise_for(N.lib().kw_debug_summarize_words(words.ctypes.data_as(C.POINTER(C.c_uint32)), self.rows, npol,
                                                   C.byref(st)), "kw_debug_summarize_words failed")
        return self

    def flagged_rows(self, plane=1):
        """The rows with a bit set in `plane` (1: a policy found something; 0: a final reject).
        ValueError on a counters-only Summary."""
        import numpy as np
        if self.planes is None:
            raise ValueError("a Summary without planes has no per-row bits")
        return np.nonzero(self.planes[:, :, plane].any(axis=1))[0]


class NoSpace(Exception):
    """KW_E_NOSPACE of a packed pass: the exception words exceed the capacity; .need holds them."""

    def __init__(self, need):
        super().__init__(f"packed verdicts need {need} exception words")
        self.need = int(need)


class DigestNoSpace(NoSpace):
    """KW_E_NOSPACE of a violation digest: .need records and .need_wide wide pairs are required."""

    def __init__(self, need, need_wide):
        Exception.__init__(self, f"the digest needs {need} records and {need_wide} wide pairs")
        self.need, self.need_wide = int(need), int(need_wide)


# kw_digest_rec as a numpy structured dtype (24 bytes, no padding)
DIGEST_REC = [("col", "<u4"), ("word", "<u4"), ("first_row", "<u8"), ("count", "<u8")]
Digest = collections.namedtuple("Digest", ["recs", "wide", "findings"])


class MembersNoSpace(NoSpace):
    """KW_E_NOSPACE of a digest drill-down: .need members are required; .off holds the exact bounds."""

    def __init__(self, need, off):
        Exception.__init__(self, f"the named groups have {need} members")
        self.need, self.off = int(need), off


# off uint64 [groups + 1], rows uint64 [n] (batch rows), words uint32 [n] or None
Members = collections.namedtuple("Members", ["off", "rows", "words"])


class MessagesNoSpace(NoSpace):
    """KW_E_NOSPACE of a messages call: .need text bytes and .nhost host items are required; .off holds
    the exact bounds."""

    def __init__(self, need, off, nhost):
        Exception.__init__(self, f"the messages need {need} bytes and {nhost} host items")
        self.need, self.off, self.nhost = int(need), off, int(nhost)


class Messages(collections.namedtuple("Messages", ["off", "text", "words", "host"])):
    """off uint64 [n + 1], text uint8 [off[n]], words uint32 [n] or None, host uint64 (the items left
    to format_response, ascending)."""
    __slots__ = ()

    def get(self, i):
        """Message i as bytes (raw UTF-8, b"" for an item left to the host)."""
        return self.text[int(self.off[i]):int(self.off[i + 1])].tobytes()


class Batch:
    """A micro-batch of requests in SoA form (kw_batch)."""

    def __init__(self, handle, keepalive=None):
        self._h = handle
        self._L = N.lib()
        self._keep = keepalive
        self.device = -1

    @classmethod
    def from_json(cls, documents, raw=False):
        L = N.lib()
        docs = [d.encode() if isinstance(d, str) else (json.dumps(d).encode() if isinstance(d, (dict, list)) else d)
                for d in documents]
        n = len(docs)
        arr = (C.c_char_p * max(n, 1))(*docs)
        lens = (C.c_size_t * max(n, 1))(*[len(d) for d in docs])
        h = C.c_void_p()
        bad = C.c_int64(-1)
        err = C.create_string_buffer(2048)
        rc = L.kw_batch_from_json(arr, lens, n, N.KW_DOC_RAW_REVIEW if raw else N.KW_DOC_ADMISSION_REVIEW,
                                  C.byref(h), C.byref(bad), err, len(err))
        if rc == N.KW_E_PAYLOAD:
            e = PayloadError(err.value.decode(errors="replace"))
            e.row = bad.value
            raise e
        raise_for(rc, err.value.decode(errors="replace"))
        return cls(h)

    @classmethod
    def from_soa(cls, soa, keepalive=None):
        L = N.lib()
        h = C.c_void_p()
        rc = L.kw_batch_from_soa(C.byref(soa), C.byref(h))
        raise_for(rc, "kw_batch_from_soa: inconsistent columns")
        return cls(h, keepalive)

    def view(self):
        s = KwSoa()
        raise_for(self._L.kw_batch_view(self._h, C.byref(s)), "view")
        s._owner = self  # the view points into this batch's columns
        return s

    @property
    def n(self):
        return self.view().n_requests

    def to_device(self, device=0):
        raise_for(self._L.kw_batch_to_device(self._h, device), f"kw_batch_to_device({device}) failed")
        self.device = device
        return self

    def validate(self, env, policies, origin=VALIDATE, stream=None):
        """All pairs rows x policies on the GPU; returns nothing (verdicts stay in HBM). stream: a
        hipStream_t (int) of the batch's device to run on, None = the batch's own stream."""
        arr = env._array(policies)
        rc = self._L.kw_validate_batch(env._h, self._h, arr, len(policies), origin,
                                       C.c_void_p(stream) if stream else None)
        raise_for(rc, "kw_validate_batch failed")
        self._npol = len(policies)

    def validate_rows(self, env, row_policy, origin=VALIDATE):
        arr = (C.c_int32 * len(row_policy))(*[env._idx(p) for p in row_policy])
        rc = self._L.kw_validate_rows(env._h, self._h, arr, origin, None)
        raise_for(rc, "kw_validate_rows failed")
        self._npol = 1

    def verdicts(self, count=None, out=None):
        """The last pass's verdict words (kw_batch_verdicts); `out`: a reused uint32 array to fill."""
        import numpy as np
        if count is None:
            count = self.n * self._npol if out is None else out.size
        if out is None:
            out = np.zeros(count, dtype=np.uint32)
        elif out.dtype != np.uint32 or not out.flags.c_contiguous or out.size < count:
            raise ValueError("out must be a contiguous uint32 array of at least count words")
        rc = self._L.kw_batch_verdicts(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), count)
        raise_for(rc, "kw_batch_verdicts failed")
        return out

    def pin_host(self, device=0):
        """Page-lock the batch's large host columns in place (kw_batch_pin_host): later bulk passes
        (validate_host) DMA them without the staging copy."""
        raise_for(self._L.kw_batch_pin_host(self._h, device), "kw_batch_pin_host failed")
        return self

    def validate_host(self, env, policies, out=None, origin=VALIDATE, device=0, chunk_rows=0):
        """Bulk host -> host pass (kw_validate_host): upload, evaluate and read back in overlapped row
        chunks; returns the [row][npol] verdict words in `out` (a reused uint32 array, pinned ones from
        PinnedWords read back by direct DMA)."""
        import numpy as np
        npol = len(policies)
        count = self.n * npol
        if out is None:
            out = np.empty(count, dtype=np.uint32)
        elif out.dtype != np.uint32 or not out.flags.c_contiguous or out.size < count:
            raise ValueError("out must be a contiguous uint32 array of at least rows x policies words")
        arr = (C.c_int32 * npol)(*[env._idx(p) for p in policies])
        rc = self._L.kw_validate_host(env._h, self._h, arr, npol, origin, device,
                                      out.ctypes.data_as(C.POINTER(C.c_uint32)), count, chunk_rows)
        raise_for(rc, "kw_validate_host failed")
        self.device = device
        self._npol = npol
        return out[:count]

    def validate_host_packed(self, env, policies, out=None, origin=VALIDATE, device=0, chunk_rows=0):
        """The bulk pass with the verdicts in the packed form (kw_validate_host_packed): returns a
        PackedVerdicts. `out`: a reused one (page-locked: direct DMA); when its exception capacity is
        too small the call raises NoSpace with the need. Without `out` the exception array is regrown
        to the reported need and the pass run once more."""
        npol = len(policies)
        own = out is None
        if own:
            out = PackedVerdicts(self.n, npol)
        elif out.rows != self.n or out.npol != npol:
            raise ValueError("out must be a PackedVerdicts of this batch's rows and these policies")
        arr = (C.c_int32 * npol)(*[env._idx(p) for p in policies])
        for attempt in (0, 1):
            st = out._struct()
            rc = self._L.kw_validate_host_packed(env._h, self._h, arr, npol, origin, device, C.byref(st), chunk_rows)
            out.exc_count = st.exc_count
            if rc != N.KW_E_NOSPACE:
                break
            self.device, self._npol = device, npol  # (the pass ran to its end on the device)
            if not own or attempt:
                raise NoSpace(st.exc_count)
            out._grow(st.exc_count)
        raise_for(rc, "kw_validate_host_packed failed")
        self.device = device
        self._npol = npol
        return out

    def last_pass(self):
        """(rows, verdict words per row) of the last device pass as the library holds it
        (kw_batch_last_pass); KW_E_ARG for a batch without one."""
        rows, rw = C.c_uint64(), C.c_uint32()
        raise_for(self._L.kw_batch_last_pass(self._h, C.byref(rows), C.byref(rw)), "the batch holds no device pass")
        return rows.value, rw.value

    @staticmethod
    def _summary_out(out, rows, npol, planes):
        """`out`, or a new Summary; `planes` None follows `out` (without `out`: with planes). A reused
        Summary of another shape goes to the library, which answers KW_E_ARG."""
        if out is None:
            return Summary(rows, npol, planes=planes is None or bool(planes))
        if planes is not None and bool(planes) != (out.planes is not None):
            raise ValueError("planes contradicts the Summary given as out")
        return out

    def summary(self, out=None, planes=None):
        """The summary of the last device pass (kw_batch_summary): per-column counters and, with
        planes, the reject / found bits of every pair, reduced on the device. `out`: a reused Summary
        of the pass's rows and columns (a validate_rows pass is one column); it decides whether planes
        are read back, and a `planes` that contradicts it is a ValueError."""
        out = self._summary_out(out, *self.last_pass(), planes)
        st = out._struct()
        raise_for(self._L.kw_batch_summary(self._h, C.byref(st)), "kw_batch_summary failed")
        return out

    def validate_host_summary(self, env, policies, out=None, origin=VALIDATE, device=0, chunk_rows=0, planes=None):
        """The bulk pass with the summary as its only output (kw_validate_host_summary): returns a
        Summary (`out` and `planes` as for summary()). The words stay on the device for verdict_rows() /
        verdicts()."""
        npol = len(policies)
        out = self._summary_out(out, self.n, npol, planes)
        arr = (C.c_int32 * npol)(*[env._idx(p) for p in policies])
        st = out._struct()
        rc = self._L.kw_validate_host_summary(env._h, self._h, arr, npol, origin, device, C.byref(st), chunk_rows)
        raise_for(rc, "kw_validate_host_summary failed")
        self.device = device
        self._npol = npol
        return out

    def verdict_rows(self, rows):
        """The full words of the chosen batch rows of the last pass (kw_batch_verdict_rows), as a
        uint32 array [len(rows)][row words]; loads the pass's side data like verdicts()."""
        import numpy as np
        rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
        # (sized by the library's own record of the pass, never by this wrapper's: the entry takes no capacity)
        out = np.zeros((rows.size, self.last_pass()[1]), dtype=np.uint32)
        rc = self._L.kw_batch_verdict_rows(self._h, rows.ctypes.data_as(C.POINTER(C.c_uint64)), rows.size,
                                           out.ctypes.data_as(C.POINTER(C.c_uint32)))
        raise_for(rc, "kw_batch_verdict_rows failed")
        return out

    def attribute_groups(self):
        """The dictionary of the rows' metrics attributes (kw_batch_attribute_groups), host only:
        (row_group uint32 [rows], first_row uint64 [groups]); ids by first appearance."""
        import numpy as np
        n = C.c_uint32()
        row_group = np.zeros(self.n, dtype=np.uint32)
        u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
        rc = self._L.kw_batch_attribute_groups(self._h, row_group.ctypes.data_as(u32p), None, 0, C.byref(n))
        if rc != N.KW_E_NOSPACE:
            raise_for(rc, "kw_batch_attribute_groups failed")
        first_row = np.zeros(n.value, dtype=np.uint64)
        raise_for(self._L.kw_batch_attribute_groups(self._h, row_group.ctypes.data_as(u32p), first_row.ctypes.data_as(u64p),
                                                    first_row.size, C.byref(n)), "kw_batch_attribute_groups failed")
        return row_group, first_row

    def outcomes(self, row_group=None, ngroups=None):
        """The grouped outcome count of the last device pass (kw_batch_outcomes), counted on the
        device: uint64 [ngroups][KW_OUT_N][row words]. row_group: a group id per batch row (None: one
        group); ngroups defaults to the largest id + 1."""
        import numpy as np
        rw = self.last_pass()[1]
        if row_group is None:
            ngroups, ptr = 1 if ngroups is None else ngroups, None
        else:
            row_group = np.ascontiguousarray(row_group, dtype=np.uint32).reshape(-1)
            if row_group.size != self.n:
                raise ValueError("row_group must hold one id per batch row")
            if ngroups is None:
                ngroups = int(row_group.max()) + 1 if row_group.size else 1
            ptr = row_group.ctypes.data_as(C.POINTER(C.c_uint32))
        out = np.zeros((ngroups, N.KW_OUT_N, rw), dtype=np.uint64)
        raise_for(self._L.kw_batch_outcomes(self._h, ptr, ngroups, out.ctypes.data_as(C.POINTER(C.c_uint64))),
                  "kw_batch_outcomes failed")
        return out

    @staticmethod
    def outcomes_from_words(words, npol, row_group=None, ngroups=None):
        """Diagnostic (kw_debug_outcome_words): the same table from full words [rows][npol] by the
        reference host reducer."""
        import numpy as np
        words = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
        rows = words.size // npol
        ptr = None
        if row_group is not None:
            row_group = np.ascontiguousarray(row_group, dtype=np.uint32).reshape(-1)
            if row_group.size != rows:
                raise ValueError("row_group must hold one id per row")
            ptr = row_group.ctypes.data_as(C.POINTER(C.c_uint32))
            if ngroups is None:
                ngroups = int(row_group.max()) + 1 if rows else 1
        ngroups = 1 if ngroups is None else ngroups
        out = np.zeros((ngroups, N.KW_OUT_N, npol), dtype=np.uint64)
        raise_for(N.lib().kw_debug_outcome_words(words.ctypes.data_as(C.POINTER(C.c_uint32)), rows, npol, ptr, ngroups,
                                                 out.ctypes.data_as(C.POINTER(C.c_uint64))), "kw_debug_outcome_words failed")
        return out

    @staticmethod
    def _digest_call(call, cap, wide_cap, grow):
        """call(struct) with arrays of cap / wide_cap entries; on KW_E_NOSPACE once more with the
        reported need when `grow`, else DigestNoSpace."""
        import numpy as np
        for attempt in (0, 1):
            recs = np.zeros(max(cap, 1), dtype=np.dtype(DIGEST_REC))
            wide = np.zeros(max(wide_cap, 1), dtype=np.uint64)
            st = N.KwDigest(recs.ctypes.data_as(C.POINTER(N.KwDigestRec)), cap, 0,
                            wide.ctypes.data_as(C.POINTER(C.c_uint64)), wide_cap, 0, 0)
            rc = call(C.byref(st))
            if rc != N.KW_E_NOSPACE:
                break
            if not grow or attempt or (st.n <= cap and st.nwide <= wide_cap):
                raise DigestNoSpace(st.n, st.nwide)
            cap, wide_cap = max(cap, st.n), max(wide_cap, st.nwide)
        raise_for(rc, "the violation digest failed")
        return Digest(recs[:st.n], wide[:st.nwide], int(st.findings))

    def digest(self, cap=None, wide_cap=None):
        """The violation digest of the last all-pairs device pass (kw_batch_digest), reduced on the
        device: Digest(recs, wide, findings) with recs a structured array (col, word, first_row, count)
        of the groups ordered by (col, reason, first_row) and wide the pair indices row * npol + col of
        the findings whose argument is in the pass's side data. Without `cap` the arrays start at 4096
        records / 1024 pairs and grow once to the reported need; with it a pass that needs more raises
        DigestNoSpace (.need, .need_wide)."""
        grow = cap is None and wide_cap is None
        return self._digest_call(lambda st: self._L.kw_batch_digest(self._h, st), 4096 if cap is None else cap,
                                 1024 if wide_cap is None else wide_cap, grow)

    def digest_from_words(self, words, npol, cap=None, wide_cap=None):
        """Diagnostic (kw_debug_digest_words): the same digest from full words [rows][npol] over this
        batch's host columns, by the reference reducer (an ordered map over the exact keys)."""
        import numpy as np
        words = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
        rows = words.size // npol
        ptr = words.ctypes.data_as(C.POINTER(C.c_uint32))
        grow = cap is None and wide_cap is None
        return self._digest_call(lambda st: self._L.kw_debug_digest_words(self._h, ptr, rows, npol, st),
                                 4096 if cap is None else cap, 1024 if wide_cap is None else wide_cap, grow)

    @staticmethod
    def _members_call(call, recs, words, cap):
        """call(record pointer, count, struct) into arrays of `cap` members: sized by the records'
        counts when they are all non-zero, else grown once to the reported need; a `cap` that is given
        and too small raises MembersNoSpace."""
        import numpy as np
        recs = np.ascontiguousarray(recs, dtype=np.dtype(DIGEST_REC)).reshape(-1)
        ptr = recs.ctypes.data_as(C.POINTER(N.KwDigestRec))
        grow = cap is None
        if grow:
            cap = int(recs["count"].sum()) if recs.size and (recs["count"] != 0).all() else 0
        off = np.zeros(recs.size + 1, dtype=np.uint64)
        for attempt in (0, 1):
            rows = np.zeros(max(cap, 1), dtype=np.uint64)
            wd = np.zeros(max(cap, 1), dtype=np.uint32) if words else None
            st = N.KwMembers(off.ctypes.data_as(C.POINTER(C.c_uint64)), rows.ctypes.data_as(C.POINTER(C.c_uint64)),
                             wd.ctypes.data_as(C.POINTER(C.c_uint32)) if words else None, cap, 0)
            rc = call(ptr, recs.size, C.byref(st))
            if rc != N.KW_E_NOSPACE:
                break
            if not grow or attempt:
                raise MembersNoSpace(st.n, off)
            cap = st.n
        raise_for(rc, "the digest's members failed")
        return Members(off, rows[:st.n], wd[:st.n] if words else None)

    def digest_members(self, recs, words=True, cap=None):
        """The members of the digest groups `recs` names (kw_batch_digest_members), found on the
        device over the last all-pairs pass: Members(off, rows, words) with off[g] .. off[g + 1]
        bounding group g's batch rows (ascending) and their verdict words, in the order of `recs` (a
        structured array as Digest.recs; col, word and first_row are read). The arrays are sized by
        recs["count"].sum() when every count is non-zero and grow once to the reported need otherwise;
        with `cap` a selection that needs more raises MembersNoSpace (.need, .off)."""
        return self._members_call(lambda p, n, st: self._L.kw_batch_digest_members(self._h, p, n, st), recs, words, cap)

    def digest_members_from_words(self, words, npol, recs, with_words=True, cap=None):
        """Diagnostic (kw_debug_digest_members_words): the same members from full words [rows][npol]
        over this batch's host columns, by the reference reducer (an ordered map over the exact keys)."""
        import numpy as np
        words = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
        nrows = words.size // npol
        wp = words.ctypes.data_as(C.POINTER(C.c_uint32))
        return self._members_call(lambda p, n, st: self._L.kw_debug_digest_members_words(self._h, wp, nrows, npol, p, n, st),
                                  recs, with_words, cap)

    @staticmethod
    def _messages_call(call, rows, cols, words, cap, host_cap=None):
        """call(rows pointer, cols pointer, n, struct) into a text buffer of `cap` bytes: without `cap`
        sized from a first KW_E_NOSPACE answer and grown once; a `cap` (or `host_cap`) that is given and
        too small raises MessagesNoSpace."""
        import numpy as np
        rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
        cols = np.ascontiguousarray(cols, dtype=np.uint32).reshape(-1)
        if rows.size != cols.size:
            raise ValueError("rows and cols must pair up")
        n = rows.size
        grow = cap is None and host_cap is None
        cap = 0 if cap is None else cap
        host_cap = n if host_cap is None else host_cap
        off = np.zeros(n + 1, dtype=np.uint64)
        wd = np.zeros(max(n, 1), dtype=np.uint32) if words else None
        for attempt in (0, 1):
            text = np.zeros(max(cap, 1), dtype=np.uint8)
            host = np.zeros(max(host_cap, 1), dtype=np.uint64)
            st = N.KwMessages(off.ctypes.data_as(C.POINTER(C.c_uint64)), text.ctypes.data, cap, 0,
                              wd.ctypes.data_as(C.POINTER(C.c_uint32)) if words else None,
                              host.ctypes.data_as(C.POINTER(C.c_uint64)), host_cap, 0)
            rc = call(rows.ctypes.data_as(C.POINTER(C.c_uint64)), cols.ctypes.data_as(C.POINTER(C.c_uint32)), n, C.byref(st))
            if rc != N.KW_E_NOSPACE:
                break
            if not grow or attempt:
                raise MessagesNoSpace(st.bytes, off, st.nhost)
            cap = st.bytes
        raise_for(rc, "the messages failed")
        return Messages(off, text[:st.bytes], wd[:n] if words else None, host[:st.nhost])

    def messages(self, env, policies, rows, cols, words=False, cap=None, host_cap=None):
        """The messages of the items (rows[i], cols[i]) of the last all-pairs device pass over
        `policies` (kw_batch_messages), rendered on the device: Messages(off, text, words, host), item
        i's message text[off[i]:off[i + 1]] (Messages.get(i)), raw UTF-8; the items in `host` have the
        empty message here and are left to format_response. Without `cap` the text is sized from a
        first KW_E_NOSPACE answer and grown once: that is two calls of the library, the first of
        which runs every length round and its read-back (only the write and the text's copy are
        skipped), so it costs well over half of a second call; a caller that knows a bound passes
        `cap` and pays for one. With `cap` a call that needs more raises MessagesNoSpace (.need, .off,
        .nhost)."""
        arr = env._array(policies)
        return self._messages_call(lambda r, c, n, st: self._L.kw_batch_messages(self._h, env._h, arr, len(policies), r, c, n, st),
                                   rows, cols, words, cap, host_cap)

    def messages_from_words(self, env, policies, words, rows, cols, how=0, with_words=False, cap=None, host_cap=None):
        """Diagnostic (kw_debug_messages_words): the same output on the host from full words
        [rows][npol] and this batch's host columns. how=0: one policy_message per item (the reference);
        how=1: the piece renderer the device runs."""
        import numpy as np
        arr = env._array(policies)
        npol = len(policies)
        words = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
        nrows = words.size // npol
        wp = words.ctypes.data_as(C.POINTER(C.c_uint32))
        return self._messages_call(
            lambda r, c, n, st: self._L.kw_debug_messages_words(env._h, self._h, arr, npol, wp, nrows, r, c, n, how, st),
            rows, cols, with_words, cap, host_cap)

    def member_messages(self, env, policies, recs, members, words=False, cap=None):
        """The messages of the members of digest groups: `members` is digest_members(recs); group g's
        members are the pairs (members.rows[off[g]:off[g + 1]], recs[g].col). One messages() call over
        them all, in the members' order. The members say how many messages there are, not how long
        they are: without `cap` this is messages()'s two calls of the library, with it one."""
        import numpy as np
        recs = np.ascontiguousarray(recs, dtype=np.dtype(DIGEST_REC)).reshape(-1)
        counts = np.diff(members.off.astype(np.int64))
        cols = np.repeat(recs["col"].astype(np.uint32), counts)
        return self.messages(env, policies, members.rows, cols, words=words, cap=cap)

    def debug_messages_stats(self):
        """Diagnostic (kw_debug_messages_stats): what the last messages() did, as a dict: the rounds,
        the staging windows written, the messages that spanned a window, the items left to the host,
        whether the call uploaded the container names."""
        out = (C.c_uint64 * 5)()
        raise_for(self._L.kw_debug_messages_stats(self._h, out), "the batch never rendered messages")
        return dict(zip(("rounds", "windows", "spanning", "host", "uploaded_names"), (int(x) for x in out)))

    def responses(self, env, policies, rows, cols, words=False, cap=None, host_cap=None):
        """The AdmissionResponse bodies of the items (rows[i], cols[i]) of the last all-pairs device
        pass over `policies` (kw_batch_responses), rendered on the device: Messages(off, text, words,
        host), item i's JSON text[off[i]:off[i + 1]] (Messages.get(i)), byte for byte what
        format_response gives with the members' words of the same row; the items in `host` have the
        empty response here and are left to format_response. `cap` and `host_cap` as for messages()."""
        arr = env._array(policies)
        return self._messages_call(lambda r, c, n, st: self._L.kw_batch_responses(self._h, env._h, arr, len(policies), r, c, n, st),
                                   rows, cols, words, cap, host_cap)

    def responses_from_words(self, env, policies, words, rows, cols, how=0, with_words=False, cap=None, host_cap=None):
        """Diagnostic (kw_debug_responses_words): the same output on the host from full words
        [rows][npol] and this batch's host columns. how=0: one format_response per item (the
        reference); how=1: the part and piece renderer the device runs."""
        import numpy as np
        arr = env._array(policies)
        npol = len(policies)
        words = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
        nrows = words.size // npol
        wp = words.ctypes.data_as(C.POINTER(C.c_uint32))
        return self._messages_call(
            lambda r, c, n, st: self._L.kw_debug_responses_words(env._h, self._h, arr, npol, wp, nrows, r, c, n, how, st),
            rows, cols, with_words, cap, host_cap)

    def debug_responses_stats(self):
        """Diagnostic (kw_debug_responses_stats): what the last responses() did, as a dict: the rounds,
        the staging windows written, the responses that spanned a window, the items left to the host,
        whether the call uploaded a side column, the pieces that grew by escaping."""
        out = (C.c_uint64 * 6)()
        raise_for(self._L.kw_debug_responses_stats(self._h, out), "the batch never rendered responses")
        return dict(zip(("rounds", "windows", "spanning", "host", "uploaded_side", "escaped"), (int(x) for x in out)))

    def patches(self, env, policies, rows, cols, form=N.KW_PATCH_RESPONSE, words=False, cap=None, host_cap=None):
        """The JSONPatch of the items (rows[i], cols[i]) of the last all-pairs device pass over
        `policies` (kw_batch_patches), rendered on the device from the columns and the patch-shape
        columns: Messages(off, text, words, host). form KW_PATCH_RESPONSE: the whole AdmissionResponse
        with the base64 patch, byte for byte format_response(doc=...)'s; KW_PATCH_OPS: the RFC 6902
        ops. The items in `host` (no KW_F_PATCH, no psp-capabilities column, an unknown shape) have
        no text here. `cap` and `host_cap` as for messages()."""
        arr = env._array(policies)
        return self._messages_call(
            lambda r, c, n, st: self._L.kw_batch_patches(self._h, env._h, arr, len(policies), r, c, n, int(form), st),
            rows, cols, words, cap, host_cap)

    def patches_from_words(self, env, policies, words, rows, cols, form=N.KW_PATCH_RESPONSE, how=0, with_words=False, cap=None,
                           host_cap=None):
        """Diagnostic (kw_debug_patches_words): the same output on the host from full words
        [rows][npol] and this batch's host columns. how=0: one format_patch per item (the reference);
        how=1: the renderer the device runs, in its rounds and windows."""
        import numpy as np
        arr = env._array(policies)
        npol = len(policies)
        words = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
        nrows = words.size // npol
        wp = words.ctypes.data_as(C.POINTER(C.c_uint32))
        return self._messages_call(
            lambda r, c, n, st: self._L.kw_debug_patches_words(env._h, self._h, arr, npol, wp, nrows, r, c, n, int(form), how, st),
            rows, cols, with_words, cap, host_cap)

    def format_patch(self, env, row, policy, verdict, form=N.KW_PATCH_RESPONSE):
        """One pair's patch from the host columns, without the document (kw_format_patch): the bytes
        of the response (KW_PATCH_RESPONSE) or of the ops (KW_PATCH_OPS). Raises (KW_E_ARG) with a
        message that names what is missing where patches() lists the item for the host."""
        need = C.c_size_t()
        buf = C.create_string_buffer(1 << 15)
        for _ in (0, 1):
            rc = self._L.kw_format_patch(env._h, self._h, int(row), env._idx(policy), int(verdict), int(form), buf, len(buf),
                                         C.byref(need))
            if rc != N.KW_E_NOSPACE:
                break
            buf = C.create_string_buffer(need.value + 1)
        raise_for(rc, buf.value.decode(errors="replace"))
        return buf.value

    def set_patch_shape(self, ctr_place, req_place):
        """Sets the patch-shape columns (kw_batch_set_patch_shape): per container
        KW_PS_* << KW_PS_SHIFT | the item's index in its JSON array, per request KW_PP_*. A batch made
        from columns holds "unknown" until this call; wrong sizes or codes raise."""
        import numpy as np
        cp = np.ascontiguousarray(ctr_place, dtype=np.uint32).reshape(-1)
        rp = np.ascontiguousarray(req_place, dtype=np.uint8).reshape(-1)
        raise_for(self._L.kw_batch_set_patch_shape(self._h, cp.ctypes.data_as(C.POINTER(C.c_uint32)), cp.size,
                                                   rp.ctypes.data_as(C.POINTER(C.c_uint8)), rp.size),
                  "the patch shape does not fit the batch")

    def patch_shape(self):
        """The patch-shape columns (kw_batch_patch_shape): (ctr_place u32 [containers], req_place u8 [rows])."""
        import numpy as np
        v = self.view()
        cp = np.zeros(int(v.ctr_off[v.n_requests]) if v.n_requests else 0, dtype=np.uint32)
        rp = np.zeros(int(v.n_requests), dtype=np.uint8)
        raise_for(self._L.kw_batch_patch_shape(self._h, cp.ctypes.data_as(C.POINTER(C.c_uint32)), cp.size,
                                               rp.ctypes.data_as(C.POINTER(C.c_uint8)), rp.size), "kw_batch_patch_shape failed")
        return cp, rp

    def debug_patches_stats(self):
        """Diagnostic (kw_debug_patches_stats): what the last patches() did, as a dict: the rounds, the
        staging windows written, the items that spanned a window, the items left to the host, whether
        the call uploaded a side column."""
        out = (C.c_uint64 * 5)()
        raise_for(self._L.kw_debug_patches_stats(self._h, out), "the batch never rendered patches")
        return dict(zip(("rounds", "windows", "spanning", "host", "uploaded_side"), (int(x) for x in out)))

    def finding_key(self, row, word):
        """The key bytes of the finding `word` at batch row `row` (kw_batch_finding_key), host only:
        (key, value) for KW_R_LABEL_CONSTRAINT, else (key, None); a numeric or empty key is b""."""
        need, split = C.c_size_t(), C.c_size_t()
        buf = C.create_string_buffer(256)
        rc = self._L.kw_batch_finding_key(self._h, row, int(word), buf, len(buf), C.byref(need), C.byref(split))
        if rc == N.KW_E_NOSPACE:
            buf = C.create_string_buffer(need.value + 1)
            rc = self._L.kw_batch_finding_key(self._h, row, int(word), buf, len(buf), C.byref(need), C.byref(split))
        raise_for(rc, "kw_batch_finding_key failed")
        raw = buf.raw[:need.value]
        if ((int(word) >> 8) & 0xff) == 11:
            return raw[:split.value], raw[split.value:]
        return raw, None

    def debug_digest_stats(self):
        """Diagnostic (kw_debug_digest_stats): what the last digest() did, as a dict: the column
        ranges that ran, the findings the verify launch handed to the host, the table's slots, the
        ranges that were cut."""
        out = (C.c_uint64 * 4)()
        raise_for(self._L.kw_debug_digest_stats(self._h, out), "the batch was never digested")
        return dict(zip(("ranges", "leftovers", "slots", "cuts"), out))

    def debug_plan(self, env, policies, origin=VALIDATE):
        """Diagnostic (kw_debug_plan): the tile kernel's plan for an all-pairs pass, on the host."""
        arr = env._array(policies)
        out = (C.c_uint32 * 16)()
        raise_for(self._L.kw_debug_plan(env._h, self._h, arr, len(policies), origin, out, 16), "kw_debug_plan failed")
        keys = ("lds_bytes", "launches", "chunks", "lds_tables", "rows", "cmax", "kmax", "lmax", "regions", "split",
                "grid", "heavy_lds_bytes", "heavy_rows", "heavy_cmax", "heavy_grid", "scan_regions")
        return dict(zip(keys, out[:16]))

    def debug_copy_jobs(self, env, policies, origin=VALIDATE):
        """Diagnostic (kw_debug_copy_jobs): the record of the tile kernel's staging copy jobs for an
        all-pairs pass planned on the host, as a uint32 array (layout: include/kwgpu.h)."""
        import numpy as np
        arr = env._array(policies)
        need = C.c_size_t()
        rc = self._L.kw_debug_copy_jobs(env._h, self._h, arr, len(policies), origin, None, 0, C.byref(need))
        if rc != N.KW_E_NOSPACE:
            raise_for(rc, "kw_debug_copy_jobs failed")
        out = np.zeros(max(need.value, 1), dtype=np.uint32)
        rc = self._L.kw_debug_copy_jobs(env._h, self._h, arr, len(policies), origin,
                                        out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size, C.byref(need))
        raise_for(rc, "kw_debug_copy_jobs failed")
        return out[:need.value]

    def debug_tile_descs(self, env, policies, origin=VALIDATE):
        """Diagnostic (kw_debug_tile_descs): the tile descriptors a resident all-pairs pass would
        upload, cut per tile at the least estimated cost per row, planned on the host, as a uint32
        array (layout: include/kwgpu.h)."""
        import numpy as np
        arr = env._array(policies)
        need = C.c_size_t()
        rc = self._L.kw_debug_tile_descs(env._h, self._h, arr, len(policies), origin, None, 0, C.byref(need))
        if rc != N.KW_E_NOSPACE:
            raise_for(rc, "kw_debug_tile_descs failed")
        out = np.zeros(max(need.value, 1), dtype=np.uint32)
        rc = self._L.kw_debug_tile_descs(env._h, self._h, arr, len(policies), origin,
                                         out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size, C.byref(need))
        raise_for(rc, "kw_debug_tile_descs failed")
        return out[:need.value]

    def debug_last_launches(self):
        """Diagnostic (kw_debug_last_launches): (workgroups launched, descriptors, static rounds or
        -1) of each tile-kernel launch of the batch's last resident pass."""
        need = C.c_size_t()
        rc = self._L.kw_debug_last_launches(self._h, None, 0, C.byref(need))
        if rc != N.KW_E_NOSPACE:
            raise_for(rc, "kw_debug_last_launches failed")
            return []
        out = (C.c_int64 * need.value)()
        raise_for(self._L.kw_debug_last_launches(self._h, out, need.value, C.byref(need)), "kw_debug_last_launches failed")
        return [tuple(out[i:i + 3]) for i in range(0, need.value, 3)]

    def debug_last_kernels(self):
        """Diagnostic (kw_debug_last_kernels): beside debug_last_launches, the tile kernel each
        launch of the batch's last resident pass took (KERNEL_GENERIC / KERNEL_PROD)."""
        need = C.c_size_t()
        rc = self._L.kw_debug_last_kernels(self._h, None, 0, C.byref(need))
        if rc != N.KW_E_NOSPACE:
            raise_for(rc, "kw_debug_last_kernels failed")
            return []
        out = (C.c_uint32 * need.value)()
        raise_for(self._L.kw_debug_last_kernels(self._h, out, need.value, C.byref(need)), "kw_debug_last_kernels failed")
        return list(out)

    def debug_plan_kernels(self, env, policies, origin=VALIDATE):
        """Diagnostic (kw_debug_plan_kernels): the tile kernel each launch of a resident all-pairs
        pass would take under the current settings, planned on the host."""
        arr = env._array(policies)
        need = C.c_size_t()
        rc = self._L.kw_debug_plan_kernels(env._h, self._h, arr, len(policies), origin, None, 0, C.byref(need))
        if rc != N.KW_E_NOSPACE:
            raise_for(rc, "kw_debug_plan_kernels failed")
            return []
        out = (C.c_uint32 * need.value)()
        raise_for(self._L.kw_debug_plan_kernels(env._h, self._h, arr, len(policies), origin, out, need.value, C.byref(need)),
                  "kw_debug_plan_kernels failed")
        return list(out)

    def debug_last_variants(self):
        """Diagnostic (kw_debug_last_variants): beside debug_last_launches, the Variant each launch
        of the batch's last resident pass asked the tile kernel's dispatch for."""
        need = C.c_size_t()
        rc = self._L.kw_debug_last_variants(self._h, None, 0, C.byref(need))
        if rc != N.KW_E_NOSPACE:
            raise_for(rc, "kw_debug_last_variants failed")
            return []
        out = (C.c_uint32 * need.value)()
        raise_for(self._L.kw_debug_last_variants(self._h, out, need.value, C.byref(need)), "kw_debug_last_variants failed")
        return [Variant.from_word(w) for w in out]

    def debug_plan_variants(self, env, policies, origin=VALIDATE):
        """Diagnostic (kw_debug_plan_variants): the Variant each tile launch of a resident
        all-pairs pass would ask for under the current settings, planned on the host."""
        arr = env._array(policies)
        need = C.c_size_t()
        rc = self._L.kw_debug_plan_variants(env._h, self._h, arr, len(policies), origin, None, 0, C.byref(need))
        if rc != N.KW_E_NOSPACE:
            raise_for(rc, "kw_debug_plan_variants failed")
            return []
        out = (C.c_uint32 * need.value)()
        raise_for(self._L.kw_debug_plan_variants(env._h, self._h, arr, len(policies), origin, out, need.value, C.byref(need)),
                  "kw_debug_plan_variants failed")
        return [Variant.from_word(w) for w in out]

    def debug_reorder(self):
        """Diagnostic (kw_debug_reorder): the device-row order kw_batch_to_device gives this batch,
        as (batch in that order, perm, light-region rows); perm[d] is the batch row at device row d."""
        import numpy as np
        perm = np.zeros(max(self.n, 1), dtype=np.uint64)
        split, h = C.c_uint64(), C.c_void_p()
        rc = self._L.kw_debug_reorder(self._h, perm.ctypes.data_as(C.POINTER(C.c_uint64)), len(perm), C.byref(split),
                                      C.byref(h))
        raise_for(rc, "kw_debug_reorder failed")
        return Batch(h.value), perm[:self.n], split.value

    def wide_arg(self, row, policy):
        """Full argument of a verdict word whose ARG is KW_ARG_WIDE (kw_batch_wide_arg), or None."""
        v = C.c_uint64()
        rc = self._L.kw_batch_wide_arg(self._h, row, policy, C.byref(v))
        return v.value if rc == N.KW_OK else None

    def group_causes(self, row, policy, verdict):
        """Member slots (settings order) of a group rejection's causes (kw_batch_group_causes): from
        the word's ARG or the pass's side data, any number of members."""
        need = C.c_size_t()
        words = (C.c_uint64 * 1)()
        rc = self._L.kw_batch_group_causes(self._h, row, policy, int(verdict), words, 1, C.byref(need))
        if rc == N.KW_E_NOSPACE:
            words = (C.c_uint64 * need.value)()
            rc = self._L.kw_batch_group_causes(self._h, row, policy, int(verdict), words, need.value, C.byref(need))
        raise_for(rc, "kw_batch_group_causes")
        return [64 * k + b for k in range(need.value) for b in range(64) if (words[k] >> b) & 1]

    def debug_host_walk(self, env, policies, origin=VALIDATE):
        """Diagnostic (tests only): the device kernel's slot compiler + entity walks run on the host
        (kw_debug_host_walk). Never part of the validate path."""
        import numpy as np
        arr = env._array(policies)
        out = np.zeros(self.n * len(policies), dtype=np.uint32)
        rc = self._L.kw_debug_host_walk(env._h, self._h, arr, len(policies), origin,
                                        out.ctypes.data_as(C.POINTER(C.c_uint32)))
        raise_for(rc, "kw_debug_host_walk failed")
        return out

    def timed(self, env, policies, origin=VALIDATE, warmup=3, reps=10):
        arr = env._array(policies)
        t = KwTiming()
        rc = self._L.kw_validate_timed(env._h, self._h, arr, len(policies), origin, warmup, reps, C.byref(t))
        raise_for(rc, "kw_validate_timed failed")
        self._npol = len(policies)
        return t

    def format_response(self, env, row, policy, verdict, member_verdicts=None, doc=None, raw=False):
        """AdmissionResponse of (row, policy, verdict); `doc` (the row's original JSON) is needed
        for an accepted mutation, whose response carries the JSONPatch."""
        mv = None
        if member_verdicts is not None:
            mv = (C.c_uint32 * len(member_verdicts))(*[int(x) for x in member_verdicts])
        need = C.c_size_t()
        d = None if doc is None else (doc.encode() if isinstance(doc, str) else doc)

        def call(buf):
            if d is not None:
                return self._L.kw_format_response_doc(env._h, self._h, row, env._idx(policy), int(verdict), mv, d, len(d),
                                                      N.KW_DOC_RAW_REVIEW if raw else N.KW_DOC_ADMISSION_REVIEW, buf,
                                                      len(buf), C.byref(need))
            return self._L.kw_format_response(env._h, self._h, row, env._idx(policy), int(verdict), mv, buf, len(buf),
                                              C.byref(need))
        buf = C.create_string_buffer(1 << 15)
        rc = call(buf)
        if rc == N.KW_E_NOSPACE:  # a long response (a big JSONPatch): the size it needs
            buf = C.create_string_buffer(need.value + 1)
            rc = call(buf)
        raise_for(rc, buf.value.decode(errors="replace"))
        return json.loads(buf.value.decode())

    def close(self):
        if getattr(self, "_h", None):
            self._L.kw_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Metrics:
    """kubewarden_policy_evaluations_total and kubewarden_policy_evaluation_latency_milliseconds
    (src/metrics.rs:49-140), aggregated per validate pass from the verdict words (kw_metrics_*)."""

    def __init__(self):
        self._L = N.lib()
        self._h = self._L.kw_metrics_create()
        if not self._h:
            raise EngineError("kw_metrics_create failed")

    def record(self, env, batch, rows, policies, verdicts, latency_ms, origin=VALIDATE):
        n = len(rows)
        if not (len(policies) == len(verdicts) == len(latency_ms) == n):
            raise ValueError("rows, policies, verdicts and latency_ms must have the same length")
        r = (C.c_uint64 * max(n, 1))(*[int(x) for x in rows])
        p = (C.c_int32 * max(n, 1))(*[env._idx(x) if isinstance(x, str) else int(x) for x in policies])
        v = (C.c_uint32 * max(n, 1))(*[int(x) for x in verdicts])
        lat = (C.c_uint64 * max(n, 1))(*[int(x) for x in latency_ms])
        raise_for(self._L.kw_metrics_record(self._h, env._h, batch._h, r, p, v, lat, n, origin), "kw_metrics_record")

    def add_outcomes(self, env, batch, policies, counts, first_row, latency_ms=0, origin=VALIDATE):
        """What record() would add for every pair of a pass (kw_metrics_add_outcomes), from its
        grouped outcome count: counts uint64 [groups][KW_OUT_N][policies] over the groups of
        batch.attribute_groups(), first_row their first rows; every pair with latency_ms."""
        import numpy as np
        npol = len(policies)
        first_row = np.ascontiguousarray(first_row, dtype=np.uint64).reshape(-1)
        counts = np.ascontiguousarray(counts, dtype=np.uint64)
        if counts.size != first_row.size * N.KW_OUT_N * npol:
            raise ValueError("counts must be [groups][KW_OUT_N][policies]")
        u64p = C.POINTER(C.c_uint64)
        raise_for(self._L.kw_metrics_add_outcomes(self._h, env._h, batch._h, env._array(policies), npol, origin, int(latency_ms),
                                                  first_row.ctypes.data_as(u64p), first_row.size, counts.ctypes.data_as(u64p)),
                  "kw_metrics_add_outcomes")

    def record_pass(self, env, batch, policies, latency_ms=0, origin=VALIDATE):
        """The metrics of the batch's last all-pairs device pass over `policies`
        (kw_metrics_record_pass): dictionary on the host, count on the device, fold on the host."""
        raise_for(self._L.kw_metrics_record_pass(self._h, env._h, batch._h, env._array(policies), len(policies), origin,
                                                 int(latency_ms)), "kw_metrics_record_pass")

    def render(self):
        need = C.c_size_t(0)
        self._L.kw_metrics_render(self._h, None, 0, C.byref(need))
        buf = C.create_string_buffer(need.value + 1)
        raise_for(self._L.kw_metrics_render(self._h, buf, len(buf), C.byref(need)), "kw_metrics_render")
        return buf.value.decode()

    def samples(self):
        """{(metric name, frozenset of (label, value)): value} parsed from render()."""
        out = {}
        for line in self.render().splitlines():
            if not line or line.startswith("#"):
                continue
            head, val = line.rsplit(" ", 1)
            name, _, labels = head.partition("{")
            kv = []
            for part in _split_labels(labels.rstrip("}")):
                k, _, v = part.partition("=")
                kv.append((k, v[1:-1].replace('\\"', '"').replace("\\n", "\n").replace("\\\\", "\\")))
            out[(name, frozenset(kv))] = int(val)
        return out

    def reset(self):
        self._L.kw_metrics_reset(self._h)

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.kw_metrics_destroy(self._h)
            self._h = None


def _split_labels(s):
    parts, cur, q, esc = [], "", False, False
    for ch in s:
        if esc:
            cur += ch
            esc = False
        elif ch == "\\":
            cur += ch
            esc = True
        elif ch == '"':
            cur += ch
            q = not q
        elif ch == "," and not q:
            parts.append(cur)
            cur = ""
        else:
            cur += ch
    if cur:
        parts.append(cur)
    return parts


def service_constraints(allowed, has_patch, has_status, mode, allowed_to_mutate):
    """validation_response_with_constraints (service.rs:160-208) on flags."""
    out = C.c_uint32()
    flags = (1 if allowed else 0) | (2 if has_patch else 0) | (4 if has_status else 0)
    fst = N.lib().kw_service_constraints(flags, mode, 1 if allowed_to_mutate else 0, C.byref(out))
    return fst, bool(out.value & 1), bool(out.value & 2), bool(out.value & 4)


def yaml_to_json(text):
    """The native host's YAML reader (kw_yaml_to_json): the JSON value of a YAML document."""
    b = text.encode() if isinstance(text, str) else text
    need = C.c_size_t()
    L = N.lib()
    L.kw_yaml_to_json(b, len(b), None, 0, C.byref(need))
    buf = C.create_string_buffer(need.value + 1)
    rc = L.kw_yaml_to_json(b, len(b), buf, len(buf), C.byref(need))
    if rc != N.KW_OK:
        raise ValueError(buf.value.decode(errors="replace"))
    return json.loads(buf.value.decode())


def pattern_match(kind, pattern, s):
    b = s.encode() if isinstance(s, str) else s
    return N.lib().kw_pattern_match(kind, pattern.encode(), b, len(b))


def pattern_match_many(kind, pattern, subjects):
    """kw_pattern_match_many: one compilation, a list of 1/0 per subject; None on a syntax error."""
    bs = [x.encode() if isinstance(x, str) else bytes(x) for x in subjects]
    n = len(bs)
    arr = (C.c_char_p * max(n, 1))(*bs)
    lens = (C.c_size_t * max(n, 1))(*[len(x) for x in bs])
    out = (C.c_int32 * max(n, 1))()
    if N.lib().kw_pattern_match_many(kind, pattern.encode(), arr, lens, n, out) != 0:
        return None
    return [int(out[k]) for k in range(n)]


def decode(v):
    """Verdict word -> dict (include/kwgpu.h layout)."""
    v = int(v)
    return {
        "allowed": bool(v & N.KW_V_ALLOWED), "mutated": bool(v & N.KW_V_MUTATED),
        "final_allowed": bool(v & N.KW_F_ALLOWED), "status": (v & N.KW_F_STATUS_MASK) >> N.KW_F_STATUS_SHIFT,
        "bypass": bool(v & N.KW_BYPASS), "patch": bool(v & N.KW_F_PATCH),
        "reason": N.REASONS.get((v >> 8) & 0xFF, (v >> 8) & 0xFF), "arg": v >> 16,
    }


class SynthBatch:
    """libkwsynth workload; .soa() is a kw_soa view valid while this object lives."""

    def __init__(self, config, n, seed, row0=0):
        self._S = N.synth()
        self._h = self._S.kws_generate(config, n, seed, row0)
        self.n = n

    def soa(self):
        s = KwSoa()
        self._S.kws_view(self._h, C.byref(s))
        s._owner = self  # the view points into this generator's columns
        return s

    def json(self, row):
        need = C.c_size_t()
        self._S.kws_json(self._h, row, None, 0, C.byref(need))
        buf = C.create_string_buffer(need.value)
        self._S.kws_json(self._h, row, buf, len(buf), C.byref(need))
        return buf.value.decode()

    def batch(self):
        return Batch.from_soa(self.soa(), keepalive=self)

    def __del__(self):
        try:
            self._S.kws_free(self._h)
        except Exception:
            pass
