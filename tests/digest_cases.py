"""Shared by tests/test_digest.py and tests/test_digest_gpu.py: the violation digest
(include/kwgpu.h kw_batch_digest) restated in Python over a batch's view, without the library's key
function: a dict keyed by (col, reason, allowed, key) with the keys cut from the columns by the table
in the header; and the comparison of two digests."""
import numpy as np

import outcomes_cases as OC
from kwgpu import _native as N

WIDE_REASONS = frozenset([1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13])  # an entity index, or a group's causes


class Columns:
    """The columns a key reads, as Python lists cut from Batch.view()."""

    def __init__(self, batch):
        v = batch.view()
        n = v.n_requests
        self.rows = n
        self.ctr_off = np.ctypeslib.as_array(v.ctr_off, shape=(n + 1,)).copy()
        self.lbl_off = np.ctypeslib.as_array(v.lbl_off, shape=(n + 1,)).copy()
        nctr = int(self.ctr_off[-1])
        self.capadd_off = np.ctypeslib.as_array(v.capadd_off, shape=(nctr + 1,)).copy()
        self.ns, self.image, self.apparmor = OC.strings(v.ns), OC.strings(v.ctr_image), OC.strings(v.ctr_apparmor)
        self.cap_add, self.lbl_key, self.lbl_val = OC.strings(v.cap_add), OC.strings(v.lbl_key), OC.strings(v.lbl_val)

    def key(self, row, word):
        """The key of a finding by the header's table: a tuple of byte strings (so two strings keep
        their lengths apart) or the argument as an int."""
        reason, arg = (word >> 8) & 0xFF, word >> 16
        if reason == 1:
            return ()
        if reason == 2:
            return (self.ns[row],)
        if 3 <= reason <= 7:
            return (self.image[self.ctr_off[row] + arg],)
        if reason == 8:
            return (self.cap_add[self.capadd_off[self.ctr_off[row]] + arg],)
        if reason == 9:
            return (self.apparmor[self.ctr_off[row] + arg],)
        if reason == 10:
            return (self.lbl_key[self.lbl_off[row] + arg],)
        if reason == 11:
            return (self.lbl_key[self.lbl_off[row] + arg], self.lbl_val[self.lbl_off[row] + arg])
        return arg


def expected(cols, words, npol):
    """(groups, wide, findings): groups {(col, reason, allowed, key): [first_row, word, count]} over
    words [rows][npol] in batch-row order, wide the sorted pair indices."""
    w = np.asarray(words, dtype=np.uint32).reshape(-1, npol)
    groups, wide = {}, []
    rr, cc = np.nonzero((w >> np.uint32(8)) & np.uint32(0xFF))
    for r, c in zip(rr.tolist(), cc.tolist()):  # (row-major: a group's first finding is its lowest row)
        word = int(w[r, c])
        reason = (word >> 8) & 0xFF
        if (word >> 16) == N.KW_ARG_WIDE and reason in WIDE_REASONS:
            wide.append(r * npol + c)
            continue
        k = (c, reason, bool(word & N.KW_F_ALLOWED), cols.key(r, word))
        g = groups.get(k)
        if g is None:
            groups[k] = [r, word, 1]
        else:
            g[2] += 1
    return groups, wide, len(rr)


def as_records(groups):
    """The dict as the library orders its records: (col, reason, first_row)."""
    recs = sorted(((k[0], k[1], g[0], g[1], g[2]) for k, g in groups.items()))
    out = np.zeros(len(recs), dtype=np.dtype([("col", "<u4"), ("word", "<u4"), ("first_row", "<u8"), ("count", "<u8")]))
    for i, (col, _, first, word, count) in enumerate(recs):
        out[i] = (col, word, first, count)
    return out


def same(a, b):
    """Two Digests, exactly: records, wide list, findings."""
    return (a.findings == b.findings and a.recs.tobytes() == b.recs.tobytes() and a.recs.size == b.recs.size and
            np.array_equal(a.wide, b.wide))
