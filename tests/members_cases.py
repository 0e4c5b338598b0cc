"""Shared by tests/test_members.py and tests/test_members_gpu.py: the digest's drill-down
(include/kwgpu.h kw_batch_digest_members) restated in Python over a batch's view, without the
library's key function: the findings bucketed by (col, reason, allowed, digest_cases.Columns.key) as
(row, word) pairs; the selections the tests name groups by; and the comparison of two results."""
import numpy as np

import digest_cases as DC
import kwgpu as K
from kwgpu import _native as N


def buckets(cols, words, npol):
    """{(col, reason, allowed, key): [(row, word), ...]} over words [rows][npol] in batch-row order;
    row-major, so each bucket's rows ascend. Wide findings belong to no bucket."""
    w = np.asarray(words, dtype=np.uint32).reshape(-1, npol)
    out = {}
    rr, cc = np.nonzero((w >> np.uint32(8)) & np.uint32(0xFF))
    for r, c in zip(rr.tolist(), cc.tolist()):
        word = int(w[r, c])
        reason = (word >> 8) & 0xFF
        if (word >> 16) == N.KW_ARG_WIDE and reason in DC.WIDE_REASONS:
            continue
        out.setdefault((c, reason, bool(word & N.KW_F_ALLOWED), cols.key(r, word)), []).append((r, word))
    return out


def expected(cols, words, npol, recs):
    """(off, rows, words) of the restatement for the records `recs`, in their order: each names the
    bucket of the finding at (first_row, col)."""
    b = buckets(cols, words, npol)
    off, rows, wd = [0], [], []
    for r in recs:
        word = int(r["word"])
        k = (int(r["col"]), (word >> 8) & 0xFF, bool(word & N.KW_F_ALLOWED), cols.key(int(r["first_row"]), word))
        for row, w in b[k]:
            rows.append(row)
            wd.append(w)
        off.append(len(rows))
    return np.array(off, dtype=np.uint64), np.array(rows, dtype=np.uint64), np.array(wd, dtype=np.uint32)


def recs_of(rows):
    """Records from (col, word, first_row, count) tuples."""
    out = np.zeros(len(rows), dtype=np.dtype(K.DIGEST_REC))
    for i, r in enumerate(rows):
        out[i] = r
    return out


def selections(recs):
    """The named selections of a digest's records: all; every third in reversed order (the output
    follows the caller's list, not the digest's); the largest group alone; the singletons; none."""
    big = recs[np.argmax(recs["count"]):][:1] if recs.size else recs
    return {"all": recs, "third_reversed": recs[::3][::-1], "largest": big, "singletons": recs[recs["count"] == 1],
            "none": recs[:0]}


def same(a, b):
    """Two Members, byte for byte: off, rows, words."""
    if (a.words is None) != (b.words is None):
        return False
    return (a.off.tobytes() == b.off.tobytes() and a.rows.tobytes() == b.rows.tobytes() and
            (a.words is None or a.words.tobytes() == b.words.tobytes()))


def check_properties(m, recs, words, npol):
    """What the header promises for the records of a digest of the same pass."""
    w2 = np.asarray(words, dtype=np.uint32).reshape(-1, npol)
    assert m.off.size == recs.size + 1 and int(m.off[0]) == 0
    assert np.array_equal(np.diff(m.off.astype(np.int64)), recs["count"].astype(np.int64))
    assert m.rows.size == int(recs["count"].sum()) == int(m.off[-1])
    for g, r in enumerate(recs):
        a, b = int(m.off[g]), int(m.off[g + 1])
        assert b > a and int(m.rows[a]) == int(r["first_row"]) and int(m.words[a]) == int(r["word"])
        rows = m.rows[a:b].astype(np.int64)
        assert (np.diff(rows) > 0).all()
        assert np.array_equal(m.words[a:b], w2[rows, int(r["col"])])
