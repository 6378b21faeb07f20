"""The engine's row order and merge rule, in one place.

Invariant: rows are ordered by (series, ts, age) and the LAST row of a
(series, ts) group is the newest. Everything that drops or folds duplicate
points sorts into that order (`sort_perm`) and then merges each group
(`merge_rows` on device, `merge_strs` for host string columns).

"Age" is one of two things, and the callers differ on purpose:

* by `seq` (the per-row sequence stored in every SST): region open
  (`Region._load_ssts`), compaction, and the last_non_null merged scan source.
  These read rows of several files whose order in the input says nothing.
* by arrival, i.e. position in the oldest-to-newest concatenation of sources
  (SSTs, flushing memtables, live memtable; a memtable's row index is its
  arrival order): flush, repartition and every query-time LastRow dedup.
  `sort_perm` is stable, so leaving `seq` out of the keys means exactly this.

Modes (`region_mode`): "append" keeps every row, "last_row" keeps the newest
row of a group whole, "last_non_null" keeps each field's newest non-NULL value.
"""

from __future__ import annotations

import numpy as np
import torch

from greptimedb_amd.ops import dedup_mark_last, merge_last_non_null


def region_mode(region) -> str:
    if region.merge_mode == "last_non_null":
        return "last_non_null"
    return "append" if region.append_mode else "last_row"


def sort_perm(*keys):
    """int64 permutation of a stable lexicographic sort, most significant key
    first; ties keep input order. One stable argsort per key, least
    significant first, each composed with the permutation so far."""
    perm = torch.argsort(keys[-1], stable=True)
    for k in reversed(keys[:-1]):
        perm = perm[torch.argsort(k[perm], stable=True)]
    return perm


def last_row_index(series, ts):
    """Rows (int64, ascending) that end a (series, ts) group of sorted input."""
    keep = dedup_mark_last(series.int().contiguous(), ts.contiguous())
    return keep.nonzero(as_tuple=True)[0]


def merge_rows(series, ts, fields, mode):
    """Merge the groups of sorted rows → (kidx | None, fields[nf, g]). kidx
    are the group-last rows, for the caller to gather its other columns by;
    None (append) means nothing was dropped."""
    if mode == "append":
        return None, fields
    if mode == "last_non_null":
        return merge_last_non_null(series, ts, fields)
    kidx = last_row_index(series, ts)
    return kidx, fields[:, kidx]


def sort_last_rows(series, ts, fields):
    """The query-time LastRow dedup of unsorted rows, ties by arrival →
    (ts, series, fields, perm, kidx): the sorted, deduplicated columns, plus
    the permutation and group-last index that made them, for a caller with
    host columns to take along (row j of the result is input row
    perm[kidx[j]])."""
    perm = sort_perm(series, ts)
    ts, series = ts[perm], series[perm]
    kidx, fields = merge_rows(series, ts, fields[:, perm], "last_row")
    return ts[kidx], series[kidx], fields, perm, kidx


def merge_str_last_non_null(kidx_h: np.ndarray, arr: np.ndarray) -> np.ndarray:
    """Host half of the last_non_null merge for one string column: `arr`
    is (series, ts, seq)-sorted, `kidx_h` the group-last rows; each group
    yields its newest non-None value, or None when it has none."""
    if len(kidx_h) == 0:
        return arr[:0]
    starts = np.concatenate(([0], kidx_h[:-1] + 1))
    valid = np.fromiter((v is not None for v in arr), dtype=bool,
                        count=len(arr))
    cand = np.where(valid, np.arange(len(arr), dtype=np.int64), -1)
    newest = np.maximum.reduceat(cand, starts)
    return arr[np.where(newest >= 0, newest, kidx_h)]


def merge_strs(mode, kidx_h, perm_h, parts) -> np.ndarray:
    """One host string column through the same sort and merge: `parts` are
    the per-source object arrays in gather order, `perm_h` the sort
    permutation and `kidx_h` merge_rows' index (None when nothing dropped)."""
    arr = np.concatenate(parts)
    if mode == "last_non_null":
        return merge_str_last_non_null(kidx_h, arr[perm_h])
    return arr[perm_h if kidx_h is None else perm_h[kidx_h]]


def gather_rows(sources, seqs, fnames=None):
    """Concatenate sources (ScanSource or SstBatch) into one unsorted row set
    → (ts, series, fields[nf, total], seq, str_parts, fnames). `fnames`
    defaults to the union of the sources' fields in order of first appearance;
    a field a source lacks is NaN there. `str_parts` maps each string column
    to per-source, None-padded object arrays for `merge_strs`. `seqs[i]`
    orders source i's rows: a seq tensor, the int sequence of its row 0
    (memtable), or None for a source without sequences, which gets synthetic
    ones in file order after the largest sequence of the seq-tensor and
    sequence-less sources before it (an int base does not move that counter)."""
    device = sources[0].ts.device
    # field name → row of s.fields: a ScanSource has the map, an SstBatch a list
    pos_of = [s.field_pos if hasattr(s, "field_pos") else
              {fn: i for i, fn in enumerate(s.field_names)} for s in sources]
    if fnames is None:
        fnames = []
        for pos in pos_of:
            fnames.extend(fn for fn in pos if fn not in fnames)
    total = sum(s.n for s in sources)
    fields = torch.full((len(fnames), total), float("nan"),
                        dtype=torch.float64, device=device)
    synth = any(q is None for q in seqs)
    seq_parts, synth_base, off = [], 0, 0
    for s, pos, q in zip(sources, pos_of, seqs):
        for fi, fn in enumerate(fnames):
            p = pos.get(fn)
            if p is not None and p < s.fields.shape[0]:
                fields[fi, off:off + s.n] = s.fields[p][: s.n]
        if q is None:
            q = torch.arange(synth_base, synth_base + s.n,
                             dtype=torch.int64, device=device)
            synth_base += s.n
        elif isinstance(q, int):    # a memtable: always after every file
            q = torch.arange(q, q + s.n, dtype=torch.int64, device=device)
        else:
            q = q.to(torch.int64)
            if synth and s.n:     # the sync is only paid when it is needed
                synth_base = max(synth_base, int(q.max().item()) + 1)
        seq_parts.append(q)
        off += s.n
    ts = torch.cat([s.ts[: s.n] for s in sources])
    series = torch.cat([s.series[: s.n].to(torch.int32) for s in sources])
    str_parts: dict[str, list] = {k: [] for s in sources for k in s.str_cols}
    for name, parts in str_parts.items():
        for s in sources:
            col = s.str_cols.get(name)
            parts.append(np.full(s.n, None, dtype=object) if col is None
                         else np.asarray(col[: s.n], dtype=object))
    return ts, series, fields, torch.cat(seq_parts), str_parts, fnames
