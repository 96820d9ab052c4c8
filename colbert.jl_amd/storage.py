"""Index directory I/O with the reference's layout: JLD2 (HDF5 subset) + JSON files (src/savers.jl,
src/loaders.jl, src/indexing.jl:82-85,140-143).  Arrays go through `jld2.save_object` / `jld2.load_object`, the
Python counterparts of `JLD2.save_object` / `JLD2.load_object` (see jld2.py for what is and is not verified).

Files: config.json, plan.json, centroids / bucket_cutoffs / bucket_weights /
avg_residual, <i>.codes, <i>.residuals, doclens.<i>, <i>.metadata.json, ivf, ivf_lengths (chunks 1-based)."""
from __future__ import annotations

import json
import os

import numpy as np

from . import jld2

EXT = ".jld2"


def _save(path: str, a) -> None:
    jld2.save_object(path + EXT, a)


def _load(path: str):
    """`<path>.jld2` (the reference's format); an index directory written by round 1 of this package holds `<path>.npy`
    instead and is still read."""
    if not os.path.isfile(path + EXT) and os.path.isfile(path + ".npy"):
        a = np.load(path + ".npy")
        return a if a.ndim == 0 else np.asfortranarray(a)
    return jld2.load_object(path + EXT)


def save_codec(index_path, centroids, bucket_cutoffs, bucket_weights, avg_residual) -> None:
    """save_codec (savers.jl:16-29)"""
    os.makedirs(index_path, exist_ok=True)
    _save(os.path.join(index_path, "centroids"), np.asfortranarray(centroids, dtype=np.float32))
    _save(os.path.join(index_path, "bucket_cutoffs"), np.asarray(bucket_cutoffs, dtype=np.float32))
    _save(os.path.join(index_path, "bucket_weights"), np.asarray(bucket_weights, dtype=np.float32))
    _save(os.path.join(index_path, "avg_residual"), np.float32(avg_residual))


def save_chunk(index_path, codes, residuals, chunk_idx: int, passage_offset: int, doclens) -> None:
    """save_chunk (savers.jl:52-84); chunk_idx and passage_offset are 1-based"""
    _save(os.path.join(index_path, f"{chunk_idx}.codes"), np.asarray(codes, dtype=np.uint32))
    _save(os.path.join(index_path, f"{chunk_idx}.residuals"), np.asfortranarray(residuals, dtype=np.uint8))
    _save(os.path.join(index_path, f"doclens.{chunk_idx}"), np.asarray(doclens, dtype=np.int64))
    with open(os.path.join(index_path, f"{chunk_idx}.metadata.json"), "w") as f:
        json.dump({"passage_offset": int(passage_offset), "num_passages": int(len(doclens)),
                   "num_embeddings": int(len(codes))}, f, indent=4)


def save_json(index_path, name, obj) -> None:
    with open(os.path.join(index_path, name), "w") as f:
        json.dump(obj, f, indent=4)


def load_json(index_path, name):
    with open(os.path.join(index_path, name)) as f:
        return json.load(f)


def check_all_files_are_saved(index_path: str) -> bool:
    """_check_all_files_are_saved (collection_indexer.jl:299-340)"""
    _finish_journal(index_path)
    if not os.path.isfile(os.path.join(index_path, "plan.json")):
        return False
    plan = load_json(index_path, "plan.json")
    files = ["config.json"] + [s + EXT for s in ("centroids", "bucket_cutoffs", "bucket_weights", "avg_residual",
                                                  "ivf", "ivf_lengths")]
    for i in range(1, plan["num_chunks"] + 1):
        files += [f"{i}.codes{EXT}", f"{i}.residuals{EXT}", f"doclens.{i}{EXT}", f"{i}.metadata.json"]
    return all(os.path.isfile(os.path.join(index_path, f)) for f in files)


def merge_ivf(ivf, ivf_lengths, n_old_emb: int, new_codes):
    """The IVF of an index grown by `new_codes` (1-based centroid codes of the embeddings n_old_emb+1 ...): per centroid
    the old list followed by the new embedding ids in their stable order -- what `_build_ivf` (collection_indexer.jl:
    349-353) gives on the concatenated codes, because every new id exceeds every old one.  Pure numpy, no sort of the
    old entries.  Returns (ivf, ivf_lengths)."""
    ivf = np.asarray(ivf, dtype=np.int64); old_len = np.asarray(ivf_lengths, dtype=np.int64)
    new_codes = np.asarray(new_codes).astype(np.int64)
    K = old_len.size
    if ivf.size != int(old_len.sum()):
        raise ValueError("length(ivf) must be equal to sum(ivf_lengths)!")
    if new_codes.size and (new_codes.min() < 1 or new_codes.max() > K):
        raise ValueError("codes outside 1..num_partitions")
    add_len = np.bincount(new_codes - 1, minlength=K).astype(np.int64)
    add = np.argsort(new_codes, kind="stable").astype(np.int64) + int(n_old_emb) + 1
    old_off = np.concatenate([[0], np.cumsum(old_len)]); add_off = np.concatenate([[0], np.cumsum(add_len)])
    out = np.empty(ivf.size + add.size, dtype=np.int64)
    # every old entry moves up by the new entries of the centroids before its own; every new one by the old entries up to its own
    out[np.arange(ivf.size) + np.repeat(add_off[:-1], old_len)] = ivf
    out[np.arange(add.size) + np.repeat(old_off[1:], add_len)] = add
    return out, old_len + add_len


def remove_from_ivf(ivf, ivf_lengths, keep):
    """The IVF of an index reduced to the embeddings with `keep[e - 1]` true (a boolean per embedding; ids 1-based): per
    centroid the old list without the dropped ids, the rest renumbered by cumsum(keep) -- what `_build_ivf`
    (collection_indexer.jl:349-353) gives on the reduced codes, because renumbering keeps the order of the ids.  Pure
    numpy, no sort.  Returns (ivf, ivf_lengths)."""
    ivf = np.asarray(ivf, dtype=np.int64); old_len = np.asarray(ivf_lengths, dtype=np.int64)
    keep = np.asarray(keep)
    if keep.dtype != np.bool_ or keep.ndim != 1:
        raise ValueError("keep must be a boolean vector, one entry per embedding")
    if ivf.size != int(old_len.sum()) or ivf.size != keep.size:
        raise ValueError("length(ivf) must be equal to sum(ivf_lengths) and to length(keep)!")
    new_id = np.cumsum(keep, dtype=np.int64)
    stays = keep[ivf - 1]
    before = np.concatenate([[0], np.cumsum(stays, dtype=np.int64)])      # kept entries in front of entry j
    off = np.concatenate([[0], np.cumsum(old_len)])
    return new_id[ivf[stays] - 1], (before[off[1:]] - before[off[:-1]]).astype(old_len.dtype)


JOURNAL = "remove.journal.json"
_TMP = ".rmtmp"
_rename = os.replace        # one rename of a journal (its own name: what a test of an interrupted removal replaces)


def _write_journal(index_path: str, renames) -> None:
    """The journal of a removal: the (temporary name, final name) pairs, complete on disk before it has its name."""
    save_json(index_path, JOURNAL + ".tmp", {"renames": [list(r) for r in renames]})
    os.replace(os.path.join(index_path, JOURNAL + ".tmp"), os.path.join(index_path, JOURNAL))


def _finish_journal(index_path: str) -> None:
    """Finish the renames of a journal an interrupted remove_passages left behind.  A temporary file that is gone was
    renamed already; the journal goes last."""
    journal = os.path.join(index_path, JOURNAL)
    if not os.path.isfile(journal):
        return
    for tmp, final in load_json(index_path, JOURNAL)["renames"]:
        if os.path.isfile(os.path.join(index_path, tmp)):
            _rename(os.path.join(index_path, tmp), os.path.join(index_path, final))
    os.remove(journal)


def _clear_staged(index_path: str) -> None:
    """Delete the staged files an interruption before the journal left behind: no journal names them, nothing reads them."""
    for f in os.listdir(index_path):
        if f.endswith(_TMP) or f.endswith(_TMP + EXT):
            os.remove(os.path.join(index_path, f))


class _Staged:
    """Files written under temporary names, and the renames a journal will make of them."""

    def __init__(self, index_path: str):
        self.index_path, self.renames = index_path, []

    def arrays(self, name, a):
        _save(os.path.join(self.index_path, name + _TMP), a)
        self.renames.append((name + _TMP + EXT, name + EXT))

    def json_file(self, name, obj):
        save_json(self.index_path, name + _TMP, obj)
        self.renames.append((name + _TMP, name))


def remove_passages(index_path: str, pids) -> int:
    """Make a removal (Searcher.remove_passages) part of the index directory; `pids` are the directory's own, 1-based, in
    any order, duplicates allowed.  The passages stay in the numbering with doclen 0: the chunks that lose embeddings get
    new `.codes`, `.residuals`, `doclens.i` and metadata `num_embeddings`, every chunk behind the first of them its new
    `embedding_offset`, and ivf, ivf_lengths and plan.json (`num_embeddings`, `embeddings_offsets`) follow; the layout stays
    the reference's.  Several files change, so: every new file is written under a temporary name, then ONE journal file
    listing the renames, then the renames, then the journal is deleted.  Before the journal exists the directory reads as
    the old index; once it exists every reader finishes the renames first (_finish_journal) and reads the new one.
    That holds against an interrupted PROCESS: neither the staged files nor the journal are fsync'ed, so after a power
    loss the file system may show a journal without the data it names.  Staged files that an interruption before the
    journal left behind are deleted on entry (nothing reads them).
    -> the number of passages that lost embeddings."""
    _finish_journal(index_path)
    _clear_staged(index_path)
    plan = load_json(index_path, "plan.json")
    n_chunks = int(plan["num_chunks"])
    chunk = lambda i, kind: os.path.join(index_path, f"doclens.{i}" if kind == "doclens" else f"{i}.{kind}")
    doclens = [np.asarray(_load(chunk(i, "doclens")), dtype=np.int64) for i in range(1, n_chunks + 1)]
    codes = [_load(chunk(i, "codes")) for i in range(1, n_chunks + 1)]
    n_docs = sum(d.size for d in doclens)
    pids = np.unique(np.asarray(pids, dtype=np.int64).reshape(-1))
    if pids.size and (pids[0] < 1 or pids[-1] > n_docs):
        raise IndexError(f"pid outside 1..{n_docs}")
    gone = np.zeros(n_docs, dtype=bool)
    gone[pids - 1] = True
    all_lens = np.concatenate(doclens) if doclens else np.zeros(0, np.int64)
    gone &= all_lens > 0
    if not gone.any():
        return 0
    keep = np.repeat(~gone, all_lens)
    all_codes = np.concatenate(codes)
    new_ivf, new_lens = remove_from_ivf(*_read_ivf(index_path, all_codes), keep)

    staged = _Staged(index_path)
    arrays, json_file = staged.arrays, staged.json_file

    p0 = e0 = 0                     # passages / OLD embeddings in front of the chunk
    offsets, moved = [], False      # new 1-based embedding offset of every chunk; moved: a chunk before this one shrank
    n_left = 0
    for i in range(1, n_chunks + 1):
        dl = doclens[i - 1]
        g = gone[p0:p0 + dl.size]
        meta = load_json(index_path, f"{i}.metadata.json")
        offsets.append(n_left + 1)
        changed = False
        if moved and "embedding_offset" in meta:
            meta["embedding_offset"] = n_left + 1
            changed = True
        if g.any():
            k = keep[e0:e0 + codes[i - 1].size]
            arrays(f"{i}.codes", np.asarray(codes[i - 1][k], dtype=np.uint32))
            arrays(f"{i}.residuals", np.asfortranarray(_load(chunk(i, "residuals"))[:, k], dtype=np.uint8))
            arrays(f"doclens.{i}", np.where(g, 0, dl).astype(np.int64))
            meta["num_embeddings"] = int(k.sum())
            changed = moved = True
        if changed:
            json_file(f"{i}.metadata.json", meta)
        n_left += int(keep[e0:e0 + codes[i - 1].size].sum())
        p0 += dl.size; e0 += codes[i - 1].size
    arrays("ivf", new_ivf)
    arrays("ivf_lengths", new_lens)
    plan["num_embeddings"] = n_left
    if "embeddings_offsets" in plan:
        plan["embeddings_offsets"] = offsets
    json_file("plan.json", plan)
    _write_journal(index_path, staged.renames)
    _finish_journal(index_path)
    return int(gone.sum())


def update_passages(index_path: str, pids, codes, residuals, doclens) -> int:
    """Make an update (Searcher.update_compressed) part of the index directory: passage `pids[i]` (the directory's own,
    1-based, any order, each at most once) gets the next `doclens[i]` columns of `codes` / `residuals` in the place of its old
    ones.  No passage moves to another chunk: the chunks that hold a changed passage get new `.codes`, `.residuals`,
    `doclens.i` and metadata `num_embeddings`, every chunk behind the first whose size changed its new `embedding_offset`,
    and ivf, ivf_lengths and plan.json (`num_embeddings`, `embeddings_offsets`) follow.  ivf is `_build_ivf`
    (collection_indexer.jl:349-353) of the changed codes: a stable sort on the host, the cost of a rewrite of the directory
    being the files'.  The protocol is remove_passages': temporary names, one journal, the renames; before the journal the
    directory reads as the old index, after it every reader finishes the renames and reads the new one.
    -> the number of named passages whose old or new length is not zero."""
    _finish_journal(index_path)
    _clear_staged(index_path)
    plan = load_json(index_path, "plan.json")
    n_chunks = int(plan["num_chunks"])
    chunk = lambda i, kind: os.path.join(index_path, f"doclens.{i}" if kind == "doclens" else f"{i}.{kind}")
    old_lens = [np.asarray(_load(chunk(i, "doclens")), dtype=np.int64) for i in range(1, n_chunks + 1)]
    old_codes = [_load(chunk(i, "codes")) for i in range(1, n_chunks + 1)]
    n_docs = sum(d.size for d in old_lens)
    pids = np.asarray(pids, dtype=np.int64).reshape(-1)
    codes = np.asarray(codes, dtype=np.uint32); doclens = np.asarray(doclens, dtype=np.int64).reshape(-1)
    residuals = np.asfortranarray(residuals, dtype=np.uint8)
    if pids.size != doclens.size or (doclens < 0).any():
        raise ValueError("one non-negative doclen per pid")
    if int(doclens.sum()) != codes.size or residuals.shape[1] != codes.size:
        raise ValueError("sum(doclens), length(codes) and the residual columns must agree")
    if pids.size and (pids.min() < 1 or pids.max() > n_docs):
        raise IndexError(f"pid outside 1..{n_docs}")
    if np.unique(pids).size != pids.size:
        raise ValueError("a pid is named twice: an update takes one new content per passage")
    K = int(_load(os.path.join(index_path, "ivf_lengths")).size)
    if codes.size and (codes.min() < 1 or codes.max() > K):
        raise ValueError("codes outside 1..num_partitions")
    all_lens = np.concatenate(old_lens) if old_lens else np.zeros(0, np.int64)
    n_changed = int(np.count_nonzero((all_lens[pids - 1] > 0) | (doclens > 0)))
    if n_changed == 0:
        return 0
    new_off = np.concatenate([[0], np.cumsum(doclens)])          # passage pids[i] among the new columns
    slot = np.full(n_docs, -1, dtype=np.int64)
    slot[pids - 1] = np.arange(pids.size)

    staged = _Staged(index_path)
    p0 = n_emb = 0                  # passages / NEW embeddings in front of the chunk
    offsets, moved = [], False      # new 1-based embedding offset of every chunk; moved: a chunk before this one changed size
    all_codes = []
    for i in range(1, n_chunks + 1):
        dl, co = old_lens[i - 1], old_codes[i - 1]
        sl = slot[p0:p0 + dl.size]
        named = np.nonzero(sl >= 0)[0]
        named = named[(dl[named] > 0) | (doclens[sl[named]] > 0)]
        meta = load_json(index_path, f"{i}.metadata.json")
        offsets.append(n_emb + 1)
        changed = False
        if moved and "embedding_offset" in meta:
            meta["embedding_offset"] = n_emb + 1
            changed = True
        if named.size:
            # the chunk's columns, passage by passage: a kept passage's old ones, a named passage's new ones (col < 0: -1 - column)
            off = np.concatenate([[0], np.cumsum(dl)])
            new_dl = dl.copy()
            new_dl[named] = doclens[sl[named]]
            start = off[:-1].copy()
            start[named] = -1 - new_off[sl[named]]
            rank = np.arange(int(new_dl.sum())) - np.repeat(np.concatenate([[0], np.cumsum(new_dl)])[:-1], new_dl)
            first = np.repeat(start, new_dl)
            from_new = first < 0
            col = np.where(from_new, -1 - first, first) + rank
            res_old = _load(chunk(i, "residuals"))
            new_co = np.empty(col.size, dtype=np.uint32)
            new_co[from_new] = codes[col[from_new]]
            new_co[~from_new] = co[col[~from_new]]
            new_res = np.empty((residuals.shape[0], col.size), dtype=np.uint8, order="F")
            new_res[:, from_new] = residuals[:, col[from_new]]
            new_res[:, ~from_new] = res_old[:, col[~from_new]]
            staged.arrays(f"{i}.codes", new_co)
            staged.arrays(f"{i}.residuals", new_res)
            staged.arrays(f"doclens.{i}", new_dl.astype(np.int64))
            meta["num_embeddings"] = int(new_co.size)
            changed = True
            moved = moved or new_co.size != co.size
            co = new_co
        if changed:
            staged.json_file(f"{i}.metadata.json", meta)
        all_codes.append(co)
        n_emb += int(co.size)
        p0 += dl.size
    all_codes = np.concatenate(all_codes)
    staged.arrays("ivf", np.argsort(all_codes, kind="stable").astype(np.int64) + 1)
    staged.arrays("ivf_lengths", np.bincount(all_codes.astype(np.int64) - 1, minlength=K).astype(np.int64))
    plan["num_embeddings"] = n_emb
    if "embeddings_offsets" in plan:
        plan["embeddings_offsets"] = offsets
    staged.json_file("plan.json", plan)
    _write_journal(index_path, staged.renames)
    _finish_journal(index_path)
    return n_changed


def append_chunk(index_path: str, codes, residuals, doclens) -> None:
    """Make appended passages (Searcher.add_compressed) part of the index directory: one more chunk behind the last.
    Order of the writes: the chunk's files; the merged ivf / ivf_lengths under temporary names, renamed into place;
    plan.json last (through a rename as well).  Until plan.json names the new chunk `load_index` and
    `check_all_files_are_saved` read the directory as the old index -- `load_index` drops the inverted-list entries of
    embeddings the plan does not know."""
    _finish_journal(index_path)
    plan = load_json(index_path, "plan.json")
    codes = np.asarray(codes, dtype=np.uint32); doclens = np.asarray(doclens, dtype=np.int64)
    residuals = np.asfortranarray(residuals, dtype=np.uint8)
    if int(doclens.sum()) != codes.size or residuals.shape[1] != codes.size:
        raise ValueError("sum(doclens), length(codes) and the residual columns must agree")
    n_chunks = int(plan["num_chunks"])
    old_codes = np.concatenate([_load(os.path.join(index_path, f"{i}.codes")) for i in range(1, n_chunks + 1)])
    n_docs = sum(_load(os.path.join(index_path, f"doclens.{i}")).size for i in range(1, n_chunks + 1))
    n_emb = int(old_codes.size)
    new_ivf, new_lens = merge_ivf(*_read_ivf(index_path, old_codes), n_emb, codes)
    chunk = n_chunks + 1
    save_chunk(index_path, codes, residuals, chunk, n_docs + 1, doclens)
    with open(os.path.join(index_path, f"{chunk}.metadata.json")) as f:
        meta = json.load(f)
    meta["embedding_offset"] = n_emb + 1                    # 1-based, like passage_offset (collection_indexer.jl:270-296)
    save_json(index_path, f"{chunk}.metadata.json", meta)
    for name, a in (("ivf", new_ivf), ("ivf_lengths", new_lens)):
        _save(os.path.join(index_path, name + ".tmp"), a)
        os.replace(os.path.join(index_path, name + ".tmp" + EXT), os.path.join(index_path, name + EXT))
    plan["num_chunks"] = chunk
    plan["num_embeddings"] = n_emb + int(codes.size)
    if "embeddings_offsets" in plan:
        plan["embeddings_offsets"] = [int(o) for o in plan["embeddings_offsets"]] + [n_emb + 1]
    save_json(index_path, "plan.json.tmp", plan)
    os.replace(os.path.join(index_path, "plan.json.tmp"), os.path.join(index_path, "plan.json"))


def _read_ivf(index_path: str, codes):
    """ivf / ivf_lengths of the directory for the embeddings `codes` (all chunks plan.json names).  A directory whose
    append_chunk was interrupted holds merged lists beside a plan that does not name the new chunk yet: a merged list is
    the old list followed by larger ids, so dropping the ids past len(codes) gives the old lists back exactly."""
    ivf, ivf_lengths = _load(os.path.join(index_path, "ivf")), _load(os.path.join(index_path, "ivf_lengths"))
    if ivf.size > codes.size:
        ivf = ivf[ivf <= codes.size]
        ivf_lengths = np.bincount(codes.astype(np.int64) - 1, minlength=ivf_lengths.size).astype(ivf_lengths.dtype)
    return ivf, ivf_lengths


def load_index(index_path: str) -> dict:
    """load_codec / load_doclens / load_compressed_embs (loaders.jl:10-38, 76-113) + ivf files."""
    _finish_journal(index_path)
    plan = load_json(index_path, "plan.json")
    cfg = load_json(index_path, "config.json")
    codes, res, dl = [], [], []
    for i in range(1, plan["num_chunks"] + 1):
        codes.append(_load(os.path.join(index_path, f"{i}.codes")))
        res.append(_load(os.path.join(index_path, f"{i}.residuals")))
        dl.append(_load(os.path.join(index_path, f"doclens.{i}")))
    codes = np.concatenate(codes)
    ivf, ivf_lengths = _read_ivf(index_path, codes)
    return {"dim": cfg["dim"], "nbits": cfg["nbits"],
            "centroids": _load(os.path.join(index_path, "centroids")),
            "bucket_cutoffs": _load(os.path.join(index_path, "bucket_cutoffs")),
            "bucket_weights": _load(os.path.join(index_path, "bucket_weights")),
            "avg_residual": np.float32(_load(os.path.join(index_path, "avg_residual"))),
            "codes": codes, "residuals": np.asfortranarray(np.concatenate(res, axis=1)),
            "doclens": np.concatenate(dl), "ivf": ivf, "ivf_lengths": ivf_lengths}
