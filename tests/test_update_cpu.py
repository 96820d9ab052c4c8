"""Replacing passages of an index in place, the parts that need no GPU: the numpy model of the updated index that the GPU
tests search with the oracle, the index directory after `storage.update_passages` (and after an interrupted one, on either
side of the journal), the argument contract of `clb_searcher_update` / `_device`, and the Julia binding."""
import ctypes as C
import os

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import storage, synthetic
from tests.test_remove_cpu import assert_loads_as_index, reduced_index, two_chunks
from tests.util_synth import tiny_index


def updated_index(idx, pids, codes, residuals, doclens):
    """idx with the columns of the passages `pids` (1-based, each once) replaced: passage pids[i] holds the columns
    sum(doclens[:i]) .. sum(doclens[:i + 1]) - 1 of codes / residuals, every other passage its own; ivf = _build_ivf of the
    spliced codes"""
    pids, doclens = np.asarray(pids, dtype=np.int64).reshape(-1), np.asarray(doclens, dtype=np.int64).reshape(-1)
    assert np.unique(pids).size == pids.size == doclens.size and int(doclens.sum()) == np.asarray(codes).size
    old_off = np.concatenate([[0], np.cumsum(idx["doclens"])])
    new_off = np.concatenate([[0], np.cumsum(doclens)])
    slot = {int(p): i for i, p in enumerate(pids)}
    co, re, dl = [], [], idx["doclens"].astype(np.int64).copy()
    for p in range(1, dl.size + 1):
        if p in slot:
            i = slot[p]
            co.append(np.asarray(codes)[new_off[i]:new_off[i + 1]]); re.append(np.asarray(residuals)[:, new_off[i]:new_off[i + 1]])
            dl[p - 1] = doclens[i]
        else:
            co.append(idx["codes"][old_off[p - 1]:old_off[p]]); re.append(idx["residuals"][:, old_off[p - 1]:old_off[p]])
    u = dict(idx)
    u["codes"] = np.concatenate(co).astype(idx["codes"].dtype)
    u["residuals"] = np.asfortranarray(np.concatenate(re, axis=1))
    u["doclens"] = dl
    u["ivf"], u["ivf_lengths"] = synthetic.build_ivf(u["codes"], idx["ivf_lengths"].size)
    return u


def content_of(idx, donors):
    """(codes, residuals, doclens): the columns of the passages `donors` (1-based, any order, repeats allowed) one after
    another -- new content for as many passages, in the codec of idx"""
    donors = np.asarray(donors, dtype=np.int64).reshape(-1)
    off = np.concatenate([[0], np.cumsum(idx["doclens"])])
    cols = np.concatenate([np.arange(off[d - 1], off[d]) for d in donors]) if donors.size else np.zeros(0, np.int64)
    return idx["codes"][cols], np.asfortranarray(idx["residuals"][:, cols]), idx["doclens"][donors - 1].astype(np.int64)


def test_model_with_all_doclens_zero_is_the_reduced_index():
    idx, _ = tiny_index()
    pids = np.array([290, 3, 151, 150, 77])
    rows = idx["residuals"].shape[0]
    got = updated_index(idx, pids, np.zeros(0, np.uint32), np.zeros((rows, 0), np.uint8), np.zeros(5, np.int64))
    want, _ = reduced_index(idx, pids)
    for name in ("codes", "residuals", "doclens", "ivf", "ivf_lengths"):
        assert np.array_equal(got[name], want[name]), name


def test_model_replacing_a_passage_by_its_own_columns_is_the_identity():
    idx, _ = tiny_index()
    pids = np.array([300, 1, 42])
    got = updated_index(idx, pids, *content_of(idx, pids))
    for name in ("codes", "residuals", "doclens", "ivf", "ivf_lengths"):
        assert np.array_equal(got[name], idx[name]), name


def test_model_moves_content_and_keeps_every_other_passage():
    idx, _ = tiny_index()
    got = updated_index(idx, [2], *content_of(idx, [9]))
    off, goff = np.concatenate([[0], np.cumsum(idx["doclens"])]), np.concatenate([[0], np.cumsum(got["doclens"])])
    assert got["doclens"][1] == idx["doclens"][8] and np.array_equal(np.delete(got["doclens"], 1), np.delete(idx["doclens"], 1))
    assert np.array_equal(got["codes"][goff[1]:goff[2]], idx["codes"][off[8]:off[9]])
    assert np.array_equal(got["residuals"][:, goff[2]:], idx["residuals"][:, off[2]:])
    assert np.array_equal(np.sort(got["ivf"]), np.arange(1, got["codes"].size + 1))


# both chunks, the chunk boundary on either side, unsorted; 77 is emptied, 3 grows or shrinks by its donor
UPDATED = np.array([290, 3, 151, 150, 77])
DONORS = np.array([10, 200, 151, 299, 5])


def update_args(idx):
    co, re, dl = content_of(idx, DONORS)
    cut = int(dl[:4].sum())
    dl = dl.copy(); dl[4] = 0                  # the last named passage (77) gets no rows
    return UPDATED, co[:cut], np.asfortranarray(re[:, :cut]), dl


def test_update_passages_rewrites_a_two_chunk_directory(tmp_path):
    idx, _ = tiny_index()
    path = str(tmp_path / "index")
    two_chunks(path, idx)
    args = update_args(idx)
    want = updated_index(idx, *args)
    assert storage.update_passages(path, *args) == 5
    assert_loads_as_index(path, want)
    n1 = int(want["doclens"][:150].sum())
    plan = storage.load_json(path, "plan.json")
    m1, m2 = storage.load_json(path, "1.metadata.json"), storage.load_json(path, "2.metadata.json")
    assert plan["num_chunks"] == 2 and plan["num_embeddings"] == want["codes"].size
    assert (m1["num_embeddings"], m1["num_passages"], m1["passage_offset"]) == (n1, 150, 1)
    assert (m2["num_embeddings"], m2["num_passages"], m2["passage_offset"]) == (want["codes"].size - n1, 150, 151)
    assert m2["embedding_offset"] == n1 + 1
    # an update of chunk 2 alone leaves chunk 1's files as they are; the emptied passage is filled again
    before = open(os.path.join(path, "1.codes" + storage.EXT), "rb").read()
    assert storage.update_passages(path, [300], *content_of(idx, [1])) == 1
    assert open(os.path.join(path, "1.codes" + storage.EXT), "rb").read() == before
    want = updated_index(want, [300], *content_of(idx, [1]))
    assert storage.update_passages(path, [77], *content_of(idx, [77])) == 1
    want = updated_index(want, [77], *content_of(idx, [77]))
    assert_loads_as_index(path, want)
    # an empty passage that stays empty changes nothing
    rows = idx["residuals"].shape[0]
    assert storage.update_passages(path, [77], *content_of(idx, [])[:2], [0]) == 1
    assert storage.update_passages(path, [77], np.zeros(0, np.uint32), np.zeros((rows, 0), np.uint8), [0]) == 0
    with pytest.raises(IndexError):
        storage.update_passages(path, [301], *content_of(idx, [1]))
    with pytest.raises(ValueError, match="twice"):
        storage.update_passages(path, [5, 5], *content_of(idx, [1, 2]))
    with pytest.raises(ValueError):
        storage.update_passages(path, [5], *content_of(idx, [1, 2])[:2], [1])


def test_an_update_interrupted_before_the_journal_reads_as_the_old_index(tmp_path, monkeypatch):
    idx, _ = tiny_index()
    path = str(tmp_path / "index")
    two_chunks(path, idx)
    args = update_args(idx)

    def stop(*a):
        raise KeyboardInterrupt
    monkeypatch.setattr(storage, "_write_journal", stop)
    with pytest.raises(KeyboardInterrupt):
        storage.update_passages(path, *args)
    monkeypatch.undo()
    assert [f for f in os.listdir(path) if "tmp" in f]            # the new files were staged ...
    got = storage.load_index(path)                                  # ... and nobody reads them
    for name in ("codes", "residuals", "doclens", "ivf", "ivf_lengths"):
        assert np.array_equal(np.asarray(got[name]), idx[name]), name
    assert storage.check_all_files_are_saved(path)
    assert storage.update_passages(path, *args) == 5               # the staged files are cleared and written again
    assert_loads_as_index(path, updated_index(idx, *args))


@pytest.mark.parametrize("reader", ["load_index", "check_all_files_are_saved", "update_passages"])
def test_an_update_interrupted_after_the_first_rename_reads_as_the_new_index(tmp_path, monkeypatch, reader):
    idx, _ = tiny_index()
    path = str(tmp_path / "index")
    two_chunks(path, idx)
    args = update_args(idx)
    calls = []

    def one_rename_then_stop(src, dst):
        if calls:
            raise KeyboardInterrupt
        calls.append(dst)
        os.replace(src, dst)
    monkeypatch.setattr(storage, "_rename", one_rename_then_stop)
    with pytest.raises(KeyboardInterrupt):
        storage.update_passages(path, *args)
    monkeypatch.undo()
    assert len(calls) == 1 and os.path.isfile(os.path.join(path, storage.JOURNAL))
    want = updated_index(idx, *args)
    if reader == "check_all_files_are_saved":
        assert storage.check_all_files_are_saved(path)
    elif reader == "update_passages":
        assert storage.update_passages(path, [1], *content_of(idx, [1])) == 1      # identical content, on the new index
    assert_loads_as_index(path, want)


@pytest.mark.parametrize("entry", ["clb_searcher_update", "clb_searcher_update_device"])
def test_clb_searcher_update_checks_its_arguments_first(entry):
    """Without a GPU: a null searcher is CLB_EARGUMENT (4) with a message, whatever the other arguments are, and
    *n_changed is cleared."""
    f = getattr(clb.lib(), entry)
    extra = (None,) if entry.endswith("_device") else ()           # hip_stream
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    pids, dl = np.array([1, 2], np.int64), np.array([1, 1], np.int64)
    co, re = np.array([1, 1], np.uint32), np.zeros((32, 2), np.uint8, order="F")
    n = C.c_int64(7)
    assert f(None, C.c_int64(2), ptr(pids), ptr(dl), C.c_int64(2), ptr(co), ptr(re), *extra, C.byref(n)) == 4
    assert b"null" in clb.lib().clb_last_error() and n.value == 0
    n = C.c_int64(7)
    assert f(None, C.c_int64(-1), ptr(pids), ptr(dl), C.c_int64(2), ptr(co), ptr(re), *extra, C.byref(n)) == 4 and n.value == 0
    n = C.c_int64(7)
    assert f(None, C.c_int64(2), None, None, C.c_int64(2), None, None, *extra, C.byref(n)) == 4 and n.value == 0
    assert f(None, C.c_int64(0), None, None, C.c_int64(0), None, None, *extra, None) == 4
    assert clb.lib().clb_last_error()


def test_symbols_and_julia_binding():
    for name in ("clb_searcher_update", "clb_searcher_update_device"):
        assert name in clb.declared_symbols()
        assert hasattr(clb.lib(), name)
    from tests.test_julia_shim_abi import header_prototypes, julia_ccalls
    calls = [c for c in julia_ccalls() if c[1] == "clb_searcher_update"]
    assert len(calls) == 1
    fn, _, ret, types, n_values = calls[0]
    assert fn == "capi.jl" and (ret, types) == header_prototypes()["clb_searcher_update"] and n_values == len(types) == 8
    assert header_prototypes()["clb_searcher_update_device"] == ("i32", ["ptr", "i64", "ptr", "ptr", "i64", "ptr", "ptr", "ptr", "ptr"])
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "julia", "ColBERT", "src")
    assert "update_passages!(searcher::Searcher, pids::Vector{Int}, codes" in open(os.path.join(src, "searching.jl")).read()
    export = [l for l in open(os.path.join(src, "ColBERT.jl")).read().splitlines() if l.startswith("export")]
    assert any("update_passages!" in l for l in export)


def test_persist_needs_an_index_path_before_any_device_call():
    s = object.__new__(clb.Searcher)
    s.index_path, s._h, s._codec = None, None, None       # no handle: a device call would fail differently
    with pytest.raises(clb.ColBERTError, match="persist=True needs a Searcher opened from an index_path"):
        s.update_compressed([1], np.ones(1, np.uint32), np.zeros((32, 1), np.uint8), [1], persist=True)
    for name in ("update_compressed", "update_embeddings", "update_passages"):
        assert hasattr(clb.Searcher, name) and hasattr(clb.ShardedSearcher, name)


def test_sharded_routing_by_position():
    """route_positions selects what route_pids selects, as positions in the caller's list"""
    from colbert_jl_amd.sharded import route_pids, route_positions
    bounds = np.array([0, 100, 100, 250, 300])               # an empty shard in the middle
    pids = np.array([300, 1, 100, 101, 250, 251, 7])
    where = route_positions(pids, bounds)
    assert [w.tolist() for w in where] == [[1, 2, 6], [], [3, 4], [0, 5]]
    for w, p in zip(where, route_pids(pids, bounds)):
        assert np.array_equal(pids[w], p)
    with pytest.raises(clb.BoundsError):
        route_positions([301], bounds)
