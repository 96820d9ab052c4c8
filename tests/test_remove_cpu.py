"""Removing passages from an index, the parts that need no GPU: the host IVF compaction against `_build_ivf` of the reduced
codes, the index directory after `storage.remove_passages` (and after an interrupted one, on either side of the journal),
the argument contract of `clb_searcher_remove`, and the Julia binding."""
import ctypes as C
import os

import numpy as np
import pytest

import colbert_jl_amd as clb
from colbert_jl_amd import storage, synthetic
from tests.test_append_cpu import head_of, tail_of, write_index
from tests.util_synth import tiny_index


def reduced_index(idx, removed):
    """idx without the embeddings of the passages `removed` (1-based pids): they stay in the numbering with doclen 0, and
    ivf = _build_ivf of the codes that are left"""
    gone = np.zeros(idx["doclens"].size, dtype=bool)
    gone[np.asarray(removed, dtype=np.int64) - 1] = True
    keep = np.repeat(~gone, idx["doclens"])
    r = dict(idx)
    r["codes"] = idx["codes"][keep]
    r["residuals"] = np.asfortranarray(idx["residuals"][:, keep])
    r["doclens"] = np.where(gone, 0, idx["doclens"]).astype(np.int64)
    r["ivf"], r["ivf_lengths"] = synthetic.build_ivf(r["codes"], idx["ivf_lengths"].size)
    return r, keep


def emptying_set(idx):
    """pids of every passage that has an embedding in the shortest non-empty inverted list: removing them empties it"""
    lens = idx["ivf_lengths"]
    c = int(np.argmin(np.where(lens > 0, lens, lens.max() + 1)))
    emb2pid = np.repeat(np.arange(1, idx["doclens"].size + 1), idx["doclens"])
    return np.unique(emb2pid[idx["codes"].astype(np.int64) == c + 1]), c


@pytest.mark.parametrize("case", ["one", "every_other", "all_but_one", "none", "empties_a_list"])
def test_remove_from_ivf_equals_build_ivf_of_the_reduced_codes(case):
    idx, _ = tiny_index()
    removed = {"one": [17], "every_other": np.arange(1, 301, 2), "all_but_one": np.delete(np.arange(1, 301), 122),
               "none": np.zeros(0, np.int64)}.get(case)
    if case == "empties_a_list":
        removed, c = emptying_set(idx)
        assert 0 < removed.size < 300
    want, keep = reduced_index(idx, removed)
    ivf, lens = storage.remove_from_ivf(idx["ivf"], idx["ivf_lengths"], keep)
    assert ivf.dtype == np.int64 and np.array_equal(ivf, want["ivf"])
    assert np.array_equal(lens, want["ivf_lengths"]) and int(lens.sum()) == want["codes"].size
    if case == "empties_a_list":
        assert idx["ivf_lengths"][c] > 0 and lens[c] == 0
    if case == "none":
        assert np.array_equal(ivf, idx["ivf"])


def test_remove_from_ivf_refuses_a_keep_of_the_wrong_kind():
    idx, _ = tiny_index()
    with pytest.raises(ValueError):
        storage.remove_from_ivf(idx["ivf"], idx["ivf_lengths"], np.ones(idx["codes"].size - 1, bool))
    with pytest.raises(ValueError):
        storage.remove_from_ivf(idx["ivf"], idx["ivf_lengths"], np.ones(idx["codes"].size, np.int64))


def two_chunks(path, idx):
    write_index(path, idx, 150)
    storage.append_chunk(path, *tail_of(idx, 150))


def assert_loads_as_index(path, want):
    got = storage.load_index(path)
    for name in ("codes", "residuals", "doclens", "ivf", "ivf_lengths"):
        assert np.array_equal(np.asarray(got[name]), want[name]), name
    assert storage.check_all_files_are_saved(path)
    assert not [f for f in os.listdir(path) if "tmp" in f or "journal" in f]


REMOVED = np.array([290, 3, 151, 3, 150, 77])     # both chunks, the chunk boundary, a duplicate, unsorted


def test_remove_passages_rewrites_a_two_chunk_directory(tmp_path):
    idx, _ = tiny_index()
    path = str(tmp_path / "index")
    two_chunks(path, idx)
    want, _ = reduced_index(idx, REMOVED)
    assert storage.remove_passages(path, REMOVED) == 5
    assert_loads_as_index(path, want)
    got = storage.load_index(path)
    assert np.all(got["doclens"][np.unique(REMOVED) - 1] == 0) and np.count_nonzero(got["doclens"] == 0) == 5
    n1 = int(want["doclens"][:150].sum())
    plan = storage.load_json(path, "plan.json")
    m1, m2 = storage.load_json(path, "1.metadata.json"), storage.load_json(path, "2.metadata.json")
    assert plan["num_chunks"] == 2 and plan["num_embeddings"] == want["codes"].size
    assert (m1["num_embeddings"], m1["num_passages"], m1["passage_offset"]) == (n1, 150, 1)
    assert (m2["num_embeddings"], m2["num_passages"], m2["passage_offset"]) == (want["codes"].size - n1, 150, 151)
    assert m2["embedding_offset"] == n1 + 1
    # again: those passages are empty already; another chunk-2-only removal leaves chunk 1's files alone
    assert storage.remove_passages(path, REMOVED) == 0
    before = open(os.path.join(path, "1.codes" + storage.EXT), "rb").read()
    assert storage.remove_passages(path, [300]) == 1
    assert open(os.path.join(path, "1.codes" + storage.EXT), "rb").read() == before
    assert_loads_as_index(path, reduced_index(idx, np.append(REMOVED, 300))[0])
    with pytest.raises(IndexError):
        storage.remove_passages(path, [301])
    # an append behind a removal numbers on from the reduced embedding count
    storage.append_chunk(path, *tail_of(idx, 290))
    assert storage.load_json(path, "3.metadata.json")["embedding_offset"] == storage.load_json(path, "plan.json")["num_embeddings"] - int(idx["doclens"][290:].sum()) + 1


def test_a_removal_interrupted_before_the_journal_reads_as_the_old_index(tmp_path, monkeypatch):
    idx, _ = tiny_index()
    path = str(tmp_path / "index")
    two_chunks(path, idx)

    def stop(*a):
        raise KeyboardInterrupt
    monkeypatch.setattr(storage, "_write_journal", stop)
    with pytest.raises(KeyboardInterrupt):
        storage.remove_passages(path, REMOVED)
    monkeypatch.undo()
    assert [f for f in os.listdir(path) if "tmp" in f]            # the new files were staged ...
    got = storage.load_index(path)                                  # ... and nobody reads them
    for name in ("codes", "residuals", "doclens", "ivf", "ivf_lengths"):
        assert np.array_equal(np.asarray(got[name]), idx[name]), name
    assert storage.check_all_files_are_saved(path)
    assert storage.remove_passages(path, [300]) == 1               # chunk 2 only: the files staged for chunk 1 are cleared too
    assert not [f for f in os.listdir(path) if "tmp" in f]
    assert storage.remove_passages(path, REMOVED) == 5
    assert_loads_as_index(path, reduced_index(idx, np.append(REMOVED, 300))[0])


def head_index(idx, P):
    """the first P passages of idx as an index of their own"""
    hc, hr, hd, _ = head_of(idx, P)
    h = dict(idx)
    h["codes"], h["residuals"], h["doclens"] = hc, np.asfortranarray(hr), hd
    h["ivf"], h["ivf_lengths"] = synthetic.build_ivf(hc, idx["ivf_lengths"].size)
    return h


@pytest.mark.parametrize("reader", ["load_index", "check_all_files_are_saved", "append_chunk", "remove_passages"])
def test_a_removal_interrupted_after_the_first_rename_reads_as_the_new_index(tmp_path, monkeypatch, reader):
    """Passages 1-290 in two chunks; the removal stops after the journal and one rename.  Each of the four readers finishes
    the renames first: the directory is the reduced index (for append_chunk: with passages 291-300 behind it)."""
    idx, _ = tiny_index()
    path = str(tmp_path / "index")
    write_index(path, idx, 150)
    storage.append_chunk(path, *tail_of(idx, 150, 290))
    calls = []

    def one_rename_then_stop(src, dst):
        if calls:
            raise KeyboardInterrupt
        calls.append(dst)
        os.replace(src, dst)
    monkeypatch.setattr(storage, "_rename", one_rename_then_stop)
    with pytest.raises(KeyboardInterrupt):
        storage.remove_passages(path, REMOVED)
    monkeypatch.undo()
    assert len(calls) == 1 and os.path.isfile(os.path.join(path, storage.JOURNAL))
    want = reduced_index(head_index(idx, 290), REMOVED)[0]
    if reader == "check_all_files_are_saved":
        assert storage.check_all_files_are_saved(path)
    elif reader == "append_chunk":
        storage.append_chunk(path, *tail_of(idx, 290))
        want = reduced_index(idx, REMOVED)[0]
    elif reader == "remove_passages":
        assert storage.remove_passages(path, REMOVED) == 0
    assert_loads_as_index(path, want)


def test_clb_searcher_remove_checks_its_arguments_first():
    """Without a GPU: a null searcher is CLB_EARGUMENT (4) with a message, whatever the other arguments are, and
    *n_removed is cleared."""
    l = clb.lib()
    pids = np.array([1, 2], np.int64)
    n = C.c_int64(7)
    assert l.clb_searcher_remove(None, pids.ctypes.data_as(C.c_void_p), C.c_int64(2), C.byref(n)) == 4
    assert b"null" in l.clb_last_error() and n.value == 0
    assert l.clb_searcher_remove(None, None, C.c_int64(0), None) == 4
    assert l.clb_searcher_remove(None, None, C.c_int64(-1), None) == 4


def test_symbol_and_julia_binding():
    assert "clb_searcher_remove" in clb.declared_symbols()
    assert hasattr(clb.lib(), "clb_searcher_remove")
    from tests.test_julia_shim_abi import header_prototypes, julia_ccalls
    calls = [c for c in julia_ccalls() if c[1] == "clb_searcher_remove"]
    assert len(calls) == 1
    fn, _, ret, types, n_values = calls[0]
    assert fn == "capi.jl" and (ret, types) == header_prototypes()["clb_searcher_remove"] and n_values == len(types) == 4
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "julia", "ColBERT", "src")
    assert "remove_passages!(searcher::Searcher, pids::Vector{Int})" in open(os.path.join(src, "searching.jl")).read()
    assert "remove_passages!" in open(os.path.join(src, "ColBERT.jl")).read()


def test_persist_needs_an_index_path_before_any_device_call():
    s = object.__new__(clb.Searcher)
    s.index_path, s._h, s._codec = None, None, None       # no handle: a device call would fail differently
    with pytest.raises(clb.ColBERTError, match="persist=True needs a Searcher opened from an index_path"):
        s.remove_passages([1], persist=True)
    assert hasattr(clb.Searcher, "remove_passages")
