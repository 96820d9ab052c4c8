# Searcher / search (src/searching.jl).  The arrays the reference keeps in host memory (codes, residuals, ivf,
# emb2pid, ...) are uploaded once into HBM and live behind `handle`.

mutable struct Searcher
    config::ColBERTConfig
    checkpoint::Checkpoint
    tokenizer::WordPieceTokenizer
    skiplist::Vector{Int}
    handle::Ptr{Cvoid}
    num_documents::Int
    function Searcher(config, checkpoint, tokenizer, skiplist, handle, num_documents)
        s = new(config, checkpoint, tokenizer, skiplist, handle, num_documents)
        finalizer(s -> _searcher_destroy(s.handle), s)
    end
end

"""
    Searcher(index_path::String)

Open an index directory (src/searching.jl:18-80): config.json, the checkpoint it names, the codec, the IVF, every
chunk's doclens / codes / residuals.  `emb2pid` (:82-91) is built by the library on the device.
"""
function Searcher(index_path::String; device::Int = 0)
    isdir(index_path) || error("Index at $(index_path) does not exist! Please build the index first and try again.")
    config = load_config(index_path)
    tokenizer, ckpt = load_hgf_pretrained_local(config.checkpoint; device = device)
    codec = load_codec(index_path)
    ivf = JLD2.load_object(joinpath(index_path, "ivf.jld2"))::Vector{Int}
    ivf_lengths = JLD2.load_object(joinpath(index_path, "ivf_lengths.jld2"))::Vector{Int}
    doclens = load_doclens(index_path)
    codes, residuals = load_compressed_embs(index_path)
    handle = _searcher_create(config.nbits, codec["centroids"], codec["bucket_weights"], doclens, codes, residuals,
        ivf, ivf_lengths; device = device)
    skiplist = Int[lookup(tokenizer, "[PAD]")]         # only the pad symbol (searching.jl:62)
    Searcher(config, ckpt, tokenizer, skiplist, handle, length(doclens))
end

"""
    add_compressed!(searcher, codes, residuals, doclens) -> UnitRange{Int}

Append passages that were compressed with the index's own codec (`compress` with its centroids and bucket cutoffs) behind
the searcher's last passage, without rebuilding the resident index; returns their pids.  Afterwards `search` answers as a
`Searcher` opened on the concatenated index would.  A `PassageFilter` made before the call is refused by `search`: make
another.  On an exception the searcher is unchanged.  No counterpart in the reference (upstream ColBERT: IndexUpdater.add).
"""
function add_compressed!(searcher::Searcher, codes::Vector{UInt32}, residuals::Matrix{UInt8}, doclens::Vector{Int})
    size(residuals, 2) == length(codes) ||
        throw(DimensionMismatch("residuals must have one column per code ($(length(codes))), got $(size(residuals, 2))"))
    first_pid = searcher.num_documents + 1
    _searcher_append(searcher.handle, doclens, codes, residuals)
    searcher.num_documents = _searcher_num_docs(searcher.handle)
    first_pid:searcher.num_documents
end
"""
    remove_passages!(searcher, pids) -> Int

Remove passages from the resident index without rebuilding it; `pids` as `search` returns them (any order, duplicates
allowed; outside 1:num_documents is a BoundsError).  Pids are stable: a removed passage stays in the numbering as an empty
passage, `num_documents` does not change and `add_compressed!` numbers from `num_documents + 1` as before.  Returns how many
passages lost embeddings.  Afterwards `search` answers as a `Searcher` opened on the reduced index would; a `PassageFilter`
made before the call stays valid.  On an exception the searcher is unchanged.  No counterpart in the reference (upstream
ColBERT: IndexUpdater.remove).
"""
remove_passages!(searcher::Searcher, pids::Vector{Int}) = _searcher_remove(searcher.handle, pids)
"""
    update_passages!(searcher, pids, codes, residuals, doclens) -> Int

Replace the content of passages in place: passage `pids[i]` loses its embeddings and receives the next `doclens[i]` columns of
`codes` / `residuals` (compressed with the index's own codec, as for `add_compressed!`).  Pids are stable -- no other passage
moves, `num_documents` does not change -- a doclen of 0 empties a passage as `remove_passages!` does, and an empty passage
may be filled again.  Each pid may be named once (twice is an ArgumentError).  Returns how many named passages had or have
embeddings.  Afterwards `search` answers as a `Searcher` opened on the changed index would; a `PassageFilter` made before the
call stays valid.  On an exception the searcher is unchanged.  No counterpart in the reference or in upstream ColBERT.
"""
function update_passages!(searcher::Searcher, pids::Vector{Int}, codes::Vector{UInt32}, residuals::Matrix{UInt8}, doclens::Vector{Int})
    size(residuals, 2) == length(codes) ||
        throw(DimensionMismatch("residuals must have one column per code ($(length(codes))), got $(size(residuals, 2))"))
    length(pids) == length(doclens) ||
        throw(DimensionMismatch("one doclen per pid: $(length(pids)) pids, $(length(doclens)) doclens"))
    _searcher_update(searcher.handle, pids, doclens, codes, residuals)
end
"number of `add_compressed!` / `remove_passages!` / `update_passages!` calls that changed the searcher"
generation(searcher::Searcher) = _searcher_generation(searcher.handle)
num_embeddings(searcher::Searcher) = _searcher_num_embeddings(searcher.handle)

"""
    search(searcher, query::String, k::Int; filter = nothing, scope = :candidates) -> (pids::Vector{Int}, scores::Vector{Float32})

Same contract as src/searching.jl:93-128: 1-based pids by descending score, ties by ascending pid; a BoundsError if
fewer than `k` passages are candidates.  `filter` / `scope`: see the method on query embeddings below.
"""
function search(searcher::Searcher, query::String, k::Int; filter = nothing, scope::Symbol = :candidates)
    c = searcher.config
    Q = encode_queries(searcher.checkpoint, searcher.tokenizer, [query], c.dim, c.index_bsize, c.query_token,
        c.attend_to_mask_tokens, searcher.skiplist, c.query_maxlen)
    @assert size(Q)[3]==1 "size(Q): $(size(Q))"
    @assert isequal(size(Q)[2], c.query_maxlen) "size(Q): $(size(Q)), query_maxlen: $(c.query_maxlen)"
    search(searcher, reshape(Q, size(Q, 1), size(Q, 2)), k; filter = filter, scope = scope)
end

"""
    PassageFilter(searcher; pids)            # or: PassageFilter(searcher; mask)

A set of passages resident on the device, for `search(...; filter = f)`: `pids` as `search` returns them (1-based, any
order, duplicates allowed; outside 1:num_documents is a BoundsError), or `mask`, one Bool per passage.  Made once,
reused over any number of searches of that searcher; freed by its finalizer (after or before the searcher's).
"""
mutable struct PassageFilter
    searcher::Searcher          # keeps the searcher alive as long as the filter
    handle::Ptr{Cvoid}
    count::Int
    function PassageFilter(searcher::Searcher; pids::Union{Nothing, AbstractVector{<:Integer}} = nothing,
            mask::Union{Nothing, AbstractVector{Bool}} = nothing)
        isnothing(pids) == isnothing(mask) && throw(ArgumentError("PassageFilter takes exactly one of pids and mask"))
        if isnothing(pids)
            length(mask) == searcher.num_documents ||
                throw(ArgumentError("mask must have num_documents = $(searcher.num_documents) entries"))
            words = zeros(UInt32, cld(length(mask), 32))
            for i in findall(mask)
                words[(i - 1) >> 5 + 1] |= UInt32(1) << ((i - 1) & 31)
            end
            handle = _filter_create_bitmap(searcher.handle, words)
        else
            handle = _filter_create_pids(searcher.handle, Vector{Int}(pids))
        end
        f = new(searcher, handle, _filter_count(handle))
        finalizer(f -> _filter_destroy(f.handle), f)
    end
end
Base.length(f::PassageFilter) = f.count

_filter_scope(scope::Symbol) = scope === :candidates ? 0 : scope === :all ? 1 :
                               throw(ArgumentError("scope must be :candidates or :all, got $(repr(scope))"))

"""
    search(searcher, Q::Matrix{Float32}, k; filter = nothing, scope = :candidates)

Search from query embeddings (dim, query_maxlen).  With a `PassageFilter` only its passages are ranked -- `scope =
:candidates`: the query's candidates that are in the filter; `:all`: every passage of the filter (a re-rank of that
list) -- and a short result is not an error: both vectors have k entries, padded with pid 0 / -Inf32.
"""
function search(searcher::Searcher, Q::Matrix{Float32}, k::Int; filter::Union{Nothing, PassageFilter} = nothing,
        scope::Symbol = :candidates)
    sc = _filter_scope(scope)
    isnothing(filter) && return _search(searcher.handle, Q, searcher.config.nprobe, k)
    GC.@preserve filter begin
        pids, scores, _ = _search_filtered(searcher.handle, Q, searcher.config.nprobe, k, filter.handle, sc)
    end
    pids, scores
end
