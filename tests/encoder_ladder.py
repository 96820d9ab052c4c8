"""The shape ladder of the encoder at bert-base width, as data: which batches tests/test_gpu_encoder_shapes.py runs, and which
tile plan every Linear of each batch must take.  tests/test_capi_cpu.py imports the same table to check, without a GPU, that
every plan a production shape takes is one the ladder runs and compares with the float64 reference.

Nothing here needs a device: plans come from the library's pure plan function (colbert_jl_amd.encoder_plan)."""
import numpy as np

import colbert_jl_amd as clb
from colbert_jl_amd.encoder import EPI_BIAS, EPI_GELU, EPI_RESID

HIDDEN, HEADS, INTER, DIM, MAX_POS, VOCAB = 768, 12, 3072, 128, 512, 1000
SHORT_BATCH_ROWS = 4096        # forward(): split-K scratch exists up to here, the LayerNorm fold turns on by itself above
ONE_QUERY_ROWS = 64            # ... and up to here the wide outputs (Q/K/V, FFN-in) are split over K too
PACK_ROWS_DEFAULT = 170 * 256  # the default of COLBERT_PACK_ROWS (colbert_jl_amd.indexer)
# what the product and the benchmark run: one query, 32 queries, the serving shape, 64 x 300 passages, a full packed batch
PRODUCTION_ROWS = (32, 1024, 4096, 19200, PACK_ROWS_DEFAULT)
STAGES = ("linear_qkv", "linear_attn_out_ln", "linear_ffn_in_gelu", "linear_ffn_out_ln", "linear_projection")


def predict_plans(gemm, rows, L, layers=2, ln_fold=-1, attention="fused", hidden=HIDDEN, inter=INTER, dim=DIM):
    """What BertEncoder.last_plans() must report for a batch of `rows` rows (sequences up to L) -- forward()'s switches on the
    row count restated, every tile plan asked of the library.  The GPU tests compare this with what was launched, so a change of
    forward() that this function does not follow fails there."""
    if gemm == "f32":
        planes = att16 = fold = False
    else:
        planes = True
        att16 = gemm == "f16x3" and attention == "fused"
        fold = gemm == "f16x3" and (ln_fold == 1 or (ln_fold < 0 and rows > SHORT_BATCH_ROWS))
    part = rows <= SHORT_BATCH_ROWS
    part_wide = rows <= ONE_QUERY_ROWS
    H, I = hidden, inter
    out = []

    def lin(stage, layer, N, K, epi, **kw):
        if planes:
            p = clb.encoder_plan(gemm, rows, N, K, epi, **kw)
            out.append(dict(stage=stage, layer=layer, M=rows, N=N, K=K, fold=bool(kw.get("fold")), att=bool(kw.get("att")), **p))

    for l in range(layers):
        if fold and l >= 1:
            lin("linear_qkv", l, 3 * H, H, EPI_BIAS, fold=True, fold_u=True, att=att16)
        else:
            lin("linear_qkv", l, 3 * H, H, EPI_BIAS, part=part_wide, att=att16)
        if attention == "unfused":
            kind, qb = "unfused", 0
        elif att16:
            kind, qb = "f16_planes", 2 if L >= 128 else 1
        else:
            kind, qb = ("f32_online" if L > 64 and attention != "resident" else "f32_resident"), 0
        out.append(dict(stage="attention", layer=l, M=rows, N=L, K=H // HEADS, att=att16, query_blocks=qb, key_tiles=(L + 31) // 32,
                        kind=kind))
        if fold:
            lin("linear_attn_out_ln", l, H, H, EPI_BIAS | EPI_RESID, fold=True, fold_stats=True)
            lin("linear_ffn_in_gelu", l, I, H, EPI_BIAS | EPI_GELU, fold=True, fold_u=True)
            lin("linear_ffn_out_ln", l, H, I, EPI_BIAS | EPI_RESID, fold=True, fold_stats=True)
        else:
            lin("linear_attn_out_ln", l, H, H, EPI_BIAS | EPI_RESID, part=part, ln=True)
            lin("linear_ffn_in_gelu", l, I, H, EPI_BIAS | EPI_GELU, part=part_wide)
            lin("linear_ffn_out_ln", l, H, I, EPI_BIAS | EPI_RESID, part=part, ln=True)
    if fold:
        lin("linear_projection", layers, dim, H, EPI_BIAS, fold=True, fold_u=True)
    else:
        lin("linear_projection", layers, dim, H, EPI_BIAS, part=part)
    return out


def signature(rec):
    """(role, tile, ring stages, K slices, reduce pass, fold) of a Linear record: what the coverage guard counts as one plan."""
    return (rec["stage"], tuple(rec["tile"]), rec["stages"], rec["ks"], rec["reduce"], bool(rec["fold"]))


def _p(tile, stages=2, ks=1, reduce="none", fold=False):
    return (tile, stages, ks, reduce, fold)


T64, T128, T128x256, T256 = (64, 64), (128, 128), (128, 256), (256, 256)
_LONG_FOLDED_19200 = {      # 64 x 300 and the full packed batch: pick_long_tile by rounds; layer 0's Q/K/V has no LayerNorm in front
    ("linear_qkv", 0): _p(T128x256), ("linear_qkv", 1): _p(T128x256, fold=True),
    ("linear_attn_out_ln", None): _p(T256, fold=True), ("linear_ffn_in_gelu", None): _p(T128, fold=True),
    ("linear_ffn_out_ln", None): _p(T256, fold=True)}

# (The folded Q/K/V projection of layers >= 1 goes by pick_long_tile alone -- the fold branch has no `att` exception -- so from
# 4 096 rows on it runs 128 x 256 where layer 0's unfolded one runs 128 x 128.)
# One entry per batch of the ladder.  `expect`: the plan every Linear role must take in the DEFAULT mode (f16x3, ln_fold -1,
# fused attention), keyed by (stage, layer or None = every layer) -> (tile, stages, ks, reduce, fold): written down by hand from
# the rule, so that a case whose shape no longer reaches the path it is named after fails.  `att`: (kind, query blocks, key tiles).
LADDER = {
    # ONE text query: the M <= 64 rule -- four-buffer ring, every Linear split over K (8 slices at K = 768 behind <= 48 column
    # tiles, 32 at K = 3072), the wide outputs too (the EPI_QKV_ATT reduce pass)
    "1x32": dict(N=1, L=32, expect={
        ("linear_qkv", None): _p(T64, 4, 8, "att"), ("linear_attn_out_ln", None): _p(T64, 4, 8, "ln4"),
        ("linear_ffn_in_gelu", None): _p(T64, 4, 8, "plain"), ("linear_ffn_out_ln", None): _p(T64, 4, 32, "ln4"),
        ("linear_projection", None): _p(T64, 4, 8, "plain")}, att=("f16_planes", 1, 1)),
    "2x32": dict(N=2, L=32, expect={         # 64 rows: the last batch of the one-query rule
        ("linear_qkv", None): _p(T64, 4, 8, "att"), ("linear_attn_out_ln", None): _p(T64, 4, 8, "ln4"),
        ("linear_ffn_in_gelu", None): _p(T64, 4, 8, "plain"), ("linear_ffn_out_ln", None): _p(T64, 4, 32, "ln4"),
        ("linear_projection", None): _p(T64, 4, 8, "plain")}, att=("f16_planes", 1, 1)),
    "5x13": dict(N=5, L=13, expect={         # 65 rows: the first of the query-batch rule (two tile rows: fewer than 64 tiles at
        # N = 768, so slices go down to 192 -- ks 4 at K = 768, 8 at K = 3072)
        ("linear_qkv", None): _p(T64), ("linear_attn_out_ln", None): _p(T64, 3, 4, "ln4"),
        ("linear_ffn_in_gelu", None): _p(T64), ("linear_ffn_out_ln", None): _p(T64, 3, 8, "ln4"),
        ("linear_projection", None): _p(T64, 3, 4, "plain")}, att=("f16_planes", 1, 1)),
    "32x32": dict(N=32, L=32, expect={       # 32 queries per encode: 64 x 64, three-tile ring, ks 2 / 4 / 4
        ("linear_qkv", None): _p(T64), ("linear_attn_out_ln", None): _p(T64, 3, 2, "ln4"),
        ("linear_ffn_in_gelu", None): _p(T64), ("linear_ffn_out_ln", None): _p(T64, 3, 4, "ln4"),
        ("linear_projection", None): _p(T64, 3, 4, "plain")}, att=("f16_planes", 1, 1)),
    "128x32": dict(N=128, L=32, expect={     # the serving shape: the `att` exception, two-slice 128 x 128 + reduce_ln4
        ("linear_qkv", None): _p(T128), ("linear_attn_out_ln", None): _p(T128, 2, 2, "ln4"),
        ("linear_ffn_in_gelu", None): _p(T128), ("linear_ffn_out_ln", None): _p(T128, 2, 2, "ln4"),
        ("linear_projection", None): _p(T64, 3, 2, "plain")}, att=("f16_planes", 1, 1)),
    "129x32": dict(N=129, L=32, expect={     # 4 128 rows: no scratch, the fold on by itself, below one 128 x 128 tile per CU at N = 768
        ("linear_qkv", 0): _p(T128), ("linear_qkv", 1): _p(T128x256, fold=True),
        ("linear_attn_out_ln", None): _p(T128, fold=True), ("linear_ffn_in_gelu", None): _p(T128, fold=True),
        ("linear_ffn_out_ln", None): _p(T128, fold=True), ("linear_projection", None): _p(T64, fold=True)},
        att=("f16_planes", 1, 1)),
    "42x128": dict(N=42, L=128, expect={     # 252 tiles of 128 x 128 at N = 768: the fold branch keeps 128 x 128
        ("linear_qkv", 0): _p(T128), ("linear_qkv", 1): _p(T128x256, fold=True),
        ("linear_attn_out_ln", None): _p(T128, fold=True), ("linear_ffn_in_gelu", None): _p(T128, fold=True),
        ("linear_ffn_out_ln", None): _p(T128, fold=True), ("linear_projection", None): _p(T64, fold=True)},
        att=("f16_planes", 2, 4)),
    "43x128": dict(N=43, L=128, expect={     # 258 tiles: pick_long_tile takes over (129 tiles of 128 x 256 in one round)
        ("linear_qkv", 0): _p(T128), ("linear_qkv", 1): _p(T128x256, fold=True),
        ("linear_attn_out_ln", None): _p(T128x256, fold=True), ("linear_ffn_in_gelu", None): _p(T128, fold=True),
        ("linear_ffn_out_ln", None): _p(T128x256, fold=True), ("linear_projection", None): _p(T64, fold=True)},
        att=("f16_planes", 2, 4)),
    "64x300": dict(N=64, L=300, expect={**_LONG_FOLDED_19200, ("linear_projection", None): _p(T64, fold=True)},
                   att=("f16_planes", 2, 10)),
    # packed batches (rows = attended tokens only): the default row budget, and the size where the round rule flips N = 768
    # from 256 x 256 (264 tiles: two rounds) to 128 x 256
    "packed_43520": dict(rows=PACK_ROWS_DEFAULT, L=300, expect={**_LONG_FOLDED_19200, ("linear_projection", None): _p(T64, fold=True)},
                         att=("f16_planes", 2, 10)),
    "packed_22386": dict(rows=22386, L=300, expect={
        ("linear_qkv", 0): _p(T128x256), ("linear_qkv", 1): _p(T128x256, fold=True),
        ("linear_attn_out_ln", None): _p(T128x256, fold=True), ("linear_ffn_in_gelu", None): _p(T128, fold=True),
        ("linear_ffn_out_ln", None): _p(T128x256, fold=True), ("linear_projection", None): _p(T64, fold=True)},
        att=("f16_planes", 2, 10)),
}
# the same batch with the fold forced the other way (ln_fold 0 at 4 128 rows, 1 at 4 096): both sides of `short_batch` in both states
LADDER_FOLD_VARIANTS = {
    ("128x32", 1): {("linear_qkv", 0): _p(T128), ("linear_qkv", 1): _p(T128x256, fold=True),
                    ("linear_attn_out_ln", None): _p(T128, fold=True), ("linear_ffn_in_gelu", None): _p(T128, fold=True),
                    ("linear_ffn_out_ln", None): _p(T128, fold=True), ("linear_projection", None): _p(T64, fold=True)},
    ("128x32", 0): LADDER["128x32"]["expect"],
    ("129x32", 0): {("linear_qkv", None): _p(T128), ("linear_attn_out_ln", None): _p(T64), ("linear_ffn_in_gelu", None): _p(T128),
                    ("linear_ffn_out_ln", None): _p(T64), ("linear_projection", None): _p(T64)},
}


def case_rows(case):
    c = LADDER[case]
    return c["rows"] if "rows" in c else c["N"] * c["L"]


def expected_signatures(expect):
    """The hand-written table of a case as the set of signatures the coverage guard compares."""
    return {(stage,) + tuple(plan) for (stage, _layer), plan in expect.items()}


def check_expectation(expect, att, recs, layers=2):
    """Every Linear record of `recs` (last_plans() or predict_plans()) against the hand-written table of its case."""
    seen = set()
    for r in recs:
        if r["stage"] == "attention":
            if att is not None:
                assert (r["kind"], r["query_blocks"], r["key_tiles"]) == tuple(att), (r, att)
            continue
        layer = min(r["layer"], 1)                      # layers >= 1 share a plan (their Q/K/V has a LayerNorm in front of it)
        key = (r["stage"], layer) if (r["stage"], layer) in expect else (r["stage"], None)
        assert key in expect, (key, sorted(expect))
        assert signature(r)[1:] == tuple(expect[key]), (r, expect[key])
        seen.add(key)
    assert seen == set(expect), set(expect) - seen


def lengths(case, seed=0):
    """Ragged sequence lengths of a ladder entry: one full-length sequence, one of length 1, random otherwise.  A packed entry:
    passage lengths with a mean near 80 and a maximum of 300 that sum to exactly its row count."""
    c = LADDER[case]
    rng = np.random.default_rng(1000 + seed + sum(map(ord, case)))
    if "rows" in c:
        rows, L = c["rows"], c["L"]
        lens = [L, 1]
        while sum(lens) < rows:
            lens.append(int(min(L, max(2, rng.gamma(2.2, 36.0)))))
        lens[-1] -= sum(lens) - rows
        if lens[-1] < 1:
            lens[-2] += lens[-1] - 1; lens[-1] = 1
        lens = np.array(lens, dtype=np.int64)
        assert lens.sum() == rows and lens.min() >= 1 and lens.max() == L
        return lens[rng.permutation(lens.size)]
    N, L = c["N"], c["L"]
    lens = rng.integers(1, L + 1, size=N)
    lens[0] = L
    if N >= 2:
        lens[N - 1] = 1
    return lens.astype(np.int64)
