"""The encoder at bert-base width in the regimes of tests/encoder_regimes.py -- rows with |mean| ~ 2 std in front of every LayerNorm
(`common_mode`), and on top of that outlier channels, wide GELU arguments and saturated sink heads (`trained_like`) -- against a
float64 evaluation of the same network, with the reference, the yardstick and the ONE constant of tests/test_gpu_encoder_shapes.py:
e_hip = max |HIP - float64| <= C_TOL * e32, e32 = max |torch fp32 - float64| over the same attended rows, C_TOL = 4, for f16x3,
f32 and bf16x6; bf16x3 must exceed it.  Every case asserts its plans through last_plans() first, then two runs with the same bits,
then every attended row.  tests/test_encoder_regimes_cpu.py asserts, without a device, that the regimes are reached.

Regimes, from the float64 model alone (tests/test_encoder_regimes_cpu.py asserts them; 32 x 32, seeds 0 to 2 | 64 x 300, seed 0):
                                      benign (test_gpu_encoder_shapes)   common_mode                    trained_like
    largest |x| a Linear / LN reads   10.6 to 11.1                       13.3 to 14.2 | 14.5            188 to 233 | 193
    |mean| / std of LN rows, median   0.02 (max 0.11)                    2.11 to 2.18 (max 3.2) | 2.12  0.46 to 0.60 (max 2.4) | 0.48 (max 2.65)
    largest |GELU argument|           7.2                                6.0 to 7.3 | 7.3               29.9 to 32.3 | 33.2
    largest |logit|, attended keys    8                                  6 to 7 | 8                     317 to 488 | 399
    rows with p_max > 0.999           none                               none                           sink heads 48 to 60 % | 42 %, other heads 0.4 to 6.5 %
    median p_max, other heads         0.17                               0.17 | 0.04                    0.43 to 0.53 | 0.20
    e32 on the host that wrote this   3.0 to 3.3e-06 (there)             4.7 to 5.3e-06 | 5.4e-06       1.47 to 1.80e-05 (spread 1.22 x) | 2.04e-05
  trained_like at 64 x 300: saturated rows by the key tile of their winning key 8 227, 5 486, 5 755, 6 213, 4 405, 5 372, 3 197, 2 669,
  125, 2 946 (all ten); in sequences 0, 1, 28 and 37 the winner is the last attended key of a tile that is not full (sequence 0: key
  299, the spike of encoder_regimes).  out_of_range: largest raw pre-LayerNorm value 5 315 with the trigger token ("hot"), 3 050
  without ("cold"; largest value read 3 121), GELU arguments to 642.

Measured on an MI355X (r = e_hip / e32; e32 from the CPU of that machine -- torch's fp32 kernels differ between hosts: the same
trained_like 32 x 32 batch gave e32 = 7.87e-06 there and 1.47e-05 where the regime table was written; float64 figures agree):
    case / entry point                          variant       plans asserted                                             e32       f16x3  f32   bf16x6 bf16x3
    1x32   doc                                  common_mode   64x64 ring 4, ks 8 (att / plain), ks 32 ln4; f16 planes      3.41e-06  0.59
    1x32   query_embeddings_device (+ graph)    common_mode   the same; replay == stream launches, bits                    2.51e-07  0.67
    1x32   doc                                  trained_like  the same                                                     5.55e-06  0.81
    1x32   query_embeddings_device (+ graph)    trained_like  the same                                                     9.45e-08  0.76
    32x32  doc                                  common_mode   64x64 ring 3, ks 2 / 4 ln4, projection ks 4 plain            3.91e-06  0.85   1.37  1.21   13.6
    32x32  query_embeddings_device (+ graph)    common_mode   the same (f32, bf16: attention_fused_kernel<1>)              3.03e-07  0.84   1.41  1.24   13.2
    32x32  doc                                  trained_like  the same                                                     7.87e-06  0.78   2.37  0.86   32.8
    32x32  query_embeddings_device (+ graph)    trained_like  the same                                                     1.04e-07  0.85   2.75  1.03   24.1
    128x32 doc, ln_fold 0 / 1                   common_mode   128x128 ks 2 ln4 / fold 128x128, folded Q/K/V 128x256        4.13e-06  1.13 / 2.40
    128x32 doc, ln_fold 0 / 1                   trained_like  the same                                                     7.51e-06  1.58 / 1.78
    129x32 doc (fold) / ln_fold 0               common_mode   fold 128x128, Q/K/V 128x256 / 64x64 ks 1 + layernorm_kernel  3.88e-06  2.23 / 1.64
    129x32 doc (fold) / ln_fold 0               trained_like  the same                                                     7.83e-06  1.69 / 1.97
    64x300 doc                                  trained_like  fold 256x256, Q/K/V 128x256; f16 planes QB 2, 10 key tiles   8.85e-06  2.17                 32.2
    64x300 doc_embeddings_device                trained_like  the same                                                     1.42e-07  1.89                 19.6
    64x300 doc, attention fused_f32             trained_like  the same Linears, attention_online_kernel                    8.85e-06  1.95
    64x300 doc, attention resident   (added)    trained_like  the same Linears, attention_fused_kernel<10>                 8.85e-06  1.76
    32x32  doc, attention unfused    (added)    trained_like  as 32x32; fp32 GEMMs around masked_softmax_kernel            7.87e-06  0.85
    packed 22 386 rows                          trained_like  packed; fold 128x256 at N = 768; f16 planes over cu          1.83e-07  1.12
    32x32  doc, dim 126              (added)    common_mode   no plane Linear: gemm_bf16split_kernel + reduce_ln<3>        3.91e-06                1.20
    32x32  doc, dim 126              (added)    trained_like  the same                                                     7.87e-06                0.94
    129x32 / 128x32 ln_fold 0 / packed, cold    out_of_range  fold / no fold / packed fold: nothing reported               9.7e-05 / 9.7e-05 / 4.7e-08  0.62 / 1.24 / 0.64
    129x32 / 128x32 ln_fold 0 / 282x300, hot    out_of_range  bf16x6, padded `doc`                                         1.2e-04                 2.28 / 1.20 / 2.28
The largest r of an fp32-faithful mode is 2.75 (fp32 MFMA, trained_like 32 x 32), of the default mode 2.40 (the fold forced on at
128 x 32, common_mode -- 1.13 without it: the mean . u cancellation shows, inside the bound); bf16x3 lies between 13 and 33.  No
ratio above C_TOL was met, so no bound is scaled and no kernel arithmetic changed.  What the range-edge cases did find: `doc`
(clb_encode) returned the NaN rows of an out-of-range batch as numbers -- the non-finite check sits in the epilogue kernels and
`doc` has none; it now runs that check on its own (nonfinite_rows_kernel) and raises DomainError like the other entry points.

Sites the table of the issue did not reach, added above: attention_fused_kernel with more than one key tile (attention="resident"),
masked_softmax_kernel (attention="unfused"), layernorm_kernel behind an unsplit f16x3 Linear (129x32, ln_fold 0) and
gemm_splitk_reduce_ln_kernel<3> (a projection width that is no multiple of 4 takes every Linear off the plane path).  NOT reachable
through BertEncoder at this width: gemm_splitk_reduce_ln_kernel<4> (the strided pass for 768 < N <= 1 024: a hidden size of 1 024).
The float64 + fp32 references of the module take about 25 s on 16 threads (packed 22 386 rows: 2 x 3 s).
"""
import numpy as np
import pytest

import colbert_jl_amd as clb
from tests import encoder_ladder as el
from tests import encoder_regimes as er
from tests import test_gpu_encoder_shapes as shapes
from tests.test_gpu_encoder_shapes import C_TOL, SKIP

pytestmark = pytest.mark.gpu

BOTH = ("common_mode", "trained_like")
# (case, variants, GEMM modes, encoder switches)
TABLE = [
    ("1x32", BOTH, ("f16x3",), {}),
    ("32x32", BOTH, ("f16x3", "f32", "bf16x6", "bf16x3"), {}),
    ("128x32", BOTH, ("f16x3",), dict(ln_fold=0)),
    ("128x32", BOTH, ("f16x3",), dict(ln_fold=1)),
    ("129x32", BOTH, ("f16x3",), {}),
    ("129x32", BOTH, ("f16x3",), dict(ln_fold=0)),                       # layernorm_kernel on its own behind an unsplit f16x3 Linear
    ("64x300", ("trained_like",), ("f16x3", "bf16x3"), {}),
    ("64x300", ("trained_like",), ("f16x3",), dict(attention="fused_f32")),
    ("64x300", ("trained_like",), ("f16x3",), dict(attention="resident")),   # attention_fused_kernel<10>: ten key tiles in registers
    ("32x32", ("trained_like",), ("f16x3",), dict(attention="unfused")),     # masked_softmax_kernel
    ("packed_22386", ("trained_like",), ("f16x3",), {}),
]
ATTENTION_KIND = {"fused_f32": "f32_online", "resident": "f32_resident", "unfused": "unfused"}


def _params():
    out = []
    for case, variants, gemms, kw in TABLE:
        for variant in variants:
            for gemm in gemms:
                name = "-".join([case, variant, gemm] + [f"{k}={v}" for k, v in kw.items()])
                out.append(pytest.param(case, variant, gemm, kw, id=name))
    return out


def _fold_expectation(case, gemm, kw):
    """The hand-written plan table of the case, where the ladder has one for these switches."""
    if gemm != "f16x3" or "attention" in kw:
        return None
    if "ln_fold" in kw:
        return el.LADDER_FOLD_VARIANTS[(case, kw["ln_fold"])]
    return el.LADDER[case]["expect"]


@pytest.mark.parametrize("case,variant,gemm,kw", _params())
def test_regime_case(case, variant, gemm, kw):
    """One ladder batch in one regime, GEMM mode and set of switches: plans, twice the same bits, every attended row; then the
    device entry points the batch is served through."""
    m = er.model(variant)
    torch = m["torch"]
    c = el.LADDER[case]
    ids0, lens, mask = shapes._inputs(case)
    packed = "rows" in c
    rows = el.case_rows(case)
    r64, r32 = er.reference(variant, case)
    ln_fold, attention = kw.get("ln_fold", -1), kw.get("attention", "fused")
    enc = clb.BertEncoder(m["w"], m["bcfg"], dim=el.DIM, gemm=gemm, **kw)
    got = shapes._run_case(enc, m, case)
    plans = shapes._assert_plans(enc, case, gemm, rows, c["L"], ln_fold=ln_fold, attention=attention,
                                 expect=_fold_expectation(case, gemm, kw), packed=packed)
    if attention != "fused":
        assert [p["kind"] for p in plans if p["stage"] == "attention"] == [ATTENTION_KIND[attention]] * 2
    again = shapes._run_case(enc, m, case)
    assert np.array_equal(shapes._bits(got), shapes._bits(again)), "two runs of the same batch differ"
    tag = f"{variant} {case}" + "".join(f" {k}={v}" for k, v in kw.items())
    ids_rows = ids0[mask]
    kept = ~np.isin(ids_rows + 1, SKIP)
    if packed:
        r, where = shapes._check(f"{tag} packed", gemm, got, r64, r32, plans, post=lambda x: shapes._normalised(x, ids_rows)[kept])
    else:
        r, where = shapes._check(f"{tag} doc", gemm, got, r64, r32, plans)
    if gemm == "bf16x3":
        assert r > C_TOL, f"{tag}: bf16x3 passes the bound of the fp32-faithful modes (r = {r:.2f}); {where}"
    d_skip = torch.tensor(SKIP, dtype=torch.int64, device="cuda")
    if case in shapes.QUERY_CASES and not kw:
        d_ids = torch.from_numpy((ids0 + 1).astype(np.int32)).cuda()
        d_mask = torch.from_numpy(mask.astype(np.uint8)).cuda()
        d_q = torch.full((ids0.shape[0], c["L"], el.DIM), float("nan"), dtype=torch.float32, device="cuda")
        enc.query_embeddings_device(d_ids, d_mask, d_skip, d_q)
        torch.cuda.synchronize()
        shapes._assert_plans(enc, case, gemm, rows, c["L"])
        q = d_q.cpu().numpy()
        assert np.all(q[~mask] == 0.0)
        shapes._check(f"{tag} query_embeddings_device", gemm, q[mask], r64, r32, plans, post=lambda x: shapes._normalised(x, ids_rows))
        d_g = torch.full_like(d_q, float("nan"))         # one captured graph replayed == the stream launches, bit for bit
        graph = enc.capture_query_graph(d_ids, d_mask, d_skip, d_g)
        d_g.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(shapes._bits(d_g.cpu().numpy()), shapes._bits(q)), "graph replay differs from the stream launches"
        del graph
    if case == "64x300" and not kw:
        d_ids = torch.from_numpy((ids0 + 1).astype(np.int32)).cuda()
        d_mask = torch.from_numpy(mask.astype(np.uint8)).cuda()
        embs, doclens = enc.doc_embeddings_device(d_ids, d_mask, d_skip)
        torch.cuda.synchronize()
        assert np.array_equal(doclens.cpu().numpy(), (mask & ~np.isin(ids0 + 1, SKIP)).sum(axis=1))
        shapes._check(f"{tag} doc_embeddings_device", gemm, embs.cpu().numpy(), r64, r32, plans,
                      post=lambda x: shapes._normalised(x, ids_rows)[kept])
    enc.check_last_ids()        # the sticky flag is clear
    enc.close()


@pytest.mark.parametrize("variant", BOTH)
def test_the_strided_layernorm_reduce_behind_linears_off_the_plane_path(variant):
    """gemm_splitk_reduce_ln_kernel<3> (split K + LayerNorm, one column per thread and pass) runs only when the Linears cannot take
    the plane path: a projection width that is no multiple of 4.  The 32 x 32 batch on the same model with the projection cut to
    126 outputs, default GEMM mode -- the Linears then split fp32 operands into three bf16 planes on the fly, six products
    (gemm_bf16split_kernel), ks 2 at K = 768 and 4 at K = 3072 in front of the LayerNorms -- against the first 126 columns of the
    same reference.  last_plans() records plane Linears only: that it holds none is the evidence that this path ran."""
    dim, case = 126, "32x32"
    m = er.model(variant)
    ids0, lens, mask = shapes._inputs(case)
    r64, r32 = er.reference(variant, case)
    enc = clb.BertEncoder(er.weights_narrowed(variant, dim), m["bcfg"], dim=dim)
    ids, jl_mask = (ids0.T + 1).astype(np.int32), mask.T
    got = enc.doc(ids, jl_mask)
    assert got.shape == (dim, ids0.shape[1], ids0.shape[0])
    plans = enc.last_plans()
    assert [p["stage"] for p in plans] == ["attention"] * 2 and all(p["kind"] == "f32_resident" for p in plans), plans
    assert np.array_equal(shapes._bits(got), shapes._bits(enc.doc(ids, jl_mask))), "two runs of the same batch differ"
    shapes._check(f"{variant} {case} dim {dim} doc", "bf16x6", got.transpose(2, 1, 0)[mask], r64[:, :dim], r32[:, :dim], plans)
    enc.check_last_ids()
    enc.close()


# ---- the range edge at production width ------------------------------------------------------------------------------------
EDGE_CASES = [("129x32", {}), ("128x32", dict(ln_fold=0)), ("packed_22386", {})]
EDGE_IDS = ["129x32-fold", "128x32-ln_fold=0", "packed_22386"]


class _Edge:
    """The entry points of one encoder on the hot / cold inputs of a case."""

    def __init__(self, case, gemm, kw):
        self.case, self.m = case, er.model("out_of_range")
        self.torch = self.m["torch"]
        self.enc = clb.BertEncoder(self.m["w"], self.m["bcfg"], dim=el.DIM, gemm=gemm, **kw)
        self.d_skip = self.torch.tensor(SKIP, dtype=self.torch.int64, device="cuda")

    def host(self, kind):
        ids0, lens, mask = er.inputs(self.case, 0, kind)
        return (ids0.T + 1).astype(np.int32), mask.T

    def doc_rows(self, kind):
        """`doc` on the padded batch -> the attended rows."""
        ids0, lens, mask = er.inputs(self.case, 0, kind)
        return self.enc.doc(*self.host(kind)).transpose(2, 1, 0)[mask]

    def device(self, kind, which):
        """One device entry point, enqueued and waited for -> its output as an array (the flag is not read)."""
        torch = self.torch
        ids0, lens, mask = er.inputs(self.case, 0, kind)
        if which == "packed":
            d = shapes._packed_device_inputs(torch, ids0, lens, mask)
            out = self.enc.doc_embeddings_packed_device(*d, int(lens.max()), self.d_skip)[0]
        else:
            d_ids = torch.from_numpy((ids0 + 1).astype(np.int32)).cuda()
            d_mask = torch.from_numpy(mask.astype(np.uint8)).cuda()
            if which == "query":
                out = torch.full(ids0.shape + (el.DIM,), float("nan"), dtype=torch.float32, device="cuda")
                self.enc.query_embeddings_device(d_ids, d_mask, self.d_skip, out)
            else:
                out = self.enc.doc_embeddings_device(d_ids, d_mask, self.d_skip)[0]
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def entry_points(self):
        return ("query", "docs", "packed")


def _assert_edge_regime(case):
    hot = er.statistics("out_of_range", case, 0, attention=False, kind="hot")
    cold = er.statistics("out_of_range", case, 0, attention=False, kind="cold")
    assert er.PLANE_RANGE <= hot["biggest_raw"] < 2 * er.PLANE_RANGE and er.PLANE_RANGE <= hot["biggest"] < 2 * er.PLANE_RANGE, hot
    assert 2048 <= cold["biggest_raw"] < er.PLANE_RANGE and cold["biggest"] < er.PLANE_RANGE, cold


@pytest.mark.parametrize("case,kw", EDGE_CASES, ids=EDGE_IDS)
def test_an_activation_beyond_the_planes_is_reported_and_the_encoder_recovers(case, kw):
    """f16x3, the largest raw pre-LayerNorm value of the float64 reference in [4 094, 8 188): the host entry points raise
    DomainError, the device entry points leave the sticky flag set; the next batch inside the range -- the same one without the
    trigger token -- leaves it clear and has the bits a fresh encoder returns."""
    _assert_edge_regime(case)
    e = _Edge(case, "f16x3", kw)
    fresh = _Edge(case, "f16x3", kw)
    want = {which: fresh.device("cold", which) for which in e.entry_points()}
    fresh.enc.check_last_ids()
    fresh.enc.close()
    with pytest.raises(clb.DomainError):
        e.enc.doc(*e.host("hot"))
    with pytest.raises(clb.DomainError):
        e.enc.query_embeddings(SKIP, *e.host("hot"))
    for which in e.entry_points():
        e.device("hot", which)
        with pytest.raises(clb.DomainError):
            e.enc.check_last_ids()
        got = e.device("cold", which)
        e.enc.check_last_ids()
        assert np.isfinite(got).all(), which
        assert np.array_equal(shapes._bits(got), shapes._bits(want[which])), f"{which}: differs from a fresh encoder after a reported batch"
    e.enc.close()


@pytest.mark.parametrize("case,kw", EDGE_CASES, ids=EDGE_IDS)
def test_just_inside_the_planes_range_nothing_is_reported_and_the_bound_holds(case, kw):
    """f16x3, the largest raw value in [2 048, 4 094): no report, every attended row within the bound."""
    _assert_edge_regime(case)
    e = _Edge(case, "f16x3", kw)
    ids0, lens, mask = er.inputs(case, 0, "cold")
    r64, r32 = er.reference("out_of_range", case, 0, "cold")
    ids_rows = ids0[mask]
    kept = ~np.isin(ids_rows + 1, SKIP)
    tag = f"inside the edge {case}" + "".join(f" {k}={v}" for k, v in kw.items())
    if "rows" in el.LADDER[case]:
        got = e.device("cold", "packed")
        post = lambda x: shapes._normalised(x, ids_rows)[kept]      # noqa: E731
    else:
        got, post = e.doc_rows("cold"), None
    plans = shapes._assert_plans(e.enc, case, "f16x3", el.case_rows(case), el.LADDER[case]["L"], ln_fold=kw.get("ln_fold", -1),
                                 expect=_fold_expectation(case, "f16x3", kw), packed="rows" in el.LADDER[case])
    e.enc.check_last_ids()
    shapes._check(tag, "f16x3", got, r64, r32, plans, post=post)
    e.enc.close()


@pytest.mark.parametrize("case,kw", EDGE_CASES, ids=EDGE_IDS)
def test_bf16x6_covers_what_the_fp16_planes_cannot_hold(case, kw):
    """The inputs f16x3 reports, on three bf16 planes (the whole fp32 exponent range): finite and within the bound.  (A packed
    batch needs the f16x3 Linears: in this mode its 282 passages are served padded, as the indexer does.)"""
    _assert_edge_regime(case)
    e = _Edge(case, "bf16x6", kw)
    r64, r32 = er.reference("out_of_range", case, 0, "hot")
    got = e.doc_rows("hot")
    plans = e.enc.last_plans()
    e.enc.check_last_ids()
    shapes._check(f"beyond the edge {case}", "bf16x6", got, r64, r32, plans)
    e.enc.close()
