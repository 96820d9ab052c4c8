"""The regimes of tests/encoder_regimes.py, asserted from the float64 reference alone (no device): conditions, not tolerances --
they keep the comparison of tests/test_gpu_encoder_regimes.py from drifting back into the benign regime of
tests/test_gpu_encoder_shapes.py (largest |activation| 10.8, |mean| / std 0.02, GELU arguments within 7, logits within 8, no
saturated row).  The 32 x 32 batch with seeds 0 to 2, and the 64 x 300 batch with seed 0."""
import numpy as np
import pytest

pytest.importorskip("torch")
pytest.importorskip("transformers")

from tests import encoder_regimes as er      # noqa: E402

BATCHES = [("32x32", 0), ("32x32", 1), ("32x32", 2), ("64x300", 0)]
SINK = list(er.SINK_HEADS)


def _stats(variant, case, seed):
    s = er.statistics(variant, case, seed)
    print(f"[regime {variant} {case} seed {seed}] {er.summary(s)}")
    return s


@pytest.mark.parametrize("case,seed", BATCHES)
def test_common_mode_offsets_every_layernorm_row_and_nothing_else(case, seed):
    s = _stats("common_mode", case, seed)
    assert np.median(s["mean_over_std"]) >= 1.5
    assert s["biggest"] < 64
    saturated = (s["pmax"] > 0.999).mean(axis=(0, 2))           # per head
    assert (saturated <= 1e-3).all(), saturated


@pytest.mark.parametrize("case,seed", BATCHES)
def test_trained_like_has_outlier_channels_wide_gelu_arguments_and_sink_heads(case, seed):
    s = _stats("trained_like", case, seed)
    assert 64 <= s["biggest"] < 2048, s["biggest"]              # six times the benign value, at most half the plane range
    assert s["gelu"] >= 16, s["gelu"]
    assert s["logit"] >= 100, s["logit"]
    sink = s["pmax"][:, SINK]
    other = np.delete(s["pmax"], SINK, axis=1)
    assert (sink > 0.999).mean() >= 0.40, (sink > 0.999).mean()
    assert np.median(other) < 0.7, np.median(other)             # unsaturated heads are still there


def test_trained_like_puts_the_winning_key_in_every_key_tile_and_at_the_end_of_the_tail_tile():
    s = _stats("trained_like", "64x300", 0)
    saturated = s["pmax"] > 0.999
    tiles = np.bincount(s["tile"][saturated].ravel(), minlength=10)
    print("[regime trained_like 64x300] saturated rows by the key tile of their winner:", tiles.tolist(),
          "; sequences whose winner is the last attended key of a tile that is not full:", s["last_in_tail"])
    assert tiles.size == 10 and (tiles > 0).all(), tiles
    assert len(s["last_in_tail"]) >= 1
    assert 0 in s["last_in_tail"]                               # the full-length sequence: key 299, tile 9 holds 12 keys


@pytest.mark.parametrize("variant", er.VARIANTS)
def test_the_yardstick_is_stable_over_seeds(variant):
    e32 = [er.statistics(variant, "32x32", seed)["e32"] for seed in range(3)]
    print(f"[regime {variant}] e32 of seeds 0 to 2: {['%.3g' % e for e in e32]}")
    assert max(e32) < 2 * min(e32), e32


@pytest.mark.parametrize("case", ["129x32", "128x32", "packed_22386"])
def test_one_token_id_moves_the_range_edge_variant_across_the_plane_range(case):
    """out_of_range with the trigger id ("hot"): the largest raw pre-LayerNorm value AND the largest value a Linear or a LayerNorm
    reads in [4 094, 8 188); without it ("cold"): the raw value in [2 048, 4 094), nothing read beyond."""
    hot = er.statistics("out_of_range", case, 0, attention=False, kind="hot")
    cold = er.statistics("out_of_range", case, 0, attention=False, kind="cold")
    print(f"[regime out_of_range {case} hot] {er.summary(hot)}\n[regime out_of_range {case} cold] {er.summary(cold)}")
    assert er.PLANE_RANGE <= hot["biggest_raw"] < 2 * er.PLANE_RANGE
    assert er.PLANE_RANGE <= hot["biggest"] < 2 * er.PLANE_RANGE
    assert 2048 <= cold["biggest_raw"] < er.PLANE_RANGE
    assert cold["biggest"] < er.PLANE_RANGE
