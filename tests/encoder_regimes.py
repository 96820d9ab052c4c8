"""The statistical regimes the encoder is compared in beyond the benign one of tests/test_gpu_encoder_shapes.py: weight surgery
on the model that module builds (bert-base width, 2 layers, WEIGHT_SCALE 2), and the statistics -- from the float64 model alone --
that prove a regime is reached.  No tests here; tests/test_encoder_regimes_cpu.py asserts the regimes without a device,
tests/test_gpu_encoder_regimes.py compares the HIP encoder in them.

Variants.
    common_mode   COMMON_OFFSET added to every attention.output.dense.bias and output.dense.bias, EMBED_OFFSET to token_type_embeddings[0]:
                  every row a LayerNorm reads (embedding, stand-alone, split-K reduce, fold) has |mean| of the order of twice
                  its standard deviation.  Nothing else changes.  (The embedding offset is small because embedding rows are:
                  standard deviation 0.07.  The layers' 4.0 there puts |mean| / std at 60, where any fp32 evaluation loses
                  digits: e32 then triples and varies 3.8 x over three seeds -- no yardstick.)
    trained_like  common_mode, plus
                  - OUTLIER_CHANNELS of EVERY LayerNorm get gamma OUTLIER_GAMMA and beta OUTLIER_BETA * beta_scale: the residual
                    stream carries tens to hundreds there, through every layer;
                  - sink heads: for head h of SINK_HEADS, row 64 h of the key weight reads SINK_CHANNELS[h] with weight 1 and
                    nothing else, row 64 h of the query weight is zero and its bias SINK_QUERY_BIAS * (2 + h): the logit of key j
                    is (2 + h) * x_j[channel] (+ the 63 benign dimensions), whatever the query and the position -- the sink of a
                    sequence is the attended token that is largest in that channel.  Two heads read channel 101, two channel
                    308, so that a sequence has two different sinks per layer;
                  - position_embeddings[SPIKE_POSITION] gets a spike in the two sink channels: the LAST token of a full-length
                    (300) sequence wins its sink heads in the first layer -- the last attended key of the tail tile (300 = 9 * 32
                    + 12), which chance alone reaches too seldom to rely on.
    out_of_range  trained_like with beta_scale = BETA_SCALE_EDGE, where ONE token id decides on which side of the fp16 planes' range
                  (scale 2^4, largest finite 65 504 / 16 = 4 094) a batch lies: channel 555 of the three embedding tables is
                  zero, but for word TRIGGER_ID (TRIGGER_VALUE), and the embedding LayerNorm has gamma EDGE_EMBED_GAMMA there.
                  inputs(case, kind="cold") -- the ladder batch without that id -- keeps the largest raw pre-LayerNorm value in
                  [2 048, 4 094), the upper half of the range; kind="hot" -- the same batch with the id planted at the first and
                  the last token of the first sequence and in the middle of the batch -- puts it, and the largest value a Linear
                  reads (the unfolded path keeps only normalised rows in planes), in [4 094, 8 188).  One encoder can so be
                  driven out of range and back.
"""
import copy
import functools

import numpy as np

from tests import encoder_ladder as el
from tests import test_gpu_encoder_shapes as shapes

VARIANTS = ("common_mode", "trained_like")
COMMON_OFFSET = 4.0
EMBED_OFFSET = 0.15                     # token_type_embeddings[0]: embedding rows have a standard deviation near 0.07
OUTLIER_CHANNELS = (101, 308, 555)
OUTLIER_GAMMA = (8.0, 6.0, 10.0)
OUTLIER_BETA = (12.0, -15.0, 20.0)
SINK_HEADS = (0, 1, 2, 3)
SINK_CHANNELS = (101, 101, 308, 308)
SINK_QUERY_BIAS = 8.0                   # x (2 + h); the logit divides by sqrt(64) = 8
SPIKE_POSITION = 299
SPIKE = 1.0                             # against embedding rows with a standard deviation near 0.07
BETA_SCALE_EDGE = 150.0
EDGE_CHANNEL = 555
EDGE_EMBED_GAMMA = 100.0
TRIGGER_ID = 321                        # 0-based
TRIGGER_VALUE = 3.0
PLANE_RANGE = 4094.0                    # 65 504 / 2^4
BETA_SCALE = {"common_mode": 1.0, "trained_like": 1.0, "out_of_range": BETA_SCALE_EDGE}
HEAD_DIM = el.HIDDEN // el.HEADS
KEY_TILE = 32
MIN_KEYS = 8                            # rows with fewer keys say nothing about saturation (one key: p = 1)


@functools.lru_cache(maxsize=None)
def model(variant, seed=0):
    """The model of test_gpu_encoder_shapes._model(2, seed) after the surgery of `variant`: the same dict (torch, bcfg, w, f32,
    f64).  The surgery is done on the fp32 parameters, so the packed blob, the fp32 and the float64 model hold the same numbers."""
    from colbert_jl_amd.encoder import pack_weights
    base = shapes._model(2, seed)
    torch = base["torch"]
    bert, linear = copy.deepcopy(base["f32"])
    beta_scale = BETA_SCALE[variant]
    outliers = variant != "common_mode"
    with torch.no_grad():
        bert.embeddings.token_type_embeddings.weight[0] += EMBED_OFFSET
        for layer in bert.encoder.layer:
            layer.attention.output.dense.bias += COMMON_OFFSET
            layer.output.dense.bias += COMMON_OFFSET
        if outliers:
            for name, p in bert.named_parameters():
                for ch, g, b in zip(OUTLIER_CHANNELS, OUTLIER_GAMMA, OUTLIER_BETA):
                    if "LayerNorm.weight" in name:
                        p[ch] = g
                    if "LayerNorm.bias" in name:
                        p[ch] = b * beta_scale
            for ch in set(SINK_CHANNELS):
                bert.embeddings.position_embeddings.weight[SPIKE_POSITION, ch] += SPIKE
            for layer in bert.encoder.layer:
                sa = layer.attention.self
                for h, ch in zip(SINK_HEADS, SINK_CHANNELS):
                    r = HEAD_DIM * h
                    sa.key.weight[r] = 0.0
                    sa.key.weight[r, ch] = 1.0
                    sa.query.weight[r] = 0.0
                    sa.query.bias[r] = SINK_QUERY_BIAS * (2 + h)
        if variant == "out_of_range":
            emb = bert.embeddings
            for table in (emb.word_embeddings, emb.position_embeddings, emb.token_type_embeddings):
                table.weight[:, EDGE_CHANNEL] = 0.0
            emb.word_embeddings.weight[TRIGGER_ID, EDGE_CHANNEL] = TRIGGER_VALUE
            emb.LayerNorm.weight[EDGE_CHANNEL] = EDGE_EMBED_GAMMA
    st = {k: v.detach().float().numpy() for k, v in bert.state_dict().items()}
    st["linear.weight"] = linear.weight.detach().numpy(); st["linear.bias"] = linear.bias.detach().numpy()
    w = pack_weights(st, base["bcfg"], el.DIM)
    return dict(torch=torch, bcfg=base["bcfg"], w=w, f32=(bert, linear), f64=(copy.deepcopy(bert).double(), copy.deepcopy(linear).double()))


def weights_narrowed(variant, dim):
    """The weight blob of model(variant) with the projection cut to its first `dim` outputs: the reference of such an encoder is
    the first `dim` columns of reference(variant, ...)."""
    from colbert_jl_amd.encoder import pack_weights
    m = model(variant)
    bert, linear = m["f32"]
    st = {k: v.detach().float().numpy() for k, v in bert.state_dict().items()}
    st["linear.weight"] = linear.weight.detach().numpy()[:dim]; st["linear.bias"] = linear.bias.detach().numpy()[:dim]
    return pack_weights(st, m["bcfg"], dim)


@functools.lru_cache(maxsize=None)
def inputs(case, seed=0, kind="base"):
    """(ids0, lens, mask) of test_gpu_encoder_shapes._inputs; kind "cold": TRIGGER_ID replaced by its neighbour; "hot": then
    planted at the first and the last token of the first (full-length) sequence and at the first token of the middle sequence."""
    ids0, lens, mask = shapes._inputs(case, seed)
    if kind == "base":
        return ids0, lens, mask
    ids0 = ids0.copy()
    ids0[ids0 == TRIGGER_ID] = TRIGGER_ID + 1
    if kind == "hot":
        ids0[0, 0] = ids0[0, lens[0] - 1] = ids0[lens.size // 2, 0] = TRIGGER_ID
    else:
        assert kind == "cold", kind
    return ids0, lens, mask


@functools.lru_cache(maxsize=None)
def reference(variant, case, seed=0, kind="base"):
    """(float64 rows, fp32 rows) of every attended token of the ladder batch `case`: test_gpu_encoder_shapes._reference on the
    model of `variant`."""
    m = model(variant, seed)
    ids0, lens, _ = inputs(case, seed, kind)
    return shapes._forward_rows(m, "f64", ids0, lens), shapes._forward_rows(m, "f32", ids0, lens)


@functools.lru_cache(maxsize=None)
def statistics(variant, case="32x32", seed=0, attention=True, kind="base"):
    """From the float64 model alone, over the attended rows of the batch (sequences grouped by length, as the reference runs them):
        biggest       the largest |activation| read by a Linear or a LayerNorm
        biggest_raw   the largest |value| a LayerNorm of the encoder layers reads (the raw rows the fold keeps in planes)
        mean_over_std |mean| / std of every row a LayerNorm reads
        gelu          the largest |GELU argument|
        logit         the largest |logit| over attended keys                       } attention=True only; rows of sequences
        pmax, tile    (layers, heads, rows): the largest attention probability of  } with at least MIN_KEYS keys
                      a row and the key tile (position // 32) that holds it        }
        last_in_tail  sequences in which, for some saturated (p > 0.999) row, the winning key is the last attended key of a tile
                      that is not full
        e32           max |fp32 forward - float64 forward| over the attended rows (attention=True only)"""
    m = model(variant, seed)
    torch = m["torch"]
    ids0, lens, mask = inputs(case, seed, kind)
    bert, linear = m["f64"]
    acc = dict(biggest=0.0, biggest_raw=0.0, gelu=0.0, logit=0.0)
    ratios, pmax, tile, last_in_tail = [], [], [], set()
    cur = {}

    def attended(t):        # (n, Lc, width) -> the attended rows
        return t[cur["am"]]

    def read_hook(mod, args):
        a = attended(args[0])
        acc["biggest"] = max(acc["biggest"], float(a.abs().max()))
        if isinstance(mod, torch.nn.LayerNorm):
            ratios.append((a.mean(dim=-1).abs() / a.std(dim=-1, unbiased=False)).numpy())
            if mod is not bert.embeddings.LayerNorm:
                acc["biggest_raw"] = max(acc["biggest_raw"], float(a.abs().max()))

    def gelu_hook(_mod, _args, out):
        acc["gelu"] = max(acc["gelu"], float(attended(out).abs().max()))

    handles = [mod.register_forward_pre_hook(read_hook) for mod in list(bert.modules()) + [linear]
               if isinstance(mod, (torch.nn.Linear, torch.nn.LayerNorm))]
    handles += [layer.intermediate.dense.register_forward_hook(gelu_hook) for layer in bert.encoder.layer]
    order = np.argsort(-lens, kind="stable")
    try:
        with torch.no_grad():
            i = 0
            while i < lens.size:
                Lc = int(lens[order[i]])
                sel = order[i:i + max(1, shapes.ROW_CHUNK // Lc)]
                am = np.arange(Lc)[None, :] < lens[sel, None]
                cur["am"] = torch.from_numpy(am)
                out = bert(input_ids=torch.from_numpy(ids0[sel, :Lc]), attention_mask=torch.from_numpy(am.astype(np.int64)),
                           output_hidden_states=attention)
                linear(out.last_hidden_state)
                i += len(sel)
                if not attention:
                    continue
                # probabilities recomputed from the hidden states that enter each layer (the model does not return them)
                pm_l, tl_l = [], []
                long_enough = torch.from_numpy(am & (lens[sel, None] >= MIN_KEYS))
                for l, layer in enumerate(bert.encoder.layer):
                    x = out.hidden_states[l]
                    sa = layer.attention.self
                    n = x.shape[0]
                    qh = sa.query(x).view(n, Lc, el.HEADS, HEAD_DIM).transpose(1, 2)
                    kh = sa.key(x).view(n, Lc, el.HEADS, HEAD_DIM).transpose(1, 2)
                    s = qh @ kh.transpose(-1, -2) / np.sqrt(HEAD_DIM)              # (n, heads, query, key)
                    both = cur["am"][:, None, :, None] & cur["am"][:, None, None, :]
                    acc["logit"] = max(acc["logit"], float(s.abs().masked_fill(~both, 0.0).max()))
                    s = s.masked_fill(~cur["am"][:, None, None, :], float("-inf"))
                    p, arg = torch.softmax(s, dim=-1).max(dim=-1)                  # (n, heads, query)
                    keep = long_enough[:, None, :].expand(-1, el.HEADS, -1)
                    pm_l.append(p.transpose(0, 1)[keep.transpose(0, 1)].view(el.HEADS, -1).numpy())
                    tl_l.append((arg // KEY_TILE).transpose(0, 1)[keep.transpose(0, 1)].view(el.HEADS, -1).numpy())
                    last = torch.from_numpy(lens[sel] - 1)[:, None, None]
                    hit = (p > 0.999) & (arg == last) & (last % KEY_TILE != KEY_TILE - 1) & keep
                    last_in_tail.update(int(sel[j]) for j in torch.nonzero(hit.any(dim=2).any(dim=1)).flatten())
                pmax.append(np.stack(pm_l)); tile.append(np.stack(tl_l))
    finally:
        for h in handles:
            h.remove()
    out = dict(acc, mean_over_std=np.concatenate(ratios))
    if attention:
        r64, r32 = reference(variant, case, seed, kind)
        out.update(pmax=np.concatenate(pmax, axis=2), tile=np.concatenate(tile, axis=2), last_in_tail=sorted(last_in_tail),
                   e32=float(np.abs(r32 - r64).max()), out_max=float(np.abs(r64).max()))
    return out


def summary(s):
    """One line of the statistics of `statistics()`."""
    q = np.quantile(s["mean_over_std"], [0.5, 1.0])
    line = (f"largest |x| {s['biggest']:.1f} (raw rows {s['biggest_raw']:.1f}), |mean|/std median {q[0]:.2f} max {q[1]:.2f}, "
            f"|GELU argument| {s['gelu']:.1f}")
    if "pmax" in s:
        sink = s["pmax"][:, list(SINK_HEADS)]
        other = np.delete(s["pmax"], list(SINK_HEADS), axis=1)
        line += (f", |logit| {s['logit']:.0f}, sink heads p > 0.999: {(sink > 0.999).mean():.1%}, other heads median p_max "
                 f"{np.median(other):.2f} (p > 0.999: {(other > 0.999).mean():.2%}), e32 {s['e32']:.3g}, largest |output| {s['out_max']:.1f}")
    return line
