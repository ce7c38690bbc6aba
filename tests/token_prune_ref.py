"""What the token-pruning tests share: the oracle model run with token elimination between its layers (fp64, CPU), the cases and
schedules the end-to-end GPU test runs, and a second, plain-Python statement of the selection order.

The CPU test (test_token_prune_cpu.py) asserts on these cases and schedules what makes the GPU comparison mean something: clear
score gaps at every cut and kept sets that are not "the first k positions"."""
import numpy as np
import torch

from conftest import case_inputs, load_case

TOL = 1e-4      # the score bound of tests/test_rollout_gpu.py: 1e-4 of the utterance's largest score

# (golden case, schedule): at least three eliminating layers each; chosen so that test_token_prune_cpu.py's input checks hold
# (the golden models carry random weights: their attention is close to uniform, and few cuts separate the scores by a hundred
# tolerances in every utterance - hence the uneven schedules)
E2E = {
    "bert_L4_outliers": [47, 10, 6],                                  # eliminates after layers 0, 1, 2
    "bert_L12": [64, 64, 64, 60, 60, 60, 60, 60, 59, 2, 2],           # eliminates after layers 3, 8, 9
}


def select_by_sorting(score, mask, k):
    """the selection order, a second time and in plain Python: position 0, then the k - 1 first of positions 1 .. S-1 sorted by
    (masked, NaN, -score, index) -> ascending list"""
    S = len(score)

    def key(j):
        s = float(score[j])
        nan = s != s
        return (0 if mask[j] else 1, 1 if nan else 0, 0.0 if nan else -s, j)

    rest = sorted(range(1, S), key=key)
    return sorted([0] + rest[:k - 1])


def counts(S, keep):
    out = [S]
    for k in keep:
        out.append(min(k, out[-1]))
    return out


_ORACLES = {}


def oracle_model(name, labels):
    """the oracle of a golden case in fp64, its metadata and its batch (CPU tensors); built once per case"""
    if name in _ORACLES:
        return _ORACLES[name]
    from oracle.encoder import EncoderConfig
    from oracle.model import OracleModel
    meta, _ = load_case(name)
    cfg, sd, batch = case_inputs(meta, labels)
    ocfg = EncoderConfig(**{k: v for k, v in cfg.to_dict().items() if k in EncoderConfig.__dataclass_fields__})
    om = OracleModel(ocfg, labels.top2bottom, labels.n_bottom, 0.0)
    om.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    om.double().eval()
    _ORACLES[name] = om, meta, {k: torch.from_numpy(v) for k, v in batch.items()}
    return _ORACLES[name]


@torch.no_grad()
def oracle_pruned(om, ids, seg, keep, kept=None):
    """The oracle's forward with tokens dropped between layers.  ``keep``: the schedule; ``kept`` None: the oracle selects
    (trainer.token_prune_reference on its own fp64 maps); else int [L-1, B, S] original positions (-1 past the count) - the
    selection of another run, followed instead.  Returns dict(top, bottoms, final, cls, kept [L-1][B][S_{l+1}] original positions,
    scores {l: (fp64 [B, S_l], origins int64 [B, S_l], mask bool [B, S_l])} for the eliminating layers l)."""
    from nbest_amd import trainer
    from oracle.encoder import position_ids_for
    import math
    enc = om.bert_encoder
    cfg = enc.cfg
    mask = ids > 0                                                            # quirk Q1: every family
    tt = torch.zeros_like(ids) if (seg is None or om.family == "xlm-roberta") else seg
    x = enc.embeddings(ids, tt, position_ids_for(cfg, ids))
    B, S = ids.shape
    org = torch.arange(S).expand(B, S).clone()
    L = len(enc.encoder.layer)
    kept_out, scores = [], {}
    for l, lyr in enumerate(enc.encoder.layer):
        sa = lyr.attention.self
        Sl, H = x.shape[1], x.shape[2]
        d = H // sa.nh
        split = lambda t: t.view(B, Sl, sa.nh, d).transpose(1, 2)
        q, k, v = split(sa.query(x)), split(sa.key(x)), split(sa.value(x))
        sc = (q @ k.transpose(-1, -2) / math.sqrt(d)).masked_fill(~mask[:, None, None, :], float("-inf"))
        probs = torch.softmax(sc, dim=-1)
        x1 = lyr.attention.output((probs @ v).transpose(1, 2).reshape(B, Sl, H), x)
        x = lyr.output(lyr.intermediate(x1), x1)
        if l == L - 1:
            break
        kl = min(int(keep[l]), Sl)
        if kl < Sl:
            score, idx = trainer.token_prune_reference(probs, mask, kl)
            scores[l] = (torch.from_numpy(score), org.clone(), mask.clone())
            idx = torch.from_numpy(idx)
            if kept is not None:       # follow the other run: its original positions -> positions among the current tokens
                want = torch.as_tensor(kept[l]).long()[:, :kl]
                pos = torch.full((B, S), -1, dtype=torch.long)
                pos.scatter_(1, org, torch.arange(Sl).expand(B, Sl))
                idx = pos.gather(1, want)
                assert (idx >= 0).all(), "layer %d: a kept position is not among the tokens that entered the layer" % l
            x = x.gather(1, idx[:, :, None].expand(B, kl, H))
            mask, org = mask.gather(1, idx), org.gather(1, idx)
        kept_out.append(org.clone())
    cls = x[:, 0, :]
    top, bottoms, final = om.clf(cls)
    return dict(top=top, bottoms=bottoms, final=final, cls=cls, kept=kept_out, scores=scores)
