#!/usr/bin/env python3
"""Generate tests/golden/alpha/G10_attend_alphas.npz: the attention maps the REFERENCE's own `attention_layer` (model2.py:73-78)
returns inside the loops of model2.py:54-62 (training) and model2.py:100-109 (greedy `sample`), on G6's exact configuration and
seeds (make_goldens_attend.py), and the doubly stochastic penalty mean_{b,p} (1 - sum_t alpha[b,t,p])^2 of the training maps.

    python tests/golden/make_goldens_alpha.py [out_dir]

The reference gathers these maps (`alpha_list`, model2.py:50,60) and drops them.  Here the instance's `attention_layer` is
wrapped by a recorder and `make_goldens_attend.py`'s own recipes (`reference_forward`, `reference_sample`) are run unchanged, so
every map is the class's own arithmetic.  The fixture lives in a directory of its own: the fixtures next to this script are the
set `make_goldens.py` + `make_goldens_attend.py` regenerate, checked file by file (tests/test_oracle_golden.py); this one is
regenerated and compared by tests/test_alpha_host.py."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_goldens_attend import build, import_model2, reference_forward, reference_sample  # noqa: E402

NAME = "G10_attend_alphas.npz"
G6 = dict(hidden=96, context=64, vocab=300, embed=32, B=4, T=12, P=16, lengths=[12, 12, 9, 5], seed=223, feat=64)


def record_alphas(m):
    """wrap the instance's attention_layer: every alpha it returns is appended to the returned list"""
    seen = []
    inner = m.attention_layer

    def attention_layer(features, context_encode, hidden):
        context, alpha = inner(features, context_encode, hidden)
        seen.append(alpha.detach().clone())
        return context, alpha
    m.attention_layer = attention_layer
    return seen


def g6_inputs(cfg):
    """features and captions exactly as make_goldens_attend.make draws them"""
    g = torch.Generator().manual_seed(cfg["seed"] + 1)
    features = torch.randn(cfg["B"], cfg["P"], cfg["feat"], generator=g).clamp(min=0)
    caps = torch.zeros(cfg["B"], cfg["T"], dtype=torch.long)
    for b, l in enumerate(cfg["lengths"]):
        caps[b, 0] = 1
        caps[b, 1:l - 1] = torch.randint(4, cfg["vocab"], (l - 2,), generator=g)
        caps[b, l - 1] = 2
    return features, caps


def main(out_dir=os.path.join(HERE, "alpha")):
    import warnings
    warnings.simplefilter("ignore")
    os.makedirs(out_dir, exist_ok=True)
    torch.set_num_threads(4)
    cfg = G6
    model2 = import_model2()
    m, _ = build(model2, cfg["hidden"], cfg["context"], cfg["vocab"], cfg["embed"], cfg["seed"], cfg["feat"])
    features, caps = g6_inputs(cfg)
    B, P, H = cfg["B"], cfg["P"], cfg["hidden"]
    l1 = [l - 1 for l in cfg["lengths"]]                                   # train.py:134
    seen = record_alphas(m)
    with torch.no_grad():
        reference_forward(m, features, caps[:, :-1], l1)
    train = list(seen)
    del seen[:]
    reference_sample(m, features, (torch.zeros(B, H), torch.zeros(B, H)))   # eval.py:82-83
    zero = torch.stack(seen, 1)
    del seen[:]
    h0, c0 = m.init_lstm(features)
    reference_sample(m, features, (h0.detach(), c0.detach()))
    init = torch.stack(seen, 1)
    cov = torch.zeros(B, P, dtype=torch.float64)
    for a in train:                                                        # packed step t holds images 0 .. batch_sizes[t]-1
        cov[:a.shape[0]] += a.double()
    out = dict(seed=cfg["seed"], dims=np.array([cfg[k] for k in ("hidden", "context", "vocab", "embed", "B", "T", "P", "feat")]),
               lengths=np.array(cfg["lengths"]), alphas_train=torch.cat(train, 0).numpy(), alphas_greedy_zero_state=zero.numpy(),
               alphas_greedy_init_state=init.numpy(), penalty_alpha_c_1=np.float64(((1.0 - cov) ** 2).mean().item()))
    path = os.path.join(out_dir, NAME)
    np.savez_compressed(path, **out)
    print(NAME, os.path.getsize(path), "penalty", float(out["penalty_alpha_c_1"]))


if __name__ == "__main__":
    main(*sys.argv[1:2])
