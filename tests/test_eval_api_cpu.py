"""Host-side checks of the validation entry points of bist_amd.train.Trainer (no device): the bound of the evaluation store, the
statistics' keys, the loss-term order the device totals are indexed by, and that the accumulation launch refuses host tensors."""
import argparse

import pytest
import torch


def _trainer(**kw):
    from oracle import bist_oracle as O
    import bist_amd.model as M
    from bist_amd.train import Trainer
    cfg = O.Cfg(d_model=64, att_h=4, nb_blocks=1, nb_venc_blocks=1, nb_cenc_blocks=1, **kw.pop("cfg", {}))
    args = argparse.Namespace(**{**cfg.__dict__, "d_ff": 4 * cfg.d_model})
    torch.manual_seed(0)
    return Trainer(M.make_model(40, 40, args, ft_sizes=[32]), args, 40, compute_dtype=torch.float32, **kw)


def test_eval_store_bound_and_statistics():
    from bist_amd.train import MAX_EVAL_GRAPHS
    with pytest.raises(ValueError):
        _trainer(max_eval_graphs=0)
    t = _trainer(max_eval_graphs=5)
    assert t.eval_graph_stats() == {"captures": 0, "hits": 0, "evictions": 0, "entries": 0, "bytes": 0, "max_eval_graphs": 5}
    assert _trainer().max_eval_graphs == MAX_EVAL_GRAPHS >= 11          # the 11 classes of DESIGN.md section 11 fit without eviction
    assert set(t.graph_stats()) == {"captures", "hits", "evictions", "entries", "bytes", "max_graphs"}


def test_term_order_follows_the_loss_heads():
    assert _trainer()._term_names() == ["out", "cap_ae", "temporal_ae", "spatial_ae"]
    assert _trainer(cfg={"auto_encoder": 0})._term_names() == ["out"]
    assert _trainer(cfg={"t2s": 0})._term_names() == ["out", "cap_ae", "temporal_ae"]


def test_eval_accumulate_refuses_host_tensors():
    from bist_amd import ops
    z = torch.zeros(1)
    n = torch.zeros((), dtype=torch.int64)
    with pytest.raises(RuntimeError):
        ops.eval_accumulate([z], [n], [n, n], torch.zeros(8, dtype=torch.float64), torch.zeros(3, dtype=torch.int64))
