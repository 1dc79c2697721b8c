"""DeviceFeeder(length_classes=...): slots that grow and never shrink, exact-shape views, features in their source dtype -- and a
class-mode Trainer fed by it computes what it computes from the same batches resident on the device."""
import argparse
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


def _host(seed, Lq, T):
    from bist_amd.data.feeder import HostBatch
    from bist_amd.data.synthetic import synthetic_batch
    b = synthetic_batch(4, T=T, S=9, C=64, Lq=Lq, Lh=9, Lc=6, Lt=6, vocab=80, seed=seed, dtype=torch.float32, device="cpu")
    return HostBatch(b.query, b.his, b.fts, b.cap, b.trg, b.trg_y)


def test_feeder_reuses_grown_slots_and_yields_exact_views():
    from bist_amd.data.classes import LengthClasses
    from bist_amd.data.feeder import DeviceFeeder
    shapes = [(12, 9), (12, 9), (11, 9), (7, 6), (5, 4), (3, 2), (12, 9)]     # the largest first through each of the three slots
    hosts = [_host(40 + i, q, T) for i, (q, T) in enumerate(shapes)]
    fd = DeviceFeeder(hosts, length_classes=LengthClasses())
    seen, caps = [], []
    for hb, b in zip(hosts, fd):
        assert tuple(b.query.shape) == tuple(hb.query.shape) and tuple(b.fts.shape) == tuple(hb.fts.shape)
        assert b.fts.dtype == torch.float32                      # handed over in the source dtype: the trainer's staging launch casts
        assert torch.equal(b.query.cpu(), hb.query) and torch.equal(b.fts.cpu(), hb.fts)
        assert "temporal_mask" not in b.__dict__ and "trg_mask" not in b.__dict__   # nothing derived unless read (SourceBatch) ...
        seen.append(b.query.untyped_storage().data_ptr())
        caps.append(fd.capacity_bytes())
    from bist_amd.data.batch import Batch
    ref = Batch(*(t.cuda() for t in (hb.query, hb.his, hb.fts, hb.cap, hb.trg, hb.trg_y)))
    for f in ("query_mask", "query_mask2", "his_mask", "cap_mask", "trg_mask", "trg_mean_mask", "temporal_mask", "ntokens", "qntokens"):
        assert torch.equal(getattr(b, f), getattr(ref, f)), f                 # ... and then what Batch builds
    assert caps[-1] == caps[2], caps              # smaller batches after the largest: nothing allocated, nothing given back
    assert all(seen[i] == seen[i + 3] for i in range(len(seen) - 3)), seen       # the same slot storage, every third batch


def test_class_trainer_fed_equals_resident():
    import bist_amd.model as M
    from bist_amd.data.batch import Batch
    from bist_amd.data.classes import LengthClasses
    from bist_amd.data.feeder import DeviceFeeder
    from bist_amd.train import Trainer
    from oracle import bist_oracle as O
    cfg = O.Cfg(d_model=64, att_h=4, nb_blocks=2, nb_venc_blocks=2, nb_cenc_blocks=2)
    args = argparse.Namespace(**{**cfg.__dict__, "d_ff": 4 * cfg.d_model})
    torch.manual_seed(0)
    m1 = M.make_model(80, 80, args, ft_sizes=[64]).cuda().eval()
    m2 = copy.deepcopy(m1)
    lc = LengthClasses({"query": (8, 16), "his": (16,), "cap": (8,), "trg": (8,), "frames": (8, 16)}, {f: 8 for f in ("query", "his", "cap", "trg", "frames")})
    t1 = Trainer(m1, args, 80, compute_dtype=torch.bfloat16, warmup=20, factor=0.0, use_graph=True, length_classes=lc)
    t2 = Trainer(m2, args, 80, compute_dtype=torch.bfloat16, warmup=20, factor=0.0, use_graph=True, length_classes=lc)
    hosts = [_host(60 + i, q, T) for i, (q, T) in enumerate([(7, 6), (12, 9), (5, 4), (12, 9)])]
    for hb, fb in zip(hosts, DeviceFeeder(hosts, length_classes=lc)):
        a = t1.step(fb)
        rb = Batch(hb.query.cuda(), hb.his.cuda(), hb.fts.cuda(), hb.cap.cuda(), hb.trg.cuda(), hb.trg_y.cuda())
        b = t2.step(rb)
        torch.cuda.synchronize()
        for k in a:
            assert abs(a[k].item() - b[k].item()) <= 1e-3 * abs(b[k].item()), (k, a[k].item(), b[k].item())
        g1, g2 = t1.flat_grad.double(), t2.flat_grad.double()
        assert (g1 @ g2 / (g1.norm() * g2.norm())).item() >= 0.9999
    assert t1.graph_stats()["captures"] == 2
