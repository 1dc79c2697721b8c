"""Trainer checkpoints, the parts that need no GPU: the methods and their signatures, the C entry in the header, the
ctypes table and the library, the refusal on a trainer that is not on the device, the lossless weight export, and every host-side
validation error of load_state_dict on a hand-built dictionary."""
import argparse
import copy
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _trainer(dtype=torch.float32, **kw):
    from oracle import bist_oracle as O
    import bist_amd.model as M
    from bist_amd.train import Trainer
    cfg = O.Cfg(d_model=64, att_h=4, nb_blocks=1, nb_venc_blocks=1, nb_cenc_blocks=1)
    args = argparse.Namespace(**{**cfg.__dict__, "d_ff": 4 * cfg.d_model})
    torch.manual_seed(0)
    return Trainer(M.make_model(40, 40, args, ft_sizes=[32]), args, 40, compute_dtype=dtype, **kw)


def _hand_built(tr):
    """A version-1 checkpoint dictionary of `tr` as TrainerSnapshot.state_dict() lays it out, from host data alone."""
    from bist_amd import checkpoint as CK
    layout, config = CK.describe(tr)
    return {"format": "bist_amd.trainer", "version": 1, "layout": layout, "config": config,
            "counters": {"step": 3, "passes": 3, "skipped": 0}, "dropout": {"seed": 0x5EED, "draws": 17},
            "hyper": torch.zeros(8), "master": tr.master.detach().float().cpu().clone(), "m": torch.zeros(tr.numel),
            "v": torch.zeros(tr.numel), "digest": {"master": 2 ** 64 - 1, "m": 0, "v": 12345678901234567890}}


def test_the_methods_exist_with_their_signatures():
    from bist_amd.checkpoint import TrainerSnapshot
    from bist_amd.train import Trainer

    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()][1:]
    assert params(Trainer.snapshot) == [("into", None)]
    assert params(Trainer.restore) == [("snap", inspect.Parameter.empty)]
    assert params(Trainer.state_dict) == []
    assert params(Trainer.load_state_dict) == [("sd", inspect.Parameter.empty), ("strict", True)]
    assert params(Trainer.save) == [("path", inspect.Parameter.empty)]
    assert params(Trainer.load) == [("path", inspect.Parameter.empty)]
    assert params(Trainer.state_digest) == [] and params(Trainer.master_state_dict) == []
    assert params(TrainerSnapshot.state_dict) == []


def test_the_entry_is_declared_bound_and_exported():
    from bist_amd import _lib
    P, I32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bist_hip.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+bist_state_copy\s*\(([^)]*)\)", src)
    assert decl
    # src_p, src_m, src_v, dst_p, dst_m, dst_v, work | work_dtype | n | digests | nslots, max_blocks | stream
    want = [P] * 7 + [I32, I64, P, I32, I32, P]
    assert _lib.SIGNATURES["bist_state_copy"] == (ctypes.c_int, want)
    assert len(decl.group(1).split(",")) == len(want)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "bist_state_copy")
    assert _lib.STATE_MAX_SLOTS == 4096
    assert re.search(r"#define\s+BIST_STATE_MAX_SLOTS\s+%d\b" % _lib.STATE_MAX_SLOTS, src)
    assert "checkpoint.hip" in open(os.path.join(ROOT, "bist_amd", "csrc", "Makefile")).read()


def test_a_trainer_that_is_not_on_the_device_cannot_take_a_snapshot():
    tr = _trainer()
    for call in (tr.snapshot, tr.state_dict, tr.state_digest):
        with pytest.raises(RuntimeError, match="device launch"):
            call()


def test_the_layout_is_kept_in_flat_order():
    tr = _trainer()
    names = dict((id(p), n) for n, p in reversed(list(tr.model.named_parameters())))
    assert len(tr._layout) == len(tr.params)
    end = 0
    for p, (name, off, numel, shape) in zip(tr.params, tr._layout):
        assert name == names[id(p)] and numel == p.numel() and shape == tuple(p.shape)
        assert off >= end and p.data_ptr() == tr.flat_param.data_ptr() + 4 * off
        end = off + numel
    assert end <= tr.numel


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_master_state_dict_has_the_models_keys_as_views_of_master(dtype):
    tr = _trainer(dtype)
    model_sd = tr.model.state_dict()
    msd = tr.master_state_dict()
    assert list(msd) == list(model_sd)
    params = {n for n, _ in tr.model.named_parameters(remove_duplicate=False)}
    lo, hi = tr.master.data_ptr(), tr.master.data_ptr() + 4 * tr.numel
    for k, t in msd.items():
        assert t.shape == model_sd[k].shape, k
        if k in params:
            assert t.dtype == torch.float32 and lo <= t.data_ptr() and t.data_ptr() + 4 * t.numel() <= hi, k
            assert torch.equal(t.to(dtype), model_sd[k]), k          # the model holds the rounded copy of what master holds
        else:
            assert t.data_ptr() == model_sd[k].data_ptr(), k        # a buffer (the positional table): the model's own tensor
    assert params and any(k not in params for k in msd)
    k = next(iter(params))
    msd[k].add_(1.0)                                               # a view: writes reach master
    assert torch.equal(tr.master_state_dict()[k], msd[k])


def _refused(tr, sd, word, **kw):
    with pytest.raises(ValueError, match=word):
        tr.load_state_dict(sd, **kw)


def test_every_validation_error_fires_before_any_launch():
    """On a CPU trainer a dictionary that passes validation reaches the device check (RuntimeError); one that does not never gets there."""
    tr = _trainer()
    good = _hand_built(tr)
    with pytest.raises(RuntimeError, match="device launch"):
        tr.load_state_dict(good)

    def broken(**edits):
        sd = copy.deepcopy(good)
        for path, value in edits.items():
            part, keys = sd, path.split("__")
            for k in keys[:-1]:
                part = part[k]
            if value is KeyError:
                del part[keys[-1]]
            else:
                part[keys[-1]] = value
        return sd
    _refused(tr, broken(format="bist_amd.model"), "format")
    _refused(tr, broken(version=2), "version")
    for path in ("master", "hyper", "digest", "layout__offsets", "config__eps", "counters__passes", "dropout__draws", "digest__v"):
        _refused(tr, broken(**{path: KeyError}), "missing key " + path.replace("__", "."))
    _refused(tr, broken(m=good["m"][:-1].clone()), r"\bm must be a float32 tensor of %d" % tr.numel)
    _refused(tr, broken(v=good["v"].double()), r"\bv must be a float32")
    _refused(tr, broken(master=good["master"].view(-1, 64)), "master must be")
    _refused(tr, broken(hyper=torch.zeros(4)), "hyper")
    names = list(good["layout"]["names"]); names[3] = names[3] + "_renamed"
    _refused(tr, broken(layout__names=names), r"layout\.names\[3\]")
    offsets = list(good["layout"]["offsets"]); offsets[5] += 64
    _refused(tr, broken(layout__offsets=offsets), r"layout\.offsets\[5\]")
    shapes = copy.deepcopy(good["layout"]["shapes"]); shapes[-1] = shapes[-1][::-1] + [1]
    _refused(tr, broken(layout__shapes=shapes), r"layout\.shapes\[%d\]" % (len(shapes) - 1))
    _refused(tr, broken(layout__numel=tr.numel + 64), r"layout\.numel")
    _refused(tr, broken(layout__n32=tr.n32 - 64), r"layout\.n32")
    _refused(tr, broken(counters__step=-1), r"counters\.step")
    _refused(tr, broken(digest__m="0"), r"digest\.m")
    _refused(tr, broken(config__compute_dtype="float16"), r"config\.compute_dtype")
    for key, value in (("d_model", 128), ("warmup", 8000.0), ("factor", 2.0), ("betas", [0.9, 0.999]), ("eps", 1e-8)):
        sd = broken(**{"config__" + key: value})
        _refused(tr, sd, r"config\.%s" % key)
        _refused(tr, sd, r"config\.%s" % key, strict=True)
        with pytest.raises(RuntimeError, match="device launch"):    # accepted: the loading trainer keeps its own value
            tr.load_state_dict(sd, strict=False)
    assert tr.warmup == 4000 and tr._step == 0
    # options that may differ between the saving and the loading trainer
    with pytest.raises(RuntimeError, match="device launch"):
        tr.load_state_dict(broken(config__compute_dtype="bfloat16", config__accumulate=True, config__max_grad_norm=1.0, config__world=8))


def test_the_dictionary_round_trips_through_a_weights_only_load(tmp_path):
    tr = _trainer()
    sd = _hand_built(tr)
    path = str(tmp_path / "hand_built.pt")
    torch.save(sd, path)
    back = torch.load(path, map_location="cpu", weights_only=True)
    assert back.keys() == sd.keys()
    for k in sd:
        if isinstance(sd[k], torch.Tensor):
            assert back[k].dtype == sd[k].dtype and torch.equal(back[k], sd[k]), k
        else:
            assert back[k] == sd[k], k
    from bist_amd import checkpoint as CK
    CK.validate(back, tr)
