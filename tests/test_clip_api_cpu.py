"""Trainer(max_grad_norm=...), the parts that need no GPU: the keyword and its refusals, the accessors on a trainer without the option,
and the four C entries in the header, the ctypes table and the library."""
import argparse
import ctypes
import inspect
import math
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _trainer(**kw):
    from oracle import bist_oracle as O
    import bist_amd.model as M
    from bist_amd.train import Trainer
    cfg = O.Cfg(d_model=64, att_h=4, nb_blocks=1, nb_venc_blocks=1, nb_cenc_blocks=1)
    args = argparse.Namespace(**{**cfg.__dict__, "d_ff": 4 * cfg.d_model})
    torch.manual_seed(0)
    return Trainer(M.make_model(40, 40, args, ft_sizes=[32]), args, 40, compute_dtype=torch.float32, **kw)


def test_trainer_has_the_keyword_with_default_none():
    from bist_amd.train import Trainer
    p = inspect.signature(Trainer.__init__).parameters["max_grad_norm"]
    assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert callable(getattr(Trainer, "grad_norm")) and callable(getattr(Trainer, "clip_stats"))


def test_a_trainer_without_the_option_has_no_buffers_and_refuses_the_accessors():
    tr = _trainer()
    assert tr.max_grad_norm is None and tr.clip is False
    assert not hasattr(tr, "clip_partials") and not hasattr(tr, "skipped")
    with pytest.raises(RuntimeError, match="max_grad_norm"):
        tr.grad_norm()
    with pytest.raises(RuntimeError, match="max_grad_norm"):
        tr.clip_stats()


def test_the_option_allocates_its_buffers_at_construction():
    from bist_amd import _lib, train
    for bound in (1.0, math.inf):
        tr = _trainer(max_grad_norm=bound)
        assert tr.max_grad_norm == bound and tr.clip is True and tr.early_adam is False
        assert tr.clip_partials.dtype == torch.float64 and tr.clip_partials.numel() == train.CLIP_SLOTS_BIG + train.CLIP_SLOTS_PREFIX
        assert tr.clip_partials.numel() <= _lib.GRAD_SUMSQ_MAX_SLOTS
        assert tr.skipped.dtype == torch.int64 and tr.skipped.tolist() == [0]
        assert tr.grad_norm().data_ptr() == tr.hyper.data_ptr() + 6 * 4


@pytest.mark.parametrize("bound", [0, 0.0, -1.0, float("nan"), 1e-46, 1e39],
                         ids=["int0", "zero", "negative", "nan", "zero-as-float32", "inf-as-float32"])
def test_a_bound_that_is_not_positive_is_refused(bound):
    with pytest.raises(ValueError, match="positive"):
        _trainer(max_grad_norm=bound)


def test_the_tail_on_a_trainer_that_is_not_on_the_device_says_why():
    tr = _trainer(max_grad_norm=1.0)
    with pytest.raises(RuntimeError, match="device launches"):
        tr._clipped_tail({})


def test_refusals_in_process(monkeypatch):
    import torch.distributed as dist
    with pytest.raises(ValueError, match="deferred_adam"):
        _trainer(max_grad_norm=1.0, use_graph=True, deferred_adam=True)
    # several ranks, as Trainer.__init__ sees them (two processes and a collective backend are not needed to be refused)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(ValueError, match="several ranks"):
        _trainer(max_grad_norm=1.0)


@pytest.mark.parametrize("var,value,word", [("BIST_FORCE_EXCHANGE", "1", "BIST_FORCE_EXCHANGE"), ("BIST_ADAM_IN_STEP", "0", "BIST_ADAM_IN_STEP"),
                                            ("BIST_ADAM_CLEARS", "1", "BIST_ADAM_CLEARS")])
def test_refusals_of_environment_switches(var, value, word):
    """Each switch in a child process of its own (BIST_ADAM_CLEARS is read at import)."""
    env = dict(os.environ, **{var: value})
    r = subprocess.run([sys.executable, "-s", os.path.abspath(__file__), "--refused", word], env=env, capture_output=True, text=True,
                       cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "refused: " + word in r.stdout


P, I32, I64, F = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
ENTRIES = {
    # g, acc, phase | n | grad_dtype | partials | slot_lo, nslots, max_blocks | stream
    "bist_grad_sumsq": [P] * 3 + [I64, I32, P] + [I32] * 3 + [P],
    # partials | nslots_total | max_norm | hyper, skipped_ctr, phase | stream
    "bist_clip_hyper": [P, I32, F] + [P] * 4,
    # the arguments of bist_adam_step_dev_bg and of bist_adam_accum_dev
    "bist_adam_step_dev_guard": None,
    "bist_adam_accum_dev_guard": None,
}


@pytest.mark.parametrize("name", list(ENTRIES))
def test_the_entries_are_declared_bound_and_exported(name):
    from bist_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bist_hip.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
    assert decl, name
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert name in _lib.SIGNATURES and hasattr(raw, name)
    res, args = _lib.SIGNATURES[name]
    want = ENTRIES[name]
    if want is None:
        want = _lib.SIGNATURES[{"bist_adam_step_dev_guard": "bist_adam_step_dev_bg", "bist_adam_accum_dev_guard": "bist_adam_accum_dev"}[name]][1]
    assert res is ctypes.c_int and args == want
    assert len(decl.group(1).split(",")) == len(want)
    assert re.search(r"#define\s+BIST_GRAD_SUMSQ_MAX_SLOTS\s+%d\b" % _lib.GRAD_SUMSQ_MAX_SLOTS, src)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    assert len(sys.argv) == 3 and sys.argv[1] == "--refused"
    try:
        _trainer(max_grad_norm=1.0)
    except ValueError as e:
        assert sys.argv[2] in str(e), str(e)
        print("refused: " + sys.argv[2])
    else:
        raise SystemExit("Trainer(max_grad_norm=1.0) accepted %s" % sys.argv[2])
    _trainer()                 # the default trainer takes the switch as before
