"""Trainer(accumulate=True), the parts that need no GPU: the keyword, and the C entry in the header, the ctypes table and the library."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_trainer_has_the_keyword_with_default_false():
    from bist_amd.train import Trainer
    p = inspect.signature(Trainer.__init__).parameters["accumulate"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert callable(getattr(Trainer, "step_group"))


def test_the_entry_is_declared_bound_and_exported():
    from bist_amd import _lib
    name = "bist_adam_accum_dev"
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bist_hip.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
    assert decl, name
    assert len(decl.group(1).split(",")) == 16
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert name in _lib.SIGNATURES and hasattr(raw, name)
    res, args = _lib.SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == 16
    # p, g, acc, m, v, work | n | hyper, phase | beta1, beta2, eps | grad_dtype, work_dtype, max_blocks | stream
    P, I32, I64, F = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    assert args == [P] * 6 + [I64] + [P] * 2 + [F] * 3 + [I32] * 3 + [P]
