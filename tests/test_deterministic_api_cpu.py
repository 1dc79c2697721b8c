"""Deterministic mode, the parts that need no GPU: the Trainer keyword, the four C entries in the header and the ctypes table, the flag's
default."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("bist_col_sum_multi_det", "bist_layernorm_param_grad_multi_det", "bist_scaled_bias_bwd_det", "bist_embed_bwd_multi_det")


def test_trainer_has_the_keyword_with_default_false():
    from bist_amd.train import Trainer
    p = inspect.signature(Trainer.__init__).parameters["deterministic"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY


def test_the_four_entries_are_declared_bound_and_exported():
    import ctypes
    from bist_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bist_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
        assert _lib.SIGNATURES[name][0] is ctypes.c_int
    assert ctypes.sizeof(_lib.BistEmbedBwd) == 48 and _lib.BistEmbedBwd.drop.offset == 24


def test_the_flag_is_off_after_import_and_the_sizing_helpers_answer_without_a_gpu():
    from bist_amd import _lib, ops
    assert ops.DETERMINISTIC is False and ops.EMBED_QUEUE is None
    arr = (_lib.BistColSum * 2)()
    arr[0].M, arr[0].N, arr[1].M, arr[1].N = 200, 96, 25088, 512          # 13 chunks of 16 rows; 128 chunks of 196
    assert _lib.lib.bist_col_sum_multi_det_workspace(arr, 2) == 4 * (13 * 96 + 128 * 512)
    ln = (_lib.BistLnGrad * 1)()
    ln[0].rows = 37                                                       # 10 waves of 4 rows
    assert _lib.lib.bist_layernorm_param_grad_multi_det_workspace(ln, 1, 512) == 4 * 10 * 2 * 512
    assert _lib.lib.bist_scaled_bias_bwd_det_workspace(32, 4, 16, 2) == 4 * 8 * 64
    assert _lib.lib.bist_scaled_bias_bwd_det_workspace(32, 4, 16, 3) == -1
