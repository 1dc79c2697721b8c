"""The slab reductions (reduce_slab.hip), the parts that need no GPU: the two workspace-size functions against their formula for
hand-computed job lists, the four symbols in the header and the ctypes table, the switch's default."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = 256          # counter words at the head of a workspace
SIGS = {
    "bist_col_sum_multi_ws_workspace": ("int64_t", r"const\s+BistColSum\s*\*\s*\w+\s*,\s*int32_t\s+\w+"),
    "bist_col_sum_multi_ws": ("int", r"const\s+BistColSum\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*,\s*void\s*\*\s*\w+\s*,\s*int64_t\s+\w+\s*,\s*void\s*\*\s*\w+"),
    "bist_layernorm_param_grad_multi_ws_workspace": ("int64_t", r"const\s+BistLnGrad\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+"),
    "bist_layernorm_param_grad_multi_ws": ("int", r"const\s+BistLnGrad\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*,\s*void\s*\*\s*\w+\s*,"
                                                  r"\s*int64_t\s+\w+\s*,\s*void\s*\*\s*\w+"),
}


def test_the_column_sum_workspace_follows_its_formula():
    """256 + 4 * sum ceil(M / max(16, ceil(M / 128))) * (N rounded up to 4)"""
    from bist_amd import _lib
    arr = (_lib.BistColSum * 3)()
    arr[0].M, arr[0].N = 200, 96              # chunks of 16 rows: 13 slabs of 96 floats
    arr[1].M, arr[1].N = 25088, 512           # chunks of 196 rows: 128 slabs of 512
    arr[2].M, arr[2].N = 2049, 7              # chunks of 17 rows: 121 slabs of 8 (7 rounded up to a 16-byte piece)
    assert _lib.lib.bist_col_sum_multi_ws_workspace(arr, 3) == HEADER + 4 * (13 * 96 + 128 * 512 + 121 * 8)
    one = (_lib.BistColSum * 1)()
    one[0].M, one[0].N = 1, 520               # one chunk
    assert _lib.lib.bist_col_sum_multi_ws_workspace(one, 1) == HEADER + 4 * 520
    one[0].M = 0
    assert _lib.lib.bist_col_sum_multi_ws_workspace(one, 1) == -1
    assert _lib.lib.bist_col_sum_multi_ws_workspace(one, 0) == -1


def test_the_layernorm_workspace_follows_its_formula():
    """256 + 4 * sum ceil(rows / (4 * max(4, ceil(rows / 512)))) * 2 * d"""
    from bist_amd import _lib
    ln = (_lib.BistLnGrad * 3)()
    ln[0].rows, ln[1].rows, ln[2].rows = 320, 25088, 5      # 20 chunks of 16 rows; 49 rows per wave: 128 chunks of 196; 1 chunk
    assert _lib.lib.bist_layernorm_param_grad_multi_ws_workspace(ln, 3, 512) == HEADER + 4 * (20 + 128 + 1) * 2 * 512
    two = (_lib.BistLnGrad * 2)()
    two[0].rows, two[1].rows = 37, 2049                      # 3 chunks of 16; 5 rows per wave: 103 chunks of 20
    assert _lib.lib.bist_layernorm_param_grad_multi_ws_workspace(two, 2, 256) == HEADER + 4 * (3 + 103) * 2 * 256
    two[1].rows = 0
    assert _lib.lib.bist_layernorm_param_grad_multi_ws_workspace(two, 2, 256) == -1
    assert _lib.lib.bist_layernorm_param_grad_multi_ws_workspace(two, 1, 1) == -1


def test_the_symbols_are_declared_alike_in_the_header_and_the_ctypes_table():
    from bist_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bist_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    ctype_of = {"int": ctypes.c_int, "int64_t": ctypes.c_int64}
    for name, (ret, params) in SIGS.items():
        m = re.search(r"\b(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, name + " is not declared in bist_hip.h"
        assert m.group(1) == ret and re.fullmatch(r"\s*" + params + r"\s*", m.group(2)), (name, m.group(0))
        assert hasattr(raw, name), name + " is not exported"
        res, args = _lib.SIGNATURES[name]
        assert res is ctype_of[ret]
        assert len(args) == m.group(2).count(",") + 1
        for want, got in zip([a.strip() for a in m.group(2).split(",")], args):
            if want.startswith("const BistColSum"):
                assert got is ctypes.POINTER(_lib.BistColSum)
            elif want.startswith("const BistLnGrad"):
                assert got is ctypes.POINTER(_lib.BistLnGrad)
            elif want.startswith("void"):
                assert got is ctypes.c_void_p
            else:
                assert got is {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}[want.split()[0]], (name, want)


def test_the_switch_reads_the_environment_and_no_workspace_is_registered_after_import():
    import subprocess
    import sys
    code = "import bist_amd.ops as o; print(o.REDUCE_SLABS, o.REDUCE_WS is None)"
    env = {k: v for k, v in os.environ.items() if k != "BIST_REDUCE_SLABS"}
    for value, want in ((None, "ln"), ("0", "0"), ("1", "all")):      # default: the LayerNorm jobs; 0: neither flush; 1: the column sums too
        e = dict(env) if value is None else dict(env, BIST_REDUCE_SLABS=value)
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True, check=True).stdout.split()
        assert out == [want, "True"], (value, out)
