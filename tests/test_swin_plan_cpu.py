"""focal_amd.swin_engine.plan_block: the one place where a Swin block's kernel forms are decided.  No GPU: the library's *_supported queries
are host-side (the library is loaded as tests/test_oracle_cpu.py::test_library_exports_every_declared_symbol loads it).  MOD geometry:
4 heads, 3 x 3 windows."""
import os

import pytest
import torch

BF, F32 = torch.bfloat16, torch.float32
HEADS, WINDOW_TOKENS = 4, 9
ROWS = {64: 73728, 128: 18432, 256: 4608}  # a step's row counts; no pinned field depends on them
SWITCHES = ("FOCAL_MLP_PROJ", "FOCAL_MLP_WIDE", "FOCAL_MLP_WIDE_BWD")

# env, dtype, C -> attn_qkv, mlp, proj, next_ln of a block that has a successor, mlp_bwd, ln2_bwd, ln1_bwd
TABLE = [
    (None, BF, 64, True, "fused", "in_mlp", True, "fused", "mlp", "dx"),
    (None, BF, 128, False, "wide", "in_mlp", True, "plain", "dx", "dx"),
    (None, BF, 256, False, "wide", "in_mlp", True, "plain", "plain", "plain"),
    (None, F32, 64, False, "plain", "resid_ln", True, "plain", "plain", "plain"),
    (None, F32, 128, False, "plain", "plain", False, "plain", "plain", "plain"),
    (None, F32, 256, False, "plain", "plain", False, "plain", "plain", "plain"),
    ("FOCAL_MLP_PROJ=0", BF, 64, True, "fused", "resid_ln", True, "fused", "mlp", "dx"),
    ("FOCAL_MLP_PROJ=0", BF, 128, False, "wide", "resid_ln", True, "plain", "dx", "dx"),
    ("FOCAL_MLP_PROJ=0", BF, 256, False, "wide", "plain", True, "plain", "plain", "plain"),
    ("FOCAL_MLP_WIDE=0", BF, 128, False, "plain", "resid_ln", True, "plain", "dx", "dx"),
    ("FOCAL_MLP_WIDE=0", BF, 256, False, "plain", "plain", False, "plain", "plain", "plain"),
    ("FOCAL_MLP_WIDE_BWD=1", BF, 128, False, "wide", "in_mlp", True, "wide", "mlp", "dx"),
    ("FOCAL_MLP_WIDE_BWD=1", BF, 256, False, "wide", "in_mlp", True, "wide", "plain", "plain"),
]


def _set_env(monkeypatch, env):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    if env is not None:
        monkeypatch.setenv(*env.split("="))


@pytest.mark.parametrize("env,ct,C,attn_qkv,mlp,proj,next_ln,mlp_bwd,ln2_bwd,ln1_bwd", TABLE)
def test_plan_is_the_pinned_table(monkeypatch, env, ct, C, attn_qkv, mlp, proj, next_ln, mlp_bwd, ln2_bwd, ln1_bwd):
    from focal_amd.swin_engine import plan_block
    _set_env(monkeypatch, env)
    for has_next in (True, False):
        p = plan_block(ct, ROWS[C], C, HEADS, WINDOW_TOKENS, has_next)
        assert (p.attn_qkv, p.mlp, p.proj, p.mlp_bwd, p.ln2_bwd, p.ln1_bwd) == (attn_qkv, mlp, proj, mlp_bwd, ln2_bwd, ln1_bwd), (has_next, p)
        assert p.next_ln is (next_ln and has_next), (has_next, p)   # never for the last block of a stage
        assert p.dw_group in (0, 1, 2)


@pytest.mark.parametrize("env", [None, "FOCAL_MLP_PROJ=0", "FOCAL_MLP_WIDE=0", "FOCAL_MLP_WIDE_BWD=1"])
def test_no_plan_names_a_combination_the_kernels_do_not_have(monkeypatch, env):
    from focal_amd import ops
    from focal_amd.swin_engine import plan_block
    _set_env(monkeypatch, env)
    for ct in (BF, F32):
        for C in (32, 64, 96, 128, 192, 256, 512):
            for M in (72, 1000, 4608, 73728):
                for has_next in (True, False):
                    p = plan_block(ct, M, C, HEADS, WINDOW_TOKENS, has_next)
                    assert p.mlp in ("fused", "wide", "plain") and p.proj in ("in_mlp", "resid_ln", "plain")
                    assert p.mlp_bwd in ("fused", "wide", "plain") and p.ln2_bwd in ("mlp", "dx", "plain") and p.ln1_bwd in ("dx", "plain")
                    if p.proj == "in_mlp":
                        assert p.mlp != "plain"
                    if p.ln2_bwd == "mlp" and p.mlp_bwd == "wide":
                        assert C <= 128
                    assert (p.mlp_bwd == "fused") == (p.mlp == "fused")
                    if p.ln2_bwd == "mlp":
                        assert p.mlp_bwd != "plain"
                    if p.next_ln:
                        assert has_next
                    # the group kind is the library's answer for the block's stand-alone weight-gradient shapes
                    shapes = [(C, C), (3 * C, C)] + ([] if p.mlp == "fused" else [(C, 4 * C), (4 * C, C)])
                    assert p.dw_group == min(ops.dw_group_kind(ops.code(ct), M, n, k) for n, k in shapes)


def test_the_removed_lab_switches_are_gone_from_the_package():
    # (the names are assembled so that this file does not hold them either)
    removed = ["FOCAL_" + n for n in ("DW_PAIR", "LN_BWD_MAX_C", "MLP_WIDE_LN256", "MLP_BWD_ATOMICS")]
    pkg = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "focal_amd")
    hits = []
    for root, dirs, files in os.walk(pkg):
        dirs[:] = [d for d in dirs if d != "__pycache__"]
        for f in files:
            if f.endswith((".so", ".pyc", ".o", ".a")):
                continue
            text = open(os.path.join(root, f), errors="replace").read()
            hits += [(os.path.join(root, f), n) for n in removed if n in text]
    assert not hits, hits


def test_the_engine_reads_one_switch_of_its_own():
    import inspect
    import re
    from focal_amd import swin_engine
    src = inspect.getsource(swin_engine)
    assert re.findall(r"os\.environ\.get\(\"(\w+)\"", src) == ["FOCAL_TAIL_FP32"] and src.count("os.environ") == 1
    assert "os.environ" not in inspect.getsource(swin_engine.SwinModEncoder._backward_blocks)
    assert "os.environ" not in inspect.getsource(swin_engine.SwinModEncoder._mlp_partials)
    assert inspect.getsource(swin_engine.SwinModEncoder.forward).count('saved["blocks"].append(') == 1
