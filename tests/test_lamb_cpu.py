"""LAMB as far as no GPU is needed: `name: LAMB` in the three optimizer sections (define_optimizer), the piece table (ops.lamb_table) on the
real arena layouts, the ABI surface of focal_lamb_multi / focal_lamb_multi_advance and their host-side argument checks (they return before
anything is launched, so the device pointers handed in are never dereferenced)."""
import argparse
import copy
import ctypes as C
import math
import os
import re
import types

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DATA = os.path.join(ROOT, "focal_amd", "src", "data")
SECTIONS = [("supervised", "pretrain", "no", ("DeepSense", "optimizer")), ("contrastive", "pretrain", "FOCAL", ("FOCAL", "pretrain_optimizer")),
            ("contrastive", "finetune", "FOCAL", ("FOCAL", "finetune_optimizer"))]


def _args(cfg, train_mode, stage, framework, **kw):
    return argparse.Namespace(model="DeepSense", dataset="MOD", device="cpu", train_mode=train_mode, learn_framework=framework, stage=stage,
                              task="vehicle_classification", tag=None, dataset_config=cfg, **kw)


def _params():
    return [torch.nn.Parameter(torch.zeros(4))]


def _lamb_cfg(cfg, where, **keys):
    c = copy.deepcopy(cfg)
    c[where[0]][where[1]]["name"] = "LAMB"
    c[where[0]][where[1]].update(keys)
    return c


# ------------------------------------------------------------------------------------------------ define_optimizer
@pytest.mark.parametrize("train_mode,stage,framework,where", SECTIONS)
def test_define_optimizer_builds_lamb_in_every_section_with_its_defaults(cfg, train_mode, stage, framework, where):
    from focal_amd.optim import FocalAdamW, FocalLAMB
    from train_utils.optimizer import define_optimizer
    opt = define_optimizer(_args(_lamb_cfg(cfg, where), train_mode, stage, framework), _params())
    assert type(opt) is FocalLAMB and isinstance(opt, FocalAdamW)
    sec = cfg[where[0]][where[1]]
    wd = sec["weight_decay"]["DeepSense"] if isinstance(sec["weight_decay"], dict) else sec["weight_decay"]
    assert opt.exclude_1d is True and opt.max_trust == math.inf and opt.max_grad_norm is None and opt._l2 is False
    assert opt.param_groups[0]["lr"] == sec["start_lr"] and opt.param_groups[0]["weight_decay"] == wd
    assert opt.trust_stats() is None and opt.clip_stats() is None  # (no step yet: nothing to read)
    opt = define_optimizer(_args(_lamb_cfg(cfg, where, lamb_exclude_1d=False, lamb_max_trust=2), train_mode, stage, framework, clip_grad=True), _params())
    assert opt.exclude_1d is False and opt.max_trust == 2.0 and opt.max_grad_norm == 5.0  # -clip_grad composes with it


@pytest.mark.parametrize("train_mode,stage,framework,where", SECTIONS)
@pytest.mark.parametrize("key,value", [("lamb_exclude_1d", 1), ("lamb_exclude_1d", "true"), ("lamb_exclude_1d", None), ("lamb_max_trust", 0),
                                       ("lamb_max_trust", -2.0), ("lamb_max_trust", float("nan")), ("lamb_max_trust", True),
                                       ("lamb_max_trust", "10")])
def test_define_optimizer_refuses_bad_lamb_keys(cfg, train_mode, stage, framework, where, key, value):
    from train_utils.optimizer import define_optimizer
    with pytest.raises(ValueError, match=rf"{where[1]}: {key}"):
        define_optimizer(_args(_lamb_cfg(cfg, where, **{key: value}), train_mode, stage, framework), _params())


def test_lamb_max_trust_accepts_inf_as_the_yaml_spells_it(cfg):
    import yaml
    from train_utils.optimizer import define_optimizer
    assert yaml.safe_load("lamb_max_trust: .inf")["lamb_max_trust"] == math.inf
    c = _lamb_cfg(cfg, SECTIONS[1][3], lamb_max_trust=math.inf)
    assert define_optimizer(_args(c, "contrastive", "pretrain", "FOCAL"), _params()).max_trust == math.inf


def test_shipped_yamls_still_get_adamw(cfg):
    """No shipped section names LAMB; AdamW / Adam build what they built, and the keys of LAMB are not read for them."""
    import glob
    from focal_amd.optim import FocalAdamW
    from oracle.config import load_config
    from train_utils.optimizer import define_optimizer
    seen = set()
    for path in sorted(glob.glob(os.path.join(DATA, "*.yaml"))):
        c = load_config(path)
        for train_mode, stage, framework, where in SECTIONS:
            if where[1] not in c.get(where[0], {}):
                continue  # (not every YAML carries every stage)
            sec = c[where[0]][where[1]]
            assert sec["name"] in ("AdamW", "Adam"), (path, where)
            seen.add(sec["name"])
            cc = copy.deepcopy(c)
            cc[where[0]][where[1]]["lamb_max_trust"] = -1  # not read
            opt = define_optimizer(_args(cc, train_mode, stage, framework), _params())
            assert type(opt) is FocalAdamW and opt._l2 is (sec["name"] == "Adam")
            assert not hasattr(opt, "trust_stats")
    assert seen == {"AdamW", "Adam"}
    c = copy.deepcopy(cfg)
    c["FOCAL"]["pretrain_optimizer"]["name"] = "LARS"
    with pytest.raises(NotImplementedError, match="LARS"):
        define_optimizer(_args(c, "contrastive", "pretrain", "FOCAL"), _params())


def test_optimizer_refuses_bad_options_on_the_host():
    from focal_amd.optim import FocalLAMB
    for bad in (0.0, -2.0, float("nan")):
        with pytest.raises(ValueError, match="max_trust"):
            FocalLAMB(_params(), max_trust=bad)
        with pytest.raises(ValueError, match="max_grad_norm"):
            FocalLAMB(_params(), max_grad_norm=bad)
    with pytest.raises(ValueError, match="exclude_1d"):
        FocalLAMB(_params(), exclude_1d=1)


def test_trust_line_format(caplog):
    import logging
    from train_utils.optimizer import log_clip_stats
    stats = {"tensors": 3, "min": 0.0812, "min_name": "class_layer.0.weight", "median": 1.93, "max": 7.41, "max_name": "a.weight", "phi": {}}
    opt = types.SimpleNamespace(trust_stats=lambda: stats, max_grad_norm=None)
    with caplog.at_level(logging.INFO):
        log_clip_stats(opt, 3)
        log_clip_stats(types.SimpleNamespace(max_grad_norm=None), 4)  # an optimizer without trust ratios logs nothing
    assert [r.getMessage() for r in caplog.records] == ["epoch 3: trust ratio min 0.081 (class_layer.0.weight), median 1.9, max 7.4 (a.weight)"]


# ------------------------------------------------------------------------------------------------ the piece table
def _net(dataset, model, stage="pretrain"):
    from oracle.config import load_config
    cfg = copy.deepcopy(load_config(os.path.join(DATA, f"{dataset}.yaml")))
    task = "vehicle_classification" if "vehicle_classification" in cfg else "activity_classification"
    args = argparse.Namespace(model=model, dataset=dataset, device=torch.device("cpu"), train_mode="contrastive", learn_framework="FOCAL",
                              stage=stage, task=task, tag=None, dataset_config=cfg, compute_dtype="fp32")
    if model == "DeepSense":
        from models.DeepSense import DeepSense
        return args, DeepSense(args)
    from models.SW_Transformer import SW_Transformer
    return args, SW_Transformer(args)


def _check_table(index, lo, hi, exclude_1d):
    """Every property the kernels and the entry points' host checks rely on, from the layout alone."""
    from focal_amd import _lib, ops
    from focal_amd.arena import ALIGN
    P = _lib.LAMB_PIECE
    assert P % 1024 == 0
    rows = list(index.values())
    tb = ops.lamb_table(rows, lo, hi, exclude_1d)
    inside = [i for i, (o, k, _) in enumerate(rows) if lo <= o < hi and k > 0]
    assert tb["rows"] == inside and tb["n"] == hi - lo and len(tb["tensors"]) == len(inside)
    at, next_piece = 0, 0
    for t, (i, (first, last, flags)) in enumerate(zip(inside, tb["tensors"])):
        o, k, shp = rows[i]
        padded = (k + ALIGN - 1) // ALIGN * ALIGN
        assert first == next_piece and last > first  # the ranges partition the list in order
        mine = tb["pieces"][first:last]
        assert all(tid == t for _, _, tid in mine)  # no piece straddles two tensors
        assert mine[0][0] == o - lo and sum(n for _, n, _ in mine) == padded  # the pieces tile the padded extent exactly ...
        for (a, n, _), (b, _, _) in zip(mine, mine[1:]):
            assert a + n == b and n == P                                      # ... back to back, full pieces up to the last
        assert all(n > 0 and n % 4 == 0 and n <= P and a % 4 == 0 for a, n, _ in mine)
        assert last - first == -(-padded // P)
        assert flags == (0 if exclude_1d and len(shp) <= 1 else _lib.LAMB_ADAPT | _lib.LAMB_DECAY), (shp, flags)
        assert o - lo == at
        at += padded
        next_piece = last
    assert next_piece == len(tb["pieces"]) and at == hi - lo  # nothing of the span is left out, nothing outside it is covered
    assert all(0 <= a and a + n <= hi - lo for a, n, _ in tb["pieces"])
    return tb


@pytest.mark.parametrize("dataset,model", [("MOD", "SW_Transformer"), ("MOD", "DeepSense"), ("HAR3LOC", "DeepSense")])
@pytest.mark.parametrize("exclude_1d", [True, False])
def test_table_on_the_real_layouts(dataset, model, exclude_1d):
    from focal_amd.arena import layout
    _, net = _net(dataset, model)
    index, total = layout(net, net._hot)
    tb = _check_table(index, 0, total, exclude_1d)
    ndim = [len(shp) for _, k, shp in index.values() if k > 0]
    assert any(d <= 1 for d in ndim) and any(d >= 2 for d in ndim)
    assert sum(f == 0 for _, _, f in tb["tensors"]) == (sum(d <= 1 for d in ndim) if exclude_1d else 0)
    assert len(tb["pieces"]) > len(tb["tensors"])  # some tensor is longer than a piece


def test_table_of_a_finetune_span_covers_the_span_only():
    """Finetuning hands the optimizer the head only: FocalAdamW._span's [lo, hi) at the arena's end, and a table whose offsets count from lo."""
    from focal_amd.arena import layout
    from focal_amd.optim import FocalLAMB
    from general_utils.weight_utils import set_learnable_params_finetune
    args, net = _net("MOD", "DeepSense", stage="finetune")
    learnable = list(set_learnable_params_finetune(args, net))
    index, total = layout(net, net._hot)
    named = dict(net.named_parameters())
    arena = types.SimpleNamespace(index=index, size=total, params={n: named[n] for n in index})
    opt = FocalLAMB(learnable)
    lo, hi = opt._span(arena)
    assert 0 < lo < hi == total
    tb = _check_table(index, lo, hi, True)
    mine = {id(p) for p in learnable}
    assert [list(index)[i] for i in tb["rows"]] == [n for n in index if id(named[n]) in mine]
    assert tb["pieces"][0][0] == 0 and tb["pieces"][-1][0] + tb["pieces"][-1][1] == hi - lo


def test_table_refuses_a_layout_that_is_not_padded():
    from focal_amd import ops
    with pytest.raises(ValueError, match="lamb_table"):
        ops.lamb_table([(0, 3, (3,)), (3, 8, (8,))], 0, 11)


# ------------------------------------------------------------------------------------------------ ABI surface and host checks
_CTYPE = {"int": C.c_int, "float": C.c_float, "long": C.c_long}


def _declared(hdr, name):
    m = re.search(rf"\bint {name}\((.*?)\);", hdr, re.S)
    assert m, name
    out = []
    for a in m.group(1).split(","):
        a = a.strip()
        out.append("ptr" if "*" in a else _CTYPE[a.replace("const ", "").split()[0]])
    return out


def test_lamb_abi_surface():
    from focal_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "focal_hip.h")).read()
    for macro, value in (("FOCAL_LAMB_PIECE", _lib.LAMB_PIECE), ("FOCAL_LAMB_RECORD_WORDS", _lib.LAMB_RECORD_WORDS)):
        assert re.search(rf"#define {macro} {value}\b", hdr), macro
    assert re.search(r"#define FOCAL_ABI_VERSION 14\b", hdr) and _lib.ABI_VERSION == 14  # exports were added, nothing changed
    lib = _lib.load()
    for name in ("focal_lamb_multi", "focal_lamb_multi_advance"):
        assert hasattr(lib, name), name
        res, args = _lib.PROTOTYPES[name]
        want = _declared(hdr, name)
        assert res is C.c_int and len(args) == len(want), (name, len(args), len(want))
        for i, (got, w) in enumerate(zip(args, want)):
            is_ptr = got is C.c_void_p or hasattr(got, "contents")
            assert is_ptr if w == "ptr" else got is w, (name, i, got, w)
    # both take the optional clip row, record and max_norm in front of the stream, as the _clip_ forms of AdamW do
    for name in ("focal_lamb_multi", "focal_lamb_multi_advance"):
        assert _lib.PROTOTYPES[name][1][-6:] == _lib.PROTOTYPES["focal_adamw_clip_multi"][1][-6:]
    m = re.search(r"typedef struct \{([^}]*)\} focal_lamb_table;", hdr)
    assert m and [f[0] for f in _lib.LambTable._fields_] == re.findall(r"(\w+)[;,]", m.group(1))
    assert C.sizeof(_lib.LambTable) == 56  # 2 pointers, 2 ints, (pointer, int + padding) twice
    for name in ("lamb_table", "lamb_table_upload", "lamb_multi"):
        assert callable(getattr(ops, name)), name
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "focal_lamb_multi" in doc and "focal_lamb_multi_advance" in doc


DUMMY = 4096  # a never-dereferenced, 16-byte aligned "device" address
GOOD = {"pieces": [(0, 8, 0), (8, 8192, 1), (8200, 16, 1)], "tensors": [(0, 1, 0), (1, 3, 3)]}


def _rc(advance, pieces=None, tensors=None, n=8216, max_trust=math.inf, partial_words=None, record_words=None, host=True, dev=DUMMY, partials=True,
        record=True, lr=True, state_words=40, l2=0, clip=None, p=DUMMY, shadow=None, npieces=None, ntensors=None):
    from focal_amd import _lib
    pieces = GOOD["pieces"] if pieces is None else pieces
    tensors = GOOD["tensors"] if tensors is None else tensors
    words = [w for row in pieces for w in (*row, 0)] + [w for row in tensors for w in (*row, 0)]
    harr = (C.c_int32 * max(len(words), 1))(*words)
    tb = _lib.LambTable(C.cast(harr, C.c_void_p) if host else None, dev, len(pieces) if npieces is None else npieces,
                        len(tensors) if ntensors is None else ntensors, DUMMY if partials else None,
                        2 * len(pieces) if partial_words is None else partial_words, DUMMY if record else None,
                        3 * len(tensors) if record_words is None else record_words)
    arr = lambda a=DUMMY: (C.c_void_p * 1)(a)
    d = _lib.AdamWDesc(0.9, 0.999, 1e-8, 0.05, l2)
    tail = (None, 0, None, 0, 0.0, None) if clip is None else clip + (None,)
    head = (C.byref(d), 1, arr(p), arr(), arr(), arr(), arr(shadow) if shadow else None, (C.c_long * 1)(n), C.byref(tb), max_trust,
            DUMMY if lr else None)
    if advance:
        return _lib.load().focal_lamb_multi_advance(*head, DUMMY, state_words, DUMMY, *tail)
    return _lib.load().focal_lamb_multi(*head, DUMMY, *tail)


@pytest.mark.parametrize("advance", [False, True])
@pytest.mark.parametrize("kw,needle", [
    (dict(lr=False), "null argument"), (dict(host=False), "null table"), (dict(dev=None), "null table"), (dict(partials=False), "null table"),
    (dict(record=False), "null table"), (dict(dev=DUMMY + 4), "16-byte aligned"), (dict(p=DUMMY + 4), "16-byte aligned buffer"),
    (dict(p=None), "null or not"), (dict(shadow=DUMMY + 2), "shadow"), (dict(n=8214), "multiple of 4"), (dict(l2=1), "l2_decay"),
    (dict(max_trust=0.0), "max_trust"), (dict(max_trust=-1.0), "max_trust"), (dict(max_trust=float("nan")), "max_trust"),
    (dict(pieces=[(0, 0, 0)], tensors=[(0, 1, 3)]), "piece 0 length 0"),
    (dict(pieces=[(0, 6, 0)], tensors=[(0, 1, 3)]), "piece 0 length 6"),
    (dict(pieces=[(0, 8196, 0)], tensors=[(0, 1, 3)], n=8196), "FOCAL_LAMB_PIECE = 8192"),
    (dict(pieces=[(0, 16, 0), (8, 8, 0)], tensors=[(0, 2, 3)]), "ascend without overlap"),
    (dict(pieces=[(8, 8, 0), (0, 8, 0)], tensors=[(0, 2, 3)]), "ascend without overlap"),
    (dict(pieces=[(2, 8, 0)], tensors=[(0, 1, 3)]), "multiples of 4"),
    (dict(pieces=[(-4, 8, 0)], tensors=[(0, 1, 3)]), "piece 0 at offset -4"),
    (dict(n=8212), "behind the segment's 8212 elements"),
    (dict(pieces=[(0, 8, 2)], tensors=[(0, 1, 3)]), "names tensor 2 of 1"), (dict(pieces=[(0, 8, -1)], tensors=[(0, 1, 3)]), "names tensor -1"),
    (dict(tensors=[(0, 1, 0), (2, 3, 3)]), "partition"), (dict(tensors=[(0, 2, 0), (1, 3, 3)]), "inside the range of tensor 0"), (dict(tensors=[(0, 1, 0), (1, 4, 3)]), "partition"),
    (dict(tensors=[(0, 1, 0), (1, 1, 3)]), "partition"), (dict(tensors=[(0, 1, 0), (1, 2, 3)]), "ranges end at piece 2 of 3"),
    (dict(pieces=[(0, 8, 0), (8, 8, 0), (16, 8, 1)], tensors=[(0, 1, 0), (1, 3, 3)]), "inside the range of tensor 1"),
    (dict(tensors=[(0, 1, 4), (1, 3, 3)]), "flags 4"), (dict(partial_words=5), "2 per piece"), (dict(record_words=5), "FOCAL_LAMB_RECORD_WORDS"),
    (dict(npieces=0), "pieces of"), (dict(ntensors=0), "pieces of"), (dict(ntensors=4), "pieces of"),
    (dict(clip=(None, 1024, DUMMY, 8, 1.0)), "null"), (dict(clip=(DUMMY, 1024, None, 8, 1.0)), "null"),
    (dict(clip=(DUMMY, 1023, DUMMY, 8, 1.0)), "FOCAL_CLIP_SCRATCH_WORDS"), (dict(clip=(DUMMY, 1024, DUMMY, 7, 1.0)), "FOCAL_CLIP_RECORD_WORDS"),
    (dict(clip=(DUMMY, 1024, DUMMY, 8, 0.0)), "max_norm"), (dict(clip=(DUMMY, 1024, DUMMY, 8, float("nan"))), "max_norm")])
def test_lamb_host_checks_refuse(advance, kw, needle):
    from focal_amd import _lib
    assert _rc(advance, **kw) != 0
    msg = _lib.load().focal_last_error().decode()
    assert needle in msg and ("lamb_multi_advance" if advance else "lamb_multi:") in msg, msg


def test_lamb_advance_needs_a_segment_and_its_step_state():
    from focal_amd import _lib
    assert _rc(True, n=0) != 0 and "no non-empty segment" in _lib.load().focal_last_error().decode()
    assert _rc(True, state_words=4) != 0 and "FOCAL_STEP_STATE_WORDS" in _lib.load().focal_last_error().decode()


def test_ops_refuse_bad_bounds_before_the_library():
    from focal_amd import ops
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_trust"):
            ops.lamb_multi([], [], None, None, max_trust=bad)
        with pytest.raises(ValueError, match="max_norm"):
            ops.lamb_multi([], [], None, None, clip=((None, None), bad))
    with pytest.raises(ValueError, match="tables"):
        ops.lamb_multi([], [{}], None, None)
