"""The device-drawn Mixup and the captured classifier step, as far as no GPU is needed: the ABI surface (focal_mixup_draw,
focal_mixup_multi and their records), the host-side argument checks of the two entry points (they return before anything is launched),
the host restatement the GPU tests compare against, and the switches of the two training loops."""
import argparse
import ctypes as C
import os
import re

import numpy as np
import pytest

import mix_restatement as mr

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_mix_abi_surface():
    from focal_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "focal_hip.h")).read()
    assert _lib.ABI_VERSION == 14 and re.search(r"#define FOCAL_ABI_VERSION 14\b", hdr)
    assert re.search(r"static_assert\(sizeof\(focal_mix_record\) == 140,", hdr) and C.sizeof(_lib.MixRecord) == 140
    assert re.search(r"static_assert\(sizeof\(focal_mix_problem\) == 40,", hdr) and C.sizeof(_lib.MixProblem) == 40
    assert re.search(r"#define FOCAL_MIX_MAX_BATCH 4096\b", hdr) and _lib.MIX_MAX_BATCH == 4096
    assert re.search(r"#define FOCAL_MIX_GAMMA_TRIES 16\b", hdr) and _lib.MIX_GAMMA_TRIES == 16
    assert _lib.MixRecord.lam.offset == 8 and _lib.MixRecord.box.offset == 12 and _lib.MixProblem.x.offset == 16 and _lib.MixProblem.slot.offset == 32
    lib = _lib.load()
    for name in ("focal_mixup_draw", "focal_mixup_multi", "focal_mixup_fwd"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    for name in ("mixup_draw", "mixup_multi", "new_mix_record", "mixup"):
        assert callable(getattr(ops, name)), name
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "focal_mixup_draw" in doc and "focal_mixup_multi" in doc


def _draw_rc(prob=1.0, switch=0.75, ma=1.0, ca=1.0, B=8, slots=((10, 1600), (10, 20)), rec=True, perm=True):
    """focal_mixup_draw with arguments its host checks refuse: it returns before a launch, so the (never dereferenced) device pointers
    are dummies."""
    from focal_amd import _lib
    n = len(slots)
    Is, Ss = (C.c_int * max(n, 1))(*[s[0] for s in slots]), (C.c_int * max(n, 1))(*[s[1] for s in slots])
    dummy = C.c_void_p(256)
    return _lib.load().focal_mixup_draw(prob, switch, ma, ca, B, n, Is, Ss, dummy, 1, 7, dummy if rec else None, dummy if perm else None, None)


@pytest.mark.parametrize("kw,needle", [
    (dict(B=0), "batch"), (dict(B=4097), "batch"), (dict(slots=((10, 20),) * 9), "slots"), (dict(slots=()), "slots"),
    (dict(ma=0.0, ca=0.0), "alpha"), (dict(ma=-1.0), "alpha"), (dict(prob=1.5), "prob"), (dict(prob=-0.1), "prob"), (dict(switch=2.0), "prob"),
    (dict(slots=((0, 20), (10, 20))), "slot 0"), (dict(slots=((10, 20), (10, 0))), "slot 1"), (dict(rec=False), "record"), (dict(perm=False), "record")])
def test_mixup_draw_host_checks_refuse(kw, needle):
    from focal_amd import _lib
    assert _draw_rc(**kw) != 0
    assert needle in _lib.load().focal_last_error().decode()


def _multi_rc(problems, rec=True, perm=True):
    from focal_amd import _lib
    arr = (_lib.MixProblem * max(len(problems), 1))()
    for q, p in zip(arr, problems):
        q.B, q.C, q.I, q.S, q.x, q.y, q.slot = p
    dummy = C.c_void_p(256)
    return _lib.load().focal_mixup_multi(len(problems), arr, dummy if rec else None, dummy if perm else None, None)


def test_mixup_multi_host_checks_refuse():
    ok = (8, 1, 10, 20, 4096, 8192, 0)
    bad = [[], [ok] * 9, [(0, 1, 10, 20, 4096, 8192, 0)], [(8, 1, 10, 20, 4096, 4096, 0)], [(8, 1, 10, 20, None, 8192, 0)],
           [(8, 1, 10, 20, 4096, 8192, 8)], [(8, 1, 10, 20, 4096, 8192, -1)], [ok, (4, 1, 10, 20, 4096, 8192, 1)],
           [(4097, 1, 10, 20, 4096, 8192, 0)], [(8, 1 << 12, 1 << 10, 1 << 9, 4096, 8192, 0)]]
    for problems in bad:
        assert _multi_rc(problems) != 0, problems
    assert _multi_rc([ok], rec=False) != 0 and _multi_rc([ok], perm=False) != 0


def test_restatement_draws_are_well_formed():
    """The host statement of the header's formulas (the GPU test compares the kernel to it bit for bit): permutations, boxes inside the
    tensor, coins at their rates, a seed sequence without short cycles."""
    cfg = dict(prob=1.0, switch_prob=0.75, mixup_alpha=1.0, cutmix_alpha=1.0)
    slots = [(10, 1600), (10, 20)]
    seed, cuts, lams, firsts, seen = 12345, 0, [], np.zeros(8, dtype=int), set()
    for _ in range(1024):
        d = mr.draw(seed, 0x4D495846, cfg, 8, slots)
        assert sorted(d["perm"].tolist()) == list(range(8)) and d["apply"] == 1 and 0.0 <= float(d["lam"]) < 1.0
        for (I, S), (yl, yh, xl, xh) in zip(slots, d["boxes"]):
            assert 0 <= yl <= yh <= I and 0 <= xl <= xh <= S
            assert d["cut"] or (yl, yh, xl, xh) == (0, 0, 0, 0)
        cuts += d["cut"]
        lams.append(float(d["lam"]))
        firsts[d["perm"][0]] += 1
        seen.add(seed)
        seed = mr.next_seed(seed)
    assert len(seen) == 1024
    assert abs(cuts - 768) < 5 * np.sqrt(1024 * 0.75 * 0.25)
    assert np.all(np.abs(firsts - 128) < 5 * np.sqrt(1024 * 0.125 * 0.875)), firsts
    mb, var, vb = mr.beta_moment_bounds(1.0, 1024)
    assert abs(np.mean(lams) - 0.5) < mb and abs(np.var(lams) - var) < vb
    ident = mr.draw(99, 1, dict(cfg, prob=0.0), 5, slots)
    assert ident["apply"] == 0 and ident["cut"] == 0 and ident["lam"] == 1.0 and all(b == [0, 0, 0, 0] for b in ident["boxes"])
    # B = 257 spans more than one pass of the kernel's workgroup over the samples: still a permutation
    assert sorted(mr.draw(7, 1, cfg, 257, slots)["perm"].tolist()) == list(range(257))


@pytest.mark.parametrize("alpha", [0.4, 2.0])
def test_numpy_beta_passes_the_bounds_the_device_draw_is_held_to(alpha):
    """The control of test_classifier_step_gpu.py's statistics: numpy.random.beta, 1024 draws, fixed seed, meets the same 5-standard-error
    bounds on mean and variance (from Beta(a, a)'s own moments) that the device draw must meet."""
    lam = np.random.default_rng(20240).beta(alpha, alpha, size=1024)
    mb, var, vb = mr.beta_moment_bounds(alpha, 1024)
    assert abs(lam.mean() - 0.5) < mb and abs(lam.var() - var) < vb, (lam.mean(), lam.var(), var)


def test_restated_mix_clamps_like_the_kernel():
    x = np.random.default_rng(3).standard_normal((3, 2, 5, 7)).astype(np.float32)
    y = mr.mix(x, [-4, 9, 1], 1, 1, 0.3, (-3, 99, 2, 1000))
    assert np.array_equal(y[:, :, :, 2:], x[[0, 2, 1]][:, :, :, 2:]) and np.array_equal(y[:, :, :, :2], x[:, :, :, :2])
    assert np.array_equal(mr.mix(x, [2, 0, 1], 0, 1, 0.3, (0, 5, 0, 7)), x)
    assert np.array_equal(mr.mix(x, [2, 0, 1], 1, 1, 0.3, (2, 2, 0, 7)), x)  # an empty box


def _aug(cfg, time=("mixup",), freq=("phase_shift",), **mix):
    import copy
    from data_augmenter.Augmenter import Augmenter
    c = copy.deepcopy(cfg)
    c["DeepSense"]["fixed_augmenters"] = {"time_augmenters": list(time), "freq_augmenters": list(freq)}
    c["mixup"].update(mix)
    args = argparse.Namespace(model="DeepSense", dataset="MOD", device="cpu", train_mode="supervised", learn_framework="no", stage="pretrain",
                              task="vehicle_classification", tag=None, dataset_config=c)
    return Augmenter(args)


def test_fixed_device_draws_supported_and_the_loop_switches(cfg, monkeypatch):
    from train_utils.supervised_train import classifier_step_form
    for model in ("DeepSense", "SW_Transformer"):  # every shipped fixed pipeline is covered
        args = argparse.Namespace(model=model, dataset="MOD", device="cpu", train_mode="supervised", learn_framework="no", stage="pretrain",
                                  task="vehicle_classification", tag=None, dataset_config=cfg)
        from data_augmenter.Augmenter import Augmenter
        assert Augmenter(args).fixed_device_draws_supported()
    assert _aug(cfg, time=("no",), freq=("no",)).fixed_device_draws_supported()
    assert not _aug(cfg, mode="batch").fixed_device_draws_supported()
    assert not _aug(cfg, cutmix_minmax=[0.2, 0.8]).fixed_device_draws_supported()
    assert not _aug(cfg, time=("mixup", "scaling")).fixed_device_draws_supported()
    assert not _aug(cfg, freq=("freq_mask",)).fixed_device_draws_supported()
    a = _aug(cfg)
    assert a.FIXED_MIX_STREAM != 0x56494557 and a.FIXED_VIEW_STREAM != 0x56494557 and a.FIXED_MIX_STREAM != a.FIXED_VIEW_STREAM
    monkeypatch.delenv("FOCAL_HOST_DRAWS", raising=False)
    ns = argparse.Namespace
    assert classifier_step_form(ns(), a, "fixed") == (True, False)
    assert classifier_step_form(ns(no_graph=True), a, "fixed") == (False, False)
    assert classifier_step_form(ns(host_draws=True), a, "fixed") == (True, True)
    assert classifier_step_form(ns(), _aug(cfg, mode="batch"), "fixed") == (True, True)   # silently the host-drawn form
    assert classifier_step_form(ns(), _aug(cfg, mode="batch"), "no") == (True, False)     # finetune draws nothing
    monkeypatch.setenv("FOCAL_HOST_DRAWS", "1")
    assert classifier_step_form(ns(no_graph=True), a, "fixed") == (False, True)


def test_captured_train_step_keeps_its_surface():
    """The refactor into a shared base left CapturedTrainStep's attributes and entry points where they were."""
    from focal_amd.graph_step import CapturedClassifierStep, CapturedTrainStep, ClassifierSegments, StepSegments
    opt = argparse.Namespace()
    for cls in (CapturedTrainStep, CapturedClassifierStep):
        s = cls(object(), object(), opt, warm_steps=3, enabled=False)
        assert (s.warm_steps, s.enabled, s.key, s.replay, s.seen, s.segments, s.loss, s.replays, s.eager_steps) == (3, False, None, None, 0, None, None, 0, 0)
        assert callable(s._step) and callable(s._capture) and callable(s.step_from_inputs)
    assert callable(CapturedTrainStep._key) and callable(CapturedTrainStep._segments)
    assert issubclass(ClassifierSegments, StepSegments)
