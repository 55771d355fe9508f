"""jitter / channel_shuffle / time_mask / freq_mask: the float64 restatement every other test of them measures against, the host draws of
data_augmenter.Augmenter against the reference classes' (tests/golden/augment_ex_seed5.npz, written by gen_golden_augment_ex.py from the
reference's JitterAugmenter / ChannelShuffleAugmenter / TimeMaskAugmenter / FreqMaskAugmenter with their draws forced), the folded ABI
surface and the constructor's refusals.  Nothing here needs a GPU."""
import copy
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment_ex_seed5.npz")
MODS = ("seismic", "audio")


# ---------------------------------------------------------------------------------------------- the restatement (float64, numpy / torch.fft)
def mix32(x):
    """focal_mix32 (include/focal_hip.h states it beside the noise formula), on uint32 arrays."""
    x = np.asarray(x, dtype=np.uint64) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def restated_noise(key, salt, shape):
    """The unit-variance jitter noise of a [B, C, I, n] tensor, the header's formula in float64: element e (flat index of the DESTINATION
    element) takes the cosine (e even) or sine (e odd) branch of the Box-Muller pair p = e >> 1 of the key mixed with the salt."""
    total = int(np.prod(shape))
    k = int(mix32(np.uint64(int(key) ^ int(mix32((int(salt) * 0x9E3779B9 + 0x85EBCA6B) & 0xFFFFFFFF)))))
    e = np.arange(total, dtype=np.uint64)
    p = e >> 1
    h1 = mix32((k + (2 * p) * 0x85EBCA6B) & 0xFFFFFFFF)
    h2 = mix32((k + (2 * p + 1) * 0x85EBCA6B) & 0xFFFFFFFF)
    u1 = 1.0 - (h1 >> 8).astype(np.float64) / 16777216.0
    u2 = (h2 >> 8).astype(np.float64) / 16777216.0
    r = np.sqrt(-2.0 * np.log(u1))
    z = np.where(e & 1 == 1, r * np.sin(2 * np.pi * u2), r * np.cos(2 * np.pi * u2))
    return torch.from_numpy(z.reshape(shape))


def restate_time(x, scale=1.0, flip=False, perm=None, noise=None, chan=None, time_mask=None):
    """The time-domain half of `restate`: float64 [B, C, I, n] rows as they enter the transform."""
    t = x.double() * scale
    if chan is not None:
        t = t[:, list(chan)]
    if flip:
        t = torch.flip(t, dims=(2, 3))
    if perm is not None:
        t = t[:, :, list(perm)]
    if noise is not None:
        t = t + noise.double()
    if time_mask is not None and time_mask[1] > 0:
        t = t.clone()
        t[..., time_mask[0]:time_mask[0] + time_mask[1]] = 0
    return t


def restate(x, scale=1.0, flip=False, perm=None, phase=0.0, noise=None, chan=None, time_mask=None, freq_mask=None):
    """float64 [B, 2C, I, n] view of x [B, C, I, n]: mask_t(perm / flip / chan-select(scale * x) + noise), the two-sided DFT packed as
    (Re, Im) channel pairs, the rotation, mask_f.  noise: the tensor ADDED (already times std), or None."""
    t = restate_time(x, scale, flip, perm, noise, chan, time_mask)
    f = torch.fft.fft(t, dim=-1) * complex(math.cos(phase), math.sin(phase))
    B, Cc, I, n = t.shape
    out = torch.view_as_real(f).permute(0, 1, 4, 2, 3).reshape(B, 2 * Cc, I, n).clone()
    if freq_mask is not None and freq_mask[1] > 0:
        out[..., freq_mask[0]:freq_mask[0] + freq_mask[1]] = 0
    return out


def rel_err(a, b):
    return (a.double() - b.double()).abs().max().item() / max(b.double().abs().max().item(), 1e-30)


# ---------------------------------------------------------------------------------------------- helpers
def args_with_pool(cfg, time_names, freq_names, **sections):
    from conftest import make_args
    c = copy.deepcopy(cfg)
    c["FOCAL"]["random_augmenters"] = {"time_augmenters": list(time_names), "freq_augmenters": list(freq_names)}
    for k, v in sections.items():
        c.setdefault(k, {}).update(v)
    return make_args(c, "SW_Transformer", torch.device("cpu"), "bf16")


ALL_TIME = ["permutation", "negation", "time_warp", "horizontal_flip", "mag_warp", "scaling", "jitter", "channel_shuffle", "time_mask"]
ALL_FREQ = ["phase_shift", "freq_mask"]
VALUE_RANGE = {"jitter": {"value_range": {"seismic": 3.0, "audio": 7.5}}}


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


# ---------------------------------------------------------------------------------------------- tests
def test_forced_host_draws_reproduce_the_reference(cfg, gold, monkeypatch):
    """(new ground) `_time_mask`, `_freq_mask`, `_channel_shuffle`, `_jitter` behind Augmenter._draw with random / randint / torch.randint /
    torch.randperm forced to the fixture's values: the keywords they return are the lo / n / order / std the reference's classes applied."""
    from data_augmenter import Augmenter as A
    # (the fixture's reference ran with the reference's own value ranges: hand the stds it computed back in as ranges)
    pct = cfg["jitter"]["std_in_percent"]
    sections = {"jitter": {"value_range": {m: float(gold[f"jitter.std.{m}"]) * 100 / pct for m in MODS}}}
    c = copy.deepcopy(cfg)
    c["loc_mod_spectrum_len"]["shake"]["audio"] = 96   # (the fixture's audio rows are 96 samples long)
    aug = A.Augmenter(args_with_pool(c, ALL_TIME, ALL_FREQ, **sections))
    x = {"shake": {m: torch.from_numpy(gold[f"in.{m}"]) for m in MODS}}
    dur, start = int(gold["draw.time_mask.duration"]), int(gold["draw.time_mask.start"])
    band, fstart = int(gold["draw.freq_mask.band"]), int(gold["draw.freq_mask.start"])
    order = [int(v) for v in gold["draw.channel_shuffle"]]
    monkeypatch.setattr(A, "random", lambda: 0.0)   # every coin hits
    log = []

    def queue(values):
        it = iter(values)
        return lambda *a, **k: (log.append(a), next(it))[1]
    # modality order of the config: seismic (n = 20), audio (n = 96); per modality the reference calls randint, then torch.randint
    monkeypatch.setattr(A, "randint", queue([dur, dur]))
    monkeypatch.setattr(torch, "randint", queue([torch.tensor([start])] * 2))
    kw = aug._draw(A.TIME_AUGMENTERS["time_mask"], "time_mask", x)
    assert all(kw["shake"][m] == {"time_mask": (start, dur)} for m in MODS)
    # randint(1, floor(10 * 0.3)) inclusive, torch.randint(0, I - duration): INTERVAL-sized numbers (the reference's quirk)
    assert log == [(1, 3), (0, 10 - dur, (1,))] * 2
    log.clear()
    monkeypatch.setattr(A, "randint", queue([band, band]))
    monkeypatch.setattr(torch, "randint", queue([torch.tensor([fstart])] * 2))
    kw = aug._draw(A.FREQ_AUGMENTERS["freq_mask"], "freq_mask", x)
    assert all(kw["shake"][m] == {"freq_mask": (fstart, band)} for m in MODS)
    assert log == [(1, math.floor(20 * 0.3)), (0, 20 - band, (1,)), (1, math.floor(96 * 0.3)), (0, 96 - band, (1,))]
    log.clear()
    monkeypatch.setattr(torch, "randperm", queue([torch.tensor(order)] * 2))
    kw = aug._draw(A.TIME_AUGMENTERS["channel_shuffle"], "channel_shuffle", x)
    assert all(kw["shake"][m] == {"chan": order} for m in MODS) and log == [(3,), (3,)]
    monkeypatch.setattr(torch, "randint", lambda *a, **k: torch.tensor([int(gold["draw.jitter.key"])]))
    kw = aug._draw(A.TIME_AUGMENTERS["jitter"], "jitter", x)
    for m in MODS:
        std, key = kw["shake"][m]["jitter"]
        assert key == int(gold["draw.jitter.key"]) and abs(std - float(gold[f"jitter.std.{m}"])) < 1e-12 * std, m
    # a mask that reaches past the row is clipped as the reference's slice clips it
    monkeypatch.setattr(A, "randint", lambda a, b: 3)
    monkeypatch.setattr(torch, "randint", lambda *a, **k: torch.tensor([6]))
    assert A._time_mask(torch.zeros(1, 1, 10, 8), {"max_duration": 3}) == {"time_mask": (6, 2)}


def test_restatement_reproduces_the_reference_spectra(gold):
    """The float64 restatement against the reference classes' outputs through the reference's own transform (float32): 1e-6 relative."""
    dur, start = int(gold["draw.time_mask.duration"]), int(gold["draw.time_mask.start"])
    band, fstart = int(gold["draw.freq_mask.band"]), int(gold["draw.freq_mask.start"])
    order = [int(v) for v in gold["draw.channel_shuffle"]]
    for m in MODS:
        x = torch.from_numpy(gold[f"in.{m}"])
        noise = torch.from_numpy(gold[f"jitter.noise.{m}"]).double() * float(gold[f"jitter.std.{m}"])
        cases = {"jitter": dict(noise=noise), "channel_shuffle": dict(chan=order), "time_mask": dict(time_mask=(start, dur)),
                 "freq_mask": dict(freq_mask=(fstart, band))}
        for name, kw in cases.items():
            assert rel_err(restate(x, **kw), torch.from_numpy(gold[f"{name}.{m}"])) < 1e-6, (name, m)
        # and the forced noise IS the documented generator's: the GPU tests compare the kernel with these spectra
        z = restated_noise(int(gold["draw.jitter.key"]), 0, x.shape)
        assert (z.float() - torch.from_numpy(gold[f"jitter.noise.{m}"])).abs().max().item() == 0.0


def test_noise_restatement_is_standard_normal():
    z = restated_noise(0x1234ABCD, 3, (4, 2, 10, 256)).reshape(-1)
    n = z.numel()
    assert abs(z.mean().item()) < 4.5 / math.sqrt(n) and abs(z.var().item() - 1) < 4.5 * math.sqrt(2 / n)
    assert not torch.equal(z, restated_noise(0x1234ABCD, 4, (4, 2, 10, 256)).reshape(-1))


def test_folded_view_abi_surface():
    """The folded surface (ABI 14): ONE pool, ONE transform problem and the extra record have the sizes include/focal_hip.h static_asserts,
    the plan and the augmentation descriptor did not move, and the exports the fold removed are gone."""
    from focal_amd import _lib
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), "include", "focal_hip.h")).read()
    assert re.search(r"static_assert\(sizeof\(focal_view_extra\) == 92,", hdr) and C.sizeof(_lib.ViewExtra) == 92
    assert re.search(r"static_assert\(sizeof\(focal_view_pool\) == 376,", hdr) and C.sizeof(_lib.ViewPool) == 376
    assert re.search(r"static_assert\(sizeof\(focal_fft_problem\) == 328,", hdr) and C.sizeof(_lib.FftProblem) == 328
    assert len(re.findall(r"static_assert\(sizeof\(focal_(?:view|fft)_", hdr)) == 3
    assert C.sizeof(_lib.AugDesc) == 148 and C.sizeof(_lib.ViewPlan) == 228
    assert re.search(r"#define FOCAL_VIEW_MAX_POOL 16\b", hdr) and _lib.VIEW_MAX_POOL == 16
    assert (_lib.VIEW_JITTER, _lib.VIEW_CHANNEL_SHUFFLE, _lib.VIEW_TIME_MASK, _lib.VIEW_FREQ_MASK) == (8, 9, 10, 11)
    assert re.search(r"FOCAL_VIEW_JITTER = 8,\s+FOCAL_VIEW_CHANNEL_SHUFFLE = 9, FOCAL_VIEW_TIME_MASK = 10, FOCAL_VIEW_FREQ_MASK = 11", hdr)
    assert "#define FOCAL_ABI_VERSION 14" in hdr and _lib.ABI_VERSION == 14
    gone = ("focal_view_draw_ex", "focal_view_draw_shared", "focal_fft_realpack_multi_ex")
    assert not any(re.search(name + r"\b", hdr) for name in gone + ("focal_view_pool_ex", "focal_fft_problem_ex", "FOCAL_VIEW_MAX_POOL_EX"))
    assert not any(name in _lib.PROTOTYPES for name in gone) and not any(hasattr(_lib, n) for n in ("ViewPoolEx", "FftProblemEx", "VIEW_MAX_POOL_EX"))
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.focal_abi_version() == 14
        assert not any(hasattr(lib, name) for name in gone)
        assert hasattr(lib, "focal_view_draw") and hasattr(lib, "focal_fft_realpack_multi")


def test_view_pool_fills_one_struct_and_refuses_bad_pools(cfg):
    """What view_pool fills and refuses; a pool of 9 .. 16 entries of the kinds 0 .. 7 is accepted and the Augmenter allocates no extras
    for it."""
    from focal_amd import _lib, ops
    old = ops.view_pool([("permutation", 0.5), ("scaling", 0.5)], [10, 10])
    assert old.n_aug == 2 and old.kind[0] == 4 and old.kind[1] == 2 and old.intervals[1] == 10
    new = ops.view_pool([("permutation", 0.5), ("jitter", 0.5), ("time_mask", 0.5)], [10, 10], jitter_std=[0.1, 0.2], time_mask=[(3, 10), (3, 10)])
    assert new.kind[1] == 8 and abs(new.jitter_std[1] - 0.2) < 1e-7 and new.tmask_d[0] == 3 and new.tmask_i[1] == 10
    assert type(old) is type(new) is _lib.ViewPool
    nine = ops.view_pool([("negation", 0.5)] * 9, [10])                               # more than 8 entries of old kinds
    assert nine.n_aug == 9 and all(nine.kind[i] == 1 for i in range(9))
    assert ops.view_pool([("negation", 0.5)] * 16, [10]).n_aug == 16
    with pytest.raises(ValueError):
        ops.view_pool([("negation", 0.5)] * 17, [10])
    with pytest.raises(ValueError):
        ops.view_pool([("jitter", 0.5)], [10, 10])                                    # jitter without its per-slot std
    assert set(ops.VIEW_KINDS) >= {"jitter", "channel_shuffle", "time_mask", "freq_mask"}
    # the Augmenter decides on the NAMES: nine old-kind entries draw no extras (the state's tensors follow the inputs: CPU ones here)
    from data_augmenter import Augmenter as A
    x = {"shake": {m: torch.zeros(2, 1, 10, 20) for m in MODS}}
    nine = A.Augmenter(args_with_pool(cfg, ["negation", "scaling", "horizontal_flip"] * 3, []))
    st = nine._device_state(x)
    assert nine.device_draws_supported() and st["pool"].n_aug == 9 and st["extras"] is None and st["plans"].shape == (4, 228)
    four = A.Augmenter(args_with_pool(cfg, ["negation", "time_mask"], []))
    st = four._device_state(x)
    assert st["pool"].n_aug == 2 and st["extras"] is not None and st["extras"].shape == (4, 92)


def test_augmenter_accepts_a_pool_naming_all_four(cfg):
    """(new ground: "Invalid augmenter provided" before)  The reference's full pool; device draws stay supported."""
    from data_augmenter import Augmenter as A
    aug = A.Augmenter(args_with_pool(cfg, ALL_TIME, ALL_FREQ, **VALUE_RANGE))
    assert len(aug.aug_names) == 11 and aug.device_draws_supported()
    d = aug._derived
    assert d["time_mask"][("shake", "audio")] == {"max_duration": 3}
    assert d["freq_mask"][("shake", "audio")] == {"max_band_width": 480} and d["freq_mask"][("shake", "seismic")] == {"max_band_width": 6}
    assert abs(d["jitter"][("shake", "audio")]["std"] - 7.5 / 100 * 0.2) < 1e-15
    # the shipped pools are what they were, and an Augmenter on them derives nothing
    from conftest import make_args
    plain = A.Augmenter(make_args(cfg, "SW_Transformer", torch.device("cpu"), "bf16"))
    assert len(plain.aug_names) == 7 and plain._derived == {}
    with pytest.raises(NotImplementedError):   # sequential composition in the supervised pipeline stays out of scope
        c = copy.deepcopy(cfg)
        c["SW_Transformer"]["fixed_augmenters"] = {"time_augmenters": ["jitter"], "freq_augmenters": ["no"]}
        c["jitter"]["value_range"] = VALUE_RANGE["jitter"]["value_range"]
        a = make_args(c, "SW_Transformer", torch.device("cpu"), "bf16")
        a.train_mode, a.stage = "supervised", "train"
        A.Augmenter(a).forward_fixed({"shake": {m: torch.zeros(1, 1, 10, 20) for m in MODS}})


@pytest.mark.parametrize("names,sections,key", [
    (["time_mask"], {"time_mask": {"mask_ratio": 0.05}}, "time_mask.mask_ratio"),        # D = floor(10 * 0.05) = 0
    (["freq_mask"], {"freq_mask": {"mask_ratio": 0.06}}, "freq_mask.mask_ratio"),        # W(seismic) = floor(20 * 0.06) = 1
    (["channel_shuffle"], {"loc_mod_in_time_channels": {"shake": {"audio": 17, "seismic": 1}}}, "loc_mod_in_time_channels.shake.audio"),
    (["jitter"], {}, "jitter.value_range"),                                              # MOD.yaml ships without one
    (["jitter"], {"jitter": {"value_range": {"audio": 1.0}}}, "jitter.value_range"),     # a modality missing
])
def test_augmenter_refuses_impossible_configurations(cfg, names, sections, key):
    from data_augmenter import Augmenter as A
    time_names = [n for n in names if n != "freq_mask"] or ["no"]
    freq_names = [n for n in names if n == "freq_mask"] or ["no"]
    with pytest.raises(ValueError) as e:
        A.Augmenter(args_with_pool(cfg, time_names, freq_names, **sections))
    assert key in str(e.value)


def test_shipped_configs_carry_the_sections_and_keep_their_pools():
    import yaml
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "focal_amd", "src", "data")
    for name, ranged in (("MOD", False), ("HAR4", True), ("HAR3LOC", True)):
        c = yaml.safe_load(open(os.path.join(root, name + ".yaml")))
        assert c["jitter"]["prob"] == 0.5 and c["jitter"]["std_in_percent"] == 0.2 and c["channel_shuffle"] == {"prob": 0.5}
        assert c["time_mask"] == {"prob": 0.5, "mask_ratio": 0.3} and c["freq_mask"] == {"prob": 0.5, "mask_ratio": 0.3}
        assert ("value_range" in c["jitter"]) == ranged
        if ranged:
            assert set(c["jitter"]["value_range"]) == set(c["modality_names"])
        pool = c["FOCAL"]["random_augmenters"]
        assert pool["time_augmenters"] == ["permutation", "negation", "time_warp", "horizontal_flip", "mag_warp", "scaling"]
        assert pool["freq_augmenters"] == ["phase_shift"]
