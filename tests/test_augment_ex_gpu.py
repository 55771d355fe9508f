"""jitter / channel_shuffle / time_mask / freq_mask on the device: the extras folded into the three DFT kernels against the float64
restatement of test_augment_ex_cpu.py (and through it the reference's classes: tests/golden/augment_ex_seed5.npz), the counter-RNG noise,
the extended draw's distributions, bit-compatibility with the existing exports, and the product path (Augmenter.forward_random_pair)."""
import copy
import math

import numpy as np
import pytest
import torch

from test_augment_ex_cpu import ALL_FREQ, ALL_TIME, GOLD, MODS, VALUE_RANGE, args_with_pool, restate, restated_noise

pytestmark = pytest.mark.gpu

DEV = "cuda"
STREAM = 0x56494557
FOCAL_POOL = [("permutation", 0.5), ("negation", 0.5), ("time_warp", 0.5), ("horizontal_flip", 0.5), ("mag_warp", 0.5), ("scaling", 0.5),
              ("phase_shift", 0.5)]   # (test_kernels_gpu.py's)
# every kernel form: the small-row launch; MFMA 16 x 16; an odd row count -> the generic kernel; n1 != n2 -> the generic kernel
SHAPES = [(2, 3, 10, 20), (2, 3, 10, 256), (1, 3, 3, 256), (2, 3, 10, 96)]
STD, KEY, SALT = 0.5, 0x0BADC0DE, 7


def rnd(*shape, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV)


def bound(n, scale=1.0, std=0.0):
    """The transform's existing bound (test_kernels_gpu.py: 2e-4 sqrt(n) max(1, |scale|) on unit-normal rows), times (1 + std) for the
    rows jitter widens."""
    return 2e-4 * math.sqrt(n) * max(1.0, abs(scale)) * (1.0 + std)


@pytest.fixture(scope="module")
def ops():
    from focal_amd import ops as o
    return o


def cases_for(shape):
    B, Cc, I, n = shape
    chan = [(c + 1) % Cc for c in range(Cc)]
    perm = [(3 * i + 1) % I for i in range(I)] if I % 3 else [(i + 1) % I for i in range(I)]
    tm, fm = (n // 4, n // 3), (n // 2 - 1, n // 5 + 1)
    return {"jitter": dict(jitter=(STD, KEY), noise_salt=SALT), "channel_shuffle": dict(chan=chan), "time_mask": dict(time_mask=tm),
            "freq_mask": dict(freq_mask=fm),
            "composed": dict(scale=-1.25, flip=True, perm=perm, phase=0.7, jitter=(STD, KEY), noise_salt=SALT, chan=chan, time_mask=tm, freq_mask=fm)}


def run_both_ways(ops, x, kw):
    """(host-argument extras, the same values read from DEVICE records: a plan for scale / flip / perm / phase, an extra for the rest)"""
    host = ops.fft_realpack(x, **kw)
    plans, extras = ops.new_view_plans(1, 1, DEV), ops.new_view_extras(1, 1, DEV)
    ops.write_view_plan(plans, 0, scale=kw.get("scale", 1.0), flip=kw.get("flip", False), perm=kw.get("perm"), phase=kw.get("phase", 0.0))
    ops.write_view_extra(extras, 0, jitter=kw.get("jitter"), chan=kw.get("chan"), time_mask=kw.get("time_mask"), freq_mask=kw.get("freq_mask"), like=x)
    dev = ops.fft_realpack_multi([dict(x=x, plan=plans[0], x_warped=x, extra=extras[0], noise_salt=kw.get("noise_salt"))])[0]
    return host, dev


def reference_for(x, kw):
    noise = None
    if "jitter" in kw:
        noise = restated_noise(kw["jitter"][1], kw.get("noise_salt", 0), x.shape) * kw["jitter"][0]
    return restate(x.cpu(), scale=kw.get("scale", 1.0), flip=kw.get("flip", False), perm=kw.get("perm"), phase=kw.get("phase", 0.0), noise=noise,
                   chan=kw.get("chan"), time_mask=kw.get("time_mask"), freq_mask=kw.get("freq_mask"))


def check_case(ops, x, name, kw):
    n = x.shape[-1]
    host, dev = run_both_ways(ops, x, kw)
    assert torch.equal(host, dev), name                      # the same kernels, the same values: only where they are read from differs
    ref = reference_for(x, kw)
    err = (host.cpu().double() - ref).abs().max().item()
    lim = bound(n, kw.get("scale", 1.0), STD if "jitter" in kw else 0.0)
    print(f"{name} {tuple(x.shape)}: max abs error {err:.3e} (bound {lim:.3e})")
    assert err < lim, (name, err, lim)
    if "freq_mask" in kw:
        lo, cnt = kw["freq_mask"]
        assert cnt > 0 and torch.all(host[..., lo:lo + cnt] == 0.0)   # masked bins are exactly 0.0, in all 2C channels
    if name == "time_mask":                                   # exactly the spectrum of the zeroed input
        lo, cnt = kw["time_mask"]
        z = x.clone()
        z[..., lo:lo + cnt] = 0
        assert torch.equal(host, ops.fft_realpack(z))
    if name == "channel_shuffle":                             # exactly the spectrum of the shuffled input
        assert torch.equal(host, ops.fft_realpack(x[:, kw["chan"]].contiguous()))
    assert not torch.equal(host, ops.fft_realpack(x))


# ---------------------------------------------------------------------------------------------- 1. forced extras against float64 torch.fft
@pytest.mark.parametrize("shape", SHAPES)
def test_forced_extras_match_the_float64_restatement(ops, shape):
    """(new ground) Each of the four alone, and all four composed with scale / flip / perm / phase, through every kernel form."""
    x = rnd(*shape, seed=sum(shape))
    for name, kw in cases_for(shape).items():
        check_case(ops, x, name, kw)


def test_forced_extras_on_the_audio_rows(ops):
    """MFMA 40 x 40 (the raised LDS grant), once: the composed case at the MOD audio row length."""
    shape = (2, 1, 10, 1600)
    x = rnd(*shape, seed=1600)
    check_case(ops, x, "composed", cases_for(shape)["composed"])
    check_case(ops, x, "jitter", cases_for(shape)["jitter"])


def test_reference_fixture_spectra(ops):
    """The reference classes' own outputs for their forced draws, within the same bound (the jitter noise the reference was handed is the
    documented generator's for the stored key, salt 0: test_augment_ex_cpu.py checks that)."""
    gold = np.load(GOLD)
    order = [int(v) for v in gold["draw.channel_shuffle"]]
    for m in MODS:
        x = torch.from_numpy(gold[f"in.{m}"]).to(DEV)
        std = float(gold[f"jitter.std.{m}"])
        cases = {"jitter": dict(jitter=(std, int(gold["draw.jitter.key"]))), "channel_shuffle": dict(chan=order),
                 "time_mask": dict(time_mask=(int(gold["draw.time_mask.start"]), int(gold["draw.time_mask.duration"]))),
                 "freq_mask": dict(freq_mask=(int(gold["draw.freq_mask.start"]), int(gold["draw.freq_mask.band"])))}
        for name, kw in cases.items():
            host, dev = run_both_ways(ops, x, kw)
            err = (host.cpu().double() - torch.from_numpy(gold[f"{name}.{m}"]).double()).abs().max().item()
            assert torch.equal(host, dev) and err < bound(x.shape[-1], 1.0, std if name == "jitter" else 0.0), (name, m, err)


def test_bad_extras_are_refused(ops):
    x = rnd(2, 3, 10, 20)
    for kw in (dict(chan=[0, 0, 1]), dict(chan=[0, 1]), dict(time_mask=(15, 6)), dict(freq_mask=(-1, 2)), dict(jitter=(-0.1, 1))):
        with pytest.raises(ValueError):
            ops.fft_realpack(x, **kw)
    from focal_amd import _lib
    arr = (_lib.FftProblem * 1)()
    d, a, xx, tw, out = ops._fft_problem(x)
    arr[0].d, arr[0].x, arr[0].twiddle, arr[0].out = d, x.data_ptr(), tw.data_ptr(), out.data_ptr()
    arr[0].has_extra = 1
    for field, val in (("tmask_n", 21), ("fmask_lo", 21), ("use_chan", 1)):   # (use_chan with chan = 0, 0, 0: not a permutation)
        e = _lib.ViewExtra()
        setattr(e, field, val)
        arr[0].extra = e
        assert _lib.load().focal_fft_realpack_multi(1, arr, None) == -1 and b"fft_realpack_multi:" in _lib.load().focal_last_error()
    for kw in (dict(time_mask=[(0, 10)] * 2), dict(time_mask=[(3, 3)] * 2), dict(freq_mask=[(1, 20)] * 2), dict(freq_mask=[(20, 20)] * 2),
               dict(channels=[17, 3])):
        name = "channel_shuffle" if "channels" in kw else next(iter(kw))
        pool = ops.view_pool([(name, 0.5)], [10, 10], **kw)
        with pytest.raises(_lib.FocalHipError):
            ops.view_draw(pool, 2, 2, ops.new_rng_state(1, DEV), STREAM, ops.new_view_plans(2, 2, DEV), extras=ops.new_view_extras(2, 2, DEV))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 2. noise quality
def recovered_noise(ops, x, key, salt, std=1.0):
    """The noise the kernel added, from its own output: the inverse float64 DFT of (out(x + noise) - float64 DFT of x)."""
    out = ops.fft_realpack(x, jitter=(std, key), noise_salt=salt)
    f = out.cpu().double()
    z = torch.fft.ifft(torch.complex(f[:, 0::2], f[:, 1::2]) - torch.fft.fft(x.cpu().double(), dim=-1), dim=-1)
    return out, z.real, z.imag


def corr(a, b):
    return abs(np.corrcoef(a.reshape(-1).numpy(), b.reshape(-1).numpy())[0, 1])


def test_jitter_noise_is_white_standard_normal(ops):
    """std 1 on a zero input: 22 080 samples over the MFMA kernel ([4, 2, 10, 256]) and the small-row kernel ([4, 2, 10, 20]).  Moments
    and correlations within 4.5 sigma of a standard normal sample of that size; a pure function of (key, salt, element index)."""
    zs, pairs = [], {"row": [], "rows": [], "halves": [], "key": [], "salt": []}
    for shape in ((4, 2, 10, 256), (4, 2, 10, 20)):
        x0 = torch.zeros(*shape, device=DEV)
        out, z, zi = recovered_noise(ops, x0, KEY, SALT)
        n = shape[-1]
        assert zi.abs().max().item() < bound(n, 1.0, 1.0)                           # real input -> Hermitian spectrum
        assert (z - restated_noise(KEY, SALT, shape)).abs().max().item() < bound(n, 1.0, 1.0)   # and it IS the documented generator
        assert torch.equal(out, recovered_noise(ops, x0, KEY, SALT)[0])             # same key and salt: identical bits
        x = rnd(*shape, seed=5)                                                     # the noise does not depend on x
        assert (recovered_noise(ops, x, KEY, SALT)[1] - z).abs().max().item() < bound(n, 1.0, 1.0)
        pairs["row"].append((z[..., :-1], z[..., 1:]))                              # lag 1 along the row
        pairs["rows"].append((z[:, :, :-1], z[:, :, 1:]))                           # neighbouring rows
        pairs["halves"].append((z[:2], z[2:]))                                      # the two batch halves
        pairs["key"].append((z, recovered_noise(ops, x0, KEY + 1, SALT)[1]))        # another key
        pairs["salt"].append((z, recovered_noise(ops, x0, KEY, SALT + 1)[1]))       # another rank's salt
        zs.append(z.reshape(-1))
    z = torch.cat(zs)
    N = z.numel()
    assert N == 22080
    mean, var = z.mean().item(), z.var(unbiased=False).item()
    kurt = ((z - mean) ** 4).mean().item() / var ** 2 - 3.0
    print(f"noise: N {N} mean {mean:.4f} var {var:.4f} excess kurtosis {kurt:.4f}")
    assert abs(mean) < 4.5 / math.sqrt(N) and abs(var - 1.0) < 4.5 * math.sqrt(2 / N) and abs(kurt) < 4.5 * math.sqrt(24 / N)
    for name, ps in pairs.items():
        a = torch.cat([p[0].reshape(-1) for p in ps])
        b = torch.cat([p[1].reshape(-1) for p in ps])
        c = corr(a, b)
        print(f"noise: correlation {name} {c:.4f} over {a.numel()} pairs (bound {4.5 / math.sqrt(N):.4f})")
        assert c < 4.5 / math.sqrt(N), (name, c)


# ---------------------------------------------------------------------------------------------- 3. draw distributions
def sigma45(p, m):
    return 4.5 * math.sqrt(p * (1 - p) / m)


def test_extended_draws_have_the_reference_distributions(ops):
    """(new ground) focal_view_draw with extras, the reference's full eleven-entry pool, 8 views x 8 slots x 200 seed words = 12 800 records and
    1 600 pool draws.  Every bound is 4.5 sigma of the binomial for the number of samples at hand."""
    from focal_amd import _lib
    names = ALL_TIME + ALL_FREQ
    n_views, n_slots, S = 8, 8, 200
    chans = [3, 3, 6, 1, 16, 3, 2, 4]
    stds = [0.05 * (s + 1) for s in range(n_slots)]
    fm = [(6, 20)] * 6 + [(480, 1600)] * 2
    pool = ops.view_pool([(n, 0.5) for n in names], [10] * n_slots, jitter_std=stds, channels=chans, time_mask=[(3, 10)] * n_slots, freq_mask=fm)
    assert type(pool) is _lib.ViewPool and pool.n_aug == 11
    per = n_views * n_slots
    plans, extras = ops.new_view_plans(S * n_views, n_slots, DEV), ops.new_view_extras(S * n_views, n_slots, DEV)
    seed = ops.new_rng_state(1, DEV)
    seeds = torch.tensor([7919 * i + 13 for i in range(S)], dtype=seed.dtype, device=DEV)
    for i in range(S):
        seed[0:1].copy_(seeds[i:i + 1])
        ops.view_draw(pool, n_views, n_slots, seed, STREAM, plans[i * per:(i + 1) * per], extras=extras[i * per:(i + 1) * per])
    P, E = ops.read_view_plans(plans), ops.read_view_extras(extras)          # (one copy each)
    assert len(P) == 12800
    # pool index: uniform over the eleven, shared by a view's slots
    k = np.array([p.pool_index for p in P]).reshape(S * n_views, n_slots)
    assert (k == k[:, :1]).all()
    freq = np.bincount(k[:, 0], minlength=11) / (S * n_views)
    assert np.abs(freq - 1 / 11).max() < sigma45(1 / 11, S * n_views), freq
    # coins at p = 0.5, independent between slots; the record's kind is the pool entry's
    kind = np.array([p.kind for p in P]).reshape(S * n_views, n_slots)
    hit = kind != 0
    assert abs(hit.mean() - 0.5) < sigma45(0.5, hit.size) and abs(np.corrcoef(hit[:, 0], hit[:, 1])[0, 1]) < 4.5 / math.sqrt(S * n_views)
    want = np.array([ops.VIEW_KINDS[n] for n in names])[k]
    assert (kind[hit] == want[hit]).all()
    slot = np.tile(np.arange(n_slots), S * n_views)
    ident = bytes(_lib.ViewExtra())
    new = {ops.VIEW_KINDS[n] for n in ops.VIEW_KINDS_EX}
    for p, e in zip(P, E):
        if p.kind not in new:                                                # old kinds and misses: the extra is the identity (zero bytes)
            assert bytes(e) == ident
        else:                                                                # new kinds: the plan applies nothing
            assert p.aug.scale == 1.0 and p.aug.flip == 0 and p.aug.use_perm == 0 and p.aug.phase_cos == 1.0 and p.aug.phase_sin == 0.0 and p.warp == 0
    sel = lambda name: [(e, s) for p, e, s in zip(P, E, slot) if p.kind == ops.VIEW_KINDS[name]]
    # jitter: the slot's std; keys differ between views, slots and seeds
    jit = sel("jitter")
    assert len(jit) > 400 and all(e.jitter_std == np.float32(stds[s]) for e, s in jit)
    assert len({e.jitter_key for e, _ in jit}) == len(jit)
    assert all(e.use_chan == 0 and e.tmask_n == 0 and e.fmask_n == 0 for e, _ in jit)
    # time mask: duration uniform on 1 .. D = 3; start uniform on 0 .. I - duration - 1 given the duration
    tm = sel("time_mask")
    dur = np.array([e.tmask_n for e, _ in tm])
    st = np.array([e.tmask_lo for e, _ in tm])
    assert len(tm) > 400 and dur.min() == 1 and dur.max() == 3
    for d in (1, 2, 3):
        m = (dur == d).sum()
        assert abs(m / len(dur) - 1 / 3) < sigma45(1 / 3, len(dur)), d
        vals = 10 - d
        f = np.bincount(st[dur == d], minlength=vals) / m
        assert len(f) == vals and np.abs(f - 1 / vals).max() < sigma45(1 / vals, m), (d, f)
    # freq mask: band uniform on 1 .. W; start uniform on 0 .. n - band - 1 given the band
    fq = sel("freq_mask")
    small = [(e.fmask_n, e.fmask_lo) for e, s in fq if s < 6]
    band = np.array([b for b, _ in small])
    assert len(small) > 300 and band.min() == 1 and band.max() == 6
    for b in range(1, 7):
        m = (band == b).sum()
        assert abs(m / len(band) - 1 / 6) < sigma45(1 / 6, len(band)), b
        vals = 20 - b
        f = np.bincount(np.array([lo for bb, lo in small if bb == b]), minlength=vals) / m
        assert len(f) == vals and np.abs(f - 1 / vals).max() < sigma45(1 / vals, m), (b, f)
    big = np.array([(e.fmask_n, e.fmask_lo) for e, s in fq if s >= 6], dtype=np.float64)
    assert len(big) > 100 and big[:, 0].min() >= 1 and big[:, 0].max() <= 480 and (big[:, 1] >= 0).all() and (big[:, 1] + big[:, 0] < 1600 + 1e-9).all()
    u_band, u_start = (big[:, 0] - 0.5) / 480, (big[:, 1] + 0.5) / (1600 - big[:, 0])          # ~ uniform on (0, 1): sigma of the mean = 1 / sqrt(12 m)
    assert abs(u_band.mean() - 0.5) < 4.5 / math.sqrt(12 * len(big)) and abs(u_start.mean() - 0.5) < 4.5 / math.sqrt(12 * len(big))
    # channel shuffle: a permutation of the slot's channels, the rest of the table untouched; uniform per position (the 3-channel slots)
    cs = sel("channel_shuffle")
    assert len(cs) > 400
    three = []
    for e, s in cs:
        c = chans[s]
        order = [e.chan[i] for i in range(16)]
        assert e.use_chan == 1 and sorted(order[:c]) == list(range(c)) and order[c:] == list(range(c, 16)), (s, order)
        if c == 3:
            three.append(order[:3])
    three = np.array(three)
    pos = np.stack([(three == v).mean(0) for v in range(3)])
    assert len(three) > 120 and np.abs(pos - 1 / 3).max() < sigma45(1 / 3, len(three)), pos
    # a pure function of (seed, stream, view, slot)
    again_p, again_e = ops.new_view_plans(n_views, n_slots, DEV), ops.new_view_extras(n_views, n_slots, DEV)
    ops.view_draw(pool, n_views, n_slots, seed, STREAM, again_p, extras=again_e)
    assert torch.equal(again_p, plans[-per:]) and torch.equal(again_e, extras[-per:])


# ---------------------------------------------------------------------------------------------- 4. compatibility
def test_extended_draw_writes_the_old_kinds_bytes(ops):
    """The draw with extras= over a pool of the kinds 0 .. 7 (ONE pool, both ways): plan bytes equal those of the draw without extras (and
    the advancing form's, state words included), extras all identity -- 50 seeds."""
    old = new = ops.view_pool(FOCAL_POOL, [10, 10])
    seed = ops.new_rng_state(1, DEV)
    pa, pb, eb = ops.new_view_plans(2, 2, DEV), ops.new_view_plans(2, 2, DEV), ops.new_view_extras(2, 2, DEV)
    for i in range(50):
        seed[0] = 104729 * i + 7
        eb.fill_(0xFF)
        ops.view_draw(old, 2, 2, seed, STREAM, pa)
        ops.view_draw(new, 2, 2, seed, STREAM, pb, extras=eb)
        assert torch.equal(pa, pb) and int(eb.max().item()) == 0, i
    sa, sb = ops.new_rng_state(4242, DEV), ops.new_rng_state(4242, DEV)
    for i in range(50):
        eb.fill_(0xFF)
        ops.view_draw_shared(old, 2, 2, sa, STREAM, pa)
        ops.view_draw_shared(new, 2, 2, sb, STREAM, pb, extras=eb)
        assert torch.equal(pa, pb) and torch.equal(sa, sb) and int(eb.max().item()) == 0, i
    assert int(sa[1].item()) == 50


@pytest.mark.parametrize("shape", SHAPES + [(2, 1, 10, 1600)])
def test_identity_extras_change_no_bit(ops, shape):
    """focal_fft_realpack_multi with identity extras (none, a zero host record, a zero device record) against the call without any:
    the plan path and the host-augmentation path."""
    x = rnd(*shape, seed=3)
    I = shape[2]
    perm = [(i + 1) % I for i in range(I)]
    aug = dict(scale=1.3, flip=True, perm=perm, phase=-0.4)
    plans, zero = ops.new_view_plans(1, 1, DEV), ops.new_view_extras(1, 1, DEV)
    ops.write_view_plan(plans, 0, **aug)
    plain_host = ops.fft_realpack_multi([dict(x=x, **aug), dict(x=x)])
    plain_plan = ops.fft_realpack_multi([dict(x=x, plan=plans[0], x_warped=x)])
    # problems WITHOUT an extra inside a call that runs the extended kernels (another problem of the call carries one, on the host or on the device)
    for carrier in (dict(x=x, time_mask=(1, 2)), dict(x=x, extra=zero[0])):
        got = ops.fft_realpack_multi([carrier, dict(x=x, **aug), dict(x=x), dict(x=x, plan=plans[0], x_warped=x), dict(x=x, noise_salt=5)])
        assert torch.equal(got[1], plain_host[0]) and torch.equal(got[2], plain_host[1]) and torch.equal(got[3], plain_plan[0]), carrier
        assert torch.equal(got[4], plain_host[1]), carrier
    for extra_kw in (dict(noise_salt=0), dict(noise_salt=5, time_mask=(0, 0)), dict(extra=zero[0])):
        got = ops.fft_realpack_multi([dict(x=x, **aug, **extra_kw), dict(x=x, **extra_kw)])
        assert torch.equal(got[0], plain_host[0]) and torch.equal(got[1], plain_host[1]), extra_kw
        got = ops.fft_realpack_multi([dict(x=x, plan=plans[0], x_warped=x, **extra_kw)])
        assert torch.equal(got[0], plain_plan[0]), extra_kw


# ---------------------------------------------------------------------------------------------- 5. product path
def product_augmenter(cfg, time_names=ALL_TIME, freq_names=ALL_FREQ, **sections):
    from data_augmenter import Augmenter as A
    merged = copy.deepcopy(VALUE_RANGE)
    for k, v in sections.items():
        merged.setdefault(k, {}).update(v)
    args = args_with_pool(cfg, time_names, freq_names, **merged)
    args.device = torch.device(DEV)
    return A.Augmenter(args)


def view_reference(x, p, e, salt=0):
    """The float64 view of x for the drawn (plan, extra) pair; the spline warps through the oracle, as test_kernels_gpu.py's product test."""
    from focal_amd import _lib
    from oracle import augment as oa
    t = x.cpu()
    if p.warp == _lib.VIEW_MAG_WARP:
        t = oa.mag_warp(t, np.array([p.knots[j] for j in range(p.nknots)], np.float64), 4)
    elif p.warp == _lib.VIEW_TIME_WARP:
        t = oa.time_warp(t, np.array([p.knots[j] for j in range(p.nknots)], np.float64), 6)
    I, Cc = x.shape[2], x.shape[1]
    noise = restated_noise(e.jitter_key, salt, x.shape) * e.jitter_std if e.jitter_std > 0 else None
    return restate(t, scale=p.aug.scale, flip=bool(p.aug.flip), perm=[p.aug.perm[j] for j in range(I)] if p.aug.use_perm else None,
                   phase=math.atan2(p.aug.phase_sin, p.aug.phase_cos), noise=noise, chan=[e.chan[c] for c in range(Cc)] if e.use_chan else None,
                   time_mask=(e.tmask_lo, e.tmask_n), freq_mask=(e.fmask_lo, e.fmask_n))


def test_product_pair_with_the_full_pool_follows_the_restatement(ops, cfg):
    """Augmenter.forward_random_pair on the reference's eleven-augmenter pool: whatever the device drew, each view is the restatement's view
    for the drawn records; over 64 seeds all eleven augmenters and the identity occur."""
    from focal_amd import runtime
    aug = product_augmenter(cfg)
    assert aug.device_draws_supported()
    tx = {"shake": {"audio": rnd(2, 1, 10, 1600, seed=1), "seismic": rnd(2, 1, 10, 20, seed=2)}}
    mods = list(tx["shake"])             # (the slots follow the input's order)
    seed = runtime.view_state(torch.device(DEV))
    saved = seed.clone()
    seen = set()
    try:
        for it in range(64):
            seed[0] = 1000 + 17 * it
            v = aug.forward_random_pair(tx)
            st = next(iter(aug._dev_states.values()))
            assert [k[1] for k in st["flat"]] == mods and st["extras"] is not None and len(aug._dev_states) == 1
            plans, extras = ops.read_view_plans(st["plans"]), ops.read_view_extras(st["extras"])
            for view in range(2):
                for i, m in enumerate(mods):
                    p, e = plans[view * 2 + i], extras[view * 2 + i]
                    seen.add(p.kind)
                    x = tx["shake"][m]
                    f = view_reference(x, p, e)
                    std = aug._derived["jitter"][("shake", m)]["std"]
                    assert e.jitter_std in (0.0, np.float32(std))
                    lim = bound(x.shape[-1], p.aug.scale, e.jitter_std)
                    if p.warp:   # (the resampling's own error: the bound of test_product_augmenter_device_pair_follows_the_oracle)
                        lim = 2e-4 * math.sqrt(x.shape[-1]) * 2 + 1e-4 * f.abs().max().item()
                    got = v[view]["shake"][m]
                    assert got.shape[0] == 2 and (got.cpu().double() - f).abs().max().item() < lim, (it, view, m, p.kind)
    finally:
        seed.copy_(saved)
    assert seen == set(range(12)), seen


def test_captured_pair_draws_fresh_jitter_on_every_replay(ops, cfg):
    """One captured graph (single branch: the draw, then the transforms, on one stream) of forward_random_pair with jitter certain: three
    replays give three different keys per (view, slot), and each replay's views are the restatement's for the keys it drew."""
    from focal_amd import runtime
    aug = product_augmenter(cfg, ["jitter"], [], jitter={"prob": 1.0})
    tx = {"shake": {"audio": rnd(2, 1, 10, 1600, seed=1), "seismic": rnd(2, 1, 10, 20, seed=2)}}
    mods = list(tx["shake"])
    saved = runtime.view_state(torch.device(DEV)).clone()
    aug.forward_random_pair(tx)          # (allocates the state; the capture below only replays launches)
    torch.cuda.synchronize()
    st = next(iter(aug._dev_states.values()))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            views = aug.forward_random_pair(tx)
    keys = []
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        plans, extras = ops.read_view_plans(st["plans"]), ops.read_view_extras(st["extras"])
        keys.append([e.jitter_key for e in extras])
        for view in range(2):
            for i, m in enumerate(mods):
                p, e = plans[view * 2 + i], extras[view * 2 + i]
                assert p.kind == ops.VIEW_KINDS["jitter"] and e.jitter_std > 0
                x = tx["shake"][m]
                err = (views[view]["shake"][m].cpu().double() - view_reference(x, p, e)).abs().max().item()
                assert err < bound(x.shape[-1], 1.0, e.jitter_std), (view, m, err)
    runtime.view_state(torch.device(DEV)).copy_(saved)
    assert len({k for ks in keys for k in ks}) == 12     # 3 replays x 2 views x 2 slots: all different


@pytest.mark.parametrize("name", ["jitter", "channel_shuffle", "time_mask", "freq_mask"])
def test_host_path_forward_random_with_forced_draws(ops, cfg, monkeypatch, name):
    """Augmenter.forward("random") end to end -- host draws (forced), keywords, focal_fft_realpack_multi -- with a one-entry pool of each
    new kind, against the restatement.  The seismic rows are 8 samples long, so the forced time mask [6, 9) is clipped to [6, 8) there."""
    from data_augmenter import Augmenter as A
    aug = product_augmenter(cfg, [name] if name != "freq_mask" else [], [name] if name == "freq_mask" else [])
    tx = {"shake": {"seismic": rnd(2, 3, 10, 8, seed=8), "audio": rnd(2, 3, 10, 96, seed=96)}}
    key, order = 0x00C0FFEE, [2, 0, 1]
    monkeypatch.setattr(A, "random", lambda: 0.0)                      # every coin hits
    monkeypatch.setattr(A, "randint", lambda a, b: 3)                  # duration / band
    monkeypatch.setattr(torch, "randint", lambda *a, **k: torch.tensor([key if name == "jitter" else 6 if name == "time_mask" else 4]))
    monkeypatch.setattr(torch, "randperm", lambda n, **k: torch.tensor(order))
    out = aug.forward("random", tx)
    for m, x in tx["shake"].items():
        n = x.shape[-1]
        std = aug._derived["jitter"][("shake", m)]["std"] if name == "jitter" else 0.0
        kw = {"jitter": dict(noise=restated_noise(key, 0, x.shape) * std), "channel_shuffle": dict(chan=order),
              "time_mask": dict(time_mask=(6, min(9, n) - 6)), "freq_mask": dict(freq_mask=(4, 3))}[name]
        got = out["shake"][m]
        ref = restate(x.cpu(), **kw)
        assert got.shape == (2, 6, 10, n) and (got.cpu().double() - ref).abs().max().item() < bound(n, 1.0, std), (name, m)
        assert not torch.equal(got, ops.fft_realpack(x))
