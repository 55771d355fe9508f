"""The view path after the fold to one pool struct, one draw export and one transform entry point (ABI 14): byte equality with what the
parent commit wrote (tests/golden/view_fold_parent.json, recorded there by tests/golden/gen_view_fold_parent.py), the library's own choice
between the plain and the extended kernel instantiations, and the refusal of an extended kind without an extras array."""
import ctypes as C
import hashlib
import json
import os

import pytest
import torch

from test_augment_ex_cpu import ALL_FREQ, ALL_TIME
from test_augment_ex_gpu import DEV, FOCAL_POOL, STREAM, cases_for, rnd

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "view_fold_parent.json")
# the small-row kernel; the MFMA kernel (16 x 16); the MFMA kernel at 40 x 40 with the raised LDS grant
FFT_SHAPES = [(2, 3, 10, 20), (2, 2, 10, 256), (2, 1, 10, 1600)]
N_SEEDS = 20


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def full_pool(ops):
    """The reference's eleven-entry pool over two slots (test_augment_ex_gpu.py builds the same one over eight)."""
    return ops.view_pool([(n, 0.5) for n in ALL_TIME + ALL_FREQ], [10, 10], jitter_std=[0.05, 0.1], channels=[3, 6], time_mask=[(3, 10)] * 2,
                         freq_mask=[(6, 20), (480, 1600)])


def fold_digests(ops):
    """SHA-256 of the raw bytes the view path writes, through Python signatures that are the same before and after the fold."""
    d = {}
    seed = ops.new_rng_state(1, DEV)
    shipped = ops.view_pool(FOCAL_POOL, [10, 10])
    plans = ops.new_view_plans(2, 2, DEV)
    for i in range(N_SEEDS):
        seed[0] = 104729 * i + 7
        ops.view_draw(shipped, 2, 2, seed, STREAM, plans)
        d[f"draw.shipped.{i}"] = sha(plans)
    state = ops.new_rng_state(4242, DEV)
    for i in range(N_SEEDS):
        ops.view_draw_shared(shipped, 2, 2, state, STREAM, plans)
        d[f"draw_shared.shipped.{i}"] = sha(plans)
    d["draw_shared.shipped.state"] = sha(state)
    full, extras = full_pool(ops), ops.new_view_extras(2, 2, DEV)
    for i in range(N_SEEDS):
        seed[0] = 104729 * i + 7
        extras.fill_(0xFF)
        ops.view_draw(full, 2, 2, seed, STREAM, plans, extras=extras)
        d[f"draw.full.plans.{i}"], d[f"draw.full.extras.{i}"] = sha(plans), sha(extras)
    for shape in FFT_SHAPES:
        x = rnd(*shape, seed=sum(shape))
        kw = cases_for(shape)["composed"]
        forced = {k: kw[k] for k in ("scale", "flip", "perm", "phase")}
        one, ex = ops.new_view_plans(1, 1, DEV), ops.new_view_extras(1, 1, DEV)
        ops.write_view_plan(one, 0, **forced)
        ops.write_view_extra(ex, 0, jitter=kw["jitter"], chan=kw["chan"], time_mask=kw["time_mask"], freq_mask=kw["freq_mask"], like=x)
        tag = "x".join(str(v) for v in shape)
        d[f"fft.{tag}.plain"] = sha(ops.fft_realpack_multi([dict(x=x)])[0])
        d[f"fft.{tag}.plan"] = sha(ops.fft_realpack_multi([dict(x=x, plan=one[0], x_warped=x)])[0])
        d[f"fft.{tag}.extra"] = sha(ops.fft_realpack_multi([dict(x=x, plan=one[0], x_warped=x, extra=ex[0], noise_salt=kw["noise_salt"])])[0])
    return d


@pytest.fixture(scope="module")
def ops():
    from focal_amd import ops as o
    return o


def traced(fn):
    """The kernel names (mangled: one per template instantiation) of the library launches fn() makes."""
    from focal_amd import _lib
    lib = _lib.load()
    torch.cuda.synchronize()
    _lib.check(lib.focal_trace_begin(64, _lib.TRACE_DISPATCH))
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        lib.focal_trace_end()
    n = lib.focal_trace_count()
    recs = (_lib.TraceRecord * max(n, 1))()
    _lib.check(lib.focal_trace_read(0, n, recs))
    return [recs[i].kernel.decode() for i in range(n)]


def test_the_fold_writes_the_parents_bytes(ops):
    """Plans, extras, view-state words and spectra against the digests recorded at the parent commit.  No kernel here has an atomic, so
    equality is the expectation, not a tolerance."""
    want = json.load(open(FIXTURE))
    assert len(want["commit"]) == 40
    got = fold_digests(ops)
    assert set(got) == set(want["sha256"]) and len(got) == 4 * N_SEEDS + 1 + 3 * len(FFT_SHAPES)
    diff = sorted(k for k in got if got[k] != want["sha256"][k])
    assert not diff, diff


def test_the_library_picks_the_plain_kernels_itself(ops):
    """The extended instantiations run if and only if a problem carries an extra (host or device record); noise_salt alone does not ask
    for them.  No kernel is named: the names only have to agree or differ."""
    xs = [rnd(2, 3, 10, 20, seed=1), rnd(2, 2, 10, 256, seed=2)]
    plain = traced(lambda: ops.fft_realpack_multi([dict(x=x) for x in xs]))
    salted = traced(lambda: ops.fft_realpack_multi([dict(x=x, noise_salt=5) for x in xs]))
    masked = traced(lambda: ops.fft_realpack_multi([dict(x=x, time_mask=(1, 2)) for x in xs]))
    assert len(plain) == 2 and salted == plain
    assert len(masked) == 2 and all(a != b for a, b in zip(masked, plain))
    rec = ops.new_view_extras(1, 1, DEV)
    on_device = traced(lambda: ops.fft_realpack_multi([dict(x=x, extra=rec[0]) for x in xs]))
    assert on_device == masked
    pool, seed, plans = ops.view_pool(FOCAL_POOL, [10, 10]), ops.new_rng_state(1, DEV), ops.new_view_plans(2, 2, DEV)
    without = traced(lambda: ops.view_draw(pool, 2, 2, seed, STREAM, plans))
    extras = ops.new_view_extras(2, 2, DEV)
    with_extras = traced(lambda: ops.view_draw(pool, 2, 2, seed, STREAM, plans, extras=extras))
    assert len(without) == 1 and len(with_extras) == 1 and without != with_extras


def test_an_extended_kind_without_extras_is_refused(ops):
    """Nothing is launched: ops refuses first, and so does the export when called with a NULL extras array."""
    from focal_amd import _lib
    pool = ops.view_pool([("negation", 0.5), ("jitter", 0.5)], [10, 10], jitter_std=[0.1, 0.2])
    seed, plans = ops.new_rng_state(1, DEV), ops.new_view_plans(2, 2, DEV)
    state = ops.new_rng_state(2, DEV)
    with pytest.raises(ValueError):
        ops.view_draw(pool, 2, 2, seed, STREAM, plans)
    with pytest.raises(ValueError):
        ops.view_draw_shared(pool, 2, 2, state, STREAM, plans)
    lib = _lib.load()
    for advance, words in ((0, seed), (1, state)):
        before = words.clone()
        names = []

        def raw():
            names.append(lib.focal_view_draw(C.byref(pool), 2, 2, words.data_ptr(), advance, STREAM, plans.data_ptr(), None, None))
        launched = traced(raw)
        assert names == [-1] and b"view_draw:" in lib.focal_last_error() and launched == []
        assert torch.equal(words, before) and int(plans.max().item()) == 0
