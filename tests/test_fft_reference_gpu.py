"""The three DFT kernels of focal_amd/csrc/fft.hip (generic four-step, MFMA N x N, short rows), plain and extended, against float64 at every
length and grid regime they accept (tests/fft_reference.py: CASES).  Every row of every case must satisfy

    row_error <= max(4 * E_plain, 8 * 2^-23)

where E_plain is the error a plain fp32 matrix DFT makes on the same rows (computed here, on the first min(rows, 64) augmented rows).
Each call runs inside a launch trace and must have launched the kernel family and grid the case was written for; the output tensor is
handed in full of NaN, so a bin no workgroup wrote fails.  Two figures are recorded per case: fft.<case>, the worst row_error / E_plain
over the normal and the offset rows (E_plain no smaller than the floor's 2 * 2^-23, so that 4.0 is the bound at every length), and
fft.<case>.impulse_eps, the worst row_error of the impulse rows in units of 2^-23 (the floor is 8)."""
import ctypes as C

import pytest
import torch

import fft_reference as fr
from conftest import record_observed

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from focal_amd import ops as o
    return o


def traced(fn, capacity=16):
    """fn() inside a dispatch trace -> [((family, extended), grid)] of the library launches it made, in order."""
    from focal_amd import _lib
    lib = _lib.load()
    torch.cuda.synchronize()
    _lib.check(lib.focal_trace_begin(capacity, _lib.TRACE_DISPATCH))
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        lib.focal_trace_end()
    cnt = lib.focal_trace_count()
    recs = (_lib.TraceRecord * max(cnt, 1))()
    _lib.check(lib.focal_trace_read(0, cnt, recs))
    out = []
    for r in recs[:cnt]:
        assert tuple(r.block) == (256, 1, 1) and tuple(r.grid)[1:] == (1, 1), r.kernel
        out.append((fr.kernel_family(r.kernel.decode()), int(r.grid[0])))
    return out


def call_abi(ops, x, n1, n2, out, scale=1.0, flip=False, perm=None, phase=0.0):
    """focal_fft_realpack_fwd / focal_augment_fft_fwd with the factorisation named in the descriptor."""
    from focal_amd import _lib
    d, a, x, tw, out = ops._fft_problem(x, scale, flip, perm, phase, out)
    d.n1, d.n2 = n1, n2
    lib = _lib.load()
    if a is None:
        _lib.check(lib.focal_fft_realpack_fwd(C.byref(d), ops._p(x), ops._p(tw), ops._p(out), ops._stream()))
    else:
        _lib.check(lib.focal_augment_fft_fwd(C.byref(d), C.byref(a), ops._p(x), ops._p(tw), ops._p(out), ops._stream()))
    return out


def case_augs(case):
    if case.path == "ex":
        from test_augment_ex_gpu import cases_for
        return {"composed": cases_for(case.shape)["composed"]}
    return {name: fr.aug_kwargs(name, case.shape) for name in case.augs}


def run_case(ops, case, x, out, aug):
    if case.path == "abi":
        call_abi(ops, x, *case.n1n2, out, **aug)
    elif case.path == "multi":
        got = ops.fft_realpack_multi([dict(x=x, out=out, **aug)])[0]
        assert got.data_ptr() == out.data_ptr()
    else:
        assert ops.fft_realpack(x, out=out, **aug).data_ptr() == out.data_ptr()


def measure(out, x, aug):
    """(row errors [rows], E_plain) of one result against float64."""
    xa = fr.augmented_fp64(x, **aug)
    return fr.row_error(out, fr.packed_fp64(x, **aug), xa), fr.e_plain(xa)


@pytest.mark.parametrize("case", fr.CASES, ids=fr.CASE_IDS)
def test_kernel_meets_the_fp32_bound(ops, case):
    B, Cc, I, n = case.shape
    rows = B * Cc * I
    want = [((case.form, case.path == "ex"), case.grid)]
    assert (case.form, case.grid) == fr.expected_launch(n, *case.n1n2, rows, case.path in ("multi", "ex"))
    worst, failures = {"ratio": 0.0, "impulse_eps": 0.0}, []
    for kind in fr.INPUTS:
        x_cpu = fr.make_input(kind, case.shape, seed=1000 + n)
        x = x_cpu.to(DEV)
        for name, aug in case_augs(case).items():
            out = torch.full((B, 2 * Cc, I, n), float("nan"), device=DEV)
            launched = traced(lambda: run_case(ops, case, x, out, aug))
            assert launched == want, (case.id, kind, name, launched, want)
            err, E = measure(out, x_cpu, aug)
            lim = fr.bound(E)
            ratio = err.max() / max(E, fr.FLOOR / fr.MARGIN)
            key, fig = ("impulse_eps", err.max() / fr.EPS) if kind == "impulse" else ("ratio", ratio)
            worst[key] = fig if not fig <= worst[key] else worst[key]          # (a NaN sticks)
            print(f"{case.id} {kind} {name}: worst row error {err.max():.3e} ({err.max() / fr.EPS:.2f} eps) E_plain {E:.3e} bound {lim:.3e} "
                  f"-> {ratio:.2f} of 4; rows over the bound: {int((~(err <= lim)).sum())} of {rows}")
            if not (err <= lim).all():
                failures.append((kind, name, float(err.max()), lim))
    record_observed(f"fft.{case.id}", worst["ratio"])
    record_observed(f"fft.{case.id}.impulse_eps", worst["impulse_eps"])
    assert not failures, (case.id, failures)


def test_mixed_multi_call(ops):
    """One call holding nine short problems, one 576 and one 2304: the short ones flush at eight, the long rows are launched where they
    stand, one short problem is left for the final flush.  Every output against float64 (not against single calls)."""
    kinds = [fr.INPUTS[i % 3] for i in range(len(fr.MIXED_SHAPES))]
    xs = [fr.make_input(k, s, seed=77 + i) for i, (k, s) in enumerate(zip(kinds, fr.MIXED_SHAPES))]
    augs = [fr.aug_kwargs("composed" if i % 2 else "identity", s) for i, s in enumerate(fr.MIXED_SHAPES)]
    outs = [torch.full((s[0], 2 * s[1], s[2], s[3]), float("nan"), device=DEV) for s in fr.MIXED_SHAPES]
    items = [dict(x=x.to(DEV), out=o, **a) for x, o, a in zip(xs, outs, augs)]
    launched = traced(lambda: ops.fft_realpack_multi(items))
    want = [((fam, False), grid) for fam, grid in fr.expected_mixed_launches(fr.MIXED_SHAPES)]
    assert [f for (f, _), _ in want] == ["mfma24", "small", "mfma48", "small"]
    assert launched == want, (launched, want)
    worst, failures = 0.0, []
    for s, k, x, o, a in zip(fr.MIXED_SHAPES, kinds, xs, outs, augs):
        err, E = measure(o, x, a)
        ratio = err.max() / max(E, fr.FLOOR / fr.MARGIN)
        worst = ratio if not ratio <= worst else worst
        print(f"mixed {s} {k} {'composed' if a else 'identity'}: worst row error {err.max():.3e} E_plain {E:.3e} -> {ratio:.2f} of 4")
        if not (err <= fr.bound(E)).all():
            failures.append((s, k, float(err.max()), fr.bound(E)))
    record_observed("fft.mixed-multi-call", worst)
    assert not failures, failures


def refused(fn, text):
    """fn() must raise FocalHipError from the argument check (FOCAL_EINVAL, the named message), with no launch recorded."""
    from focal_amd import _lib
    lib = _lib.load()
    torch.cuda.synchronize()
    _lib.check(lib.focal_trace_begin(4, _lib.TRACE_DISPATCH))
    try:
        with pytest.raises(_lib.FocalHipError) as e:
            fn()
    finally:
        lib.focal_trace_end()
    assert lib.focal_trace_count() == 0
    assert "error -1:" in str(e.value) and text in str(e.value), str(e.value)


def test_refusals_launch_nothing(ops):
    from focal_amd import _lib
    lib = _lib.load()
    # one past the largest accepted length (3277 = 29 x 113)
    assert not fr.accepted(3277)
    x = fr.make_input("normal", (1, 1, 2, 3277), seed=1).to(DEV)
    out = torch.full((1, 2, 2, 3277), float("nan"), device=DEV)
    refused(lambda: ops.fft_realpack(x, out=out), "too long")
    refused(lambda: ops.fft_realpack_multi([dict(x=x, out=out)]), "too long")
    assert torch.isnan(out).all()
    # a descriptor whose factors do not give n
    x = fr.make_input("normal", (1, 1, 2, 96), seed=2).to(DEV)
    out = torch.full((1, 2, 2, 96), float("nan"), device=DEV)
    refused(lambda: call_abi(ops, x, 12, 9, out), "n1*n2 != n")
    refused(lambda: call_abi(ops, x, 96, 0, out), "n1*n2 != n")
    assert torch.isnan(out).all()
    # a permutation over 33 intervals: one more than the table holds (ops cannot even spell it: the descriptor by hand)
    x = fr.make_input("normal", (1, 1, 33, 96), seed=3).to(DEV)
    out = torch.full((1, 2, 33, 96), float("nan"), device=DEV)
    d, _, _, tw, _ = ops._fft_problem(x, out=out)
    a = _lib.AugDesc()
    a.scale, a.use_perm, a.phase_cos = 1.0, 1, 1.0
    for i in range(32):
        a.perm[i] = i
    refused(lambda: _lib.check(lib.focal_augment_fft_fwd(C.byref(d), C.byref(a), ops._p(x), ops._p(tw), ops._p(out), ops._stream())),
            "exceed the permutation table")
    assert torch.isnan(out).all()
    a.use_perm = 0                     # the same 33 intervals without a permutation are fine
    assert traced(lambda: _lib.check(lib.focal_augment_fft_fwd(C.byref(d), C.byref(a), ops._p(x), ops._p(tw), ops._p(out), ops._stream()))) \
        == [(("generic", False), 33)]
    err, E = measure(out, x.cpu(), {})
    assert (err <= fr.bound(E)).all()
