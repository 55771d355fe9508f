"""The yardstick of the DFT kernel tests, checked without a GPU: the bound of tests/fft_reference.py is attainable by a correct fp32
implementation of the four-step algorithm at every (n, n1, n2) and input of the table, the restated dispatch agrees with ops._factor and
with what the table says each case is for, and the error metric behaves as the GPU tests rely on."""
import numpy as np
import pytest
import torch

import fft_reference as fr

FACTORISATIONS = sorted({(c.shape[-1],) + c.n1n2 for c in fr.CASES} | {(s[-1],) + fr.factor(s[-1]) for s in fr.MIXED_SHAPES})
ROWS = 12


@pytest.mark.parametrize("n,n1,n2", FACTORISATIONS, ids=[f"{n}={a}x{b}" for n, a, b in FACTORISATIONS])
def test_four_step_fp32_meets_the_bound(n, n1, n2):
    """An fp32 restatement of fft.hip's header comment against float64, inputs (a) to (c), identity and the composed augmentation: every
    row within max(4 E_plain, 8 * 2^-23).  (The rotation is applied in fp32 as the kernels apply it: the fourth rounding stage.)"""
    shape = (1, 2, ROWS // 2, n)
    for kind in fr.INPUTS:
        x = fr.make_input(kind, shape, seed=n)
        for name in fr.BOTH:
            aug = fr.aug_kwargs(name, shape)
            xa = fr.augmented_fp64(x, **aug)
            ref = fr.packed_fp64(x, **aug)
            re, im = fr.four_step_fp32(xa.numpy().reshape(-1, n).astype(np.float32), n1, n2)
            pc, ps = np.float32(np.cos(aug.get("phase", 0.0))), np.float32(np.sin(aug.get("phase", 0.0)))
            re, im = re * pc - im * ps, re * ps + im * pc
            assert re.dtype == np.float32
            got = torch.from_numpy(np.stack([re.reshape(1, 2, ROWS // 2, n), im.reshape(1, 2, ROWS // 2, n)], axis=2).reshape(1, 4, ROWS // 2, n))
            E = fr.e_plain(xa)
            err = fr.row_error(got, ref, xa)
            print(f"n {n} = {n1} x {n2} {kind} {name}: worst row error {err.max():.3e} = {err.max() / max(E, 1e-300):.2f} E_plain "
                  f"({err.max() / fr.EPS:.2f} eps); E_plain {E:.3e}")
            assert (err <= fr.bound(E)).all(), (kind, name, err.max(), E)


@pytest.mark.parametrize("n,n1,n2", [(1600, 40, 40), (3276, 63, 52)])
def test_a_table_made_from_fp32_angles_fails_the_bound(n, n1, n2):
    """What the bound is for: the same algorithm with a twiddle table whose ANGLES were formed in fp32 (entries off by up to ~1e-6) stays
    more than 100 times inside 2e-4 sqrt(n) on unit-normal rows, and exceeds this bound on the impulse rows."""
    ang = np.float32(2 * np.pi) * np.arange(n, dtype=np.float32) / np.float32(n)
    table = np.cos(ang.astype(np.float64)).astype(np.float32), (-np.sin(ang.astype(np.float64))).astype(np.float32)
    shape = (1, 2, 6, n)
    figures = {}
    for kind in ("normal", "impulse"):
        x = fr.make_input(kind, shape, seed=n)
        xa, ref = fr.augmented_fp64(x), fr.packed_fp64(x)
        re, im = fr.four_step_fp32(xa.numpy().reshape(-1, n).astype(np.float32), n1, n2, table=table)
        got = torch.from_numpy(np.stack([re.reshape(1, 2, 6, n), im.reshape(1, 2, 6, n)], axis=2).reshape(1, 4, 6, n))
        figures[kind] = (got.double() - ref).abs().max().item(), fr.row_error(got, ref, xa).max(), fr.bound(fr.e_plain(xa))
    assert figures["normal"][0] < 2e-4 * np.sqrt(n) / 100
    assert figures["impulse"][1] > figures["impulse"][2], figures


def test_expected_launch_agrees_with_the_default_factorisation_and_the_table():
    from focal_amd import ops
    for n in list(range(1, 130)) + [256, 360, 576, 1024, 1600, 2304, 3276, 3277]:
        assert fr.factor(n) == ops._factor(n), n
    assert fr.accepted(3276) and not fr.accepted(3277) and fr.factor(3276) == (63, 52) and fr.factor(97) == (97, 1)
    for c in fr.CASES:
        B, C, I, n = c.shape
        assert c.n1n2[0] * c.n1n2[1] == n and fr.accepted(n), c.id
        if c.path != "abi":
            assert c.n1n2 == ops._factor(n), c.id
        assert fr.expected_launch(n, *c.n1n2, B * C * I, c.path in ("multi", "ex")) == (c.form, c.grid), c.id
        assert fr.case_passes(c) == c.passes, c.id
        assert B * 2 * C * I * n * 4 <= 27 * 2 ** 20, c.id          # the largest tensor of the table: 26 MB
    # every form, every MFMA side, and each form's second pass, are in the table
    forms = {c.form for c in fr.CASES}
    assert forms == {"generic", "small"} | {f"mfma{s}" for s in fr.MFMA_SIDES}
    assert {c.form[:4] for c in fr.CASES if c.passes > 1} == {"gene", "smal", "mfma"}
    # the same length goes three ways: by the call, and by the parity of the row count
    assert fr.expected_launch(64, 64, 1, 150, True)[0] == "small" and fr.expected_launch(64, 64, 1, 150, False)[0] == "generic"
    assert fr.expected_launch(64, 8, 8, 150, True) == ("mfma8", 75) and fr.expected_launch(1600, 40, 40, 3, False) == ("generic", 3)
    assert fr.expected_launch(65, 65, 1, 150, True)[0] == "generic"
    # the mixed call: nine short problems flush at eight, the long rows go out where they stand
    got = fr.expected_mixed_launches(fr.MIXED_SHAPES)
    assert [f for f, _ in got] == ["mfma24", "small", "mfma48", "small"] and got[0][1] == 30 and got[2][1] == 30 and got[3][1] == 2
    assert sum(1 for s in fr.MIXED_SHAPES if s[-1] <= 64) == 9


def test_kernel_family_reads_both_spellings():
    assert fr.kernel_family("_Z24fft_realpack_mfma_kernelILi48ELi48ELb1EEvPKfS1_Pf14focal_fft_desci6AugArgIXT1_EE") == ("mfma48", True)
    assert fr.kernel_family("void fft_realpack_mfma_kernel<16, 16, false>(float const*, float const*)") == ("mfma16", False)
    assert fr.kernel_family("_Z19fft_realpack_kernelILb0EEvPKfS1_Pf14focal_fft_desci6AugArgIXT_EE") == ("generic", False)
    assert fr.kernel_family("void fft_small_multi_kernel<true>(FftSmallTable<true>)") == ("small", True)
    assert fr.kernel_family("_Z15adamw_kernelPf") is None


def test_row_error_is_scale_invariant_and_flags_one_bin():
    shape = (2, 3, 4, 40)
    x = fr.make_input("offset", shape, seed=1)
    ref, xa = fr.packed_fp64(x), fr.augmented_fp64(x)
    got = ref.float()
    e1 = fr.row_error(got, ref, xa)
    assert e1.shape == (24,) and 0 < e1.max() < 2 * fr.EPS          # one rounding of each bin, |X_k| <= sqrt(n) ||x||
    x3 = 3 * x.double()                                             # (in float64: 3x and 3 * got are then the same data, scaled)
    e3 = fr.row_error(3 * got.double(), fr.packed_fp64(x3), fr.augmented_fp64(x3))
    assert np.allclose(e1, e3, rtol=1e-6, atol=0)                   # x -> 3x: unchanged
    # one wrong bin, in the Im half of row (b, c, i) = (1, 2, 3): that row alone is flagged, by exactly the size of the fault
    bad = got.clone()
    bad[1, 2 * 2 + 1, 3, 17] += 1e-2
    eb = fr.row_error(bad, ref, xa)
    r = (1 * 3 + 2) * 4 + 3
    norm = xa.reshape(-1, 40)[r].norm().item()
    assert abs(eb[r] - 1e-2 / norm) < 1e-5 / norm and np.array_equal(np.delete(eb, r), np.delete(e1, r))
    assert eb[r] > fr.bound(fr.e_plain(xa))
    # an unwritten (NaN) bin passes no bound; an all-zero row must be exactly zero
    bad = got.clone()
    bad[0, 0, 0, 5] = float("nan")
    assert not (fr.row_error(bad, ref, xa) <= 1e30).all()
    z = torch.zeros(1, 1, 2, 8)
    z[0, 0, 1, 3] = 1.0
    rz, za = fr.packed_fp64(z), fr.augmented_fp64(z)
    assert fr.row_error(rz.float(), rz, za)[0] == 0.0
    dirty = rz.float()
    dirty[0, 1, 0, 2] = 1e-30
    assert fr.row_error(dirty, rz, za)[0] == np.inf


def test_plain_dft_is_a_dft():
    """The yardstick against numpy's float64 transform, and its table against the definition."""
    x = fr.make_input("normal", (1, 1, 6, 97), seed=2).reshape(6, 97).numpy()
    re, im = fr.plain_fp32_dft(x)
    f = np.fft.fft(x.astype(np.float64), axis=-1)
    assert re.dtype == np.float32 and np.abs(re - f.real).max() < 1e-4 and np.abs(im - f.imag).max() < 1e-4
    imp = fr.make_input("impulse", (1, 1, 6, 97), seed=0)
    assert fr.e_plain(fr.augmented_fp64(imp)) < fr.EPS            # an impulse: one table entry per bin, rounded once
