"""Host restatement of focal_mixup_draw / focal_mixup_multi from the formulas include/focal_hip.h states (numpy, uint32 / float32
arithmetic as the kernel's), shared by test_classifier_step_cpu.py and test_classifier_step_gpu.py.  Only the alpha == 1 branch of lambda
is restated bit for bit (one uniform draw); the Gamma branch is held to Beta(a, a)'s moments instead."""
import numpy as np

GOLDEN, STEP, MIX_TAG, PERM_TAG = 0x9E3779B9, 0x85EBCA6B, 0x4D495855, 0x5045524D
M32 = 0xFFFFFFFF


def mix32(x):
    x = int(x) & M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def mix32_array(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x.astype(np.uint32)


def next_seed(seed):
    """The state word after one advancing draw."""
    return mix32(seed + GOLDEN)


def uniform(km, i):
    return np.float32(mix32(km + i * STEP) >> 8) * np.float32(1.0 / 16777216.0)


def draw(seed, stream_id, cfg, B, slots):
    """-> dict(apply, cut, lam (np.float32), boxes [8][4], perm [B]) of the draw keyed by state word `seed` (alpha == 1 only)."""
    km = mix32(seed * GOLDEN + stream_id * STEP + MIX_TAG)
    apply = bool(uniform(km, 0) < np.float32(cfg["prob"]))
    ma, ca = np.float32(cfg["mixup_alpha"]), np.float32(cfg["cutmix_alpha"])
    cut, lam = False, np.float32(1.0)
    if apply:
        cut = bool(uniform(km, 1) < np.float32(cfg["switch_prob"])) if (ma > 0 and ca > 0) else bool(ca > 0)
        alpha = ca if cut else ma
        assert alpha == 1.0, "only the one-uniform branch is restated"
        lam = uniform(km, 2)
    boxes = [[0, 0, 0, 0] for _ in range(8)]
    if apply and cut:
        ratio = np.sqrt(np.float32(1.0) - lam, dtype=np.float32)
        for q, (I, S) in enumerate(slots):
            cut_h, cut_w = int(np.float32(I) * ratio), int(np.float32(S) * ratio)
            cy = min(int(uniform(km, 8 + 2 * q) * np.float32(I)), I - 1)
            cx = min(int(uniform(km, 9 + 2 * q) * np.float32(S)), S - 1)
            boxes[q] = [int(np.clip(cy - cut_h // 2, 0, I)), int(np.clip(cy + cut_h // 2, 0, I)),
                        int(np.clip(cx - cut_w // 2, 0, S)), int(np.clip(cx + cut_w // 2, 0, S))]
    kp = mix32(km ^ PERM_TAG)
    h = mix32_array(kp + np.arange(B, dtype=np.uint64) * STEP)
    # the rank of each hash, ties broken by index: a stable argsort's inverse
    order = np.argsort(h, kind="stable")
    perm = np.empty(B, dtype=np.int64)
    perm[order] = np.arange(B)
    return dict(apply=int(apply), cut=int(cut), lam=lam, boxes=boxes, perm=perm)


def mix(x, perm, apply, cut, lam, box):
    """focal_mixup_multi on one [B, C, I, S] float32 array, with the clamps the kernel applies to a device record."""
    if not apply:
        return x.copy()
    B, _, I, S = x.shape
    perm = np.clip(np.asarray(perm), 0, B - 1)
    o = x[perm]
    if not cut:
        lam = np.float32(lam)
        return lam * x + (np.float32(1.0) - lam) * o
    yl, yh = (int(np.clip(v, 0, I)) for v in box[:2])
    xl, xh = (int(np.clip(v, 0, S)) for v in box[2:])
    y = x.copy()
    y[:, :, yl:yh, xl:xh] = o[:, :, yl:yh, xl:xh]
    return y


def beta_moment_bounds(alpha, n, k=5.0):
    """(|mean - 1/2| bound, variance, |sample variance - variance| bound) for n draws of Beta(alpha, alpha), k standard errors, from the
    distribution's own moments: variance 1 / (4 (2 alpha + 1)), kurtosis 3 - 6 / (2 alpha + 3)."""
    var = 1.0 / (4.0 * (2.0 * alpha + 1.0))
    kurt = 3.0 - 6.0 / (2.0 * alpha + 3.0)
    return k * np.sqrt(var / n), var, k * np.sqrt((kurt - 1.0) * var * var / n)
