/* libfocal_hip -- C ABI of the MI355X (gfx950) FOCAL pretraining hot path.
 *
 * The reference (tomoyoshki/focal) is pure PyTorch and has no FFI of its own; its boundary for this path is the
 * Python plugin surface (`src/train_utils/model_selection.py:14-59`, the modules under `src/models/`).  This library sits
 * *underneath* that surface: the modules under `focal_amd/src/models/` keep the reference's classes / state-dict names and calls
 * the entry points below through ctypes, one per ATen operator group the reference step executes
 * (the reference site each entry replaces is cited on the declaration).
 *
 * Conventions (all entry points):
 *   - plain C: pointers + sizes, no torch / C++ types;
 *   - every tensor pointer is a CALLER-OWNED DEVICE pointer, row-major contiguous unless a leading dimension is
 *     given; descriptor structs and pointer *arrays* live on the host;
 *   - work is enqueued asynchronously on `stream` (a hipStream_t passed as void*); nothing allocates, frees or
 *     synchronises, so every call is hipGraph-capturable;
 *   - returns FOCAL_OK (0) or a negative error code; `focal_last_error()` gives a thread-local message;
 *   - "dtype" is the storage type of activations and of the weight operand handed to the matrix cores:
 *     FOCAL_F32 (exact-fp32 MFMA, the 1e-3 parity mode) or FOCAL_BF16 (bf16 operands, fp32 accumulate).
 *     Residual streams, statistics, loss values, master weights, gradients and optimizer state are always fp32.
 */
#ifndef FOCAL_HIP_H
#define FOCAL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 14: one view pool (16 entries), one focal_view_draw, one focal_fft_problem that carries the extra; 7: launch trace (focal_trace_*), focal_adamw_multi_advance takes the step-state length; 2: BatchNorm scratch of 2C + 1 floats; 3: fused MLP, warps, Mixup; 4: row-sharded loss head, weight-gradient launch queries */
#define FOCAL_ABI_VERSION 14

enum { FOCAL_OK = 0, FOCAL_EINVAL = -1, FOCAL_EUNSUPPORTED = -2, FOCAL_EWORKSPACE = -3, FOCAL_EHIP = -4 };
enum { FOCAL_F32 = 0, FOCAL_BF16 = 1 };

int focal_abi_version(void);
/* diagnostics: the kernel template the GEMM-family entry points launched last on this thread ("" before the first one) */
const char* focal_last_kernel(void);
const char* focal_last_error(void);

/* ------------------------------------------------------------------------------------------------ launch trace (measurement only)
 * Per-kernel durations of eager steps for bench.py's in-step roofline.  Between focal_trace_begin and focal_trace_end
 * every kernel launch of the library is recorded: FOCAL_TRACE_DISPATCH attaches a start / stop event pair to the dispatch itself
 * (hipExtLaunchKernel: the duration is the dispatch's own begin -> end timestamps, as rocprofv3 --kernel-trace reports it),
 * FOCAL_TRACE_EVENTS records one event directly before and one directly behind the launch.  Launches onto a stream that is being
 * captured into a hipGraph are not recorded.  These calls own a pool of events and focal_trace_read synchronises on them: they are
 * the one exception to "nothing allocates or synchronises", and no product path calls them. */
enum { FOCAL_TRACE_DISPATCH = 1, FOCAL_TRACE_EVENTS = 2 };
typedef struct {
  char kernel[384];        /* symbol name of the launched kernel (mangled: one per template instantiation = one row of `rocprofv3 --stats -M`) */
  unsigned grid[3], block[3];
  void* stream;
  float us;                /* duration in microseconds */
} focal_trace_record;
int focal_trace_begin(int capacity, int mode); /* drops the records of an earlier trace, records up to `capacity` launches */
int focal_trace_end(void);
int focal_trace_count(void);
int focal_trace_read(int first, int n, focal_trace_record* out); /* waits for the launches; records stay until the next begin */

/* ------------------------------------------------------------------------------------------------ RNG state
 * Device-resident {seed, step} pair (uint32[4], two words used).  Dropout masks are pure functions of
 * (seed, stream id, element index): backward regenerates the forward mask, and a captured graph gets new masks
 * on every replay because `focal_rng_advance` bumps the words on the device.  Replaces torch's Philox stream
 * for nn.Dropout / DropPath (models/SwinModules.py:26,115,257; models/ConvModules.py:96). */
int focal_rng_advance(uint32_t* state, void* stream);
/* Diagnostic marker (round 6): slots[index] = the device wall clock (100 MHz ticks) at the moment a one-thread launch on `stream` runs.
 * Usable inside a captured hipGraph: the only way to time the BRANCHES of a replayed step (tools/phase_marks.py). */
int focal_mark(unsigned long long* slots, int index, void* stream);

typedef struct {
  const uint32_t* rng;   /* device RNG state or NULL (seed 0) */
  uint32_t stream_elem;  /* stream id of the element-wise dropout */
  float p_elem;          /* element-wise drop probability, 0 = off */
  uint32_t stream_path;  /* stream id of the per-sample stochastic depth (DropPath) */
  float p_path;          /* DropPath probability, 0 = off */
  int rows_per_sample;   /* rows of the [M, N] activation that belong to one sample */
} focal_drop_desc;

/* ------------------------------------------------------------------------------------------------ row 3: FFT
 * Augmenter.fft_preprocess (data_augmenter/Augmenter.py:141-158): full two-sided complex DFT of a real
 * [B, C, I, n] tensor along n, packed as [B, 2C, I, n] (channel 2c = Re, 2c+1 = Im).  n = n1 * n2 (four-step
 * DFT; n2 = 1 gives a direct DFT); `twiddle` is a device table of n {cos, -sin}(2 pi k / n) pairs. */
typedef struct { int B, C, I, n, n1, n2; } focal_fft_desc;
int focal_fft_realpack_fwd(const focal_fft_desc* d, const float* x, const float* twiddle, float* out, void* stream);
/* Same transform with one FOCAL view augmentation folded in (the data_augmenter package), applied to the whole
 * [B, C, I, n] tensor as the reference does per (location, modality):
 *   time domain, before the DFT:  x' = scale * x            NegationAugmenter.py:34 (scale = -1), ScalingAugmenter.py:35-36
 *                                 x'[i][s] = x[I-1-i][n-1-s]  HorizontalFlipAugmenter.py:34 (torch.flip dims 2, 3)
 *                                 x'[i] = x[perm[i]]          PermutationAugmenter.py:35-36 (one order for the whole batch)
 *   frequency domain, after it:   every bin times e^(i*angle)  PhaseShiftAugmenter.py:39-54
 * The reference applies exactly one of them per call; if several are set they compose as permute(flip(scale * x)), then the
 * rotation.  The random draws (coin flips, factor, order, angle) stay on the host, as in the reference. */
#define FOCAL_AUG_MAX_INTERVALS 32
typedef struct { float scale; int flip; int use_perm; int perm[FOCAL_AUG_MAX_INTERVALS]; float phase_cos, phase_sin; } focal_aug_desc;
int focal_augment_fft_fwd(const focal_fft_desc* d, const focal_aug_desc* a, const float* x, const float* twiddle, float* out,
                          void* stream);
typedef struct focal_view_plan focal_view_plan;
/* (focal_fft_realpack_multi, the call the product path makes, is declared behind the view records below: a problem carries one) */

/* ------------------------------------------------------------------------------------------------ views drawn on the device
 * The reference draws a view's augmentation in Python before every forward (data_augmenter/Augmenter.py:76-113 forward_random: ONE
 * augmenter of the pool per call, np.random.randint; each augmenter class then flips its coin per (location, modality), random() < p, and
 * draws its own parameters: ScalingAugmenter.py:35-36 N(1, std), PermutationAugmenter.py:35-36 torch.randperm(intervals),
 * PhaseShiftAugmenter.py:39-54 an angle in (-pi, pi), tsai's random-curve knots N(1, magnitude) for the two warps, ...).  focal_view_draw
 * makes exactly these draws on the device from a counter RNG keyed by (seed word, stream id, view, slot) and writes one focal_view_plan
 * and, when asked, one focal_view_extra per (view, slot); slot = a (location, modality) pair.  Nothing of a random view is left on the
 * host: the draw, the warp tables (focal_warp_plan_multi) and the transform (focal_fft_realpack_multi with `plan` / `extra_dev`) are
 * launches of fixed shape, so the whole view generation sits inside the captured step.
 *
 * Twelve kinds.  0 .. 7 travel in the plan: its focal_aug_desc (negation, scaling, horizontal flip, permutation, phase shift: what
 * focal_augment_fft_fwd applies) or its warp knots (magnitude warp, time warp).  8 .. 11 travel in the extra record, which is the identity
 * when zeroed:
 *   time domain   jitter           x' = x + N(0, 1) * std, i.i.d. per element                    JitterAugmenter.py:37-40
 *                 channel shuffle  x'[:, c] = x[:, chan[c]]: one order for the whole batch        ChannelShuffleAugmenter.py:34-37
 *                                  (packed spectrum: output pair (2c, 2c+1) = transform of source channel chan[c])
 *                 time mask        x'[..., tmask_lo : tmask_lo + tmask_n] = 0, in every interval   TimeMaskAugmenter.py:37-41
 *                                  (the reference draws interval-sized numbers and applies them to the SAMPLE axis; clipped at n)
 *   freq domain   freq mask        bins [fmask_lo, fmask_lo + fmask_n) of all 2C channels = 0     FreqMaskAugmenter.py:44-48
 * If several fields are set (the product sets one): mask_t(perm / flip / chan-select(scale * x) + noise), the DFT, the rotation, mask_f.
 *
 * The jitter noise is a pure function of (jitter_key, noise_salt, e), e = the flat index (mod 2^32) of the DESTINATION element in
 * [B, C, I, n]; elements 2p and 2p + 1 share one Box-Muller pair.  With mix32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15;
 * x *= 0x846ca68b; x ^= x >> 16 (uint32 arithmetic):
 *   k  = mix32(jitter_key ^ mix32(noise_salt * 0x9E3779B9 + 0x85EBCA6B))
 *   u1 = 1 - (mix32(k + (2p) * 0x85EBCA6B) >> 8) / 2^24          in (0, 1]
 *   u2 =     (mix32(k + (2p + 1) * 0x85EBCA6B) >> 8) / 2^24      in [0, 1)
 *   z[2p] = sqrt(-2 ln u1) cos(2 pi u2),  z[2p + 1] = sqrt(-2 ln u1) sin(2 pi u2),  x'[e] += jitter_std * z[e]      (fp32)
 * Under data parallelism every rank draws the same key (focal_view_draw with advance = 1); noise_salt = the rank gives the samples of the
 * global batch independent noise, as the reference's one torch.randn over the batch does. */
#define FOCAL_VIEW_MAX_KNOTS 16
#define FOCAL_VIEW_MAX_POOL 16
#define FOCAL_VIEW_MAX_SLOTS 8
#define FOCAL_VIEW_MAX_CHANNELS 16
enum { FOCAL_VIEW_NONE = 0, FOCAL_VIEW_NEGATION = 1, FOCAL_VIEW_SCALING = 2, FOCAL_VIEW_HFLIP = 3, FOCAL_VIEW_PERMUTATION = 4,
       FOCAL_VIEW_PHASE_SHIFT = 5, FOCAL_VIEW_MAG_WARP = 6, FOCAL_VIEW_TIME_WARP = 7, FOCAL_VIEW_JITTER = 8,
       FOCAL_VIEW_CHANNEL_SHUFFLE = 9, FOCAL_VIEW_TIME_MASK = 10, FOCAL_VIEW_FREQ_MASK = 11 };
struct focal_view_plan {
  focal_aug_desc aug;                  /* what the transform applies: the identity when the coin flip missed */
  int kind;                            /* the augmenter drawn for this (view, slot): FOCAL_VIEW_*, 0 = the coin flip missed */
  int pool_index;                      /* which pool entry the view drew (the same for all its slots) */
  int warp;                            /* 0, FOCAL_VIEW_MAG_WARP or FOCAL_VIEW_TIME_WARP: the transform reads the warped copy */
  int nknots;                          /* 3 (ord - 1) + 1 */
  float knots[FOCAL_VIEW_MAX_KNOTS];   /* the warp's random-curve ordinates */
};
typedef struct {
  float jitter_std;                       /* 0 = no noise */
  uint32_t jitter_key;
  int use_chan; int chan[FOCAL_VIEW_MAX_CHANNELS]; /* source channel of output channel c (a permutation of range(C)) */
  int tmask_lo, tmask_n;                  /* samples [lo, lo + n) of every row zeroed before the DFT; n = 0: none */
  int fmask_lo, fmask_n;                  /* bins [lo, lo + n) of every output row zeroed; n = 0: none */
} focal_view_extra;
typedef struct {
  int n_aug;                                                   /* pool size: one entry is drawn per view, uniformly */
  int kind[FOCAL_VIEW_MAX_POOL]; float prob[FOCAL_VIEW_MAX_POOL]; /* FOCAL_VIEW_* and the per-slot coin of each entry */
  float scaling_std, mag_magnitude, time_magnitude;
  int mag_order, time_order;                                   /* spline `ord` of the warps (tsai defaults 4 / 6) */
  int intervals[FOCAL_VIEW_MAX_SLOTS];                         /* per slot: the interval count the permutation shuffles */
  float jitter_std[FOCAL_VIEW_MAX_SLOTS];  /* value_range[mod] / 100 * std_in_percent */
  int channels[FOCAL_VIEW_MAX_SLOTS];      /* C of the slot's tensor, <= FOCAL_VIEW_MAX_CHANNELS */
  int tmask_d[FOCAL_VIEW_MAX_SLOTS], tmask_i[FOCAL_VIEW_MAX_SLOTS]; /* D = floor(num_segments * mask_ratio); I = x.shape[2] */
  int fmask_w[FOCAL_VIEW_MAX_SLOTS], fmask_n[FOCAL_VIEW_MAX_SLOTS]; /* W = floor(spectrum_len * mask_ratio); n = row length */
} focal_view_pool;
/* plans, extras: device [n_views][n_slots]; stream_id separates this draw from the dropout streams.
 *   advance = 0: `state` is the device seed word (the one the optimizer advances every step), read only; NULL = 0.
 *   advance = 1: `state` = 4 device words {seed, draw count, 0, 0} of the draw's own that the kernel advances after drawing
 *     (seed <- mix32(seed + golden), count += 1), so consecutive calls -- consecutive replays of a captured step -- draw different views
 *     without any other kernel touching the words.  Under data parallelism every rank holds a copy started from ONE broadcast seed: the
 *     ranks then draw identical plans, i.e. the global batch gets one augmenter / coin / permutation / scale / phase per view as the
 *     reference's batch does (Augmenter.py:76-113, ScalingAugmenter.py:35 size=(1,), PermutationAugmenter.py:35-36), while the dropout
 *     streams (keyed by the word the optimizer advances) stay per-rank.
 * extras may be NULL: no extra record is written, and a pool that names one of the kinds 8 .. 11 is refused (FOCAL_EINVAL).  The plan
 * bytes of a draw do not depend on whether extras are written; for a kind 0 .. 7 (and a missed coin) the extra is the identity.  The kinds
 * 8 .. 11 leave the plan's `aug` the identity and draw from indices of the (view, slot) key no other kind uses (those use 0 .. 39):
 *   jitter           jitter_key = raw draw 40, jitter_std = the slot's
 *   time mask        duration = 1 + floor(u41 * D), start = floor(u42 * (I - duration))     (randint(1, D), torch.randint(0, I - duration))
 *   freq mask        band = 1 + floor(u43 * W), start = floor(u44 * (n - band))
 *   channel shuffle  Fisher-Yates over the slot's C channels, step i (C - 1 .. 1) from draw 48 + i
 * Checked: pool of 1 .. 16; C <= 16; D >= 1 and I - D >= 1; W >= 2 and n - W >= 1 (for the slots in use, when the kind is pooled). */
int focal_view_draw(const focal_view_pool* pool, int n_views, int n_slots, uint32_t* state, int advance, uint32_t stream_id,
                    focal_view_plan* plans, focal_view_extra* extras, void* stream);
/* The warps of up to 8 (view, slot) pairs whose plans may ask for one, as TWO launches (the tables of all of them, then the passes over
 * their windows); a problem whose plan says "no warp" costs nothing and leaves its y unwritten.  Per problem: the random curve through the
 * plan's knots and, for the time warp, its cumulative positions (one workgroup per problem; focal_amd/warp.py is the host statement of the
 * same arithmetic), then x [rows][L] -> y with the 24 resampling weights of focal_warp_fwd's tables formed per position by the pass.  end_coef: device fp32 [47][4][48], the
 * not-a-knot basis splines of a 48-sample end window (focal_amd.warp.end_window_coefficients(), a constant of the method); tables:
 * device workspace of 2 L floats per problem (multipliers, or floor | fraction of the positions), 16-byte aligned. */
typedef struct { int rows, L; const float* x; const focal_view_plan* plan; float* tables; float* y; } focal_warp_problem;
int focal_warp_plan_multi(int n, const focal_warp_problem* problems, const float* end_coef, void* stream);

/* n transforms (each with or without an augmentation: the two views x the modalities of a step) in ONE call: problems with short rows
 * (n <= 64 samples as a direct DFT, n2 == 1: the 20-sample sensor modalities) share one launch -- a thread per output bin, 256 / n
 * rows per workgroup pass, a problem table in the kernel arguments, up to 8 problems per launch -- the others are launched as by
 * focal_fft_realpack_fwd / focal_augment_fft_fwd.  Results are those of the single calls.
 * plan non-NULL: the augmentation of this transform is read from that DEVICE record when the kernel runs (focal_view_draw fills it inside
 * the same captured step) instead of from `aug`; when the record says the view is warped, rows come from x_warped.
 * The extra of a problem: extra_dev non-NULL = a DEVICE record read when the kernel runs (as `plan` is), else the host `extra` when
 * has_extra, else none.  Host extras are checked (C <= 16 and chan a permutation of range(C) when use_chan; mask ranges inside [0, n];
 * std >= 0); a device record cannot be checked by the host, so the kernel clamps its values (channel entries to [0, C), mask ranges to
 * [0, n], a negative std to 0) and IGNORES use_chan on a tensor of more than 16 channels: the table has no order for them.
 * focal_view_draw never writes such a record (it refuses a pooled channel shuffle with C > 16); whoever writes records by hand for C > 16
 * gets jitter and the masks, not the shuffle.
 * The library chooses the kernels per call: if some problem has has_extra or a non-NULL extra_dev, every problem of the call runs the
 * kernels that resolve an extra, where a problem without one (or with the identity) takes one workgroup-uniform branch and computes
 * exactly what the plain kernels compute; otherwise -- noise_salt alone does not count -- the call runs the plain kernels, which have the
 * extended code compiled out. */
typedef struct { focal_fft_desc d; int has_aug; focal_aug_desc aug; const float* x; const float* twiddle; float* out;
                 const focal_view_plan* plan; const float* x_warped;
                 int has_extra; focal_view_extra extra; const focal_view_extra* extra_dev; uint32_t noise_salt; } focal_fft_problem;
int focal_fft_realpack_multi(int n, const focal_fft_problem* problems, void* stream);
#ifdef __cplusplus
static_assert(sizeof(focal_view_extra) == 92, "focal_view_extra");
static_assert(sizeof(focal_view_pool) == 376, "focal_view_pool");
static_assert(sizeof(focal_fft_problem) == 328, "focal_fft_problem");
#endif

/* TimeWarp / MagWarp (data_augmenter/TimeWarpAugmenter.py:18,44, MagWarpAugmenter.py:18,44 -> tsai 0.3.7 TSTimeWarp / TSMagWarp;
 * SURVEY 8f rank 1): one smooth random curve per call over the flattened (I*S) axis of [B, C, I, S], shared by batch and channels;
 * x, y fp32 [rows = B*C][L = I*S].  Exactly one of the two table sets:
 *   mult [L]                      y[r][n] = x[r][n] * mult[n]                                  (magnitude warp)
 *   k0 [L] int32, w [L][taps]     y[r][n] = sum_t w[n][t] * x[r][clamp(k0[n] + t, 0, L-1)]     (time warp: the interpolating cubic
 *                                 spline of each row evaluated at the warped positions, cardinal form; taps = 24)
 * The curve (a dozen Gaussian knots) and the tables are drawn / built on the host, as the reference draws them in numpy. */
int focal_warp_fwd(int rows, int L, const float* x, const float* mult, const int* k0, const float* w, int taps, float* y, void* stream);

/* Mixup / CutMix of the supervised `fixed` pipeline (data_augmenter/MixupAugmenter.py -> input_utils/mixup_utils.py:252-281, mode
 * "random_batch"): x, y fp32 [B, C, I, S] (y != x), perm int32 [B] = the ONE batch permutation of the call;
 *   cut = 0: y[b] = lam x[b] + (1 - lam) x[perm[b]];   cut = 1: y[b][:, yl:yh, xl:xh] = x[perm[b]][:, yl:yh, xl:xh], y[b] = x[b] elsewhere. */
int focal_mixup_fwd(int B, int C, int I, int S, const float* x, const int* perm, float lam, int cut, int yl, int yh, int xl, int xh,
                    float* y, void* stream);

/* Mixup's draws on the device (the host draws of Mixup._params_per_batch + _mix_batch_random + rand_bbox, input_utils/mixup_utils.py:154-176,
 * :252-281, :32-54, mode "random_batch"), so that the `fixed` pipeline sits inside a captured step: ONE launch of ONE workgroup writes a
 * focal_mix_record and the batch permutation, both in device memory, which focal_mixup_multi reads when it runs.
 * state: 4 device words {seed, draw count, 0, 0} as for focal_view_draw; advance = 1: the kernel moves them on after everybody has read them
 * (seed <- mix32(seed + 0x9E3779B9), count += 1), so every replay of a captured step draws a new mix.  advance = 0: read only; NULL = seed 0.
 * With mix32 as stated beside the jitter noise, uint32 arithmetic throughout, s = state[0]:
 *   km   = mix32(s * 0x9E3779B9 + stream_id * 0x85EBCA6B + 0x4D495855)                      the key of this draw
 *   r(i) = mix32(km + i * 0x85EBCA6B),  u(i) = (r(i) >> 8) / 2^24 in [0, 1)                  draw i (vd_uniform of the view draws)
 *   n(i) = sqrt(-2 ln(1 - u(2i))) cos(2 pi u(2i + 1))                                        (vd_normal: Box-Muller on draws 2i, 2i + 1)
 *   apply = u(0) < prob
 *   cut   = u(1) < switch_prob when mixup_alpha > 0 and cutmix_alpha > 0, else cutmix_alpha > 0
 *   lam ~ Beta(a, a), a = cut ? cutmix_alpha : mixup_alpha:
 *     a == 1: lam = u(2), exactly one uniform draw.
 *     else  : lam = G0 / (G0 + G1), two Gamma(a) draws by Marsaglia-Tsang, Gg (g = 0, 1): a' = a < 1 ? a + 1 : a, d = a' - 1/3,
 *             c = 1 / sqrt(9 d); try t = 0 .. FOCAL_MIX_GAMMA_TRIES - 1: x = n(32 + 16 g + t), v = (1 + c x)^3, w = 1 - u(128 + 16 g + t);
 *             accepted when v > 0 and ln w < x^2 / 2 + d - d v + d ln v, then Gg = d v, times (1 - u(4 + g))^(1 / a) when a < 1 (the boost).
 *             If either draw runs out of tries (probability < 0.05^16 each) lam = 0.5, the distribution's mean.  A NaN or 0 / 0 gives 0.5 too.
 *   perm: key kp = mix32(km ^ 0x5045524D), h(b) = mix32(kp + b * 0x85EBCA6B) for b in [0, B);
 *         perm[b] = #{ j : h(j) < h(b), or h(j) == h(b) and j < b } -- the rank of sample b's hash, ties broken by index: a uniformly random
 *         permutation (up to hash ties, 2^-32 a pair), computed by all threads at once; ONE permutation for all slots, as the reference's.
 *   box of slot q (its tensor is [B, C, I, S]; written when cut, all in fp32 as rand_bbox's numpy arithmetic rounds):
 *         ratio = sqrtf(1 - lam), cut_h = (int)((float)I * ratio), cut_w = (int)((float)S * ratio),
 *         cy = min((int)(u(8 + 2 q) * (float)I), I - 1), cx = min((int)(u(9 + 2 q) * (float)S), S - 1),
 *         yl = clip(cy - cut_h / 2, 0, I), yh = clip(cy + cut_h / 2, 0, I), xl = clip(cx - cut_w / 2, 0, S), xh = clip(cx + cut_w / 2, 0, S)
 *   apply == 0: the record is the identity (apply = cut = 0, lam = 1, every box 0 0 0 0) and perm is still written.
 *   apply == 1, cut == 0: the boxes are 0 0 0 0 (the reference draws none).  Slots >= n_slots: 0 0 0 0.
 * Checked on the host: prob, switch_prob in [0, 1]; an alpha > 0 (neither negative); 1 <= B <= FOCAL_MIX_MAX_BATCH; 1 <= n_slots <=
 * FOCAL_VIEW_MAX_SLOTS; every I, S >= 1. */
#define FOCAL_MIX_MAX_BATCH 4096
#define FOCAL_MIX_GAMMA_TRIES 16
typedef struct { int apply; int cut; float lam; int box[FOCAL_VIEW_MAX_SLOTS][4]; /* yl, yh, xl, xh */ } focal_mix_record;
int focal_mixup_draw(float prob, float switch_prob, float mixup_alpha, float cutmix_alpha, int B, int n_slots, const int* I, const int* S,
                     uint32_t* state, int advance, uint32_t stream_id, focal_mix_record* rec, int* perm, void* stream);
/* The mix pass of all slots of a step in ONE launch, reading the DEVICE record and permutation when the kernel runs.  Per problem
 * x, y fp32 [B, C, I, S] (y != x; every problem has the batch's B), slot = which box of the record is this tensor's.  focal_mixup_fwd's
 * arithmetic, the same expressions: cut = 0: y[b] = lam * x[b] + (1 - lam) * x[perm[b]]; cut = 1: the box of x[perm[b]] pasted into x[b];
 * apply = 0: y = x, copied through (the launch sequence of a step never depends on the draw).  The sample index comes from the grid; 16-byte
 * loads and stores where C*I*S % 4 == 0 and x, y are 16-byte aligned, scalar otherwise.  A device record cannot be checked by the host,
 * so the kernel clamps what it says before it moves a read: perm entries to [0, B), box bounds to [0, I] / [0, S]. */
typedef struct { int B, C, I, S; const float* x; float* y; int slot; } focal_mix_problem;
int focal_mixup_multi(int n, const focal_mix_problem* problems, const focal_mix_record* rec, const int* perm, void* stream);
#ifdef __cplusplus
static_assert(sizeof(focal_mix_record) == 140, "focal_mix_record");
static_assert(sizeof(focal_mix_problem) == 40, "focal_mix_problem");
#endif

/* ------------------------------------------------------------------------------------------------ row 8: embed
 * SW_Transformer.pad_input + PatchEmbed (models/SW_Transformer.py:184-208, models/SwinModules.py:547-558):
 * zero-pad [B, cin, I, S] to (Hp*1, Wp*pw), Conv2d(cin -> C0, kernel = stride = [1, pw]), flatten, LayerNorm.
 * Output tokens fp32 [B, Hp*Wp, C0].  Frozen in pretraining (general_utils/weight_utils.py:85-94): no backward. */
typedef struct { int B, cin, I, S, Hp, Wp, pw, C0; float eps; } focal_embed_desc;
int focal_pad_patch_embed_ln_fwd(const focal_embed_desc* d, const float* x, const float* w, const float* b,
                                 const float* gamma, const float* beta, float* tokens, void* stream);
/* The same, plus the LayerNorm that reads these tokens next (block 0's norm1, SwinModules.py:253): y_ln = LayerNorm(tokens;
 * gamma2, beta2, eps2) in `ln_dtype` and stats fp32 [tokens][2] = {mean, rstd} from the same kernel. */
int focal_pad_patch_embed_ln2_fwd(const focal_embed_desc* d, const float* x, const float* w, const float* b,
                                  const float* gamma, const float* beta, float* tokens, const float* gamma2, const float* beta2,
                                  float eps2, int ln_dtype, void* y_ln, float* stats, void* stream);
/* The same two with the reference's `in_stride` and `APE` switches (SW_Transformer.py:184-208, :222-224).  cin and S describe the RAW
 * input [B, cin, I, S]; the kernel folds `stride` neighbouring spectrum bins into channels inside its patch gather (embedded channel
 * (s % stride) * cin + c at position s / stride; S % stride == 0), so w is [C0, cin * stride, 1, pw] and Wp * pw >= S / stride.
 * ape: NULL, or fp32 [Hp*Wp, C0] added to the LayerNorm output by the token's position inside its sample: tokens = LN(embed) + ape, and
 * in the ln2 form y_ln / stats are those of the position-embedded tokens.  stride == 1 with ape == NULL issues the launch of the entry
 * points above.  x, w, b, gamma, beta, ape, tokens, gamma2, beta2, y_ln, stats: 16-byte aligned. */
typedef struct { int B, cin, I, S, Hp, Wp, pw, C0, stride; float eps; } focal_embed2_desc;
int focal_pad_patch_embed_ape_ln_fwd(const focal_embed2_desc* d, const float* x, const float* w, const float* b,
                                     const float* gamma, const float* beta, const float* ape, float* tokens, void* stream);
int focal_pad_patch_embed_ape_ln2_fwd(const focal_embed2_desc* d, const float* x, const float* w, const float* b,
                                      const float* gamma, const float* beta, const float* ape, float* tokens, const float* gamma2,
                                      const float* beta2, float eps2, int ln_dtype, void* y_ln, float* stats, void* stream);
/* Gradient of the absolute position embedding: dape[j] += sum_n g[n][j], g fp32 [N, cols] the residual-stream gradient at block 0's
 * input (N samples of the pass, cols = Hp*Wp*C0, cols % 4 == 0, both pointers 16-byte aligned).  Accumulates (fp32 atomics when the
 * samples are split over workgroups). */
int focal_ape_bwd(int N, int cols, const float* g, float* dape, void* stream);
/* The add alone, in place, for a caller that embeds with other kernels (the supervised path): x[n][j] += ape[j], x fp32 [N, cols]. */
int focal_ape_add_fwd(int N, int cols, float* x, const float* ape, void* stream);

/* ------------------------------------------------------------------------------------------------ LayerNorm
 * nn.LayerNorm(eps 1e-5) of models/SwinModules.py:253,258,376.  x fp32 [rows, C]; y `dtype`; stats fp32
 * [rows, 2] = {mean, rstd}.  gather = 1 is PatchMerging's 2x2 gather fused in front of its LayerNorm
 * (SwinModules.py:388-399): x is [B, H, W, Cin], rows = B*(H/2)*(W/2), C = 4*Cin.
 * Accepted widths: C a power of two in [16, 1024]; any other C is refused (FOCAL_EINVAL) before a launch.
 * Gather rule: with gather = 1 the descriptor must satisfy Cin*4 == C, H and W even, rows == B*(H/2)*(W/2) and Cin % 4 == 0, else refused.
 * Backward: dx (fp32) += or = the input gradient (scattered back to [B, H, W, Cin] when gather = 1);
 * dgamma / dbeta (fp32 [C]) are accumulated (+=).
 * dx_masked / mask (both optional): additionally writes dtype(dx * mask) -- dx being the COMPLETED residual-stream
 * gradient -- where mask is the dropout x drop-path mask of the residual branch that consumes dx next (the forward
 * epilogue's index convention); that branch's dX / dW GEMMs then take it as a plain `dtype` dy (y_dtype = dtype, no
 * residual epilogue in their descriptor).  focal_mask_cast is the same product for a gradient no LayerNorm completes. */
typedef struct { int dtype; int rows, C; float eps; int gather; int B, H, W, Cin; } focal_ln_desc;
int focal_layernorm_fwd(const focal_ln_desc* d, const float* x, const float* gamma, const float* beta, void* y,
                        float* stats, void* stream);
int focal_layernorm_bwd(const focal_ln_desc* d, const void* dy, const float* x, const float* stats,
                        const float* gamma, float* dx, int accumulate_dx, float* dgamma, float* dbeta,
                        void* dx_masked, const focal_drop_desc* mask, void* stream);
int focal_mask_cast(int dtype, int rows, int C, const float* g, const focal_drop_desc* mask, void* out, void* stream);

/* ------------------------------------------------------------------------------------------------ Linear family
 * y[M, N] = epilogue( x[M, K] . w[N, K]^T + bias ), i.e. nn.Linear of models/SwinModules.py:22-34,113-116,375 and
 * models/SW_Transformer.py:121-124,157-161, with the element-wise neighbours of each call site fused:
 *   epilogue FOCAL_EPI_RESIDUAL  y = resid + out_drop(DropPath(.)): proj_drop / Mlp.drop + drop_path + shortcut
 *            FOCAL_EPI_GELU      y = out_drop(gelu_erf(.)) AND act_grad = d y / d(.)  (Mlp.act + Mlp.drop; the
 *                                derivative is emitted once here so that no pass ever re-evaluates erf)
 *            FOCAL_EPI_RELU      y = relu(.)
 *   act_in   FOCAL_ACT_GELU      x came out of an upstream FOCAL_EPI_GELU linear: bwd_data multiplies dx by that
 *                                linear's act_grad, which is passed in the `x` slot
 *            FOCAL_ACT_RELU_OUT  x is a ReLU output: bwd_data masks dx by x > 0
 * x_dtype / y_dtype are FOCAL_F32 or `dtype`; w is `dtype` (the bf16 shadow of the fp32 master in bf16 mode).
 * splits > 1 = split-K with fp32 atomics (y must be zeroed, fp32, epilogue NONE).
 * bwd_data  : dx = [(dy * out_mask) . w] (* act_grad | * (x > 0));  dy has y's dtype, dx has x's dtype.
 * bwd_weight: dw[N, K] += (dy * out_mask)^T . x;  dbias[N] += column sums (either may be NULL). */
enum { FOCAL_ACT_NONE = 0, FOCAL_ACT_GELU = 1, FOCAL_ACT_RELU_OUT = 2 };
enum { FOCAL_EPI_NONE = 0, FOCAL_EPI_RESIDUAL = 1, FOCAL_EPI_RELU = 2, FOCAL_EPI_GELU = 3 };
typedef struct {
  int dtype;
  int M, N, K;
  int x_dtype, y_dtype;
  int act_in, epilogue;
  int splits;
  focal_drop_desc out_drop;
  int dw_workgroups;  /* bwd_weight only: workgroups the token-split plan aims at; 0 = the default (~512: one launch fills the chip).  A
                       * caller that runs several passes side by side on their own streams (the DeepSense engine: two views x two
                       * modalities) asks for ~192: the launches share the chip anyway, and a third of the workgroups is a third of the
                       * fp32 atomics of their small outputs */
} focal_linear_desc;
int focal_linear_fwd(const focal_linear_desc* d, const void* x, const void* w, const float* bias, const float* resid,
                     void* y, void* act_grad, void* stream);
/* y = resid + out_drop(DropPath(x w^T + bias)) (epilogue FOCAL_EPI_RESIDUAL, fp32 y) AND, from the same kernel, the LayerNorm
 * that follows it in the Swin block (SwinModules.py:253,258: norm2 after the attention branch, the next block's norm1 after
 * the MLP branch): y_ln = LayerNorm(y; gamma, beta, eps) in `dtype`, stats fp32 [M][2] = {mean, rstd}.  One wave must own whole
 * rows: N = 64, or 128 / 256 in bf16 (focal_linear_resid_ln_supported); other widths: focal_linear_fwd followed by focal_layernorm_fwd.  Saves one pass over the residual
 * stream and one launch per LayerNorm. */
int focal_linear_resid_ln_fwd(const focal_linear_desc* d, const void* x, const void* w, const float* bias, const float* resid,
                              float* y, const float* gamma, const float* beta, float eps, void* y_ln, float* stats, void* stream);
/* row widths the fused form takes: N == 64 (any dtype), N == 128 / 256 with bf16 operands and K % 64 == 0 (csrc/gemm_pipe.hpp with
 * row-complete wave tiles) */
int focal_linear_resid_ln_supported(int dtype, int N, int K);
int focal_linear_bwd_data(const focal_linear_desc* d, const void* dy, const void* w, const void* x, void* dx,
                          void* stream);
/* focal_linear_bwd_data for a layer whose input x came out of a LayerNorm (qkv after norm1, fc1 after norm2: SwinModules.py:253,258)
 * TOGETHER with that LayerNorm's backward (focal_layernorm_bwd with accumulate_dx = 1): g (fp32 [M, K], the residual-stream gradient) +=
 * dLN(dy . w; ln_x, ln_stats, ln_gamma); dgamma / dbeta += ...; g_masked (optional, `dtype`) = dtype(g * mask).  The [M, K] product never
 * reaches memory.  bf16, K = 64 or 128 (focal_linear_bwd_data_ln_supported); d describes the LINEAR layer (plain `dtype` x / y). */
/* (g == NULL: only dgamma / dbeta are produced -- the LayerNorm's input is a leaf nobody differentiates, e.g. norm1 of the first block behind
 * the frozen patch embedding in FOCAL pretraining; the residual-stream gradient is then neither read, updated nor re-cast) */
int focal_linear_bwd_data_ln(const focal_linear_desc* d, const void* dy, const void* w, const float* ln_x, const float* ln_stats,
                             const float* ln_gamma, float* g, float* dgamma, float* dbeta, void* g_masked, const focal_drop_desc* mask,
                             void* stream);
int focal_linear_bwd_data_ln_supported(int dtype, int N, int K);
int focal_linear_bwd_weight(const focal_linear_desc* d, const void* dy, const void* x, float* dw, float* dbias,
                            void* stream);
/* Number of workgroups focal_linear_bwd_weight launches for this descriptor (output tiles x token splits): lets a caller match its
 * calls against the launch shapes of a profiler trace (bench.py's in-step roofline).  0 = invalid descriptor. */
int focal_linear_bwd_weight_workgroups(const focal_linear_desc* d);
/* Which kernel that launch runs: 1 = focal_gemm_kernel (register-staged, any dtype / loader), 2 = focal_dw_ring_kernel (the LDS-DMA
 * ring for bf16 shapes made of whole 64-tiles, given 16-byte aligned operands; 512-thread workgroups of two token slices each).  0 = invalid descriptor. */
int focal_linear_bwd_weight_kernel(const focal_linear_desc* d);

#define FOCAL_DW_GROUP_MAX_PROBLEMS 20
/* The weight gradients of up to FOCAL_DW_GROUP_MAX_PROBLEMS linear layers in ONE launch (the four linears of a Swin block: qkv, proj, fc1, fc2 --
 * of one block, or of several consecutive blocks whose operands the caller keeps alive: round 6): per problem
 * dw[N, K] += dy[M, N]^T . x[M, K], dbias[N] += column sums of dy (dbias may be NULL) -- n calls of focal_linear_bwd_weight with
 * plain `dtype` operands (bf16; dy already carries its dropout mask), as one kernel on 128 x 128 output tiles
 * (csrc/gemm_dw_group.hpp).  Needs M % 64 == 0 and N, K % 128 == 0 per problem (focal_linear_bwd_weight_group_supported), 16-byte
 * aligned tensors.  `exclusive` != 0 promises that nothing else adds to this dw while the launch runs (another stream, another
 * problem of the same call): tiles that one workgroup owns then leave with plain read-add-write instead of atomics. */
typedef struct {
  const void* dy; const void* x; float* dw; float* dbias;
  int M, N, K;
  int exclusive;
} focal_dw_problem;
int focal_linear_bwd_weight_group(int dtype, int n, const focal_dw_problem* problems, void* stream);
int focal_linear_bwd_weight_group_supported(int dtype, int M, int N, int K);
/* Narrower problems -- M % 64 == 0 and N, K % 64 == 0 for EVERY problem, at most 4 of them (the qkv [192, 64] and proj [64, 64]
 * gradients of a 64-channel block) -- run as one launch of the 64 x 64 ring tiles behind a problem table (csrc/gemm_dw_ring.hpp,
 * always atomics).  focal_linear_bwd_weight_group_kind: 2 = a shape for the 128 x 128 group, 1 = for the 64-tile group only, 0 = neither. */
int focal_linear_bwd_weight_group_kind(int dtype, int M, int N, int K);
/* workgroups that launch consists of (profiler-trace matching, as focal_linear_bwd_weight_workgroups); 0 = invalid */
int focal_linear_bwd_weight_group_workgroups(int dtype, int n, const focal_dw_problem* problems);
/* The same for linears whose dy and x are FP32 tensors (DeepSense's nn.GRU: weight_ih / weight_hh of a layer's two directions,
 * models/RecurrentModule.py:5-31 -- dgi, dgh, the hidden states and the layer input are fp32): up to 8 problems of any shape as ONE launch
 * of the 64 x 64 tiles focal_linear_bwd_weight uses for them (operands rounded to `compute` on load, fp32 atomics; `exclusive` is not
 * used).  workgroups: the launch's target over all problems (0 = default), cf. focal_linear_desc.dw_workgroups. */
int focal_linear_bwd_weight_group_f32(int compute, int n, const focal_dw_problem* problems, int workgroups, void* stream);
int focal_linear_bwd_weight_group_f32_workgroups(int compute, int n, const focal_dw_problem* problems, int workgroups);

/* Fused MLP branch of a Swin block (models/SwinModules.py:18-34 Mlp.forward + the residual / DropPath of :339-341), bf16,
 * C = 64 -> hidden = 256 -> C (Swin stage 0, where 2/3 of the model's hidden-activation bytes are; focal_mlp_supported says
 * whether a shape is built):
 *   fwd: y = resid + drop_out( drop_hidden(gelu(a w1^T + b1)) w2^T + b2 ); the hidden activation never reaches HBM.  With y_ln
 *        non-NULL the LayerNorm that reads y next is emitted too (y_ln bf16 [M, C], ln_stats fp32 [M][2] = {mean, rstd}).
 *   bwd: gm = dtype(dL/dy x drop_out mask) (what focal_layernorm_bwd / focal_mask_cast emit as dx_masked); the hidden
 *        activation and its derivative are RECOMPUTED from `a` (dropout mask regenerated), da = dL/da (bf16), dw1 / db1 / dw2 /
 *        db2 accumulated (+=) in fp32 -- one pass over gm and a instead of four GEMMs over two saved [M, 4C] tensors.
 *        (Round 4: every wave owns 16 hidden units for the whole launch; the recomputed h / du re-enter the matrix cores from
 *        registers for the weight gradients and only du crosses LDS, for dL/da: focal_amd/csrc/mlp_bwd.hip.)
 *        With ln_x non-NULL the norm2 backward is fused behind it: da is not written; instead g (fp32 [M, C], the residual-
 *        stream gradient) += LayerNorm-backward(da; ln_x, ln_stats, ln_gamma), gm_next (bf16 [M, C], optional) = g x next_mask,
 *        dgamma / dbeta accumulated.
 * drop_hidden is a per-(row, lane group) xorshift stream seeded from (seed word, stream id, row); the forward kernel writes its keep
 * decisions to mask_bits (uint32 [M][8], one bit per hidden unit: 32 bytes per token; ignored when drop_hidden.p_elem == 0;
 * otherwise focal_mlp_bwd requires it, and focal_mlp_fwd takes NULL only from a caller that never differentiates the call -- a
 * forward-only pass with dropout on) and the backward kernel reads them back: the saved state of the branch is `a` plus these words.
 * drop_out follows the element / DropPath convention of FOCAL_EPI_RESIDUAL (over [M, C]). */
typedef struct { int dtype; int M, C, hidden; focal_drop_desc drop_hidden, drop_out; float ln_eps; } focal_mlp_desc;
int focal_mlp_supported(int dtype, int C, int hidden);
int focal_mlp_fwd(const focal_mlp_desc* d, const void* a, const float* resid, const void* w1, const float* b1, const void* w2,
                  const float* b2, float* y, const float* ln_gamma, const float* ln_beta, void* y_ln, float* ln_stats,
                  uint32_t* mask_bits, void* stream);
/* Round 6: the attention branch's tail in front of the MLP, in the same launch -- x_mid = x + drop_proj(o wp^T + bp) (the 64-channel proj
 * Linear, its Dropout, DropPath and the residual add: SwinModules.py:147, :336-338), a2 = norm2(x_mid) (:339), then the MLP branch as
 * focal_mlp_fwd.  x_mid [M, C] fp32, a2 [M, C] dtype and st2 [M, 2] are OUTPUTS (the backward pass reads them): everything
 * focal_linear_resid_ln_fwd + focal_mlp_fwd produce, bit-identical with the masks off, in one launch instead of two.
 * FOCAL_MLP_PROJ=0 makes focal_mlp_proj_supported return 0. */
int focal_mlp_proj_supported(int dtype, int C, int hidden);
int focal_mlp_proj_fwd(const focal_mlp_desc* d, const void* o, const float* x, const void* wp, const float* bp, const focal_drop_desc* drop_proj,
                       const float* g2, const float* bt2, float* x_mid, void* a2, float* st2, const void* w1, const float* b1, const void* w2,
                       const float* b2, float* y, const float* ln_gamma, const float* ln_beta, void* y_ln, float* ln_stats,
                       uint32_t* mask_bits, void* stream);
int focal_mlp_bwd(const focal_mlp_desc* d, const void* gm, const void* a, const void* w1, const float* b1, const void* w2,
                  void* da, float* dw1, float* db1, float* dw2, float* db2,
                  const float* ln_x, const float* ln_stats, const float* ln_gamma, float* g, void* gm_next,
                  const focal_drop_desc* next_mask, float* dgamma, float* dbeta, const uint32_t* mask_bits, float* dw_partials, void* stream);
/* dw_partials (round 5; NULL = every workgroup adds its 128 KB of weight gradients with fp32 atomics, 33.5 MB per launch at the memory
 * side's 1.3 TB/s): a device workspace of focal_mlp_bwd_partials_floats(d) floats, 16-byte aligned -- the workgroups store their images
 * there with plain stores and a second, small launch on the same stream sums them into dw1 / dw2. */
long focal_mlp_bwd_partials_floats(const focal_mlp_desc* d);
/* The same branch at 128 / 256 channels (Swin stages 1-2; round 6): ONE launch instead of the fc1 and fc2 launches of focal_linear_fwd /
 * focal_linear_resid_ln_fwd.  The weights (256 KB / 1 MB) stream through an LDS ring 64 hidden units at a time; a wave keeps its 16 token
 * rows' [16, C] fc2 accumulators in registers across the slices and feeds each slice's activation to fc2 straight from the fc1
 * accumulators, so the hidden tensor's tiles never leave the chip between the two products.  h and hg ([M, hidden], dtype: the activation
 * and its derivative x dropout mask) are still WRITTEN -- once -- because the backward pass of these widths reads them (a recomputing
 * backward needs 1 MB of weight-gradient accumulators per workgroup).  y_ln / ln_* (C = 128 only): the LayerNorm that reads y next, as
 * focal_linear_resid_ln_fwd emits it.  Every output is bit-identical to the two-launch form (same k order, same element math, same mask
 * indices; with the masks on, to an ulp where hipcc contracts the residual expression differently).  Back to back on cold operands it only
 * ties the two launches (profiles/r6_mlp_wide.txt); inside the replayed step it is worth +1.5 % (tools/ab_wide.sh).  FOCAL_MLP_WIDE=0 makes
 * focal_mlp_wide_supported return 0 (the engine then issues the two launches), =128 / =256 restrict it to one width. */
int focal_mlp_wide_supported(int dtype, int C, int hidden);
int focal_mlp_wide_bwd_supported(int dtype, int C, int hidden);
int focal_mlp_wide_fwd(const focal_mlp_desc* d, const void* a, const float* resid, const void* w1, const float* b1, const void* w2,
                       const float* b2, float* y, void* h, void* hg, const float* ln_gamma, const float* ln_beta, void* y_ln,
                       float* ln_stats, void* stream);
/* focal_mlp_proj_fwd's form for these widths (round 6): proj + residual + DropPath + norm2 of the attention branch in front of the MLP, in its
 * launch -- the proj weight rides the same ring, 64 output channels per step; x_mid, a2, st2 are outputs.  Bit-identical to
 * focal_linear_resid_ln_fwd (128) / focal_linear_fwd + focal_layernorm_fwd (256) followed by focal_mlp_wide_fwd with the masks off. */
int focal_mlp_wide_proj_supported(int dtype, int C, int hidden);
int focal_mlp_wide_proj_fwd(const focal_mlp_desc* d, const void* o, const float* x, const void* wp, const float* bp, const focal_drop_desc* drop_proj,
                            const float* g2, const float* bt2, float* x_mid, void* a2, float* st2, const void* w1, const float* b1, const void* w2,
                            const float* b2, float* y, void* h, void* hg, const float* ln_gamma, const float* ln_beta, void* y_ln,
                            float* ln_stats, void* stream);
/* The data path of the same branch's backward pass as one launch: du = (gm w2) x hg ([M, hidden], written once: fc1's weight gradient reads
 * it), then dc = du w1 = dL/da2, either stored (dc, dtype [M, C]; ln_x == NULL) or -- C = 128 -- finished on the row as the backward of
 * the LayerNorm that produced a2 (norm2), exactly as focal_linear_bwd_data_ln does: g += dLN (in place), g_masked = dtype(g x mask),
 * dgamma / dbeta accumulate.  Replaces focal_linear_bwd_data (GELU derivative) + focal_linear_bwd_data / _ln; the two weights are read
 * through the hardware transpose from the same ring the forward kernel uses.  Equal to the two launches up to the order inside an MFMA's
 * 32-term sum.  Measured inside the replayed step: neutral at 128 channels, -1.2 % at 256 (tools/ab_wide_bwd.sh): NOT the default --
 * focal_mlp_wide_bwd_supported answers 1 only under FOCAL_MLP_WIDE_BWD=1 (or =128 / =256 for one width); the entry point itself always works. */
int focal_mlp_wide_bwd_data(const focal_mlp_desc* d, const void* gm, const void* hg, const void* w1, const void* w2, void* du, void* dc,
                            const float* ln_x, const float* ln_stats, const float* ln_gamma, float* g, void* g_masked,
                            const focal_drop_desc* mask, float* dgamma, float* dbeta, void* stream);

/* ------------------------------------------------------------------------------------------------ row 10: W-MSA
 * WindowAttention between its qkv and proj Linears (models/SwinModules.py:121-152) with the cyclic shift, window
 * partition / reverse of SwinTransformerBlock.forward (:294-334) folded into the addressing: qkv is the token-major
 * [B*H*W, 3C] output of the qkv Linear in ORIGINAL token order, out is [B*H*W, C] in original order.
 * (sh, sw) > 0 on both axes = rolled windows + the -100 region mask of :262-289.  Attention dropout via rng. */
typedef struct {
  int dtype;
  int B, H, W, C, heads;
  int wh, ww, sh, sw;
  float p_attn;
  const uint32_t* rng;
  uint32_t stream;
} focal_attn_desc;
int focal_window_attn_fwd(const focal_attn_desc* d, const void* qkv, const float* bias_table, void* out, void* stream);
int focal_window_attn_bwd(const focal_attn_desc* d, const void* qkv, const float* bias_table, const void* dout,
                          void* dqkv, float* dbias_table, void* stream);
/* The same two operators with the qkv Linear (models/SwinModules.py:113, 128-130) folded in, for 64-channel blocks (bf16, 4 heads of
 * 16: Swin stage 0; focal_window_attn_qkv_supported): a1 [B*H*W, C] is the output of norm1, wqkv [3C, C] / bqkv [3C] the qkv layer.  A
 * wave's head is fixed, so its 48 rows of wqkv are loop-invariant MFMA operands and q / k / v of a (window, head) item are projected
 * from the window's a1 rows inside the kernel: the [B*H*W, 3C] qkv tensor never reaches HBM -- the forward pass saves a1 only, the
 * backward pass recomputes (and still emits dqkv for the layer's weight / input gradients).  Results equal focal_linear_fwd +
 * focal_window_attn_fwd / _bwd up to the accumulation order of the projection. */
int focal_window_attn_qkv_supported(int dtype, int C, int heads, int window_tokens);
int focal_window_attn_qkv_fwd(const focal_attn_desc* d, const void* a1, const void* wqkv, const float* bqkv, const float* bias_table,
                              void* out, void* stream);
/* _bwd: wproj == NULL: dout = dL/d(attention output) as in focal_window_attn_bwd; wproj [C, C] (the proj Linear's weight): dout = dL/d(proj
 * output) [B*H*W, C] (already x the branch's dropout / drop-path mask) and the kernel forms its head's slice of dout . wproj per item itself --
 * the proj layer's input-gradient launch and the [B*H*W, C] tensor between the two are gone. */
int focal_window_attn_qkv_bwd(const focal_attn_desc* d, const void* a1, const void* wqkv, const float* bqkv, const float* bias_table,
                              const void* dout, const void* wproj, void* dqkv, float* dbias_table, void* stream);


/* ------------------------------------------------------------------------------------------------ row 5: DeepSense convs
 * ConvBlock (models/ConvModules.py:115-216) on CHANNEL-LAST tokens: activation [B*I*S, C] (row = (b, interval, s)).
 * in-conv: Conv2d(cin -> C, [1,k], stride [1,stride], zero pad `pad_left`) read straight from the reference's NCHW fp32
 * spectrum [B, cin, I, S_in]; fp32; its input is a leaf, so only the weight gradient exists.  w: [C, cin, 1, k]. */
typedef struct { int B, cin, I, S_in, S_out, k, stride, pad_left, C; } focal_conv_in_desc;
int focal_conv_in_fwd(const focal_conv_in_desc* d, const float* x, const float* w, const float* bias, float* z, void* stream);
int focal_conv_in_bwd_weight(const focal_conv_in_desc* d, const float* x, const void* dz, int dz_dtype, float* dw, float* dbias,
                             void* stream);
/* The in-conv's data gradient where its input is NOT a leaf: the second ConvBlock of a multi-location DeepSense (mod_extractors.*) reads
 * the mean of the L first-level outputs as a one-channel spectrum.  cin == 1, stride == 1, S_in == S_out, C == 64, 1 <= k <= 192 (the
 * reference hard-codes in_channels = 1 there); anything else is FOCAL_EINVAL before any launch.
 *   dx[b, 0, i, s] = scale * sum_{c < 64} sum_{t < k} dz[(b, i, s + pad_left - t), c] * w[c, 0, 0, t],  rows outside [0, S) dropped
 * dz [B*I*S, 64] channel-last, fp32 or bf16 (dz_dtype), 16-byte aligned; w the fp32 master [64][1][1][k]; fp32 accumulation; dx fp32
 * [B*I, S], written (not accumulated).  One pass over dz, no atomics: bit-identical from call to call.  `scale` carries the 1 / L of
 * the mean's backward: the one dx is then the output gradient of all L first-level blocks. */
int focal_conv_in_bwd_data(const focal_conv_in_desc* d, const void* dz, int dz_dtype, const float* w, float scale, float* dx, void* stream);
/* y[i] = (sum_{l < L} xs.p[l][i]) / L, fp32, 2 <= L <= 8 (DeepSense's MeanFusionBlock over a modality's L first-level outputs).  The
 * L device pointers travel by value: no pointer table is uploaded, the launch is capturable.  One launch. */
typedef struct { const float* p[8]; } focal_ptr8;
int focal_rows_mean(int n, int L, focal_ptr8 xs, float* y, void* stream);
/* [1,k] "same" convs (any k >= 1; k - 1 zeros in all, (k - 1) / 2 on the left and the rest on the right, as torch pads an even filter;
 * the data gradient runs the flipped taps with k / 2 on the left) = MFMA GEMMs over a sliding token window.  Operand orders: w_fwd [C_out][k][C_in],
 * w_bwd [C_in][k][C_out] with taps flipped, both `dtype`, produced from the reference layout [C_out][C_in][1][k] by
 * focal_permute_pack / focal_conv_pack_bwd (the flatten + Conv1d(1x1) output layer, ConvModules.py:207-216, is
 * focal_linear_* on weights re-ordered from (c*S + s) to (s*C + c) by focal_permute_pack).
 * fwd: z (fp32) = conv(x) + bias.  bwd_data: g_out = g_in + conv^T(dz) (fp32; the residual-gradient stream).
 * bwd_weight: dw_packed [C_out][k][C_in] += dz^T window(x); dbias += column sums; focal_permute_unpack_add folds
 * dw_packed back into the [C_out][C_in][1][k] gradient. */
typedef struct { int dtype; int rows, S, C_in, C_out, k; int dw_workgroups; /* bwd_weight: as focal_linear_desc.dw_workgroups */ } focal_conv_desc;
int focal_permute_pack(int A, int Bd, int Cd, const float* src, void* dst, int dtype, void* stream);      /* dst[a][c][b] = src[a][b][c] */
int focal_permute_unpack_add(int A, int Bd, int Cd, const float* src, float* dst, void* stream);          /* dst[a][b][c] += src[a][c][b] */
int focal_conv_pack_bwd(const focal_conv_desc* d, const float* w, void* w_bwd, void* stream);
/* Several re-orderings in one launch (an encoder's 13 per pass): kind FOCAL_PACK_PERMUTE = focal_permute_pack's dst[a][c][b] = src[a][b][c]
 * (A, B, C as there), FOCAL_PACK_CONV_BWD = focal_conv_pack_bwd's dst[ci][t][co] = src[co][ci][k-1-t] with (A, B, C) = (C_out, C_in, k);
 * src fp32, dst `dtype`.  focal_unpack_add_multi: dst[a][b][c] += src[a][c][b] per entry (fp32; focal_permute_unpack_add). */
enum { FOCAL_PACK_PERMUTE = 0, FOCAL_PACK_CONV_BWD = 1, FOCAL_PACK_FRAG = 2, FOCAL_PACK_FRAG_T = 3 };
/* FOCAL_PACK_FRAG: the matrix src[A][B] (C = 1; A % 16 == 0, B % 32 == 0) in MFMA-fragment order:
 *   dst[((r / 16) * (B / 32) + c / 32) * 512 + ((c % 32) / 8 * 16 + r % 16) * 8 + c % 8] = src[r][c];
 * FOCAL_PACK_FRAG_T: the same of its TRANSPOSE m[r][c] = src[c][r] (an [B][A] matrix: B % 16 == 0, A % 32 == 0). */
#define FOCAL_PACK_MAX 24
typedef struct { const void* src; void* dst; int A, B, C; int kind; } focal_pack_entry;
int focal_pack_multi(int dtype, int n, const focal_pack_entry* entries, void* stream);
int focal_unpack_add_multi(int n, const focal_pack_entry* entries, void* stream);
int focal_conv_fwd(const focal_conv_desc* d, const void* x, const void* w_fwd, const float* bias, float* z, void* stream);
int focal_conv_bwd_data(const focal_conv_desc* d, const void* dz, const void* w_bwd, const float* g_in, float* g_out, void* stream);
int focal_conv_bwd_weight(const focal_conv_desc* d, const void* dz, const void* x, float* dw_packed, float* dbias, void* stream);

/* BatchNorm2d(eps 1e-5, momentum 0.1) + GELU + Dropout2d + residual of ConvLayer2D (ConvModules.py:98-112,203-204).
 * focal_bn_stats: training -> batch mean / biased variance of z [rows, C] into mean_rstd [2C] and the momentum update of the
 * running buffers (unbiased variance); eval -> mean_rstd from the running buffers.  scratch: 2C + 1 floats (the sums and an arrival counter:
 * in FOCAL_BN_TRAIN mode the last workgroup of the statistics kernel finalises mean / rstd / running buffers itself).
 * focal_bn_act_fwd: y = resid + drop2d(gelu(gamma * zhat + beta)) (fp32), optional `dtype` copy y_cast for the next GEMM.
 * focal_bn_act_bwd: dz (`dtype`) from g = dL/dy (fp32); dgamma / dbeta accumulated (+=).
 * Data-parallel exact ("sync") statistics: the per-channel sums are exposed so that the caller can all-reduce the 2C
 * floats of `scratch` between the two halves of each call --
 *   focal_bn_stats   training = FOCAL_BN_PARTIAL: scratch <- local {sum z, sum z^2};   FOCAL_BN_FINALIZE: mean_rstd and
 *                    running buffers from scratch, normalising by d->stat_rows (the GLOBAL row count);
 *   focal_bn_act_bwd phase = FOCAL_BN_PARTIAL: scratch <- local {sum da, sum da*zhat}, dgamma / dbeta += the LOCAL sums;
 *                    FOCAL_BN_FINALIZE: dz from the (all-reduced) scratch and d->stat_rows.
 * stat_rows = 0 means rows. */
typedef struct { int dtype; int rows, C, rows_per_sample; float eps, momentum, p_drop; const uint32_t* rng; uint32_t stream; int stat_rows; int groups; } focal_bn_desc;
/* groups (0 or 1: one): the tensor's `rows` are `groups` equal, consecutive row ranges with batch statistics of their OWN -- the two
 * augmented views of a FOCAL step as one batch of 2B windows (models/FOCALModules.py:21-34 calls the backbone once per view, so
 * every BatchNorm2d normalises each view by itself, ConvModules.py:86).  With groups > 1 every per-call array is `groups` copies of its
 * one-group layout, group after group: scratch, mean_rstd [groups][2C], running_mean / running_var [groups][C] (sinks that RECORD each
 * group's statistics: d->momentum = 1, then focal_bn_running_combine); gamma / beta / dgamma / dbeta stay [C] (the gradients are the sum
 * over the groups).  Dropout2d samples are numbered through the whole tensor.  Training mode on one rank only (stat_rows = 0). */
enum { FOCAL_BN_EVAL = 0, FOCAL_BN_TRAIN = 1, FOCAL_BN_PARTIAL = 2, FOCAL_BN_FINALIZE = 3 };
/* OR into `training` / `phase`: the caller guarantees `scratch` holds zeros (e.g. a slice of a per-step zeroed pool), so the call
 * does not enqueue its own memset (one launch less per BatchNorm pass). */
#define FOCAL_BN_SCRATCH_ZEROED 16
int focal_bn_stats(const focal_bn_desc* d, const float* z, float* scratch, float* mean_rstd, float* running_mean, float* running_var,
                   int training, void* stream);
/* focal_conv_fwd AND the training-mode statistics of the BatchNorm that follows it (ConvModules.py:54-112: conv -> BatchNorm2d), from the
 * convolution's epilogue: what focal_bn_stats(bn, z, ..., FOCAL_BN_TRAIN) would compute, without reading z back and without its launch.
 * bf16 operands.  scratch: FOCAL_BN_STAT_SLOTS x 2C + 1 floats, ZERO on entry (column sums in 16 slots + the arrival counter of the last-
 * workgroup finalisation); mean_rstd [2C] out; running_mean / running_var updated with bn->momentum (both NULL: not touched). */
#define FOCAL_BN_STAT_SLOTS 16
int focal_conv_fwd_bn(const focal_conv_desc* d, const void* x, const void* w_fwd, const float* bias, float* z,
                      const focal_bn_desc* bn, float* scratch, float* mean_rstd, float* running_mean, float* running_var, void* stream);
/* Round 6: the sums-only form.  Where focal_conv_fwd_bn_sums_supported(...) != 0 (64 -> 64 channels, k = 3 / 4 / 5, bf16, whole 64-row tiles per
 * statistics group: csrc/conv_ring.hpp), focal_conv_fwd_bn may be called with mean_rstd = NULL (running buffers ignored): the launch then only
 * adds its per-channel sums into `scratch` and ends, and focal_bn_act_fwd_sums -- focal_bn_act_fwd reading `scratch` instead of mean_rstd --
 * finishes the statistics in its prologue (mean_rstd [groups x 2C] out for the backward pass, running buffers updated with d->momentum).  Same
 * arithmetic as the one-launch form; the convolution loses three dependent memory-side round trips (~9 us per launch). */
int focal_conv_fwd_bn_sums_supported(const focal_conv_desc* d, const focal_bn_desc* bn, const void* x, const void* w_fwd);
int focal_bn_act_fwd_sums(const focal_bn_desc* d, const float* z, const float* sums, float* mean_rstd, float* running_mean, float* running_var,
                          const float* gamma, const float* beta, const float* resid, float* y, void* y_cast, void* stream);
/* The running-buffer updates of TWO passes (the two augmented views of a FOCAL step), applied after both have run: each pass records
 * its batch statistics instead of updating the buffers (focal_bn_stats with d->momentum = 1 and a per-pass sink in place of the running
 * buffers), this applies r <- (1 - m) ((1 - m) r + m s1) + m s2 to n buffers of C values in one launch -- what the reference's two
 * sequential backbone calls leave behind (models/FOCALModules.py:21-34), without ordering the passes. */
#define FOCAL_BN_COMBINE_MAX 24
int focal_bn_running_combine(int n, float* const* running, const float* const* view1, const float* const* view2, int C, float momentum,
                             void* stream);
int focal_bn_act_fwd(const focal_bn_desc* d, const float* z, const float* mean_rstd, const float* gamma, const float* beta,
                     const float* resid, float* y, void* y_cast, void* stream);
int focal_bn_act_bwd(const focal_bn_desc* d, const float* z, const float* g, const float* mean_rstd, const float* gamma,
                     const float* beta, float* scratch, void* dz, float* dgamma, float* dbeta, int phase, void* stream);

/* ------------------------------------------------------------------------------------------------ row 6: bi-GRU
 * nn.GRU(2 layers, bidirectional) + time mean (models/RecurrentModule.py:5-31).  Matrix products go through
 * focal_linear_*; these are the per-step gate kernels.  gi: [B*T, 3H] (rows (b, t), b_ih included), gh: [B, 3H] (b_hh
 * included), out: [B, T, 2H], save: [4][B][H] per step (r, z, n, W_hn h + b_hn).
 * bwd: dh = scale * dout[b*ld_b + t*ld_t + dir_offset + j] + dh_rec + dhz_in; writes dgi rows (b, t), dgh [B, 3H], dhz_out. */
typedef struct { int B, T, H; int whh_frag; } focal_gru_desc;
/* whh_frag (focal_gru_seq_fwd / _bwd only; 0 = as documented below): the W_hh operands are given in MFMA-fragment order instead of
 * row-major -- 16-row x 32-column tiles, tile-major, inside a tile the 64 lanes' 16-byte pieces back to back
 * (FOCAL_PACK_FRAG / FOCAL_PACK_FRAG_T of focal_pack_multi): every load instruction of the kernels' prologue then reads one contiguous KB
 * instead of sixteen 64-byte row segments. */
int focal_gru_gate_fwd(const focal_gru_desc* d, int t, int dir_offset, const float* gi, const float* gh, const float* h_prev,
                       float* h_new, float* out, float* save, void* stream);
int focal_gru_gate_bwd(const focal_gru_desc* d, int t, int dir_offset, const float* dout, long ld_b, long ld_t, float scale,
                       const float* dh_rec, const float* dhz_in, const float* save, const float* h_prev, float* dgi, float* dgh,
                       float* dhz_out, void* stream);
/* Whole-sequence form (bf16 W_hh; H in {128, 256}): ONE launch runs all T steps of one layer for n_dir (1 or 2) directions
 * (direction 0 walks t = 0..T-1, direction 1 t = T-1..0 and writes out[..., H:2H]).  Per-direction HOST arrays of device
 * pointers: gi [B*T, 3H] (b_ih included), whh bf16 [3H, H], bhh [3H], hs [T+1, B, H] (hs[0] = h0, written from hs[1]),
 * save [T, 4, B, H] indexed by step s.  Backward: whh_t = bf16 [H, 3H] (the transposed W_hh), dgi [B*T, 3H], dgh [T, B, 3H]
 * (step-indexed) are written for the weight / input gradient GEMMs; dout as in focal_gru_gate_bwd.
 * Tensors must stay below 4 GB (32-bit byte offsets).  A batch that is not a multiple of the kernel's samples per workgroup (8 while
 * ceil(B / 8) * n_dir <= 128 at H = 256, else 16) is handled by recomputing the last sample in the spare lanes. */
int focal_gru_seq_fwd(const focal_gru_desc* d, int n_dir, const float* const* gi, const void* const* whh, const float* const* bhh,
                      float* const* hs, float* const* save, float* out, void* stream);
int focal_gru_seq_bwd(const focal_gru_desc* d, int n_dir, const float* dout, long ld_b, long ld_t, float scale,
                      const void* const* whh_t, const float* const* hs, const float* const* save, float* const* dgi,
                      float* const* dgh, void* stream);
int focal_mean_time(int B, int T, int D, const float* x, float* y, void* stream);                       /* y[b] = mean_t x[b][t] */
int focal_dropout(long n, const float* x, float* y, const uint32_t* rng, uint32_t stream_id, float p, void* stream); /* y = x * mask */
int focal_axpy(long n, float a, const float* x, float* y, void* stream);                                   /* y += a * x */
int focal_mul(long n, const float* a, float* y, void* stream);                                             /* y *= a (element-wise, fp32) */

/* ------------------------------------------------------------------------------------------------ classifier head (8f rank 4)
 * Finetuning path, `backbone(freq_x, class_head=True)` (models/SW_Transformer.py:269-276, models/FusionModules.py:61-140):
 * focal_fusion_attn_*: the attention core of TransformerFusionBlock -- one query per sample (the mean of the M fused tokens,
 * after in_proj) over the M modality tokens, nn.MultiheadAttention semantics with head_dim 64: q [B, E] (in_proj applied),
 * kv [B*M, 2E] rows (b, j) = {k | v}, out [B, E] (before out_proj); probs / weights [B, heads, M] = softmax and softmax x
 * attention-dropout mask (saved for backward).  Backward writes dq [B, E] and dkv [B*M, 2E].
 * focal_cross_entropy: nn.CrossEntropyLoss(), mean reduction: loss[0] and dlogits = d loss / d logits in one launch. */
int focal_fusion_attn_fwd(int B, int M, int E, int heads, const float* q, const float* kv, float* out, float* probs, float* weights,
                          const uint32_t* rng, uint32_t stream_id, float p_drop, void* stream);
int focal_fusion_attn_bwd(int B, int M, int E, int heads, const float* q, const float* kv, const float* probs, const float* weights,
                          const float* dout, float* dq, float* dkv, void* stream);
int focal_cross_entropy(int B, int C, const float* logits, const long* labels, float* loss, float* dlogits, void* stream);
/* The evaluation loop's accumulator (train_utils/eval_functions.py:29-62): one launch per batch, no host read.  Exactly one of
 * logits (fp32 [B, C]) and preds_in ([B]) is given.  Logits mode: acc[0] += the batch's mean cross-entropy -- bit-identical to
 * focal_cross_entropy's loss[0] on the same arguments --, acc[1] += 1 (the mean of acc[0] over acc[1] batches is the reference's
 * np.mean(classifier_loss_list): per batch, not per sample); the prediction of a row is the first index of its maximum.
 * Prediction mode: the matrix alone (the KNN path of pretraining validation).  conf is int [C*C + 1]: conf[label*C + pred] += 1
 * per row; a row whose label or prediction is outside [0, C) adds to neither the matrix nor the loss, never indexes logits with
 * the label, and adds 1 to conf[C*C] -- the caller reads that word with the matrix and refuses the result when it is not 0.
 * preds_out ([B] or NULL) receives the predictions.  1 <= C <= 64, B >= 1.  One workgroup: launches that share acc / conf must
 * be ordered by their stream. */
int focal_eval_accumulate(int B, int C, const float* logits, const long* preds_in, const long* labels, double* acc, int* conf,
                          long* preds_out, void* stream);
/* KNN scoring of un-projected backbone features (train_utils/knn.py: GpuKNNClassifier.predict_fused, src/eval_knn.py): the k nearest
 * training rows of every query under d2 = (|q|^2 + |t|^2) - 2 q.t in exact fp32 (v_mfma_f32_16x16x4_f32), ordered by (d2, training
 * index); a NaN distance orders behind every number.  Two launches, no allocation and no host read: both can be captured.
 * focal_knn_search: q fp32 [nq, D], t fp32 [nt, D], t_sq fp32 [nt] = the rows' squared norms (|q|^2 is taken in the kernel).  The
 * training rows are cut into `slices` contiguous slices of ceil(nt / slices) rows; a workgroup owns 128 queries and one slice and
 * writes that slice's k best per query to part_d2 / part_idx, each [nq, slices, k], ascending; slots beyond the slice's row count
 * carry +inf and index -1.  d2 of a pair depends on the two rows alone -- not on the row's place in t, the tile or `slices` -- so the
 * outputs of focal_knn_vote are bit-identical for every `slices`, and duplicate training rows tie exactly (the smaller index wins).
 * focal_knn_vote: merges the slices into the k_eff = min(k, nt) neighbours of each query; preds [nq] = the most frequent of their
 * t_labels, ties to the smallest label (sklearn's mode).  nbr_idx / nbr_d2 ([nq, k] or NULL) receive the sorted lists, columns from
 * k_eff on -1 / +inf.  conf (int [C*C + 1] or NULL, needs q_labels [nq]) += the confusion matrix, with the semantics of
 * focal_eval_accumulate's prediction mode (a row whose label or prediction is outside [0, C) adds 1 to conf[C*C] and nothing else),
 * by integer atomics: calls that share conf need no ordering beyond the stream's.
 * Limits (FOCAL_EINVAL before any launch): 1 <= k <= 16, 1 <= n_classes <= 64, D >= 4, D % 4 == 0, nt, nq, slices >= 1, q and t
 * 16-byte aligned. */
typedef struct { int nq, nt, D, k, n_classes, slices; } focal_knn_desc;
int focal_knn_search(const focal_knn_desc* d, const float* q, const float* t, const float* t_sq, float* part_d2, int* part_idx,
                     void* stream);
int focal_knn_vote(const focal_knn_desc* d, const float* part_d2, const int* part_idx, const long* t_labels, const long* q_labels,
                   long* preds, int* nbr_idx, float* nbr_d2, int* conf, void* stream);
/* Rank of one named gallery row per query (train_utils/retrieval.py: cross_modal_ranks, src/eval_retrieval.py): q fp32 [nq, D], t fp32
 * [nt, D], t_sq fp32 [nt] = the gallery rows' squared norms as the caller computed them (|q|^2 is taken in the kernel), pos int [nq].
 * d2(i, j) = (|q_i|^2 + t_sq[j]) - 2 q_i.t_j is the very bits focal_knn_search produces for that pair.  With p = pos[i] in [0, nt) and
 * key the search's order-preserving key of a distance: pos_d2[i] = d2(i, p); before[i] = the j != p whose (key(d2(i, j)), j) orders
 * before (key(d2(i, p)), p) -- the search's (d2, index) order, so the rank is before + 1 and a NaN distance orders behind every number;
 * tied[i] = the j != p with key(d2(i, j)) == key(d2(i, p)).  A pos[i] outside [0, nt) gives before = tied = -1 and pos_d2 = NaN and
 * never indexes t or t_sq.  tied and pos_d2 may be NULL.  The outputs are written, not accumulated, and are bit-identical for every
 * `slices` (contiguous slices of ceil(nt / slices) gallery rows, as in the search).  Two launches -- the positives' distances from the
 * gathered rows t[pos], then the scan, whose per-slice counts meet in integer atomics -- with no allocation, no host read and no
 * floating-point atomic: the call can be captured.  The [nq, nt] distances exist in LDS tiles only.  ws: focal_rank_workspace(d) bytes.
 * Limits (FOCAL_EINVAL before any launch): D >= 4, D % 4 == 0, nq, nt >= 1, 1 <= slices <= 65535, q and t 16-byte aligned,
 * ws_bytes >= focal_rank_workspace(d). */
typedef struct { int nq, nt, D, slices; } focal_rank_desc;
size_t focal_rank_workspace(const focal_rank_desc* d);
int focal_rank_positive(const focal_rank_desc* d, const float* q, const float* t, const float* t_sq, const int* pos, int* before, int* tied,
                        float* pos_d2, void* ws, size_t ws_bytes, void* stream);
/* Sums of a function of the distance over all pairs (train_utils/geometry.py: silhouette, uniformity; src/eval_geometry.py): q fp32
 * [nq, D], t fp32 [nt, D], t_sq fp32 [nt] as for focal_rank_positive, group int [nt] (NULL with G = 1: every row is in group 0), S fp32
 * [nq, G].  S[i, g] = sum over the j with group[j] == g and j != self_offset + i of f(max(d2(i, j), 0)), d2 the very bits
 * focal_knn_search produces for that pair; f = x (FOCAL_PAIR_SQDIST), sqrt(x) (FOCAL_PAIR_DIST) or exp(-scale x) (FOCAL_PAIR_GAUSS).
 * self_offset >= 0 says that query row i IS gallery row self_offset + i: that one candidate is left out by its index (a duplicate of
 * the row elsewhere still counts); -1 leaves nothing out.  A group[j] outside [0, G) means row j is not counted; a group without rows
 * gets exactly 0; a non-finite term of a counted row makes its sum non-finite and may make the query's other groups' sums NaN, an uncounted
 * row reaches no sum.  The gallery is cut into `slices` contiguous slices of ceil(nt / slices) rows; each
 * (128 queries, slice) workgroup writes its partial [128, G] to ws and a second launch adds the partials in slice order (one slice: one
 * launch that writes S).  No floating-point atomic: the order of every addition is fixed by (nq, nt, D, G, slices), so equal arguments
 * give equal bits; another `slices` is another order and may differ in the last bits.  S is written, not accumulated.  No allocation, no
 * host read: the call can be captured.  The [nq, nt] distances exist in LDS tiles only.  ws: focal_pair_sums_workspace(d) bytes (never
 * 0 for a valid descriptor).  Limits (FOCAL_EINVAL before any launch): D >= 4, D % 4 == 0, nq, nt >= 1, 1 <= G <= 64, group non-NULL
 * unless G = 1, 1 <= slices <= 65535, ceil(nq / 128) * slices and nq * G / 256 within the launch grid, fn one of the three, scale finite
 * and >= 0, self_offset >= -1, q and t 16-byte aligned, ws_bytes >= focal_pair_sums_workspace(d). */
enum { FOCAL_PAIR_SQDIST = 0, FOCAL_PAIR_DIST = 1, FOCAL_PAIR_GAUSS = 2 };
#define FOCAL_PAIR_MAX_GROUPS 64
typedef struct { int nq, nt, D, G, slices, fn, self_offset; float scale; } focal_pairsum_desc;
size_t focal_pair_sums_workspace(const focal_pairsum_desc* d);
int focal_pair_sums(const focal_pairsum_desc* d, const float* q, const float* t, const float* t_sq, const int* group, float* S, void* ws,
                    size_t ws_bytes, void* stream);
/* Sequence ranking counts of the temporal constraint (train_utils/temporal.py: sequence_ranking; src/eval_temporal.py): z fp32 [n, D]
 * with n = S L, rows a L .. a L + L - 1 = sequence a, z_sq fp32 [n] as for focal_rank_positive.  d2(i, j) is the very bits
 * focal_knn_search produces for that pair, f = x (FOCAL_PAIR_SQDIST) or sqrt(x) (FOCAL_PAIR_DIST) of max(d2, 0).
 * intra_d2 [n, L]: d2(i, a(i) L + c), self column included.  intra_sum [S]: sum over i != j in a of f, added in row-major (i, j) order.
 * With P(a, b) = sum over i in a, j in b of f, added in row-major order inside the block:
 * before [S] (int): the b != a with P(a, b) (L^2 - L) < intra_sum[a] L^2 -- the mean block distance below the mean intra distance;
 * viol [S] (int): the same with margin L^2 (L^2 - L) added to the right-hand side -- the loss's hinge active for (a, b);
 * hinge_sum [S]: sum over b != a of max(0, intra_sum[a] / (L^2 - L) - P(a, b) / L^2 + margin), carried as the difference of viol's two
 * sides and divided by L^2 (L^2 - L) once, after the last addition; inter_sum [S]: sum over b != a of P(a, b).
 * The block b = a is left out by index.  A NaN pooled value is never counted and makes that sequence's two float sums NaN.  Every output
 * is written, not accumulated.  z is cut into `slices` contiguous slices of whole 64-row tiles; the integer counts meet in integer
 * atomics and are bit-identical for every `slices`; the float partials go to ws and a last launch adds them in slice order (one slice:
 * the scan writes them itself), so equal arguments give equal bits and another `slices` may differ in the last bits.  No floating-point
 * atomic, no allocation, no host read: the call can be captured.  The [n, n] distances and the [S, S] pooled values exist in LDS tiles
 * and registers only.  ws: focal_seq_rank_workspace(d) bytes (never 0 for a valid descriptor).  Limits (FOCAL_EINVAL before any
 * launch): D >= 4, D % 4 == 0, L in {2, 4, 8, 16}, n % L == 0, S >= 2, 1 <= slices <= 65535, ceil(n / 128) * slices within the launch
 * grid, fn one of the two, margin finite, z 16-byte aligned, ws_bytes >= focal_seq_rank_workspace(d). */
typedef struct { int n, D, L, slices, fn; float margin; } focal_seqrank_desc;
size_t focal_seq_rank_workspace(const focal_seqrank_desc* d);
int focal_seq_rank(const focal_seqrank_desc* d, const float* z, const float* z_sq, float* intra_d2, float* intra_sum, int* before, int* viol,
                   float* hinge_sum, float* inter_sum, void* ws, size_t ws_bytes, void* stream);
/* K-means on the same features (train_utils/kmeans.py: GpuKMeans, src/eval_cluster.py): R restarts of K centroids are ONE matrix c fp32
 * [R*K, D], restart r in rows r*K .. r*K + K - 1, with c_sq fp32 [R*K] their squared norms; x is fp32 [n, D].  One Lloyd iteration of all
 * restarts is focal_kmeans_assign + focal_kmeans_update: three launches, no allocation, no host read (capturable), x read twice while
 * R * K <= 160 (beyond that the update reads it once per group of floor(160 / K) restarts), and no floating-point atomic: the same
 * arguments give the same bits.
 * focal_kmeans_assign: labels[r*n + i] (int [R, n], read AND written) <- the k that minimises d2(x_i, c[r*K + k]), ordered by (d2, k); d2
 * is the very function of the two rows that focal_knn_search computes (so for R = 1 the labels are its nearest neighbour over c, bit for
 * bit); a NaN distance orders behind every number and a row whose distances are all NaN gets 0.  The [n, R*K] distances exist in LDS
 * tiles only.  min_d2 ([R, n] or NULL) receives d2 of the chosen centroid; changed (int [R] or NULL) += the rows of restart r whose
 * label differs from the value labels held on entry (integer atomics; the caller zeroes it).  `slices` is not read.
 * focal_kmeans_update: c[r*K + k] <- the mean of the rows labelled k in restart r (a label outside [0, K) joins no cluster) and c_sq its
 * squared norm, both in place; an EMPTY cluster keeps its centroid and its norm, bits unchanged (sklearn relocates it instead).
 * counts (int [R, K]) <- the cluster sizes; inertia ([R] or NULL, needs min_d2 [R, n]) <- the sum of min_d2 over the rows.  The rows are
 * cut into `slices` contiguous slices whose partial sums are added in slice order: the results depend on `slices`, and on nothing else.
 * ws: focal_kmeans_update_workspace(d) bytes (0 for a descriptor outside the limits), written before it is read.
 * Limits (FOCAL_EINVAL before any launch): D >= 4, D % 4 == 0, 1 <= K <= 64, R >= 1, R * K <= 1024, n >= 1, 1 <= slices <= 65535, x and
 * c 16-byte aligned. */
typedef struct { int n, D, K, R, slices; } focal_kmeans_desc;
int focal_kmeans_assign(const focal_kmeans_desc* d, const float* x, const float* c, const float* c_sq, int* labels, float* min_d2,
                        int* changed, void* stream);
size_t focal_kmeans_update_workspace(const focal_kmeans_desc* d);
int focal_kmeans_update(const focal_kmeans_desc* d, const float* x, const int* labels, const float* min_d2, float* c, float* c_sq,
                        int* counts, float* inertia, void* ws, size_t ws_bytes, void* stream);
/* Linear probe on the same features (train_utils/linear_probe.py: GpuLinearProbe, src/eval_linear.py): the objective and gradient of
 * softmax regression for R regularisation strengths at once.  Problem r holds W_r [C, D], b_r [C] and lambda_r; all problems are ONE
 * matrix w fp32 [R*C, D] with b fp32 [R*C] and lam fp32 [R]; x is fp32 [n, D], y int [n] the class of each row.
 *   F_r = (1/n) sum_i CE(softmax(W_r x_i + b_r), y_i) + (lambda_r / 2) |W_r|^2          (the bias is not penalised)
 * One evaluation is focal_probe_forward + focal_probe_grad: three launches, no allocation, no host read (capturable), x read twice
 * while R * C <= 64 (beyond that the gradient pass reads it once per 64-row chunk of R*C), and no floating-point atomic: the same
 * arguments give the same bits, and a problem's outputs do not depend on which other problems share the launch.
 * focal_probe_forward: z = x w^T + b by the exact-fp32 product of focal_knn_search, held in LDS tiles only; per row and problem the
 * log-sum-exp with the maximum subtracted (expf / logf, not the fast intrinsics).  Writes whichever of these is not NULL:
 * ce [R, n] = lse - z_y; g [n, R*C] = softmax - onehot; preds int [R, n] = the arg-max class, ties to the smallest class, a NaN logit
 * never beats a number (all NaN: 0).  ce and g need y; a predict-only call passes NULL for y, ce and g.  y is NOT range-checked on the
 * device (the caller refuses labels outside [0, C) before the launch); such a label selects no logit and no one-hot.  `slices` is
 * not read.
 * focal_probe_grad: gw [R*C, D] = (1/n) g^T x + lambda_r W_r, gb [R*C] = (1/n) sum_i g, f double [R] = F_r from ce and w.  The rows
 * are cut into `slices` contiguous slices whose partial products are added in slice order: gw and gb depend on `slices`, and on
 * nothing else.  ws: focal_probe_grad_workspace(d) bytes (0 for a descriptor outside the limits), written before it is read.
 * Limits (FOCAL_EINVAL before any launch): D >= 4, D % 4 == 0, 2 <= C <= 64, R >= 1, R * C <= 1024, n >= 1, 1 <= slices <= 65535, x
 * and w 16-byte aligned. */
typedef struct { int n, D, C, R, slices; } focal_probe_desc;
int focal_probe_forward(const focal_probe_desc* d, const float* x, const float* w, const float* b, const int* y, float* ce, float* g,
                        int* preds, void* stream);
size_t focal_probe_grad_workspace(const focal_probe_desc* d);
int focal_probe_grad(const focal_probe_desc* d, const float* x, const float* g, const float* ce, const float* w, const float* lam,
                     float* gw, float* gb, double* f, void* ws, size_t ws_bytes, void* stream);
/* Exact t-SNE of the same features (train_utils/tsne.py: GpuTSNE, src/eval_tsne.py): x fp32 [n, D] -> y fp32 [n, 2].  Three setup calls
 * build the joint-probability matrix P fp32 [n, n] in ONE buffer, in place; one descent iteration is focal_tsne_grad + focal_tsne_step:
 * two launches, P read once, no [n, n] temporary, no allocation, no host read (capturable), no floating-point atomic: the same arguments,
 * `slices` included, give the same bits.  Every [n, n] offset is 64-bit.
 * focal_tsne_dist: x_sq [n] <- the rows' squared norms by focal_knn_search's tree for |q|^2; d2 [n, n] <- (|x_i|^2 + |x_j|^2) - 2 x_i.x_j,
 * the very function of the two rows that focal_knn_search computes when handed x_sq as t_sq; the diagonal is written as +0.
 * focal_tsne_perplexity: per row i, beta_i by exactly 64 steps (beta = 1; doubled while no upper bound exists, bisected after; no early
 * exit) on H(beta) = log sum p + beta sum (d2 - dmin) p / sum p against log(perplexity), p_j = exp(-(d2_ij - dmin_i) beta) over j != i with
 * dmin_i the row's smallest off-diagonal distance; H > log(perplexity) raises the lower bound.  p (holding d2 on entry) <- the conditional
 * row p_j|i, diagonal 0; beta [n] <- beta_i.  One workgroup per row with the row in LDS: n <= 32 768.
 * focal_tsne_symmetrize: p <- (p_j|i + p_i|j) / 2n, bitwise symmetric, diagonal 0; p_log_p (one double) <- sum P log P, from per-tile
 * double partials in ws (focal_tsne_symmetrize_workspace(d) bytes) added in tile order.
 * focal_tsne_grad: with q_ij = 1 / (1 + |y_i - y_j|^2) over j != i, per row and column slice the partial sums of P q (y_i - y_j) (2),
 * q^2 (y_i - y_j) (2), q, and with want_kl P log q, to ws laid out [slices][6][n] (focal_tsne_grad_workspace(d) bytes).  The columns are
 * cut into `slices` contiguous slices of ceil(n / slices) columns rounded up to a multiple of 4.
 * focal_tsne_step (one workgroup): Z = sum q in double, g_i = 4 (exaggeration attr_i - rep_i / Z) with the slices added in slice order,
 * then sklearn's update: gains <- (upd g < 0 ? gains + 0.2 : gains 0.8) floored at 0.01, upd <- momentum upd - lr gains g, y += upd.
 * record (double [2 + 3 cap] or NULL): record[0] += 1 per call (the iteration count); with want_kl the entry {iteration, KL = sum P log P -
 * sum P log q + log Z, |g|_2} is appended at 2 + 3 record[1] while record[1] < cap, and record[1] += 1.  KL is the divergence only at
 * exaggeration 1.  want_kl must be the value focal_tsne_grad was called with.
 * Limits (FOCAL_EINVAL before any launch): D >= 4, D % 4 == 0, 2 <= n <= 32768, 1 <= perplexity < n, 1 <= slices <= 65535, x and p
 * 16-byte aligned. */
typedef struct { int n, D, slices; } focal_tsne_desc;
int focal_tsne_dist(const focal_tsne_desc* d, const float* x, float* x_sq, float* d2, void* stream);
int focal_tsne_perplexity(const focal_tsne_desc* d, float perplexity, float* p, float* beta, void* stream);
size_t focal_tsne_symmetrize_workspace(const focal_tsne_desc* d);
int focal_tsne_symmetrize(const focal_tsne_desc* d, float* p, double* p_log_p, void* ws, size_t ws_bytes, void* stream);
size_t focal_tsne_grad_workspace(const focal_tsne_desc* d);
int focal_tsne_grad(const focal_tsne_desc* d, const float* y, const float* p, int want_kl, void* ws, size_t ws_bytes, void* stream);
int focal_tsne_step(const focal_tsne_desc* d, const void* ws, size_t ws_bytes, const double* p_log_p, float* y, float* upd, float* gains,
                    float lr, float momentum, float exaggeration, int want_kl, double* record, int record_cap, void* stream);

/* ------------------------------------------------------------------------------------------------ location fusion (SW_Transformer)
 * Multi-location datasets: per modality, the L location features of a sample are a sequence of L tokens that runs through
 * loc_block_num nn.TransformerEncoderLayer and one TransformerFusionBlock (models/SW_Transformer.py, focal_amd/loc_engine.py).
 * focal_loc_attn_*: the encoder layer's self-attention core, nn.MultiheadAttention semantics with head_dim 64: qkv [N*L, 3E] rows
 * (n, i) = {q | k | v} (in_proj applied), out [N*L, E] (before out_proj); probs / weights [N, heads, L, L] = softmax(q k^T / 8) and
 * softmax x attention-dropout mask (saved for backward).  Backward writes dqkv [N*L, 3E] in the same packing.  2 <= L <= 8,
 * E = heads * 64 <= 256.  One workgroup per sequence.
 * focal_loc_stack: out [N, L, E] <- feats[l] [N, E] (L device pointers, host array).  focal_loc_unstack_add: dst[l] [N, E] <-
 * a[:, l, :] + b[:, l, :].  focal_loc_mean_bwd_add: dx [N, L, E] += dq [N, E] / L.  E % 4 == 0, 16-byte aligned tensors. */
int focal_loc_attn_fwd(int N, int L, int E, int heads, const float* qkv, float* out, float* probs, float* weights, const uint32_t* rng,
                       uint32_t stream_id, float p_drop, void* stream);
int focal_loc_attn_bwd(int N, int L, int E, int heads, const float* qkv, const float* probs, const float* weights, const float* dout,
                       float* dqkv, void* stream);
int focal_loc_stack(int N, int L, int E, const float* const* feats, float* out, void* stream);
int focal_loc_unstack_add(int N, int L, int E, const float* a, const float* b, float* const* dst, void* stream);
int focal_loc_mean_bwd_add(int N, int L, int E, const float* dq, float* dx, void* stream);
/* The class layer nn.Linear(K -> n_cls) (a few output columns, fp32): y = x w^T + bias; backward accumulates dw / dbias (+=) and
 * writes dx when it is non-NULL. */
int focal_small_linear_fwd(int B, int N, int K, const float* x, const float* w, const float* bias, float* y, void* stream);
int focal_small_linear_bwd(int B, int N, int K, const float* dy, const float* x, const float* w, float* dw, float* dbias, float* dx,
                           void* stream);

/* ------------------------------------------------------------------------------------------------ rows 11-13: loss
 * FOCALLoss.forward (models/loss.py:139-218): 2 InfoNCE families on the shared / private halves, orthogonality,
 * temporal ranking.  feats / dfeats are HOST arrays of 2*n_mod device pointers, view-major
 * ([view0 mod0, view0 mod1, .., view1 mod0, ..]), each fp32 [B, dim]; B = b*seq whole subsequences.
 * terms (device fp32[5]) = {shared, private, orth, rank, weighted total}; dfeats receive d total / d feat.
 * Limit: n_mod <= 4 (the problem tables of the head's grouped launches travel as kernel arguments: n_mod^2 <= 16 InfoNCE problems and
 * n_mod (n_mod + 1) <= 20 orthogonality problems fit the 4 KB argument segment; a fifth modality is rejected with FOCAL_EINVAL
 * "too many modality pairs" -- the reference's datasets have 2 (MOD) and the authored HAR4 config 4). */
typedef struct {
  int n_mod, B, dim, seq;
  float temperature, margin;
  float w_shared, w_private, w_orth, w_rank;
  int no_private;  /* args.tag == "noPrivate": shared InfoNCE on the full features (loss.py:163-170) */
} focal_loss_desc;
size_t focal_loss_head_workspace(const focal_loss_desc* d);
int focal_loss_head(const focal_loss_desc* d, const float* const* feats, float* terms, float* const* dfeats,
                    void* workspace, size_t workspace_bytes, void* stream);
/* The same loss evaluated by `world` data-parallel ranks, each over the rows of its own samples (round 2).  `d` describes the GLOBAL
 * batch (B = world x the rank's batch, rank-major sample order as an all-gather leaves it; b = B / seq must divide by world); feats
 * are the gathered [B, dim] embeddings, identical on every rank.  Every cross-sample matrix of the loss is symmetric and a sample's
 * gradient needs only its own row of it, so rank r computes 1 / world of every product and row pass:
 *   _shard_a   zeroes dfeats / terms, evaluates the similarity rows, log-sum-exps, distances, block means and hinges of the rank's
 *              rows and the orthogonality term, and writes what other ranks need of them -- lse of its rows, diagonal block means,
 *              its partial loss terms -- into `chunk` (focal_loss_head_exchange_floats(d, world) floats);
 *   (caller)   all-gathers the chunks in rank order -> `chunks` [world][that many floats]   (the ONE collective of the head: ~70 KB);
 *   _shard_b   finishes: coefficient rows, dL/dz of the rank's own samples into their rows of dfeats (other rows stay zero), and the
 *              global terms[5] (sum of the partial terms).
 * Same workspace in both calls (focal_loss_head_workspace(d) bytes), untouched in between.  focal_loss_head is world = 1. */
size_t focal_loss_head_exchange_floats(const focal_loss_desc* d, int world);
int focal_loss_head_shard_a(const focal_loss_desc* d, int rank, int world, const float* const* feats, float* terms,
                            float* const* dfeats, float* chunk, void* workspace, size_t workspace_bytes, void* stream);
int focal_loss_head_shard_b(const focal_loss_desc* d, int rank, int world, const float* const* feats, float* terms,
                            float* const* dfeats, const float* chunks, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------ row 14: AdamW
 * torch.optim.AdamW (train_utils/optimizer.py:27-32) over `nseg` contiguous fp32 segments (the parameter arena's
 * trainable region; grad-less parameters are simply not listed, which is how torch skips them).  lr comes from a
 * device scalar and the step count from rng_state[1] (1-based after focal_rng_advance) so a captured graph stays
 * valid across epochs.  shadow (nullable) receives the bf16 copy of the updated weights for the matrix cores. */
typedef struct { float beta1, beta2, eps, weight_decay; int l2_decay; /* 0: decoupled decay (torch.optim.AdamW); 1: L2 form, g += wd * p (torch.optim.Adam, the finetune optimizer) */ } focal_adamw_desc;
int focal_adamw_multi(const focal_adamw_desc* d, int nseg, float* const* p, const float* const* g, float* const* m,
                      float* const* v, void* const* shadow_bf16, const long* n, const float* lr_dev,
                      const uint32_t* rng_state, void* stream);
/* The same update with the step's bookkeeping folded in: the step count used is step_state[1] + 1, and the workgroup that finishes last
 * advances step_state (as focal_rng_advance would have before the call) and, when non-NULL, seed_state (the dropout seed words of the
 * next forward pass) -- two one-thread launches less on the serial tail of every step.  step_state holds FOCAL_STEP_STATE_WORDS
 * 32-bit words: {seed, step count, ticket, -, -, -, -, -, 32 group tickets}; the tickets are zero between calls; step_state_words = the
 * length of the caller's buffer, checked against FOCAL_STEP_STATE_WORDS (the 4-word state of focal_rng_advance has the same pointer
 * type and would be written out of bounds).  seed_state: the 4 words of focal_rng_advance. */
#define FOCAL_STEP_STATE_WORDS 40
int focal_adamw_multi_advance(const focal_adamw_desc* d, int nseg, float* const* p, const float* const* g, float* const* m,
                              float* const* v, void* const* shadow_bf16, const long* n, const float* lr_dev,
                              uint32_t* step_state, int step_state_words, uint32_t* seed_state, void* stream);
/* Gradient clipping by global L2 norm (torch.nn.utils.clip_grad_norm_(params, max_norm, 2.0) between backward and the update), in two
 * launches and without a host read.
 *   focal_grad_norm_multi: one pass over up to FOCAL_CLIP_MAX_SEGMENTS gradient segments (lengths multiples of 4, as above).  At most
 *     FOCAL_CLIP_MAX_BLOCKS workgroups of 256 lanes, one float4 per lane and trip of the grid-stride loop; workgroup b stores its sum
 *     of squares into partials[b], the slots behind the grid are stored as zero: all FOCAL_CLIP_SCRATCH_WORDS words are written by
 *     every call, in a fixed summation order (no atomics: the row is bit-repeatable).
 *   focal_adamw_clip_multi / _advance: focal_adamw_multi / _advance on g * coef, coef = min(1, max_norm / (total_norm + 1e-6)) in
 *     fp32, total_norm = sqrt(sum of the partials) -- every workgroup re-sums the row in the same order.  g * coef is rounded once
 *     before anything is added to it: the result is bit-identical to the plain update on pre-scaled gradients, and to the plain
 *     update on g when total_norm + 1e-6 <= max_norm (coef is then exactly 1; torch's formula, which already scales by
 *     max_norm / (max_norm + 1e-6) at total_norm == max_norm, is kept as it is).  max_norm = +inf clips nothing and still records.
 *     A non-finite total_norm SKIPS the step (clip_grad_norm_ would write NaN into every weight): p, m, v, shadow and the step count
 *     stay as they are; the _advance form still advances seed_state.
 *   record: FOCAL_CLIP_RECORD_WORDS 32-bit words, updated once per call (by the launch of the last non-empty segment), zeroed by the
 *     reader: {u32 steps, u32 clipped steps, u32 skipped steps, f32 sum of the finite norms, f32 largest finite norm, f32 last norm,
 *     f32 last sum of squares, f32 last coef (0 on a skipped step)}. */
#define FOCAL_CLIP_MAX_SEGMENTS 8
#define FOCAL_CLIP_MAX_BLOCKS 1024
#define FOCAL_CLIP_SCRATCH_WORDS 1024
#define FOCAL_CLIP_RECORD_WORDS 8
int focal_grad_norm_multi(int nseg, const float* const* g, const long* n, float* partials, int partial_words, void* stream);
int focal_adamw_clip_multi(const focal_adamw_desc* d, int nseg, float* const* p, const float* const* g, float* const* m,
                           float* const* v, void* const* shadow_bf16, const long* n, const float* lr_dev,
                           const uint32_t* rng_state, const float* partials, int partial_words, uint32_t* record, int record_words,
                           float max_norm, void* stream);
int focal_adamw_clip_multi_advance(const focal_adamw_desc* d, int nseg, float* const* p, const float* const* g, float* const* m,
                                   float* const* v, void* const* shadow_bf16, const long* n, const float* lr_dev,
                                   uint32_t* step_state, int step_state_words, uint32_t* seed_state, const float* partials,
                                   int partial_words, uint32_t* record, int record_words, float max_norm, void* stream);
/* LAMB (You et al. 2020, Algorithm 2) with AdamW's conventions -- the same bias correction, the same place for eps, the same device lr
 * scalar and step count, the same m / v state --: per tensor T of the arena
 *     m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  r = (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps);  u = r + lambda_T w
 *     phi_T = |w_T| / |u_T| if T is adapted and both norms are positive and finite, else 1;  phi_T = min(phi_T, max_trust)
 *     w -= lr phi_T u
 * in two launches per segment over one grid, a workgroup per PIECE (at most FOCAL_LAMB_PIECE elements inside one tensor's padded extent):
 * the first writes m, v and the piece's sum(w^2), sum(u^2) to partials[2 piece], [2 piece + 1]; in the second every workgroup adds its
 * tensor's partials in one fixed order, forms phi_T and writes w and the bf16 shadow.  Plain stores, no floating-point atomics: bit-repeatable.
 * g is not written.  d->weight_decay is lambda of the decayed tensors; d->l2_decay must be 0.
 *   table: host = 4 * npieces + 4 * ntensors 32-bit words, {offset, length, tensor, 0} per piece (elements from the segment's start; lengths
 *     positive multiples of 4 up to FOCAL_LAMB_PIECE, offsets multiples of 4, ascending, not overlapping, inside the segment), then
 *     {first piece, last piece (exclusive), flags, 0} per tensor (the ranges partition the pieces in order; flags: 1 adapted, 2 decayed).
 *     All of this is checked on `host` before a launch; dev = the same words in device memory (16-byte aligned), which the kernels read.
 *   partials: 2 * npieces floats of scratch; record: FOCAL_LAMB_RECORD_WORDS floats per tensor, {phi_T, |w_T| before the update, |u_T|},
 *     one writer per tensor and call.
 *   clip_partials / clip_record (both null: no clipping): the row focal_grad_norm_multi left and the record of focal_adamw_clip_multi, with
 *     the same meaning: the update runs on g * coef, a non-finite norm leaves w, m, v, the shadow, the LAMB record and the step count alone
 *     and counts a skipped step.
 *   _advance: the step count used is step_state[1] + 1 and the second launch of the last non-empty segment advances step_state and
 *     seed_state, exactly as focal_adamw_multi_advance does. */
#define FOCAL_LAMB_PIECE 8192
#define FOCAL_LAMB_RECORD_WORDS 3
typedef struct { const int32_t* host; const int32_t* dev; int npieces, ntensors; float* partials; int partial_words; float* record; int record_words; } focal_lamb_table;
int focal_lamb_multi(const focal_adamw_desc* d, int nseg, float* const* p, const float* const* g, float* const* m, float* const* v,
                     void* const* shadow_bf16, const long* n, const focal_lamb_table* tables, float max_trust, const float* lr_dev,
                     const uint32_t* rng_state, const float* clip_partials, int clip_partial_words, uint32_t* clip_record,
                     int clip_record_words, float max_norm, void* stream);
int focal_lamb_multi_advance(const focal_adamw_desc* d, int nseg, float* const* p, const float* const* g, float* const* m,
                             float* const* v, void* const* shadow_bf16, const long* n, const focal_lamb_table* tables, float max_trust,
                             const float* lr_dev, uint32_t* step_state, int step_state_words, uint32_t* seed_state,
                             const float* clip_partials, int clip_partial_words, uint32_t* clip_record, int clip_record_words,
                             float max_norm, void* stream);
/* fp32 -> bf16 cast of a weight segment (refreshing the shadow after load_state_dict) */
int focal_cast_bf16(const float* src, void* dst, long n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FOCAL_HIP_H */
