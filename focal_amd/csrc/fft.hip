// Real-input full-spectrum DFT along the last axis, packed as [B, 2C, I, n] (Re / Im channel pairs), fp32.
// n = n1 * n2 four-step DFT held entirely in LDS by one workgroup per row:
//   X[k1 + n1*k2] = sum_{m2} W_{n2}^{m2 k2} * ( W_n^{m2 k1} * sum_{m1} x[n2*m1 + m2] W_{n1}^{m1 k1} )
// (m = n2*m1 + m2, k = k1 + n1*k2).  For the MOD audio rows n = 1600 = 40 x 40; n2 = 1 degenerates to the direct
// DFT used for the 20-point seismic rows.  The twiddle table holds {cos, -sin}(2 pi j / n), j < n, computed in
// fp64 on the host.
#include <stdlib.h>
#include "common.hpp"

// View augmentations that commute with (or fold into) the transform, applied while the rows are staged / stored instead of as
// separate passes over the window (the reference data_augmenter package): scaling / negation (x * a), horizontal flip (intervals and samples
// reversed), interval permutation, and the frequency-domain phase shift (every bin rotated by one angle).
// plan != NULL (round 5): the values come from that device record instead -- focal_view_draw wrote it earlier in the same stream, so
// a captured step draws a fresh view on every replay -- and when the record says the view is warped the rows are read from x_alt.
struct AugParams {
  float scale, pc, ps;
  int flip, use_perm;
  int perm[FOCAL_AUG_MAX_INTERVALS];
  const focal_view_plan* plan;
  const float* x_alt;
};
static AugParams aug_identity() {
  AugParams a;
  memset(&a, 0, sizeof(a));
  a.scale = 1.f; a.pc = 1.f;
  return a;
}
// The augmentation a kernel applies, resolved once per workgroup: from the kernel arguments, or from the device plan.  The interval
// permutation goes to LDS (s_perm, FOCAL_AUG_MAX_INTERVALS ints; the caller's next __syncthreads() publishes it).
struct AugLive {
  float scale, pc, ps;
  int flip, use_perm;
  const float* x;
};
__device__ __forceinline__ AugLive aug_resolve(const AugParams& a, const float* x, int* s_perm, int tid) {
  AugLive v{a.scale, a.pc, a.ps, a.flip, a.use_perm, x};
  if (a.plan != nullptr) {  // (uniform)
    const focal_view_plan* pl = a.plan;
    v.scale = pl->aug.scale; v.pc = pl->aug.phase_cos; v.ps = pl->aug.phase_sin;
    v.flip = pl->aug.flip != 0; v.use_perm = pl->aug.use_perm != 0;
    if (focal_plan_warp(pl) != 0) v.x = a.x_alt;
    if (tid < FOCAL_AUG_MAX_INTERVALS) s_perm[tid] = pl->aug.perm[tid];
  } else if (tid < FOCAL_AUG_MAX_INTERVALS) {
    s_perm[tid] = a.perm[tid];
  }
  return v;
}
// source row of output row `row` = (bc, i)
__device__ __forceinline__ int aug_src_row(const AugLive& a, const int* s_perm, int row, int I) {
  const int i = row % I, bc = row / I;
  int j = a.use_perm ? s_perm[i] : i;
  if (a.flip) j = I - 1 - j;
  return bc * I + j;
}


// ---- jitter / channel shuffle / time mask / freq mask (include/focal_hip.h: focal_view_extra), folded into the same two places: the
// time-domain ones while a row is staged, the bin mask where the spectrum is stored.  Every kernel (fft_kernels.inc) is compiled twice from
// one text: the plain one (the extended parts compiled out: the code it always was) behind the existing exports, and the _ex one, which
// resolves the extra once per workgroup and takes ONE uniform branch -- `any` -- between the plain arithmetic and the extended staging.
struct ExParams { const focal_view_extra* dev; int has; uint32_t salt; focal_view_extra host; };
template <bool EX> struct ExArg { int unused; };
template <> struct ExArg<true> { ExParams e; };
struct ExLive {
  float std; uint32_t key;
  int any, use_chan, tlo, thi, flo, fhi;
};
// s_chan: FOCAL_VIEW_MAX_CHANNELS ints of LDS (published by the caller's next __syncthreads(), as s_perm is).  A device record is not
// trusted: channel entries are clamped to the tensor's channels and the mask ranges to [0, n], so no value of it can move a read.
__device__ __forceinline__ ExLive ex_resolve(const ExParams& p, int C, int n, int* s_chan, int tid) {
  float sd = 0.f;
  uint32_t key = 0u;
  int uc = 0, tlo = 0, tn = 0, flo = 0, fn = 0, ch = tid;
  if (p.dev != nullptr) {  // (uniform)
    const focal_view_extra* e = p.dev;
    sd = e->jitter_std; key = e->jitter_key; uc = e->use_chan; tlo = e->tmask_lo; tn = e->tmask_n; flo = e->fmask_lo; fn = e->fmask_n;
    if (tid < FOCAL_VIEW_MAX_CHANNELS) ch = e->chan[tid];
  } else if (p.has) {
    sd = p.host.jitter_std; key = p.host.jitter_key; uc = p.host.use_chan; tlo = p.host.tmask_lo; tn = p.host.tmask_n;
    flo = p.host.fmask_lo; fn = p.host.fmask_n;
    if (tid < FOCAL_VIEW_MAX_CHANNELS) ch = p.host.chan[tid];
  }
  if (tid < FOCAL_VIEW_MAX_CHANNELS) s_chan[tid] = min(max(ch, 0), C - 1);
  ExLive v;
  v.std = sd > 0.f ? sd : 0.f;
  v.key = focal_mix32(key ^ focal_mix32(p.salt * 0x9E3779B9U + 0x85EBCA6BU));
  v.use_chan = uc != 0 && C <= FOCAL_VIEW_MAX_CHANNELS;
  v.tlo = min(max(tlo, 0), n); v.thi = v.tlo + min(max(tn, 0), n - v.tlo);
  v.flo = min(max(flo, 0), n); v.fhi = v.flo + min(max(fn, 0), n - v.flo);
  v.any = v.std > 0.f || v.use_chan || v.thi > v.tlo || v.fhi > v.flo;
  return v;
}
__device__ __forceinline__ int ex_src_row(const AugLive& a, const ExLive& ex, const int* s_perm, const int* s_chan, int row, int I, int C) {
  const int i = row % I;
  int bc = row / I;
  int j = a.use_perm ? s_perm[i] : i;
  if (a.flip) j = I - 1 - j;
  if (ex.use_chan) {
    const int c = bc % C;
    bc += s_chan[c] - c;
  }
  return bc * I + j;
}
// the Box-Muller pair of elements 2p, 2p + 1 (the formula is part of the header: tests restate it)
__device__ __forceinline__ void ex_noise_pair(uint32_t k, uint32_t p, float& z0, float& z1) {
  const float u1 = 1.0f - (focal_mix32(k + (2u * p) * 0x85EBCA6BU) >> 8) * (1.0f / 16777216.0f);
  const float u2 = (focal_mix32(k + (2u * p + 1u) * 0x85EBCA6BU) >> 8) * (1.0f / 16777216.0f);
  const float r = sqrtf(-2.0f * __logf(u1)), a = 6.283185307179586f * u2;
  z0 = r * __cosf(a);
  z1 = r * __sinf(a);
}
__device__ __forceinline__ float ex_noise(uint32_t k, uint32_t e) {
  float z0, z1;
  ex_noise_pair(k, e >> 1, z0, z1);
  return (e & 1u) ? z1 : z0;
}

// ---- matrix-core form of the same four-step DFT (n1, n2 <= 48, multiples of 8): both stages are small real GEMMs, so
// they run on the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32) instead of 6 LDS reads per complex MAC on the VALU path above.
// Two rows per workgroup iteration (2*n2 and 2*n1 are multiples of the 16-row MFMA tile):
//   stage 1   Y[(row, m2)][k1] = sum_m1 x[row][n2*m1 + m2] * W_n1[m1][k1]         A straight from global, K = n1
//   twiddle   Y *= W_n^(m2 k1), in registers; Y -> LDS as Yr / Yi [row][m2][k1]
//   stage 2   X[(row, k1)][k2] = sum_m2 Y[row][m2][k1] * W_n2[m2][k2] (complex)    K = 2*n2 over (Yr | Yi)
// Each wave owns whole 16-row tiles and walks the three 16-column pairs (re tile, im tile), so a lane always holds the
// real and imaginary part of the same element.  Output rows leave as 16-byte stores (4 consecutive k1 per lane).
typedef float f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f4 mfma4(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// N1 / N2 are compile-time: the index arithmetic below is full of divisions by them (runtime divisors cost ~40
// instructions each and dominated the first version of this kernel).
#define FFT_MULTI_MAX 8
struct FftSmallProblem { const float* x; const float* tw; float* out; int rows, I, n, rpb; AugParams aug; };  // (aug.plan / aug.x_alt as above)
struct FftSmallTable { int nprob; int wg_end[FFT_MULTI_MAX]; FftSmallProblem p[FFT_MULTI_MAX]; };
struct FftSmallProblemEx { const float* x; const float* tw; float* out; int rows, I, n, rpb; AugParams aug; int C; ExArg<true> ex; };
struct FftSmallTableEx { int nprob; int wg_end[FFT_MULTI_MAX]; FftSmallProblemEx p[FFT_MULTI_MAX]; };
static_assert(sizeof(FftSmallTableEx) <= 4096, "the problem table travels in the kernel arguments");
template <bool EX> struct FftSmallTableSel { typedef FftSmallTable type; };
template <> struct FftSmallTableSel<true> { typedef FftSmallTableEx type; };

#define FFT_EX 0
#include "fft_kernels.inc"
#undef FFT_EX
#define FFT_EX 1
#include "fft_kernels.inc"
#undef FFT_EX

template <bool EX>
static int fft_launch_t(const focal_fft_desc* d, const AugParams& aug, const ExArg<EX>& exa, const float* x, const float* twiddle, float* out,
                        void* stream) {
  FOCAL_CHECK_ARG(d && x && twiddle && out, "fft_realpack: null argument");
  FOCAL_CHECK_ARG(d->n1 >= 1 && d->n2 >= 1 && d->n1 * d->n2 == d->n, "fft_realpack: n1*n2 != n");
  const size_t sm = (size_t)5 * d->n * sizeof(float);
  FOCAL_CHECK_ARG(sm <= 64 * 1024, "fft_realpack: n=%d too long for the LDS-resident DFT", d->n);
  const int rows = d->B * d->C * d->I;
  const bool mfma_shape = (d->n1 == d->n2) && (d->n1 == 8 || d->n1 == 16 || d->n1 == 24 || d->n1 == 32 || d->n1 == 40 || d->n1 == 48);
  if (mfma_shape && rows % 2 == 0) {
    const size_t smm = (size_t)(2 * d->n + 2 * 48 * d->n1 + (d->n1 == d->n2 ? 0 : 2 * 48 * d->n2) + 4 * 48 * d->n2 + 2 * d->n) * sizeof(float);
    static size_t lds_granted = 48 * 1024;
    if (smm > lds_granted) {  // above the default dynamic-LDS grant: raise it for this kernel (160 KB per CU on gfx950)
      hipError_t e = hipSuccess;
#define FFT_ATTR(N_) if (e == hipSuccess) e = hipFuncSetAttribute(EX ? reinterpret_cast<const void*>(fft_realpack_mfma_ex_kernel<N_, N_>) : reinterpret_cast<const void*>(fft_realpack_mfma_kernel<N_, N_>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smm)
      FFT_ATTR(8); FFT_ATTR(16); FFT_ATTR(24); FFT_ATTR(32); FFT_ATTR(40); FFT_ATTR(48);
#undef FFT_ATTR
      if (e != hipSuccess) {
        focal_set_error("fft_realpack: cannot reserve %zu bytes of LDS: %s", smm, hipGetErrorString(e));
        return FOCAL_EHIP;
      }
      lds_granted = smm;
    }
    const int maxb = 1024;
    int blocks = rows / 2 < maxb ? rows / 2 : maxb;
#define FFT_GO(N_) case N_: \
      if constexpr (EX) FOCAL_LAUNCH((fft_realpack_mfma_ex_kernel<N_, N_>), dim3(blocks), dim3(256), smm, (hipStream_t)stream, x, twiddle, out, *d, rows, aug, exa); \
      else FOCAL_LAUNCH((fft_realpack_mfma_kernel<N_, N_>), dim3(blocks), dim3(256), smm, (hipStream_t)stream, x, twiddle, out, *d, rows, aug); \
      break
    switch (d->n1) { FFT_GO(8); FFT_GO(16); FFT_GO(24); FFT_GO(32); FFT_GO(40); default: FFT_GO(48); }
#undef FFT_GO
    FOCAL_LAUNCH_CHECK();
    return FOCAL_OK;
  }
  int blocks = rows < 4096 ? rows : 4096;
  if constexpr (EX) FOCAL_LAUNCH(fft_realpack_ex_kernel, dim3(blocks), dim3(256), sm, (hipStream_t)stream, x, twiddle, out, *d, rows, aug, exa);
  else FOCAL_LAUNCH(fft_realpack_kernel, dim3(blocks), dim3(256), sm, (hipStream_t)stream, x, twiddle, out, *d, rows, aug);
  FOCAL_LAUNCH_CHECK();
  return FOCAL_OK;
}
static int fft_launch(const focal_fft_desc* d, const AugParams& aug, const float* x, const float* twiddle, float* out, void* stream) {
  return fft_launch_t<false>(d, aug, ExArg<false>{0}, x, twiddle, out, stream);
}

// ---- several short transforms in one launch.  The sensor modalities' rows are 20 samples long (100 Hz x 0.2 s): a direct DFT of 400
// MACs per row, for which fft_realpack_kernel's one-workgroup-per-row form keeps 20 of 256 lanes busy, and of which a step has one
// launch per (view, modality) on its serial head -- 8 launches of ~20 us + gaps for the four-modality config.  Here a thread owns one
// output bin of one row (256 / n rows per workgroup pass), and a table in the kernel arguments maps blockIdx ranges to problems.
static int aug_params(const focal_fft_desc* d, const focal_aug_desc* a, AugParams* p) {
  *p = aug_identity();
  if (a == nullptr) return FOCAL_OK;
  p->scale = a->scale;
  p->flip = a->flip != 0;
  p->use_perm = a->use_perm != 0;
  p->pc = a->phase_cos;
  p->ps = a->phase_sin;
  if (p->use_perm) {
    FOCAL_CHECK_ARG(d->I <= FOCAL_AUG_MAX_INTERVALS, "augment_fft: %d intervals exceed the permutation table (%d)", d->I, FOCAL_AUG_MAX_INTERVALS);
    for (int i = 0; i < d->I; ++i) {
      FOCAL_CHECK_ARG(a->perm[i] >= 0 && a->perm[i] < d->I, "augment_fft: permutation entry %d out of range", a->perm[i]);
      p->perm[i] = a->perm[i];
    }
  }
  return FOCAL_OK;
}

static int ex_params(const focal_fft_problem_ex& qe, int i, ExParams* e) {
  memset(e, 0, sizeof(*e));
  e->salt = qe.noise_salt;
  if (qe.extra_dev != nullptr) {  // (what the record holds is known only when the kernel runs: include/focal_hip.h says what the kernel does with it)
    e->dev = qe.extra_dev;
    return FOCAL_OK;
  }
  if (!qe.has_extra) return FOCAL_OK;
  const focal_view_extra& x = qe.extra;
  const int C = qe.p.d.C, n = qe.p.d.n;
  FOCAL_CHECK_ARG(x.jitter_std >= 0.f, "fft_realpack_multi_ex: negative jitter std in problem %d", i);
  FOCAL_CHECK_ARG(x.tmask_lo >= 0 && x.tmask_n >= 0 && x.tmask_lo <= n && x.tmask_n <= n - x.tmask_lo, "fft_realpack_multi_ex: time mask [%d, +%d) of problem %d leaves [0, %d]", x.tmask_lo, x.tmask_n, i, n);
  FOCAL_CHECK_ARG(x.fmask_lo >= 0 && x.fmask_n >= 0 && x.fmask_lo <= n && x.fmask_n <= n - x.fmask_lo, "fft_realpack_multi_ex: freq mask [%d, +%d) of problem %d leaves [0, %d]", x.fmask_lo, x.fmask_n, i, n);
  if (x.use_chan) {
    FOCAL_CHECK_ARG(C <= FOCAL_VIEW_MAX_CHANNELS, "fft_realpack_multi_ex: %d channels exceed the channel table (%d)", C, FOCAL_VIEW_MAX_CHANNELS);
    unsigned seen = 0;
    for (int c = 0; c < C; ++c) {
      FOCAL_CHECK_ARG(x.chan[c] >= 0 && x.chan[c] < C && !(seen >> x.chan[c] & 1u), "fft_realpack_multi_ex: chan of problem %d is not a permutation of range(%d)", i, C);
      seen |= 1u << x.chan[c];
    }
  }
  e->has = 1;
  e->host = x;
  return FOCAL_OK;
}

template <bool EX>
static int fft_multi(int n, const void* probs_v, void* stream) {
  FOCAL_CHECK_ARG(n >= 1 && probs_v, "fft_realpack_multi: no problems");
  const bool no_multi = false;
  typename FftSmallTableSel<EX>::type t;
  memset(&t, 0, sizeof(t));
  auto flush = [&]() -> int {
    if (t.nprob == 0) return FOCAL_OK;
    if constexpr (EX) FOCAL_LAUNCH(fft_small_multi_ex_kernel, dim3(t.wg_end[t.nprob - 1]), dim3(256), 0, (hipStream_t)stream, t);
    else FOCAL_LAUNCH(fft_small_multi_kernel, dim3(t.wg_end[t.nprob - 1]), dim3(256), 0, (hipStream_t)stream, t);
    FOCAL_LAUNCH_CHECK();
    memset(&t, 0, sizeof(t));
    return FOCAL_OK;
  };
  for (int i = 0; i < n; ++i) {
    const focal_fft_problem* qp;
    ExArg<EX> exa;
    memset(&exa, 0, sizeof(exa));
    if constexpr (EX) {
      const focal_fft_problem_ex& qe = static_cast<const focal_fft_problem_ex*>(probs_v)[i];
      qp = &qe.p;
      if (int rc = ex_params(qe, i, &exa.e)) return rc;
    } else {
      qp = static_cast<const focal_fft_problem*>(probs_v) + i;
    }
    const focal_fft_problem& q = *qp;
    FOCAL_CHECK_ARG(q.x && q.twiddle && q.out, "fft_realpack_multi: null tensor in problem %d", i);
    FOCAL_CHECK_ARG(q.d.B > 0 && q.d.C > 0 && q.d.I > 0 && q.d.n > 0, "fft_realpack: bad shape");
    AugParams ap;
    if (int rc = aug_params(&q.d, q.has_aug ? &q.aug : nullptr, &ap)) return rc;
    if (q.plan != nullptr) {
      FOCAL_CHECK_ARG(q.x_warped != nullptr && q.d.I <= FOCAL_AUG_MAX_INTERVALS, "fft_realpack_multi: a device plan needs x_warped and at most %d intervals", FOCAL_AUG_MAX_INTERVALS);
      ap.plan = q.plan;
      ap.x_alt = q.x_warped;
    }
    if (!no_multi && q.d.n <= 64 && q.d.n2 == 1 && q.d.n1 == q.d.n) {  // short rows: the shared launch
      auto& P = t.p[t.nprob];
      if constexpr (EX) { P.C = q.d.C; P.ex = exa; }
      P.x = q.x; P.tw = q.twiddle; P.out = q.out;
      P.rows = q.d.B * q.d.C * q.d.I; P.I = q.d.I; P.n = q.d.n; P.rpb = 256 / q.d.n;
      P.aug = ap;
      int blocks = ceil_div(P.rows, P.rpb);
      if (blocks > 1024) blocks = 1024;
      t.wg_end[t.nprob] = (t.nprob ? t.wg_end[t.nprob - 1] : 0) + blocks;
      if (++t.nprob == FFT_MULTI_MAX)
        if (int rc = flush()) return rc;
    } else if (int rc = fft_launch_t<EX>(&q.d, ap, exa, q.x, q.twiddle, q.out, stream)) {
      return rc;
    }
  }
  return flush();
}

extern "C" int focal_fft_realpack_multi(int n, const focal_fft_problem* probs, void* stream) { return fft_multi<false>(n, probs, stream); }
extern "C" int focal_fft_realpack_multi_ex(int n, const focal_fft_problem_ex* probs, void* stream) { return fft_multi<true>(n, probs, stream); }

extern "C" int focal_fft_realpack_fwd(const focal_fft_desc* d, const float* x, const float* twiddle, float* out, void* stream) {
  return fft_launch(d, aug_identity(), x, twiddle, out, stream);
}

extern "C" int focal_augment_fft_fwd(const focal_fft_desc* d, const focal_aug_desc* a, const float* x, const float* twiddle, float* out,
                                     void* stream) {
  FOCAL_CHECK_ARG(d && a, "augment_fft: null descriptor");
  AugParams p = aug_identity();
  p.scale = a->scale;
  p.flip = a->flip != 0;
  p.use_perm = a->use_perm != 0;
  p.pc = a->phase_cos;
  p.ps = a->phase_sin;
  if (p.use_perm) {
    FOCAL_CHECK_ARG(d->I <= FOCAL_AUG_MAX_INTERVALS, "augment_fft: %d intervals exceed the permutation table (%d)", d->I, FOCAL_AUG_MAX_INTERVALS);
    for (int i = 0; i < d->I; ++i) {
      FOCAL_CHECK_ARG(a->perm[i] >= 0 && a->perm[i] < d->I, "augment_fft: permutation entry %d out of range", a->perm[i]);
      p.perm[i] = a->perm[i];
    }
  }
  return fft_launch(d, p, x, twiddle, out, stream);
}
