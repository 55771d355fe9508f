// Real-input full-spectrum DFT along the last axis, packed as [B, 2C, I, n] (Re / Im channel pairs), fp32.
// n = n1 * n2 four-step DFT held entirely in LDS by one workgroup per row:
//   X[k1 + n1*k2] = sum_{m2} W_{n2}^{m2 k2} * ( W_n^{m2 k1} * sum_{m1} x[n2*m1 + m2] W_{n1}^{m1 k1} )
// (m = n2*m1 + m2, k = k1 + n1*k2).  For the MOD audio rows n = 1600 = 40 x 40; n2 = 1 degenerates to the direct
// DFT used for the 20-point seismic rows.  The twiddle table holds {cos, -sin}(2 pi j / n), j < n, computed in
// fp64 on the host.
#include <stdlib.h>
#include <type_traits>
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
// time-domain ones while a row is staged, the bin mask where the spectrum is stored.  Every kernel below is a template on `bool EX`:
// EX = false is the plain kernel (the extended parts compiled out, no extra in its arguments: a call without extras pays nothing), EX = true
// resolves the extra once per workgroup and takes ONE uniform branch -- `any` -- between the plain arithmetic and the extended staging.
struct ExParams { const focal_view_extra* dev; int has; uint32_t salt; focal_view_extra host; };
template <bool EX> struct AugArg : AugParams {};  // what a kernel takes: the augmentation and, for EX, the extra behind it
template <> struct AugArg<true> : AugParams { ExParams ex; };
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
struct FftSmallExtraProblem : FftSmallProblem { int C; ExParams ex; };
template <bool EX> struct FftSmallTable { int nprob; int wg_end[FFT_MULTI_MAX]; std::conditional_t<EX, FftSmallExtraProblem, FftSmallProblem> p[FFT_MULTI_MAX]; };
static_assert(sizeof(FftSmallTable<true>) <= 4096, "the problem table travels in the kernel arguments");

template <bool EX>
__global__ __launch_bounds__(256) void fft_realpack_kernel(const float* __restrict__ x_arg, const float* __restrict__ tw,
                                                           float* __restrict__ out, focal_fft_desc d, int rows, AugArg<EX> aug_arg) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ int s_perm[FOCAL_AUG_MAX_INTERVALS];
  const AugLive aug = aug_resolve(aug_arg, x_arg, s_perm, threadIdx.x);
  const float* x = aug.x;
  const int n = d.n, n1 = d.n1, n2 = d.n2;
  const int* s_chan = nullptr;
  ExLive ex{};
  if constexpr (EX) {
    __shared__ int chan_tab[FOCAL_VIEW_MAX_CHANNELS];
    ex = ex_resolve(aug_arg.ex, d.C, n, chan_tab, threadIdx.x);
    s_chan = chan_tab;
  }
  float* xs = smem;            // [n]
  float* yr = smem + n;        // [n2][n1]  stage-1 output, real
  float* yi = yr + n;          //           imag
  float* twc = yi + n;         // [n] cos
  float* tws = twc + n;        // [n] -sin
  const int tid = threadIdx.x;
  for (int i = tid; i < n; i += 256) {
    twc[i] = tw[2 * i];
    tws[i] = tw[2 * i + 1];
  }
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    __syncthreads();
    if (EX && ex.any) {  // (uniform)
      const float* xr = x + (long)ex_src_row(aug, ex, s_perm, s_chan, row, d.I, d.C) * n;
      const uint32_t e0 = (uint32_t)row * (uint32_t)n;
      for (int i = tid; i < n; i += 256) {
        float v = aug.scale * xr[aug.flip ? n - 1 - i : i];
        if (ex.std > 0.f) v += ex.std * ex_noise(ex.key, e0 + (uint32_t)i);
        xs[i] = (i >= ex.tlo && i < ex.thi) ? 0.f : v;
      }
    } else {
      const float* xr = x + (long)aug_src_row(aug, s_perm, row, d.I) * n;
      for (int i = tid; i < n; i += 256) xs[i] = aug.scale * xr[aug.flip ? n - 1 - i : i];
    }
    __syncthreads();
    // stage 1: for each m2, n1-point DFT over m1, then twiddle W_n^{m2 k1}
    for (int o = tid; o < n; o += 256) {
      const int m2 = o / n1, k1 = o % n1;
      float re = 0.f, im = 0.f;
      int ph = 0;  // (m1 * k1 mod n1) * n2 indexes W_{n1} inside the n-point table
      for (int m1 = 0; m1 < n1; ++m1) {
        const float v = xs[n2 * m1 + m2];
        re += v * twc[ph * n2];
        im += v * tws[ph * n2];
        ph += k1;
        if (ph >= n1) ph -= n1;
      }
      const int t = (m2 * k1) % n;
      const float c = twc[t], s = tws[t];
      yr[o] = re * c - im * s;
      yi[o] = re * s + im * c;
    }
    __syncthreads();
    // stage 2: for each k1, n2-point DFT over m2 -> X[k1 + n1*k2]
    const int ci = row % d.I, bc = row / d.I;  // row = (b*C + c)*I + i
    float* ore = out + ((long)(2 * bc) * d.I + ci) * n;
    float* oim = out + ((long)(2 * bc + 1) * d.I + ci) * n;
    for (int o = tid; o < n; o += 256) {
      const int k = o, k1 = k % n1, k2 = k / n1;
      float re = 0.f, im = 0.f;
      int ph = 0;  // (m2 * k2 mod n2) * n1 indexes W_{n2}
      for (int m2 = 0; m2 < n2; ++m2) {
        const float a = yr[m2 * n1 + k1], b = yi[m2 * n1 + k1];
        const float c = twc[ph * n1], s = tws[ph * n1];
        re += a * c - b * s;
        im += a * s + b * c;
        ph += k2;
        if (ph >= n2) ph -= n2;
      }
      float orr = re * aug.pc - im * aug.ps, oii = re * aug.ps + im * aug.pc;
      if (EX && k >= ex.flo && k < ex.fhi) orr = oii = 0.f;
      ore[k] = orr;
      oim[k] = oii;
    }
  }
}
// ---- matrix-core form of the four-step DFT (see above)
template <int N1, int N2, bool EX>
__global__ __launch_bounds__(256) void fft_realpack_mfma_kernel(const float* __restrict__ x_arg, const float* __restrict__ tw,
                                                                float* __restrict__ out, focal_fft_desc d, int rows, AugArg<EX> aug_arg) {
  constexpr int P = 48;  // padded tile pitch (3 x 16)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ int s_perm[FOCAL_AUG_MAX_INTERVALS];
  const AugLive aug = aug_resolve(aug_arg, x_arg, s_perm, threadIdx.x);
  const float* x = aug.x;
  constexpr int n = N1 * N2, n1 = N1, n2 = N2;
  const int* s_chan = nullptr;
  ExLive ex{};
  if constexpr (EX) {
    __shared__ int chan_tab[FOCAL_VIEW_MAX_CHANNELS];
    ex = ex_resolve(aug_arg.ex, d.C, n, chan_tab, threadIdx.x);
    s_chan = chan_tab;
  }
  float* twc = smem;                 // [n]  cos(2 pi j / n)
  float* tws = twc + n;              // [n] -sin
  float* w1c = tws + n;              // [n1][P]  W_n1[m1][k1]  (zero beyond k1 >= n1)
  float* w1s = w1c + n1 * P;
  constexpr bool same = n1 == n2;    // square factorisation (MOD audio: 40 x 40): one table serves both stages
  float* w2c = same ? w1c : w1s + n1 * P;  // [n2][P]  W_n2[m2][k2]
  float* w2s = same ? w1s : w2c + n2 * P;
  float* yr = (same ? w1s : w2s) + n2 * P;  // [2][n2][P]
  float* yi = yr + 2 * n2 * P;
  float* xs = yi + 2 * n2 * P;       // [2][n]  the two input rows of this pass
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lj = lane & 15, lg = lane >> 4;
  for (int i = tid; i < n; i += 256) { twc[i] = tw[2 * i]; tws[i] = tw[2 * i + 1]; }
  for (int i = tid; i < n1 * P; i += 256) {
    const int m = i / P, k = i % P;
    const int t = ((m * k) % n1) * n2;
    w1c[i] = k < n1 ? tw[2 * t] : 0.f;
    w1s[i] = k < n1 ? tw[2 * t + 1] : 0.f;
  }
  for (int i = tid; i < (same ? 0 : n2 * P); i += 256) {
    const int m = i / P, k = i % P;
    const int t = ((m * k) % n2) * n1;
    w2c[i] = k < n2 ? tw[2 * t] : 0.f;
    w2s[i] = k < n2 ? tw[2 * t + 1] : 0.f;
  }
  constexpr int mt1 = 2 * n2 / 16, mt2 = 2 * n1 / 16;  // 16-row tiles of stage 1 / stage 2
  // the next pass's rows are fetched (coalesced, 16 B per lane) while stage 2 of the current pass runs
  constexpr int XV = (2 * n / 4 + 255) / 256;  // float4 per thread
  float4 xn[XV];
  auto fetch = [&](int pair) {
#pragma unroll
    for (int i = 0; i < XV; ++i) {
      const int e = tid + 256 * i;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (e < 2 * n / 4 && pair < rows / 2) {
        const int rl = e / (n / 4), q = e - rl * (n / 4);
        const int srow = (EX && ex.any) ? ex_src_row(aug, ex, s_perm, s_chan, pair * 2 + rl, d.I, d.C) : aug_src_row(aug, s_perm, pair * 2 + rl, d.I);
        const float4* src = reinterpret_cast<const float4*>(x + (long)srow * n);
        if (aug.flip) {
          const float4 t = src[n / 4 - 1 - q];
          v = make_float4(t.w, t.z, t.y, t.x);
        } else {
          v = src[q];
        }
        v.x *= aug.scale; v.y *= aug.scale; v.z *= aug.scale; v.w *= aug.scale;
        if (EX && ex.any) {  // (uniform) the four elements 4q .. 4q + 3 of destination row pair * 2 + rl: two Box-Muller pairs (n % 4 == 0)
          if (ex.std > 0.f) {
            const uint32_t p0 = ((uint32_t)(pair * 2 + rl) * (uint32_t)n + 4u * (uint32_t)q) >> 1;
            float z0, z1, z2, z3;
            ex_noise_pair(ex.key, p0, z0, z1);
            ex_noise_pair(ex.key, p0 + 1u, z2, z3);
            v.x += ex.std * z0; v.y += ex.std * z1; v.z += ex.std * z2; v.w += ex.std * z3;
          }
          const int i0 = 4 * q;
          if (i0 >= ex.tlo && i0 < ex.thi) v.x = 0.f;
          if (i0 + 1 >= ex.tlo && i0 + 1 < ex.thi) v.y = 0.f;
          if (i0 + 2 >= ex.tlo && i0 + 2 < ex.thi) v.z = 0.f;
          if (i0 + 3 >= ex.tlo && i0 + 3 < ex.thi) v.w = 0.f;
        }
      }
      xn[i] = v;
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int i = 0; i < XV; ++i) {
      const int e = tid + 256 * i;
      if (e < 2 * n / 4) reinterpret_cast<float4*>(xs)[e] = xn[i];
    }
  };
  __syncthreads();  // s_perm
  fetch(blockIdx.x);
  stash();
  for (int pair = blockIdx.x; pair < rows / 2; pair += gridDim.x) {
    __syncthreads();  // tables and xs ready; previous pass done with yr / yi
    const float* x0 = xs;
    // ---- stage 1
    constexpr int np1 = (n1 + 15) / 16, np2 = (n2 + 15) / 16;  // 16-column (re, im) tile pairs
    for (int u = wave; u < mt1 * np1; u += 4) {  // unit = (16-row tile, column pair)
      const int mt = u / np1, p = u - mt * np1;
      const int f = 16 * mt + lj, row = f / n2, m2 = f - row * n2;  // this lane's A row
      const float* xa = x0 + row * n + m2;
      float a[12];
#pragma unroll
      for (int ks = 0; ks < 12; ++ks) {
        const int m1 = 4 * ks + lg;
        a[ks] = m1 < n1 ? xa[n2 * m1] : 0.f;
      }
      {
        // four independent accumulator chains (even / odd k-steps): back-to-back dependent MFMAs would wait out the
        // matrix pipe's latency on every step
        f4 re = {0.f, 0.f, 0.f, 0.f}, im = re, re2 = re, im2 = re;
#pragma unroll
        for (int ks = 0; ks < 12; ks += 2) {
          if (4 * ks >= n1) break;
          const int bi = (4 * ks + lg) * P + 16 * p + lj;
          re = mfma4(a[ks], w1c[bi], re);
          im = mfma4(a[ks], w1s[bi], im);
          if (4 * (ks + 1) < n1) {
            re2 = mfma4(a[ks + 1], w1c[bi + 4 * P], re2);
            im2 = mfma4(a[ks + 1], w1s[bi + 4 * P], im2);
          }
        }
        re += re2;
        im += im2;
        const int k1 = 16 * p + lj;
        if (k1 < n1) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int fo = 16 * mt + 4 * lg + r, ro = fo / n2, mo = fo - ro * n2;
            const int t = (mo * k1) % n;
            const float c = twc[t], sn = tws[t];
            yr[(ro * n2 + mo) * P + k1] = re[r] * c - im[r] * sn;
            yi[(ro * n2 + mo) * P + k1] = re[r] * sn + im[r] * c;
          }
        }
      }
    }
    __syncthreads();
    fetch(pair + gridDim.x);
    // ---- stage 2
    for (int u = wave; u < mt2 * np2; u += 4) {
      const int mt = u / np2, p = u - mt * np2;
      const int f = 16 * mt + lj, row = f / n1, k1 = f - row * n1;
      const float* ya = yr + row * n2 * P + k1;
      const float* yb = yi + row * n2 * P + k1;
      const int fo = 16 * mt + 4 * lg, ro = fo / n1, ko = fo - ro * n1;  // this lane's 4 output k1: ko .. ko + 3
      const int grow = pair * 2 + ro;
      const int ci = grow % d.I, bc = grow / d.I;  // row = (b*C + c)*I + i
      float* ore = out + ((long)(2 * bc) * d.I + ci) * n + ko;
      float* oim = out + ((long)(2 * bc + 1) * d.I + ci) * n + ko;
      {
        f4 re = {0.f, 0.f, 0.f, 0.f}, im = re, re2 = re, im2 = re;
#pragma unroll
        for (int ks = 0; ks < 12; ++ks) {
          if (4 * ks >= n2) break;
          const int m2 = 4 * ks + lg;
          const float ar = ya[m2 * P], ai = yb[m2 * P];
          const int bi = m2 * P + 16 * p + lj;
          const float c = w2c[bi], sn = w2s[bi];
          re = mfma4(ar, c, re);
          im = mfma4(ar, sn, im);
          re2 = mfma4(ai, -sn, re2);
          im2 = mfma4(ai, c, im2);
        }
        re += re2;
        im += im2;
        const int k2 = 16 * p + lj;
        if (k2 < n2) {
          f4 orr = re * aug.pc - im * aug.ps, oii = re * aug.ps + im * aug.pc;
          if (EX && ex.fhi > ex.flo) {  // (uniform) bins ko + r + n1 * k2
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int k = ko + r + n1 * k2;
              if (k >= ex.flo && k < ex.fhi) { orr[r] = 0.f; oii[r] = 0.f; }
            }
          }
          *reinterpret_cast<float4*>(ore + n1 * k2) = make_float4(orr[0], orr[1], orr[2], orr[3]);
          *reinterpret_cast<float4*>(oim + n1 * k2) = make_float4(oii[0], oii[1], oii[2], oii[3]);
        }
      }
    }
    stash();  // xs is free since the barrier after stage 1
  }
}
// ---- several short transforms in one launch (see fft_multi below)
template <bool EX>
__global__ __launch_bounds__(256) void fft_small_multi_kernel(const FftSmallTable<EX> t) {
  __shared__ float xs[256], twc[64], tws[64];
  const int b = blockIdx.x, tid = threadIdx.x;
  int pi = 0;
#pragma unroll
  for (int q = 0; q < FFT_MULTI_MAX - 1; ++q) pi += (q < t.nprob - 1 && b >= t.wg_end[q]) ? 1 : 0;
  const auto& P = t.p[pi];
  __shared__ int s_perm[FOCAL_AUG_MAX_INTERVALS];
  const AugLive aug = aug_resolve(P.aug, P.x, s_perm, tid);
  int Cc = 1;
  const int* s_chan = nullptr;
  ExLive ex{};
  if constexpr (EX) {
    __shared__ int chan_tab[FOCAL_VIEW_MAX_CHANNELS];
    Cc = P.C;
    ex = ex_resolve(P.ex, Cc, P.n, chan_tab, threadIdx.x);
    s_chan = chan_tab;
  }
  const int start = pi > 0 ? t.wg_end[pi - 1] : 0, nb = t.wg_end[pi] - start;
  const int n = P.n, rpb = P.rpb;
  if (tid < n) { twc[tid] = P.tw[2 * tid]; tws[tid] = P.tw[2 * tid + 1]; }
  const int r = tid / n, k = tid - r * n;
  const bool active = r < rpb;
  for (int row0 = (b - start) * rpb; row0 < P.rows; row0 += nb * rpb) {
    const int row = row0 + r;
    const bool ok = active && row < P.rows;
    __syncthreads();
    if (EX && ex.any) {  // (uniform)
      if (ok) {
        float v = aug.scale * aug.x[(long)ex_src_row(aug, ex, s_perm, s_chan, row, P.I, Cc) * n + (aug.flip ? n - 1 - k : k)];
        if (ex.std > 0.f) v += ex.std * ex_noise(ex.key, (uint32_t)row * (uint32_t)n + (uint32_t)k);
        xs[tid] = (k >= ex.tlo && k < ex.thi) ? 0.f : v;
      }
    } else if (ok) {
      xs[tid] = aug.scale * aug.x[(long)aug_src_row(aug, s_perm, row, P.I) * n + (aug.flip ? n - 1 - k : k)];
    }
    __syncthreads();
    if (!ok) continue;
    const float* xr = xs + r * n;
    float re = 0.f, im = 0.f;
    int ph = 0;  // m * k mod n
    for (int m = 0; m < n; ++m) {
      const float v = xr[m];
      re += v * twc[ph];
      im += v * tws[ph];
      ph += k;
      if (ph >= n) ph -= n;
    }
    const int ci = row % P.I, bc = row / P.I;  // row = (b*C + c)*I + i
    float orr = re * aug.pc - im * aug.ps, oii = re * aug.ps + im * aug.pc;
    if (EX && k >= ex.flo && k < ex.fhi) orr = oii = 0.f;
    P.out[((long)(2 * bc) * P.I + ci) * n + k] = orr;
    P.out[((long)(2 * bc + 1) * P.I + ci) * n + k] = oii;
  }
}

template <bool EX>
static int fft_launch_t(const focal_fft_desc* d, const AugArg<EX>& aug, const float* x, const float* twiddle, float* out, void* stream) {
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
#define FFT_ATTR(N_) if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(fft_realpack_mfma_kernel<N_, N_, EX>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smm)
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
#define FFT_GO(N_) case N_: FOCAL_LAUNCH((fft_realpack_mfma_kernel<N_, N_, EX>), dim3(blocks), dim3(256), smm, (hipStream_t)stream, x, twiddle, out, *d, rows, aug); break
    switch (d->n1) { FFT_GO(8); FFT_GO(16); FFT_GO(24); FFT_GO(32); FFT_GO(40); default: FFT_GO(48); }
#undef FFT_GO
    FOCAL_LAUNCH_CHECK();
    return FOCAL_OK;
  }
  int blocks = rows < 4096 ? rows : 4096;
  FOCAL_LAUNCH(fft_realpack_kernel<EX>, dim3(blocks), dim3(256), sm, (hipStream_t)stream, x, twiddle, out, *d, rows, aug);
  FOCAL_LAUNCH_CHECK();
  return FOCAL_OK;
}

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

static int ex_params(const focal_fft_problem& q, int i, ExParams* e) {
  memset(e, 0, sizeof(*e));
  e->salt = q.noise_salt;
  if (q.extra_dev != nullptr) {  // (what the record holds is known only when the kernel runs: include/focal_hip.h says what the kernel does with it)
    e->dev = q.extra_dev;
    return FOCAL_OK;
  }
  if (!q.has_extra) return FOCAL_OK;
  const focal_view_extra& x = q.extra;
  const int C = q.d.C, n = q.d.n;
  FOCAL_CHECK_ARG(x.jitter_std >= 0.f, "fft_realpack_multi: negative jitter std in problem %d", i);
  FOCAL_CHECK_ARG(x.tmask_lo >= 0 && x.tmask_n >= 0 && x.tmask_lo <= n && x.tmask_n <= n - x.tmask_lo, "fft_realpack_multi: time mask [%d, +%d) of problem %d leaves [0, %d]", x.tmask_lo, x.tmask_n, i, n);
  FOCAL_CHECK_ARG(x.fmask_lo >= 0 && x.fmask_n >= 0 && x.fmask_lo <= n && x.fmask_n <= n - x.fmask_lo, "fft_realpack_multi: freq mask [%d, +%d) of problem %d leaves [0, %d]", x.fmask_lo, x.fmask_n, i, n);
  if (x.use_chan) {
    FOCAL_CHECK_ARG(C <= FOCAL_VIEW_MAX_CHANNELS, "fft_realpack_multi: %d channels exceed the channel table (%d)", C, FOCAL_VIEW_MAX_CHANNELS);
    unsigned seen = 0;
    for (int c = 0; c < C; ++c) {
      FOCAL_CHECK_ARG(x.chan[c] >= 0 && x.chan[c] < C && !(seen >> x.chan[c] & 1u), "fft_realpack_multi: chan of problem %d is not a permutation of range(%d)", i, C);
      seen |= 1u << x.chan[c];
    }
  }
  e->has = 1;
  e->host = x;
  return FOCAL_OK;
}

// ---- several short transforms in one launch.  The sensor modalities' rows are 20 samples long (100 Hz x 0.2 s): a direct DFT of 400
// MACs per row, for which fft_realpack_kernel's one-workgroup-per-row form keeps 20 of 256 lanes busy, and of which a step has one
// launch per (view, modality) on its serial head -- 8 launches of ~20 us + gaps for the four-modality config.  In fft_small_multi_kernel
// a thread owns one output bin of one row (256 / n rows per workgroup pass), and a table in the kernel arguments maps blockIdx ranges
// to problems.
template <bool EX>
static int fft_multi(int n, const focal_fft_problem* probs, void* stream) {
  FftSmallTable<EX> t;
  memset(&t, 0, sizeof(t));
  auto flush = [&]() -> int {
    if (t.nprob == 0) return FOCAL_OK;
    FOCAL_LAUNCH(fft_small_multi_kernel<EX>, dim3(t.wg_end[t.nprob - 1]), dim3(256), 0, (hipStream_t)stream, t);
    FOCAL_LAUNCH_CHECK();
    memset(&t, 0, sizeof(t));
    return FOCAL_OK;
  };
  for (int i = 0; i < n; ++i) {
    const focal_fft_problem& q = probs[i];
    FOCAL_CHECK_ARG(q.x && q.twiddle && q.out, "fft_realpack_multi: null tensor in problem %d", i);
    FOCAL_CHECK_ARG(q.d.B > 0 && q.d.C > 0 && q.d.I > 0 && q.d.n > 0, "fft_realpack: bad shape");
    AugArg<EX> ap;
    if (int rc = aug_params(&q.d, q.has_aug ? &q.aug : nullptr, &ap)) return rc;
    if constexpr (EX)
      if (int rc = ex_params(q, i, &ap.ex)) return rc;
    if (q.plan != nullptr) {
      FOCAL_CHECK_ARG(q.x_warped != nullptr && q.d.I <= FOCAL_AUG_MAX_INTERVALS, "fft_realpack_multi: a device plan needs x_warped and at most %d intervals", FOCAL_AUG_MAX_INTERVALS);
      ap.plan = q.plan;
      ap.x_alt = q.x_warped;
    }
    if (q.d.n <= 64 && q.d.n2 == 1 && q.d.n1 == q.d.n) {  // short rows: the shared launch
      auto& P = t.p[t.nprob];
      if constexpr (EX) { P.C = q.d.C; P.ex = ap.ex; }
      P.x = q.x; P.tw = q.twiddle; P.out = q.out;
      P.rows = q.d.B * q.d.C * q.d.I; P.I = q.d.I; P.n = q.d.n; P.rpb = 256 / q.d.n;
      P.aug = ap;
      int blocks = ceil_div(P.rows, P.rpb);
      if (blocks > 1024) blocks = 1024;
      t.wg_end[t.nprob] = (t.nprob ? t.wg_end[t.nprob - 1] : 0) + blocks;
      if (++t.nprob == FFT_MULTI_MAX)
        if (int rc = flush()) return rc;
    } else if (int rc = fft_launch_t<EX>(&q.d, ap, q.x, q.twiddle, q.out, stream)) {
      return rc;
    }
  }
  return flush();
}

// The extended kernels run iff some problem of the call carries an extra; noise_salt alone does not ask for them.
extern "C" int focal_fft_realpack_multi(int n, const focal_fft_problem* probs, void* stream) {
  FOCAL_CHECK_ARG(n >= 1 && probs, "fft_realpack_multi: no problems");
  bool ex = false;
  for (int i = 0; i < n; ++i) ex = ex || probs[i].has_extra || probs[i].extra_dev != nullptr;
  return ex ? fft_multi<true>(n, probs, stream) : fft_multi<false>(n, probs, stream);
}

extern "C" int focal_fft_realpack_fwd(const focal_fft_desc* d, const float* x, const float* twiddle, float* out, void* stream) {
  return fft_launch_t<false>(d, AugArg<false>{aug_identity()}, x, twiddle, out, stream);
}

extern "C" int focal_augment_fft_fwd(const focal_fft_desc* d, const focal_aug_desc* a, const float* x, const float* twiddle, float* out,
                                     void* stream) {
  FOCAL_CHECK_ARG(d && a, "augment_fft: null descriptor");
  AugArg<false> p;
  if (int rc = aug_params(d, a, &p)) return rc;
  return fft_launch_t<false>(d, p, x, twiddle, out, stream);
}
