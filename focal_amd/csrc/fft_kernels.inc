// The three DFT kernels of fft.hip, included twice: FFT_EX 0 = the plain kernels behind the existing exports (the extended parts are
// compiled out: the code they always were), FFT_EX 1 = the *_ex_kernel forms that also apply a focal_view_extra.
#if FFT_EX
#define FFT_K(name) name##_ex_kernel
#define FFT_EXPARAM , ExArg<true> exa
#define FFT_TABLE FftSmallTableEx
#define FFT_EX_RESOLVE(C_, n_) __shared__ int s_chan[FOCAL_VIEW_MAX_CHANNELS]; const ExLive ex = ex_resolve(exa.e, (C_), (n_), s_chan, threadIdx.x);
#else
#define FFT_K(name) name##_kernel
#define FFT_EXPARAM
#define FFT_TABLE FftSmallTable
#define FFT_EX_RESOLVE(C_, n_) const int* s_chan = nullptr; const ExLive ex{};
#endif

__global__ __launch_bounds__(256) void FFT_K(fft_realpack)(const float* __restrict__ x_arg, const float* __restrict__ tw,
                                                           float* __restrict__ out, focal_fft_desc d, int rows, AugParams aug_arg FFT_EXPARAM) {
  constexpr bool EX = FFT_EX;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ int s_perm[FOCAL_AUG_MAX_INTERVALS];
  const AugLive aug = aug_resolve(aug_arg, x_arg, s_perm, threadIdx.x);
  const float* x = aug.x;
  const int n = d.n, n1 = d.n1, n2 = d.n2;
  FFT_EX_RESOLVE(d.C, n)
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
// ---- matrix-core form of the four-step DFT (see fft.hip)
template <int N1, int N2>
__global__ __launch_bounds__(256) void FFT_K(fft_realpack_mfma)(const float* __restrict__ x_arg, const float* __restrict__ tw,
                                                                float* __restrict__ out, focal_fft_desc d, int rows, AugParams aug_arg FFT_EXPARAM) {
  constexpr bool EX = FFT_EX;
  constexpr int P = 48;  // padded tile pitch (3 x 16)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ int s_perm[FOCAL_AUG_MAX_INTERVALS];
  const AugLive aug = aug_resolve(aug_arg, x_arg, s_perm, threadIdx.x);
  const float* x = aug.x;
  constexpr int n = N1 * N2, n1 = N1, n2 = N2;
  FFT_EX_RESOLVE(d.C, n)
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
// ---- several short transforms in one launch (see fft.hip)
__global__ __launch_bounds__(256) void FFT_K(fft_small_multi)(const FFT_TABLE t) {
  constexpr bool EX = FFT_EX;
  __shared__ float xs[256], twc[64], tws[64];
  const int b = blockIdx.x, tid = threadIdx.x;
  int pi = 0;
#pragma unroll
  for (int q = 0; q < FFT_MULTI_MAX - 1; ++q) pi += (q < t.nprob - 1 && b >= t.wg_end[q]) ? 1 : 0;
  const auto& P = t.p[pi];
  __shared__ int s_perm[FOCAL_AUG_MAX_INTERVALS];
  const AugLive aug = aug_resolve(P.aug, P.x, s_perm, tid);
#if FFT_EX
  const int Cc = P.C;
  const ExArg<true>& exa = P.ex;
#else
  const int Cc = 1;
#endif
  FFT_EX_RESOLVE(Cc, P.n)
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
#undef FFT_K
#undef FFT_EXPARAM
#undef FFT_TABLE
#undef FFT_EX_RESOLVE
