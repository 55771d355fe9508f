// Exact t-SNE of un-projected backbone features (train_utils/tsne.py: GpuTSNE, src/eval_tsne.py).  The joint-probability matrix P [n, n]
// is built once by three setup exports; one gradient-descent iteration is two launches -- focal_tsne_grad + focal_tsne_step -- that read P
// once, make no [n, n] temporary, use no floating-point atomic and read nothing on the host.
//
// focal_tsne_dist: d2 [n, n] by knn_dist.hpp's PairTile, one tile (128 rows x 64 columns) per workgroup; |x_j|^2 from the vector the first
// launch filled with knn_row_norms' tree, so d2[i, j] is the bits focal_knn_search computes for the pair.  The diagonal is written as +0.
// focal_tsne_perplexity: one workgroup per row, the row's distances minus their off-diagonal minimum in LDS (n <= 32 768: 128 KiB).  64
// steps on beta, never fewer: double while no upper bound exists, bisect after; every thread carries the same (lo, beta, hi) because every
// thread adds the waves' sums in the same order.  The conditional row replaces the distances.
// focal_tsne_symmetrize: the 64 x 64 tile (a, b), a < b, and its mirror belong to one workgroup, which writes (p_j|i + p_i|j) / 2n to both:
// P is symmetric bit for bit.  sum P log P leaves as one double per tile and a one-workgroup launch adds the tiles in order.
// focal_tsne_grad: a workgroup of 8 waves owns 32 rows (4 per wave) and one of `slices` column slices, walked in chunks of 2048 columns
// whose y_j sit in LDS; lane <-> column (4 consecutive ones when n % 4 == 0: 16-byte loads of P), the next visit's P requested before this
// one's pairs are computed, 4 rows x 5 (6 with the KL term) running sums per lane, joined by a fixed xor tree.  Partials [slices][6][n].
// focal_tsne_step: ONE workgroup: Z and sum P log q in double in a fixed order, then per row the slices in slice order, the gradient,
// sklearn's gains / momentum update, |g|^2 in double, and the record.
#include <type_traits>

#include "knn_dist.hpp"

#define TSNE_MAX_N 32768
constexpr int TS_ROWS_WAVE = 4;                  // rows of P a wave carries through a slice
constexpr int TS_GRAD_THREADS = 512;             // 8 waves per gradient workgroup
constexpr int TS_ROWS = TS_GRAD_THREADS / 64 * TS_ROWS_WAVE;  // rows per gradient workgroup (32: _lib.TSNE_ROW_TILE)
constexpr int TS_CHUNK = 2048;                   // columns whose y sit in LDS at a time (16 KiB)
constexpr int TS_TILE = 64;                      // symmetrize tile
constexpr int TS_STEP_THREADS = 1024;
constexpr int TS_STEP_ROWS = 4;                  // rows a thread of the finishing launch carries together
constexpr int TS_BISECT = 64;

// ------------------------------------------------------------------------------------------------ distances
__global__ __launch_bounds__(256) void tsne_norms_kernel(const focal_tsne_desc d, const float* __restrict__ x, float* __restrict__ x_sq) {
  __shared__ float qsq_s[KNN_BQ];
  const int tid = threadIdx.x, q0 = (int)blockIdx.x * KNN_BQ, q_ext = d.n - q0;
  knn_row_norms(x + (long)q0 * d.D, d.D, q_ext, tid, qsq_s);
  __syncthreads();
  if (tid < KNN_BQ && tid < q_ext) x_sq[q0 + tid] = qsq_s[tid];
}

// grid (column tiles of 64, row tiles of 128)
__global__ __launch_bounds__(256) void tsne_dist_kernel(const focal_tsne_desc d, const float* __restrict__ x, const float* __restrict__ x_sq,
                                                        float* __restrict__ d2) {
  __shared__ PairTile::Lds lds;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D = d.D, n = d.n;
  const int t0 = (int)blockIdx.x * KNN_BT, q0 = (int)blockIdx.y * KNN_BQ;
  const int q_ext = n - q0, t_ext = n - t0;
  const float* qb = x + (long)q0 * D;

  knn_row_norms(qb, D, q_ext, tid, lds.qsq);

  // the one tile of this workgroup: tile 0 of the rows t0 .. n - 1
  PairTile pt(lds, qb, D, q_ext);
  auto load = [&](int ti, int ks) { pt.load(x, t0, n, ti, ks); };
  load(0, 0);
  f32x4 acc[2][4];
  pt.product(acc, 0, 1, load);
  float ts[4];
  pt.col_norms(ts, x_sq, t0, n);
  pt.write_d2(acc, ts);
  // rows of 64 columns leave coalesced: wave w takes rows w, w + 4, ..
  if (lane < t_ext)
    for (int r = wave; r < KNN_BQ && r < q_ext; r += 4) {
      const int gi = q0 + r, gj = t0 + lane;
      d2[(long)gi * n + gj] = gi == gj ? 0.f : lds.d2[r * PairTile::DP + lane];
    }
}

// ------------------------------------------------------------------------------------------------ perplexity
// The sums of a workgroup in an order that depends on NT alone: a wave's xor tree, then the waves in index order, added by every thread.
template <int NT> __device__ __forceinline__ void ts_block_sum2(float& a, float& b, float (*red)[NT / 64], int tid) {
#pragma unroll
  for (int w = 1; w < 64; w <<= 1) {
    a += __shfl_xor(a, w, 64);
    b += __shfl_xor(b, w, 64);
  }
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = a;
    red[1][tid >> 6] = b;
  }
  __syncthreads();
  a = 0.f;
  b = 0.f;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    a += red[0][w];
    b += red[1][w];
  }
}

template <int NT>
__global__ __launch_bounds__(NT) void tsne_perplexity_kernel(const focal_tsne_desc d, float* __restrict__ p, float* __restrict__ beta_out,
                                                             float log_perp) {
  extern __shared__ __attribute__((aligned(16))) float ts_row[];  // the row's d2 - dmin
  __shared__ float red[2][2][NT / 64];                             // two generations: one barrier per reduction
  __shared__ float min_s[NT / 64];
  const int tid = threadIdx.x, n = d.n, i = (int)blockIdx.x;
  float* row_g = p + (long)i * n;

  float dmin = __uint_as_float(0x7F800000u);
  for (int j = tid; j < n; j += NT) {
    const float v = row_g[j];
    ts_row[j] = v;
    if (j != i) dmin = fminf(dmin, v);
  }
#pragma unroll
  for (int w = 1; w < 64; w <<= 1) dmin = fminf(dmin, __shfl_xor(dmin, w, 64));
  if ((tid & 63) == 0) min_s[tid >> 6] = dmin;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) dmin = fminf(dmin, min_s[w]);
  for (int j = tid; j < n; j += NT) ts_row[j] -= dmin;  // (a thread reads back only what it wrote: no barrier)

  float beta = 1.f, lo = 0.f, hi = __uint_as_float(0x7F800000u);
  for (int step = 0; step <= TS_BISECT; ++step) {  // TS_BISECT updates of beta, then the sum at the final beta
    float sp = 0.f, sdp = 0.f;
    for (int j = tid; j < n; j += NT)
      if (j != i) {
        const float dd = ts_row[j], e = expf(-dd * beta);
        sp += e;
        sdp = fmaf(dd, e, sdp);
      }
    ts_block_sum2<NT>(sp, sdp, red[step & 1], tid);
    if (step == TS_BISECT) {
      for (int j = tid; j < n; j += NT) row_g[j] = j == i ? 0.f : expf(-ts_row[j] * beta) / sp;
      if (tid == 0) beta_out[i] = beta;
      break;
    }
    const float H = logf(sp) + beta * sdp / sp;
    const bool up = H > log_perp;  // the entropy is too high: beta is a lower bound
    const float nlo = up ? beta : lo, nhi = up ? hi : beta;
    beta = up ? (hi == __uint_as_float(0x7F800000u) ? beta * 2.f : (beta + hi) * 0.5f) : (beta + lo) * 0.5f;
    lo = nlo;
    hi = nhi;
  }
}

// ------------------------------------------------------------------------------------------------ symmetrize
// grid (T, T), T = ceil(n / 64); a workgroup with a > b has nothing to do (its mirror does both tiles) and writes a zero partial
__global__ __launch_bounds__(256) void tsne_symmetrize_kernel(const focal_tsne_desc d, float* __restrict__ p, double* __restrict__ part) {
  __shared__ float ta[TS_TILE][TS_TILE + 1];
  __shared__ float tb[TS_TILE][TS_TILE + 1];
  __shared__ double red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = d.n;
  const int a = (int)blockIdx.y, b = (int)blockIdx.x, T = (int)gridDim.x;
  if (a > b) {
    if (tid == 0) part[(long)a * T + b] = 0.0;
    return;
  }
  const int r0 = a * TS_TILE, c0 = b * TS_TILE;
  const float inv = 2.0f * (float)n;
  // ta[r][c] = p[r0 + r, c0 + c], tb[r][c] = p[c0 + r, r0 + c]  (both read along rows)
  for (int r = wave; r < TS_TILE; r += 4) {
    ta[r][lane] = (r0 + r < n && c0 + lane < n) ? p[(long)(r0 + r) * n + c0 + lane] : 0.f;
    tb[r][lane] = (c0 + r < n && r0 + lane < n) ? p[(long)(c0 + r) * n + r0 + lane] : 0.f;
  }
  __syncthreads();
  float plogp = 0.f;
  for (int r = wave; r < TS_TILE; r += 4) {
    const int gi = r0 + r, gj = c0 + lane;
    if (gi < n && gj < n) {
      const float v = gi == gj ? 0.f : (ta[r][lane] + tb[lane][r]) / inv;
      p[(long)gi * n + gj] = v;
      if (v > 0.f) plogp = fmaf(v, logf(v), plogp);
    }
    if (a != b) {
      const int mi = c0 + r, mj = r0 + lane;
      if (mi < n && mj < n) p[(long)mi * n + mj] = (ta[lane][r] + tb[r][lane]) / inv;  // (the same two addends: the same bits)
    }
  }
  double s = (double)plogp;
#pragma unroll
  for (int w = 1; w < 64; w <<= 1) s += __shfl_xor(s, w, 64);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  if (tid == 0) part[(long)a * T + b] = (a == b ? 1.0 : 2.0) * (((red[0] + red[1]) + red[2]) + red[3]);
}

// the sum of `count` doubles in an order that depends on `count` alone (one workgroup of 1024)
__device__ __forceinline__ double ts_block_sum_f64(double v, double* red, int tid) {
#pragma unroll
  for (int w = 1; w < 64; w <<= 1) v += __shfl_xor(v, w, 64);
  __syncthreads();  // (red may still be read from the previous call)
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < TS_STEP_THREADS / 64; ++w) s += red[w];
  return s;
}

__global__ __launch_bounds__(TS_STEP_THREADS) void tsne_sum_kernel(long count, const double* __restrict__ part, double* __restrict__ out) {
  __shared__ double red[TS_STEP_THREADS / 64];
  double s = 0.0;
  for (long k = threadIdx.x; k < count; k += TS_STEP_THREADS) s += part[k];
  s = ts_block_sum_f64(s, red, threadIdx.x);
  if (threadIdx.x == 0) out[0] = s;
}

// ------------------------------------------------------------------------------------------------ the gradient pass
struct TsAcc {
  float ax, ay, rx, ry, z, kl;
};

template <bool KL> __device__ __forceinline__ void ts_pair(TsAcc& a, float pij, float yix, float yiy, float yjx, float yjy, bool live) {
  const float dx = yix - yjx, dy = yiy - yjy;
  float q = 1.0f / (1.0f + fmaf(dx, dx, dy * dy));
  q = live ? q : 0.f;  // the diagonal and the columns past n
  const float pq = pij * q, q2 = q * q;
  a.ax = fmaf(pq, dx, a.ax);
  a.ay = fmaf(pq, dy, a.ay);
  a.rx = fmaf(q2, dx, a.rx);
  a.ry = fmaf(q2, dy, a.ry);
  a.z += q;
  if (KL) a.kl = fmaf(pij, live ? logf(q) : 0.f, a.kl);
}

// grid (slices, ceil(n / 32)); per = columns per slice (a multiple of 4)
template <bool KL, bool VEC>
__global__ __launch_bounds__(TS_GRAD_THREADS) void tsne_grad_kernel(const focal_tsne_desc d, int per, const float* __restrict__ y, const float* __restrict__ p,
                                                        float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float ys[2 * TS_CHUNK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = d.n;
  const int s = (int)blockIdx.x, row0 = (int)blockIdx.y * TS_ROWS + wave * TS_ROWS_WAVE;
  const long lo_l = (long)s * per < (long)n ? (long)s * per : (long)n;
  const int lo = (int)lo_l, hi = (int)(lo_l + per < (long)n ? lo_l + per : (long)n);

  float yix[TS_ROWS_WAVE], yiy[TS_ROWS_WAVE];
  TsAcc acc[TS_ROWS_WAVE];
#pragma unroll
  for (int r = 0; r < TS_ROWS_WAVE; ++r) {
    const int i = row0 + r < n ? row0 + r : n - 1;  // (a row past n: computed on the last row's y, never written)
    yix[r] = y[2 * i];
    yiy[r] = y[2 * i + 1];
    acc[r] = TsAcc{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  }
  // A lane visits the columns lo + W lane + 64 W t (W = 4 with 16-byte loads, else 1), t = 0, 1, ..: the chunks only partition that walk
  // (TS_CHUNK is a multiple of 64 W), so the P of the next visit is requested before the pairs of this one are computed -- across chunk
  // ends too -- and a wave keeps TS_ROWS_WAVE loads in flight while it works.
  constexpr int W = VEC ? 4 : 1;
  using PV = typename std::conditional<VEC, float4, float>::type;
  auto fetch = [&](PV (&pv)[TS_ROWS_WAVE], int col) {
#pragma unroll
    for (int r = 0; r < TS_ROWS_WAVE; ++r) {
      if (row0 + r < n && col < hi) pv[r] = *reinterpret_cast<const PV*>(p + (long)(row0 + r) * n + col);
      else pv[r] = PV{};
    }
  };
  PV cur[TS_ROWS_WAVE], nxt[TS_ROWS_WAVE];
  fetch(cur, lo + lane * W);
  for (int c0 = lo; c0 < hi; c0 += TS_CHUNK) {
    const int cn = hi - c0 < TS_CHUNK ? hi - c0 : TS_CHUNK;
    __syncthreads();  // the previous chunk's y has been read
    for (int t = tid; t < 2 * cn; t += TS_GRAD_THREADS) ys[t] = y[2 * (long)c0 + t];
    __syncthreads();
    for (int jj = lane * W; jj < cn; jj += 64 * W) {  // (VEC: n % 4 == 0, so c0, cn and every row's start are multiples of 4)
      const int j = c0 + jj;
      fetch(nxt, j + 64 * W);
      if constexpr (VEC) {
        const float4 ya = *reinterpret_cast<const float4*>(ys + 2 * jj), yb = *reinterpret_cast<const float4*>(ys + 2 * jj + 4);
#pragma unroll
        for (int r = 0; r < TS_ROWS_WAVE; ++r) {
          const int i = row0 + r;
          ts_pair<KL>(acc[r], cur[r].x, yix[r], yiy[r], ya.x, ya.y, j != i);
          ts_pair<KL>(acc[r], cur[r].y, yix[r], yiy[r], ya.z, ya.w, j + 1 != i);
          ts_pair<KL>(acc[r], cur[r].z, yix[r], yiy[r], yb.x, yb.y, j + 2 != i);
          ts_pair<KL>(acc[r], cur[r].w, yix[r], yiy[r], yb.z, yb.w, j + 3 != i);
        }
      } else {
        const float2 yj = *reinterpret_cast<const float2*>(ys + 2 * jj);
#pragma unroll
        for (int r = 0; r < TS_ROWS_WAVE; ++r) ts_pair<KL>(acc[r], cur[r], yix[r], yiy[r], yj.x, yj.y, j != row0 + r);
      }
#pragma unroll
      for (int r = 0; r < TS_ROWS_WAVE; ++r) cur[r] = nxt[r];
    }
  }
#pragma unroll
  for (int r = 0; r < TS_ROWS_WAVE; ++r) {
    float v[6] = {acc[r].ax, acc[r].ay, acc[r].rx, acc[r].ry, acc[r].z, acc[r].kl};
#pragma unroll
    for (int k = 0; k < (KL ? 6 : 5); ++k) {
#pragma unroll
      for (int w = 1; w < 64; w <<= 1) v[k] += __shfl_xor(v[k], w, 64);
    }
    if (lane == 0 && row0 + r < n) {
#pragma unroll
      for (int k = 0; k < (KL ? 6 : 5); ++k) part[((long)s * 6 + k) * n + row0 + r] = v[k];
    }
  }
}

// ------------------------------------------------------------------------------------------------ the finishing launch
struct TsStepArgs {
  int n, slices, want_kl, record_cap;
  float lr, momentum, exaggeration;
  const float* part;
  const double* p_log_p;
  float *y, *upd, *gains;
  double* record;
};

__global__ __launch_bounds__(TS_STEP_THREADS) void tsne_step_kernel(const TsStepArgs a) {
  __shared__ double red[TS_STEP_THREADS / 64];
  const int tid = threadIdx.x, n = a.n, S = a.slices;
  const float* __restrict__ part = a.part;
  float2* __restrict__ y2 = reinterpret_cast<float2*>(a.y);
  float2* __restrict__ u2 = reinterpret_cast<float2*>(a.upd);
  float2* __restrict__ g2v = reinterpret_cast<float2*>(a.gains);
  // The one workgroup is bound by the latency of its loads, so a thread takes TS_STEP_ROWS rows at a time, their loads issued together.
  // Z = sum_i sum_s z[s][i] and sum P log q: per row the slices in order (fp32), the rows of a thread in order (double)
  double z = 0.0, plq = 0.0;
  for (int i0 = tid; i0 < n; i0 += TS_STEP_ROWS * TS_STEP_THREADS) {
    float zi[TS_STEP_ROWS], ki[TS_STEP_ROWS];
#pragma unroll
    for (int r = 0; r < TS_STEP_ROWS; ++r) zi[r] = ki[r] = 0.f;
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int r = 0; r < TS_STEP_ROWS; ++r) {
        const int i = i0 + r * TS_STEP_THREADS;
        if (i < n) {
          zi[r] += part[((long)s * 6 + 4) * n + i];
          if (a.want_kl) ki[r] += part[((long)s * 6 + 5) * n + i];
        }
      }
#pragma unroll
    for (int r = 0; r < TS_STEP_ROWS; ++r) {
      z += (double)zi[r];
      plq += (double)ki[r];
    }
  }
  const double Z = ts_block_sum_f64(z, red, tid);
  const double PLQ = a.want_kl ? ts_block_sum_f64(plq, red, tid) : 0.0;
  const float inv_z = (float)(1.0 / Z), e = a.exaggeration;
  double g2 = 0.0;
  for (int i0 = tid; i0 < n; i0 += TS_STEP_ROWS * TS_STEP_THREADS) {
    float v[TS_STEP_ROWS][4];
    float2 yv[TS_STEP_ROWS], uv[TS_STEP_ROWS], gv[TS_STEP_ROWS];
#pragma unroll
    for (int r = 0; r < TS_STEP_ROWS; ++r) {
      const int i = i0 + r * TS_STEP_THREADS;
      v[r][0] = v[r][1] = v[r][2] = v[r][3] = 0.f;
      yv[r] = uv[r] = gv[r] = make_float2(0.f, 0.f);
      if (i < n) {
        yv[r] = y2[i];
        uv[r] = u2[i];
        gv[r] = g2v[i];
      }
    }
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int r = 0; r < TS_STEP_ROWS; ++r) {
        const int i = i0 + r * TS_STEP_THREADS;
        if (i < n) {
#pragma unroll
          for (int k = 0; k < 4; ++k) v[r][k] += part[((long)s * 6 + k) * n + i];
        }
      }
#pragma unroll
    for (int r = 0; r < TS_STEP_ROWS; ++r) {
      const int i = i0 + r * TS_STEP_THREADS;
      if (i >= n) continue;
      float yc[2] = {yv[r].x, yv[r].y}, uc[2] = {uv[r].x, uv[r].y}, gc[2] = {gv[r].x, gv[r].y};
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const float g = 4.0f * (e * v[r][c] - v[r][2 + c] * inv_z);
        float gn = (uc[c] * g < 0.f) ? gc[c] + 0.2f : gc[c] * 0.8f;
        gn = fmaxf(gn, 0.01f);
        const float u1 = a.momentum * uc[c] - a.lr * (gn * g);
        gc[c] = gn;
        uc[c] = u1;
        yc[c] += u1;
        g2 += (double)g * (double)g;
      }
      y2[i] = make_float2(yc[0], yc[1]);
      u2[i] = make_float2(uc[0], uc[1]);
      g2v[i] = make_float2(gc[0], gc[1]);
    }
  }
  if (!a.record) return;  // (uniform)
  const double G2 = ts_block_sum_f64(g2, red, tid);
  if (tid == 0) {
    const double it = a.record[0] + 1.0;
    a.record[0] = it;
    if (a.want_kl) {
      const long k = (long)a.record[1];
      if (k < a.record_cap) {
        a.record[2 + 3 * k] = it;
        a.record[3 + 3 * k] = a.p_log_p[0] - PLQ + log(Z);
        a.record[4 + 3 * k] = sqrt(G2);
      }
      a.record[1] = (double)(k + 1);
    }
  }
}

// ------------------------------------------------------------------------------------------------ exports
static int tsne_check_desc(const focal_tsne_desc* d, const char* who) {
  FOCAL_CHECK_ARG(d, "%s: null descriptor", who);
  const int rc = knn_check_tile_desc(who, d->D, d->slices, d->n, "n");  // (its grid bound holds for every n <= TSNE_MAX_N)
  if (rc != FOCAL_OK) return rc;
  FOCAL_CHECK_ARG(d->n >= 2 && d->n <= TSNE_MAX_N, "%s: need 2 <= n <= %d (got n=%d)", who, TSNE_MAX_N, d->n);
  return FOCAL_OK;
}

extern "C" int focal_tsne_dist(const focal_tsne_desc* d, const float* x, float* x_sq, float* d2, void* stream) {
  const int rc = tsne_check_desc(d, "tsne_dist");
  if (rc != FOCAL_OK) return rc;
  FOCAL_CHECK_ARG(x && x_sq && d2, "tsne_dist: null tensor");
  FOCAL_CHECK_ARG(((uintptr_t)x & 15) == 0, "tsne_dist: x must be 16-byte aligned");
  FOCAL_LAUNCH(tsne_norms_kernel, dim3((unsigned)ceil_div(d->n, KNN_BQ)), dim3(256), 0, (hipStream_t)stream, *d, x, x_sq);
  FOCAL_LAUNCH_CHECK();
  const dim3 grid((unsigned)ceil_div(d->n, KNN_BT), (unsigned)ceil_div(d->n, KNN_BQ));
  FOCAL_LAUNCH(tsne_dist_kernel, grid, dim3(256), 0, (hipStream_t)stream, *d, x, (const float*)x_sq, d2);
  FOCAL_LAUNCH_CHECK();
  return FOCAL_OK;
}

template <int NT> static int tsne_perplexity_launch(const focal_tsne_desc* d, float* p, float* beta, float log_perp, hipStream_t stream) {
  const int lds_bytes = d->n * 4;
  static std::atomic<bool> attr_set{false};
  if (!attr_set.load(std::memory_order_acquire)) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(tsne_perplexity_kernel<NT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            TSNE_MAX_N * 4) != hipSuccess) {
      focal_set_error("tsne_perplexity: cannot reserve %d bytes of LDS", TSNE_MAX_N * 4);
      return FOCAL_EHIP;
    }
    attr_set.store(true, std::memory_order_release);
  }
  FOCAL_LAUNCH(tsne_perplexity_kernel<NT>, dim3((unsigned)d->n), dim3(NT), lds_bytes, stream, *d, p, beta, log_perp);
  FOCAL_LAUNCH_CHECK();
  return FOCAL_OK;
}

extern "C" int focal_tsne_perplexity(const focal_tsne_desc* d, float perplexity, float* p, float* beta, void* stream) {
  const int rc = tsne_check_desc(d, "tsne_perplexity");
  if (rc != FOCAL_OK) return rc;
  FOCAL_CHECK_ARG(p && beta, "tsne_perplexity: null tensor");
  FOCAL_CHECK_ARG(perplexity >= 1.0f && perplexity < (float)d->n, "tsne_perplexity: need 1 <= perplexity < n (got perplexity=%g n=%d)",
                  (double)perplexity, d->n);
  const float log_perp = logf(perplexity);
  // a row of at most 4096 distances: 256 threads (several workgroups per CU); beyond: 1024 (the row's LDS leaves room for one)
  return d->n <= 4096 ? tsne_perplexity_launch<256>(d, p, beta, log_perp, (hipStream_t)stream)
                      : tsne_perplexity_launch<1024>(d, p, beta, log_perp, (hipStream_t)stream);
}

extern "C" size_t focal_tsne_symmetrize_workspace(const focal_tsne_desc* d) {
  if (tsne_check_desc(d, "tsne_symmetrize_workspace") != FOCAL_OK) return 0;
  const size_t T = (size_t)ceil_div(d->n, TS_TILE);
  return T * T * 8;
}

extern "C" int focal_tsne_symmetrize(const focal_tsne_desc* d, float* p, double* p_log_p, void* ws, size_t ws_bytes, void* stream) {
  const int rc = tsne_check_desc(d, "tsne_symmetrize");
  if (rc != FOCAL_OK) return rc;
  FOCAL_CHECK_ARG(p && p_log_p && ws, "tsne_symmetrize: null tensor");
  FOCAL_CHECK_ARG(((uintptr_t)ws & 7) == 0 && ((uintptr_t)p_log_p & 7) == 0, "tsne_symmetrize: ws and p_log_p must be 8-byte aligned");
  FOCAL_CHECK_ARG(ws_bytes >= focal_tsne_symmetrize_workspace(d), "tsne_symmetrize: workspace of %zu bytes, need %zu", ws_bytes,
                  focal_tsne_symmetrize_workspace(d));
  const int T = ceil_div(d->n, TS_TILE);
  FOCAL_LAUNCH(tsne_symmetrize_kernel, dim3((unsigned)T, (unsigned)T), dim3(256), 0, (hipStream_t)stream, *d, p, (double*)ws);
  FOCAL_LAUNCH_CHECK();
  FOCAL_LAUNCH(tsne_sum_kernel, dim3(1), dim3(TS_STEP_THREADS), 0, (hipStream_t)stream, (long)T * T, (const double*)ws, p_log_p);
  FOCAL_LAUNCH_CHECK();
  return FOCAL_OK;
}

extern "C" size_t focal_tsne_grad_workspace(const focal_tsne_desc* d) {
  if (tsne_check_desc(d, "tsne_grad_workspace") != FOCAL_OK) return 0;
  return (size_t)d->slices * 6 * (size_t)d->n * 4;
}

extern "C" int focal_tsne_grad(const focal_tsne_desc* d, const float* y, const float* p, int want_kl, void* ws, size_t ws_bytes, void* stream) {
  const int rc = tsne_check_desc(d, "tsne_grad");
  if (rc != FOCAL_OK) return rc;
  FOCAL_CHECK_ARG(y && p && ws, "tsne_grad: null tensor");
  FOCAL_CHECK_ARG(((uintptr_t)y & 7) == 0 && ((uintptr_t)p & 15) == 0, "tsne_grad: y must be 8-byte and P 16-byte aligned");
  FOCAL_CHECK_ARG(ws_bytes >= focal_tsne_grad_workspace(d), "tsne_grad: workspace of %zu bytes, need %zu", ws_bytes,
                  focal_tsne_grad_workspace(d));
  const int per = ceil_div(ceil_div(d->n, d->slices), 4) * 4;
  const dim3 grid((unsigned)d->slices, (unsigned)ceil_div(d->n, TS_ROWS));
  const bool vec = d->n % 4 == 0;
  void (*kern)(const focal_tsne_desc, int, const float*, const float*, float*) =
      want_kl ? (vec ? tsne_grad_kernel<true, true> : tsne_grad_kernel<true, false>) : (vec ? tsne_grad_kernel<false, true> : tsne_grad_kernel<false, false>);
  FOCAL_LAUNCH(kern, grid, dim3(TS_GRAD_THREADS), 0, (hipStream_t)stream, *d, per, y, p, (float*)ws);
  FOCAL_LAUNCH_CHECK();
  return FOCAL_OK;
}

extern "C" int focal_tsne_step(const focal_tsne_desc* d, const void* ws, size_t ws_bytes, const double* p_log_p, float* y, float* upd,
                               float* gains, float lr, float momentum, float exaggeration, int want_kl, double* record, int record_cap,
                               void* stream) {
  const int rc = tsne_check_desc(d, "tsne_step");
  if (rc != FOCAL_OK) return rc;
  FOCAL_CHECK_ARG(ws && y && upd && gains, "tsne_step: null tensor");
  FOCAL_CHECK_ARG(((uintptr_t)y & 7) == 0 && ((uintptr_t)upd & 7) == 0 && ((uintptr_t)gains & 7) == 0,
                  "tsne_step: y, upd and gains must be 8-byte aligned");
  FOCAL_CHECK_ARG(!want_kl || (record && p_log_p && record_cap >= 1), "tsne_step: the KL value needs p_log_p and a record of at least one entry");
  FOCAL_CHECK_ARG(!record || record_cap >= 0, "tsne_step: negative record capacity");
  FOCAL_CHECK_ARG(ws_bytes >= focal_tsne_grad_workspace(d), "tsne_step: workspace of %zu bytes, need %zu", ws_bytes,
                  focal_tsne_grad_workspace(d));
  TsStepArgs a;
  a.n = d->n; a.slices = d->slices; a.want_kl = want_kl ? 1 : 0; a.record_cap = record_cap;
  a.lr = lr; a.momentum = momentum; a.exaggeration = exaggeration;
  a.part = (const float*)ws; a.p_log_p = p_log_p; a.y = y; a.upd = upd; a.gains = gains; a.record = record;
  FOCAL_LAUNCH(tsne_step_kernel, dim3(1), dim3(TS_STEP_THREADS), 0, (hipStream_t)stream, a);
  FOCAL_LAUNCH_CHECK();
  return FOCAL_OK;
}
