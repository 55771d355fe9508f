// Linear probe on un-projected backbone features (train_utils/linear_probe.py: GpuLinearProbe, src/eval_linear.py): the objective and the
// gradient of softmax regression for R regularisation strengths at once.  Problem r holds W_r [C, D], b_r [C] and lambda_r; all problems
// are ONE matrix w [R*C, D] with b [R*C], the layout focal_kmeans_assign walks for R restarts.  One evaluation is three launches --
// forward, accumulate, finish -- with no floating-point atomic in any of them.
//
// focal_probe_forward: kmeans_assign_kernel's product with the centroids replaced by the weight rows.  A workgroup owns KNN_BQ = 128 rows
// of x and walks ALL R*C weight rows in tiles of KNN_BT = 64: the product of knn_dist.hpp's PairTile, z = x.w + b written to its LDS tile
// and no further.  One thread per row scans the tile's columns in order; column j belongs to problem j / C, so the thread
// carries the problem's running (max, sum of exp, z_y, argmax) and closes the problem when the column counter reaches C -- whether or not
// a tile boundary fell inside it.  The softmax of a closed problem is a second pass over its C logits: those of this tile from LDS, those
// of the tile before (C <= 64: never more than one) from g, where the same thread parked them when that tile ended.
// focal_probe_grad: a workgroup owns one of `slices` contiguous row slices, 64 columns of D and 64 rows of R*C; g^T x of the slice is the
// same MFMA with both operands read k-major from LDS blocks of 32 rows, rows in index order.  Partials [slices, R*C, D] are summed in
// slice order by the finishing launch, which adds lambda_r W_r, divides by n and reduces ce and |W_r|^2 (fp32 terms, double sums, a fixed
// tree) into f.  Same arguments -> same bits; a problem's outputs are functions of its own rows of w, b and lambda.
#include "knn_dist.hpp"

#define PROBE_MAX_C 64
#define PROBE_MAX_RC 1024
constexpr int PG_TILE = 64;   // rows of R*C and columns of D per accumulate workgroup
constexpr int PG_ROWS = 32;   // rows of x per staged block (8 k-steps of the 16x16x4 product)
constexpr int PG_PITCH = 80;  // LDS pitch of both blocks: 80 % 32 == 16, so the k-major ds_read_b32 of lanes l and l + 16 miss each other

__global__ __launch_bounds__(256) void probe_forward_kernel(const focal_probe_desc d, const float* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ b, const int* __restrict__ y, float* __restrict__ ce,
                                                            float* g, int* __restrict__ preds) {
  __shared__ PairTile::Lds lds;  // (the logits tile is its d2; its qsq is not used)
  constexpr int DP = PairTile::DP;
  float* zs = lds.d2;

  const int tid = threadIdx.x;
  const int D = d.D, C = d.C, RC = d.R * d.C, n = d.n;
  const int q0 = (int)blockIdx.x * KNN_BQ;
  const int q_ext = n - q0;
  const float* qb = x + (long)q0 * D;

  // the scan's state: the problem and the class within it of the next column (the same in every thread), and the row's running softmax
  const float NEG_INF = __uint_as_float(0xFF800000u), QNAN = __uint_as_float(0x7FC00000u);
  const bool live = tid < KNN_BQ && tid < q_ext;
  const int lab = (live && y) ? y[q0 + tid] : -1;
  int cur_r = 0, cur_c = 0, arg = 0;
  float m = NEG_INF, s = 0.f, zy = 0.f, bz = QNAN;
  float* grow = g ? g + (long)(q0 + (live ? tid : 0)) * RC : nullptr;

  const int nT = (RC + KNN_BT - 1) / KNN_BT;
  PairTile pt(lds, qb, D, q_ext);
  auto load = [&](int ti, int ks) { pt.load(w, 0, RC, ti, ks); };
  load(0, 0);
  for (int ti = 0; ti < nT; ++ti) {
    f32x4 acc[2][4];
    pt.product(acc, ti, nT, load);
    // the logits tile, in the place and under the barriers of PairTile::write_d2
    const int t0 = ti * KNN_BT;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int tc = pt.col(j);
      const float bias = (t0 + tc < RC) ? b[t0 + tc] : 0.f;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) zs[pt.row(i, r) * DP + tc] = acc[i][j][r] + bias;
    }
    __syncthreads();
    if (tid < KNN_BQ) {
      const int valid = RC - t0 < KNN_BT ? RC - t0 : KNN_BT;
      const float* row = zs + tid * DP;
      for (int col = 0; col < valid; ++col) {
        const float z = row[col];
        if (z > m) {  // (a NaN logit: the sum and with it ce become NaN; m stays a number)
          s = s * expf(m - z) + 1.0f;
          m = z;
        } else {
          s += expf(z - m);
        }
        if (cur_c == lab) zy = z;
        if (z == z && (!(bz == bz) || z > bz)) {  // ties to the smallest class; a NaN never beats a number
          bz = z;
          arg = cur_c;
        }
        if (++cur_c == C) {  // the problem's last column
          const float lse = m + logf(s);
          const long o = (long)cur_r * n + q0 + tid;
          if (live) {
            if (ce) ce[o] = lse - zy;
            if (preds) preds[o] = arg;
            if (g) {
              float* gp = grow + cur_r * C;
              const int first = col + 1 - C;  // the problem's first column within this tile; negative: it began in the tile before
              for (int c = 0; c < C; ++c) {
                const float zc = first + c >= 0 ? row[first + c] : gp[c];
                gp[c] = expf(zc - lse) - (c == lab ? 1.0f : 0.0f);
              }
            }
          }
          m = NEG_INF; s = 0.f; zy = 0.f; bz = QNAN; arg = 0;
          cur_c = 0;
          ++cur_r;
        }
      }
      if (g && live && cur_c > 0 && ti + 1 < nT) {  // an open problem: its logits of this tile wait in g for the tile that closes it
        float* gp = grow + cur_r * C;
        for (int c = 0; c < cur_c; ++c) gp[c] = row[valid - cur_c + c];
      }
    }
  }
}

// grid (slices, ceil(D / 64), ceil(R*C / 64)); wave w owns the tile's columns 16 w .. 16 w + 15 of D and all of its rows of R*C
__global__ __launch_bounds__(256) void probe_accum_kernel(const focal_probe_desc d, const float* __restrict__ x, const float* __restrict__ g,
                                                          float* __restrict__ part, float* __restrict__ part_b) {
  __shared__ __attribute__((aligned(16))) float gs[PG_ROWS * PG_PITCH];
  __shared__ __attribute__((aligned(16))) float xs[PG_ROWS * PG_PITCH];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D = d.D, n = d.n, RC = d.R * d.C;
  const int s = blockIdx.x, col0 = blockIdx.y * PG_TILE, rc0 = blockIdx.z * PG_TILE;
  const int rc_ext = RC - rc0 < PG_TILE ? RC - rc0 : PG_TILE;
  const long per = ((long)n + d.slices - 1) / d.slices;
  const long lo_l = (long)s * per < (long)n ? (long)s * per : (long)n;
  const int lo = (int)lo_l, hi = (int)(lo_l + per < (long)n ? lo_l + per : (long)n);
  const bool tally = blockIdx.y == 0;  // the column sums of g do not depend on the chunk of D: its first workgroup takes them

  f32x4 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;

  // the next block's global loads wait in registers while this one is multiplied
  float4 xr[2];
  float gr[8];
  auto load = [&](int i0) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {  // x: 16 threads x 16 bytes per row (D % 4 == 0: a float4 lies inside the row or past it)
      const int idx = tid + 256 * p, rr = idx >> 4, cc = (idx & 15) * 4;
      xr[p] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (i0 + rr < hi && col0 + cc < D) xr[p] = *reinterpret_cast<const float4*>(x + (long)(i0 + rr) * D + col0 + cc);
    }
#pragma unroll
    for (int p = 0; p < 8; ++p) {  // g: a row's R*C floats carry no alignment, one float per thread
      const int idx = tid + 256 * p, rr = idx >> 6, cc = idx & 63;
      gr[p] = (i0 + rr < hi && cc < rc_ext) ? g[(long)(i0 + rr) * RC + rc0 + cc] : 0.f;
    }
  };
  if (lo < hi) load(lo);
  for (int i0 = lo; i0 < hi; i0 += PG_ROWS) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int idx = tid + 256 * p, rr = idx >> 4, cc = (idx & 15) * 4;
      *reinterpret_cast<float4*>(xs + rr * PG_PITCH + cc) = xr[p];
    }
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      const int idx = tid + 256 * p, rr = idx >> 6, cc = idx & 63;
      gs[rr * PG_PITCH + cc] = gr[p];
    }
    __syncthreads();
    if (i0 + PG_ROWS < hi) load(i0 + PG_ROWS);
#pragma unroll
    for (int kk = 0; kk < PG_ROWS / 4; ++kk) {
      const int krow = (kk * 4 + (lane >> 4)) * PG_PITCH + (lane & 15);
      const float xb = xs[krow + wave * 16];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i * 16 < rc_ext) acc[i] = mma16(gs[krow + i * 16], xb, acc[i]);  // (uniform: a whole wave takes the product or skips it)
    }
    if (tally && tid < PG_TILE) {
#pragma unroll 8
      for (int k = 0; k < PG_ROWS; ++k) bsum += gs[k * PG_PITCH + tid];  // rows in index order (rows past the slice are zeros)
    }
    __syncthreads();
  }
  // acc[i][r] = row 16 i + 4 (lane >> 4) + r of the R*C chunk, column 16 wave + (lane & 15) of the D chunk
  const int col = col0 + wave * 16 + (lane & 15);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rr = i * 16 + 4 * (lane >> 4) + r;
      if (rr < rc_ext && col < D) part[((long)s * RC + rc0 + rr) * D + col] = acc[i][r];
    }
  if (tally && tid < rc_ext) part_b[(long)s * RC + rc0 + tid] = bsum;
}

// workgroups 0 .. R*C - 1: one row of gw and its gb; workgroups R*C .. R*C + R - 1: one problem's f
__global__ __launch_bounds__(256) void probe_finish_kernel(const focal_probe_desc d, const float* __restrict__ part, const float* __restrict__ part_b,
                                                           const float* __restrict__ ce, const float* __restrict__ w, const float* __restrict__ lam,
                                                           float* __restrict__ gw, float* __restrict__ gb, double* __restrict__ f) {
  __shared__ double red[256];
  const int tid = threadIdx.x, D = d.D, C = d.C, RC = d.R * d.C, n = d.n;
  const float nf = (float)n;
  if ((int)blockIdx.x < RC) {
    const int rk = blockIdx.x;
    const float l = lam[rk / C];
    for (int col = tid; col < D; col += 256) {
      float sum = 0.f;
#pragma unroll 8
      for (int s = 0; s < d.slices; ++s) sum += part[((long)s * RC + rk) * D + col];  // (the loads of 8 slices in flight; the adds in slice order)
      gw[(long)rk * D + col] = fmaf(l, w[(long)rk * D + col], sum / nf);
    }
    if (tid == 0) {
      float sum = 0.f;
      for (int s = 0; s < d.slices; ++s) sum += part_b[(long)s * RC + rk];
      gb[rk] = sum / nf;
    }
    return;
  }
  const int r = (int)blockIdx.x - RC;
  double a = 0.0, q = 0.0;
  const float* cr = ce + (long)r * n;
  // eight loads in flight, the adds in index order (an element past the end adds an exact zero)
  for (long i0 = tid; i0 < n; i0 += 256 * 8) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = i0 + 256 * k < n ? cr[i0 + 256 * k] : 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) a += (double)v[k];
  }
  const float* wr = w + (long)r * C * D;
  for (long i0 = tid; i0 < C * D; i0 += 256 * 8) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = i0 + 256 * k < C * D ? wr[i0 + 256 * k] : 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) q += (double)(v[k] * v[k]);
  }
  red[tid] = a / (double)n + 0.5 * (double)lam[r] * q;
  __syncthreads();
#pragma unroll
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) f[r] = red[0];
}

static int probe_check_desc(const focal_probe_desc* d, const char* who) {
  FOCAL_CHECK_ARG(d, "%s: null descriptor", who);
  FOCAL_CHECK_ARG(d->D >= 4 && d->D % 4 == 0, "%s: need D >= 4 and D %% 4 == 0 (got D=%d)", who, d->D);
  FOCAL_CHECK_ARG(d->C >= 2 && d->C <= PROBE_MAX_C, "%s: need 2 <= C <= %d (got C=%d)", who, PROBE_MAX_C, d->C);
  FOCAL_CHECK_ARG(d->R >= 1 && (long)d->R * d->C <= PROBE_MAX_RC, "%s: need R >= 1 and R * C <= %d (got R=%d C=%d)", who, PROBE_MAX_RC,
                  d->R, d->C);
  FOCAL_CHECK_ARG(d->n >= 1 && d->slices >= 1 && d->slices <= 65535, "%s: need n >= 1 and 1 <= slices <= 65535 (got n=%d slices=%d)", who,
                  d->n, d->slices);
  return FOCAL_OK;
}

extern "C" int focal_probe_forward(const focal_probe_desc* d, const float* x, const float* w, const float* b, const int* y, float* ce, float* g,
                                   int* preds, void* stream) {
  const int rc = probe_check_desc(d, "probe_forward");
  if (rc != FOCAL_OK) return rc;
  FOCAL_CHECK_ARG(x && w && b, "probe_forward: null tensor");
  FOCAL_CHECK_ARG(ce || g || preds, "probe_forward: no output asked for");
  FOCAL_CHECK_ARG(y || !(ce || g), "probe_forward: ce and g need the labels");
  FOCAL_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)w & 15) == 0, "probe_forward: x and w must be 16-byte aligned");
  FOCAL_LAUNCH(probe_forward_kernel, dim3((unsigned)ceil_div(d->n, KNN_BQ)), dim3(256), 0, (hipStream_t)stream, *d, x, w, b, y, ce, g, preds);
  FOCAL_LAUNCH_CHECK();
  return FOCAL_OK;
}

extern "C" size_t focal_probe_grad_workspace(const focal_probe_desc* d) {
  if (probe_check_desc(d, "probe_grad_workspace") != FOCAL_OK) return 0;
  const size_t RC = (size_t)d->R * d->C;
  return ((size_t)d->slices * RC * d->D + (size_t)d->slices * RC) * 4;
}

extern "C" int focal_probe_grad(const focal_probe_desc* d, const float* x, const float* g, const float* ce, const float* w, const float* lam,
                                float* gw, float* gb, double* f, void* ws, size_t ws_bytes, void* stream) {
  const int rc = probe_check_desc(d, "probe_grad");
  if (rc != FOCAL_OK) return rc;
  FOCAL_CHECK_ARG(x && g && ce && w && lam && gw && gb && f && ws, "probe_grad: null tensor");
  FOCAL_CHECK_ARG(((uintptr_t)x & 15) == 0, "probe_grad: x must be 16-byte aligned");
  FOCAL_CHECK_ARG(ws_bytes >= focal_probe_grad_workspace(d), "probe_grad: workspace of %zu bytes, need %zu", ws_bytes,
                  focal_probe_grad_workspace(d));
  const int RC = d->R * d->C;
  float* part = (float*)ws;
  float* part_b = part + (size_t)d->slices * RC * d->D;
  const dim3 grid((unsigned)d->slices, (unsigned)ceil_div(d->D, PG_TILE), (unsigned)ceil_div(RC, PG_TILE));
  FOCAL_LAUNCH(probe_accum_kernel, grid, dim3(256), 0, (hipStream_t)stream, *d, x, g, part, part_b);
  FOCAL_LAUNCH_CHECK();
  FOCAL_LAUNCH(probe_finish_kernel, dim3((unsigned)(RC + d->R)), dim3(256), 0, (hipStream_t)stream, *d, part, part_b, ce, w, lam, gw, gb, f);
  FOCAL_LAUNCH_CHECK();
  return FOCAL_OK;
}
