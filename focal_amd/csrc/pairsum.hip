// Sums of a function of the distance over all pairs, per query row and per group of gallery rows, for the embedding-geometry scores
// (train_utils/geometry.py: silhouette, uniformity; src/eval_geometry.py).  The [nq, nt] distances exist in LDS tiles only.
//
// focal_pair_sums walks slices of t in knn_dist.hpp's PairTile, as focal_rank_positive's scan (rank.hip) does -- d2 of a pair is the bits
// focal_knn_search produces for it -- with another epilogue, which adds f(max(d2, 0)) of every candidate to the sum of the candidate's
// group.
// Where the accumulators live (NB):
// NB = 0, group == NULL (one group, the uniformity case): two threads per query row scan 32 candidates each of the distance tile, as the
// rank kernel does, and each keeps ONE register; the halves meet once, half 0 + half 1, through the distance tile after the last tile.
// NB = 1 (G <= 16) and NB = 4 (G <= 64): the per-group sums of a tile are the product F [128, 64] x onehot [64, G], and the wave that
// owns 32 query rows takes it with the same exact-fp32 MFMA: lane (row = lane & 15, c = lane >> 4) reads 16 consecutive candidates of
// its rows from the distance tile, applies f (0 for the row's own candidate and for a candidate without a group) and feeds one per step
// as the A operand; the B operand is 1.0 where that candidate's group is the lane's column.  x * 1 and x * 0 are exact, so this IS the
// sum, in the order the MFMA adds its four k; the [128, G] accumulators are 8 NB registers per lane across all tiles.  No LDS beyond
// the search's (+ 64 ids): two workgroups per CU for every G.  (Priced and dropped: per-thread accumulators in LDS, G KiB per workgroup
// -- one workgroup per CU from G = 19 on, and a dependent read-add-write per candidate; 4 ms slower at 65 536 x 1024, G = 7.)  The 0 of an uncounted candidate is
// selected before the product, so such a candidate cannot reach a sum; a non-finite f of a COUNTED candidate makes every group's sum of
// that query row NaN (inf * 0).
// Order of the additions: fixed per tile by the lane layout, tile after tile; the slices' partials [128, G] are added in slice order by
// pairsum_reduce_kernel.  Nothing is accumulated with an atomic, so the bits are a function of (nq, nt, D, G, slices) and the inputs
// alone; another `slices` is another order and may differ in the last bits.
#include "knn_dist.hpp"

#include <cmath>

template <int FN, int NB>
__global__ __launch_bounds__(256) void pairsum_kernel(const focal_pairsum_desc d, const float* __restrict__ q, const float* __restrict__ t,
                                                      const float* __restrict__ t_sq, const int* __restrict__ group, float* __restrict__ out) {
  static_assert(NB * 16 <= FOCAL_PAIR_MAX_GROUPS, "16 groups per block of columns");
  constexpr int DP = PairTile::DP;
  constexpr int NBR = NB > 0 ? NB : 1;
  __shared__ PairTile::Lds lds;
  __shared__ __attribute__((aligned(16))) int grp_s[KNN_BT];  // the tile's group ids, -1 = not counted (NB > 0)
  float* d2s = lds.d2;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D = d.D, G = d.G;
  const int s = (int)(blockIdx.x % (unsigned)d.slices);
  const int q_tile = (int)(blockIdx.x / (unsigned)d.slices);
  const int q0 = q_tile * KNN_BQ;
  int lo, hi;
  knn_slice(d.nt, d.slices, s, lo, hi);
  const int q_ext = d.nq - q0;
  const float* qb = q + (long)q0 * D;

  knn_row_norms(qb, D, q_ext, tid, lds.qsq);
  __syncthreads();

  // NB = 0: scan state of thread (row = tid & 127, half = tid >> 7).  NB > 0: the lane's two A rows (wave * 32 + i * 16 + (lane & 15))
  const int srow = tid & (KNN_BQ - 1), shalf = tid >> 7;
  const long self_base = d.self_offset >= 0 ? (long)d.self_offset + q0 : -1L - KNN_BQ;  // (no row + self_base reaches a candidate)
  const long self_j = self_base + srow;
  float sum1 = 0.f;
  f32x4 sacc[2][NBR];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int nb = 0; nb < NBR; ++nb) sacc[i][nb] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nT = (hi - lo + KNN_BT - 1) / KNN_BT;
  PairTile pt(lds, qb, D, q_ext);
  auto load = [&](int ti, int ks) { pt.load(t, lo, hi, ti, ks); };
  if (nT > 0) load(0, 0);
  for (int ti = 0; ti < nT; ++ti) {
    // the tile's norms and group ids are asked for before the k loop, so that their latency is not paid between the loop and the epilogue
    const int t0 = lo + ti * KNN_BT;
    float ts_pre[4];
    pt.col_norms(ts_pre, t_sq, t0, hi);
    int g_pre = -1;
    if (NB > 0 && tid < KNN_BT && t0 + tid < hi) {
      g_pre = group ? group[t0 + tid] : 0;
      if (g_pre < 0 || g_pre >= G) g_pre = -1;
    }
    f32x4 acc[2][4];
    pt.product(acc, ti, nT, load);
    // the columns' groups go with the distance tile: written after the k loop's last barrier, published by write_d2's
    if (NB > 0 && tid < KNN_BT) grp_s[tid] = g_pre;
    pt.write_d2(acc, ts_pre);
    if (NB > 0) {
      // S tile [32 rows of this wave, 16 NB groups] += F [32, 64] x onehot [64, 16 NB].  The product does not care which candidate is
      // which k as long as A and B agree: lane (row = lane & 15, c = lane >> 4) owns the 16 consecutive candidates 16 c .. 16 c + 15 of
      // its rows (16-byte LDS reads) and step kk of the 16 takes candidate 16 c + kk from every lane.
      const int c16 = (lane >> 4) * 16;
      int self_col[2];  // the row's own candidate as a column of this tile, or -1
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const long sc = self_base + (wave * 32 + i * 16 + (lane & 15)) - t0;
        self_col[i] = (sc >= 0 && sc < KNN_BT) ? (int)sc : -1;
      }
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int4 gv = *reinterpret_cast<const int4*>(grp_s + c16 + 4 * m);
        const int gs[4] = {gv.x, gv.y, gv.z, gv.w};
        float fv[2][4];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const float4 v = *reinterpret_cast<const float4*>(d2s + (wave * 32 + i * 16 + (lane & 15)) * DP + c16 + 4 * m);
          fv[i][0] = v.x; fv[i][1] = v.y; fv[i][2] = v.z; fv[i][3] = v.w;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int col = c16 + 4 * m + e, g = gs[e];
          float a[2];
#pragma unroll
          for (int i = 0; i < 2; ++i) a[i] = (g >= 0 && col != self_col[i]) ? pair_fn<FN>(fv[i][e], d.scale) : 0.f;
#pragma unroll
          for (int nb = 0; nb < NBR; ++nb) {
            const float b = g == nb * 16 + (lane & 15) ? 1.f : 0.f;
#pragma unroll
            for (int i = 0; i < 2; ++i) sacc[i][nb] = mma16(a[i], b, sacc[i][nb]);  // rows (4 (lane >> 4) + reg) = queries, column (lane & 15) = group
          }
        }
      }
    } else {
      const int c0 = shalf * (KNN_BT / 2), valid = hi - t0 < KNN_BT ? hi - t0 : KNN_BT;
      const float4* row = reinterpret_cast<const float4*>(d2s + srow * DP + c0);
#pragma unroll 4
      for (int c = 0; c < KNN_BT / 8; ++c) {
        const float4 v = row[c];
        const float f[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int col = c0 + 4 * c + e;
          const float term = pair_fn<FN>(f[e], d.scale);
          sum1 += (col < valid && (long)t0 + col != self_j) ? term : 0.f;
        }
      }
    }
  }
  // to the slice's partial [128, G] (or, with one slice, to S itself)
  const bool direct = d.slices == 1;
  float* dst = direct ? out + (long)q0 * G : out + ((long)q_tile * d.slices + s) * (long)(KNN_BQ * G);
  if (NB > 0) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int nb = 0; nb < NBR; ++nb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int qr = wave * 32 + i * 16 + 4 * (lane >> 4) + r, g = nb * 16 + (lane & 15);
          if (g < G && (!direct || qr < q_ext)) dst[qr * G + g] = sacc[i][nb][r];
        }
  } else {
    // one group: the row's two halves, half 0 + half 1, through the distance tile's first 256 words
    __syncthreads();
    d2s[tid] = sum1;
    __syncthreads();
    if (tid < KNN_BQ && (!direct || tid < q_ext)) dst[tid] = d2s[tid] + d2s[KNN_BQ + tid];
  }
}

// S[i, g] = the slices' partials in slice order
__global__ __launch_bounds__(256) void pairsum_reduce_kernel(const focal_pairsum_desc d, const float* __restrict__ part, float* __restrict__ S) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)d.nq * d.G) return;
  const long i = idx / d.G;
  const int g = (int)(idx - i * d.G);
  const float* p = part + (i / KNN_BQ) * (long)d.slices * (KNN_BQ * d.G) + (i % KNN_BQ) * d.G + g;
  float sum = p[0];
  for (int s = 1; s < d.slices; ++s) sum += p[(long)s * (KNN_BQ * d.G)];
  S[idx] = sum;
}

static int pairsum_check_desc(const focal_pairsum_desc* d, const char* who) {
  FOCAL_CHECK_ARG(d, "%s: null descriptor", who);
  const int rc = knn_check_tile_desc(who, d->D, d->slices, d->nq, "nq");
  if (rc != FOCAL_OK) return rc;
  FOCAL_CHECK_ARG(d->nq >= 1 && d->nt >= 1, "%s: need nq >= 1 and nt >= 1 (got nq=%d nt=%d)", who, d->nq, d->nt);
  FOCAL_CHECK_ARG(d->G >= 1 && d->G <= FOCAL_PAIR_MAX_GROUPS, "%s: need 1 <= G <= %d (got G=%d)", who, FOCAL_PAIR_MAX_GROUPS, d->G);
  FOCAL_CHECK_ARG(((long)d->nq * d->G + 255) / 256 < (1L << 31), "%s: nq * G / 256 exceeds the launch grid (nq=%d G=%d)", who, d->nq, d->G);
  FOCAL_CHECK_ARG(d->fn >= FOCAL_PAIR_SQDIST && d->fn <= FOCAL_PAIR_GAUSS, "%s: need fn in 0 .. 2 (sqdist, dist, gauss; got fn=%d)", who, d->fn);
  FOCAL_CHECK_ARG(std::isfinite(d->scale) && d->scale >= 0.f, "%s: need a finite scale >= 0 (got scale=%g)", who, (double)d->scale);
  FOCAL_CHECK_ARG(d->self_offset >= -1, "%s: need self_offset >= -1 (got self_offset=%d)", who, d->self_offset);
  return FOCAL_OK;
}

// the slices' partials [q tiles, slices, 128, G]; with one slice the kernel writes S itself and the workspace is not touched
extern "C" size_t focal_pair_sums_workspace(const focal_pairsum_desc* d) {
  if (pairsum_check_desc(d, "pair_sums_workspace") != FOCAL_OK) return 0;
  if (d->slices == 1) return 16;
  return (size_t)ceil_div(d->nq, KNN_BQ) * (size_t)d->slices * (size_t)(KNN_BQ * d->G) * sizeof(float);
}

typedef void (*pairsum_kern_t)(const focal_pairsum_desc, const float*, const float*, const float*, const int*, float*);

extern "C" int focal_pair_sums(const focal_pairsum_desc* d, const float* q, const float* t, const float* t_sq, const int* group, float* S,
                               void* ws, size_t ws_bytes, void* stream) {
  const int rc = pairsum_check_desc(d, "pair_sums");
  if (rc != FOCAL_OK) return rc;
  FOCAL_CHECK_ARG(q && t && t_sq && S, "pair_sums: null tensor");
  FOCAL_CHECK_ARG(group || d->G == 1, "pair_sums: G=%d groups need the group ids (group may be NULL for G = 1 only)", d->G);
  FOCAL_CHECK_ARG(((uintptr_t)q & 15) == 0 && ((uintptr_t)t & 15) == 0, "pair_sums: q and t must be 16-byte aligned");
  FOCAL_CHECK_ARG(ws && ws_bytes >= focal_pair_sums_workspace(d), "pair_sums: workspace of %zu bytes, need %zu", ws ? ws_bytes : (size_t)0,
                  focal_pair_sums_workspace(d));
  // group == NULL: the one-register form; otherwise 16 or 64 group columns
  static const pairsum_kern_t kerns[3][3] = {
      {pairsum_kernel<FOCAL_PAIR_SQDIST, 0>, pairsum_kernel<FOCAL_PAIR_SQDIST, 1>, pairsum_kernel<FOCAL_PAIR_SQDIST, 4>},
      {pairsum_kernel<FOCAL_PAIR_DIST, 0>, pairsum_kernel<FOCAL_PAIR_DIST, 1>, pairsum_kernel<FOCAL_PAIR_DIST, 4>},
      {pairsum_kernel<FOCAL_PAIR_GAUSS, 0>, pairsum_kernel<FOCAL_PAIR_GAUSS, 1>, pairsum_kernel<FOCAL_PAIR_GAUSS, 4>}};
  pairsum_kern_t kern = kerns[d->fn][!group ? 0 : d->G <= 16 ? 1 : 2];
  const int q_tiles = ceil_div(d->nq, KNN_BQ);
  float* part = d->slices == 1 ? S : (float*)ws;
  FOCAL_LAUNCH(kern, dim3((unsigned)q_tiles * (unsigned)d->slices), dim3(256), 0, (hipStream_t)stream, *d, q, t, t_sq, group, part);
  FOCAL_LAUNCH_CHECK();
  if (d->slices > 1) {
    const unsigned blocks = (unsigned)(((long)d->nq * d->G + 255) / 256);
    FOCAL_LAUNCH(pairsum_reduce_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, *d, (const float*)ws, S);
    FOCAL_LAUNCH_CHECK();
  }
  return FOCAL_OK;
}
