// K-means on un-projected backbone features (train_utils/kmeans.py: GpuKMeans, src/eval_cluster.py): one Lloyd iteration of all R restarts
// together is three launches -- assign, accumulate, finish -- with no floating-point atomic in any of them.
//
// focal_kmeans_assign: knn.hip's search with the training rows replaced by the R*K centroids and the k-best scan by a per-restart best.  A
// workgroup owns KNN_BQ = 128 rows of x and walks ALL R*K centroid rows in tiles of KNN_BT = 64: knn_dist.hpp's PairTile, d2 written to
// its LDS tile and no further.  One thread per row scans the tile's columns in order; column g belongs to restart g / K, so the thread
// carries ONE 64-bit best, (key of d2) << 32 | k, and hands it in when the column counter reaches K -- whether or not a tile boundary
// fell inside the restart.  d2 of a (row, centroid) pair is focal_knn_search's, so for R = 1 the labels are its nearest neighbour bit
// for bit.
// focal_kmeans_update: a workgroup owns one of `slices` contiguous row slices, 64 feature columns and a group of restarts whose
// accumulators [restarts * K][64] fit in LDS.  Rows go through an LDS block of 64 rows x 64 columns; wave w takes the group's restarts
// w, w + 4, ..: lane <-> column, rows in order, acc[label][lane] += x -- every accumulator cell belongs to one lane and sees its rows in
// index order.  Partials [slices, R*K, D] are summed in slice order by the finishing launch, which divides, writes |c|^2 (fixed tree),
// the counts and the inertia.  Same arguments -> same bits.
#include "knn_dist.hpp"

#define KMEANS_MAX_K 64
#define KMEANS_MAX_RK 1024
constexpr int KM_COLS = 64;        // feature columns per update workgroup (one per lane)
constexpr int KM_ROWS = 64;        // rows per staged block
constexpr int KM_ACC_ROWS = 160;   // accumulator rows (restarts of a group x K) per update workgroup: 40 KiB of LDS

__global__ __launch_bounds__(256) void kmeans_assign_kernel(const focal_kmeans_desc d, const float* __restrict__ x, const float* __restrict__ c,
                                                            const float* __restrict__ c_sq, int* __restrict__ labels,
                                                            float* __restrict__ min_d2, int* __restrict__ changed) {
  __shared__ PairTile::Lds lds;
  constexpr int DP = PairTile::DP;

  const int tid = threadIdx.x, lane = tid & 63;
  const int D = d.D, K = d.K, RK = d.R * d.K, n = d.n;
  const int q0 = (int)blockIdx.x * KNN_BQ;
  const int q_ext = n - q0;
  const float* qb = x + (long)q0 * D;

  knn_row_norms(qb, D, q_ext, tid, lds.qsq);

  // the scan's state: the restart and the centroid within it of the next column, and the best of the restart so far (all but `best` are
  // the same in every thread)
  int cur_r = 0, cur_k = 0;
  unsigned long long best = KNN_EMPTY;

  const int nT = (RK + KNN_BT - 1) / KNN_BT;
  PairTile pt(lds, qb, D, q_ext);
  auto load = [&](int ti, int ks) { pt.load(c, 0, RK, ti, ks); };
  load(0, 0);
  for (int ti = 0; ti < nT; ++ti) {
    f32x4 acc[2][4];
    pt.product(acc, ti, nT, load);
    const int t0 = ti * KNN_BT;
    float ts[4];
    pt.col_norms(ts, c_sq, t0, RK);
    pt.write_d2(acc, ts);
    if (tid < KNN_BQ) {  // (waves 0 and 1, whole: the ballot below counts a wave's 64 rows)
      const int valid = RK - t0 < KNN_BT ? RK - t0 : KNN_BT;
      const bool live = tid < q_ext;
      const float4* row = reinterpret_cast<const float4*>(lds.d2 + tid * DP);
      for (int cc = 0; cc < KNN_BT / 4; ++cc) {
        const float4 v = row[cc];
        const float f[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (4 * cc + e >= valid) break;
          const unsigned long long cand = ((unsigned long long)knn_key(f[e]) << 32) | (uint32_t)cur_k;
          best = cand < best ? cand : best;
          if (++cur_k == K) {  // the restart's last column: hand its best in (an all-NaN row: key all ones, k = 0)
            const long o = (long)cur_r * n + q0 + tid;
            const int lab = (int)(uint32_t)best;
            bool moved = false;
            if (live) {
              if (changed) moved = labels[o] != lab;
              labels[o] = lab;
              if (min_d2) min_d2[o] = knn_unkey((uint32_t)(best >> 32));
            }
            if (changed) {
              const int cnt = __popcll(__ballot(moved));
              if (lane == 0 && cnt) atomicAdd(changed + cur_r, cnt);
            }
            best = KNN_EMPTY;
            cur_k = 0;
            ++cur_r;
          }
        }
      }
    }
  }
}

// grid (slices, ceil(D / 64), restart groups); rg = restarts per group
__global__ __launch_bounds__(256) void kmeans_accum_kernel(const focal_kmeans_desc d, int rg, const float* __restrict__ x,
                                                           const int* __restrict__ labels, const float* __restrict__ min_d2,
                                                           float* __restrict__ part, int* __restrict__ part_cnt,
                                                           float* __restrict__ part_inertia) {
  __shared__ __attribute__((aligned(16))) float acc[KM_ACC_ROWS * KM_COLS];
  __shared__ __attribute__((aligned(16))) float xs[KM_ROWS * KM_COLS];
  __shared__ int cnt_s[KM_ACC_ROWS];
  __shared__ float inert_s[KM_ACC_ROWS];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D = d.D, K = d.K, n = d.n, RK = d.R * d.K;
  const int s = blockIdx.x, col0 = blockIdx.y * KM_COLS;
  const int r0 = blockIdx.z * rg, r1 = r0 + rg < d.R ? r0 + rg : d.R;
  const long per = ((long)n + d.slices - 1) / d.slices;
  const long lo_l = (long)s * per < (long)n ? (long)s * per : (long)n;
  const int lo = (int)lo_l, hi = (int)(lo_l + per < (long)n ? lo_l + per : (long)n);
  const bool tally = blockIdx.y == 0;  // the counts and the inertia do not depend on the column chunk: its first workgroup takes them

  for (int i = tid; i < KM_ACC_ROWS * KM_COLS; i += 256) acc[i] = 0.f;
  if (tid < KM_ACC_ROWS) { cnt_s[tid] = 0; inert_s[tid] = 0.f; }
  __syncthreads();

  for (int i0 = lo; i0 < hi; i0 += KM_ROWS) {
    const int rows = hi - i0 < KM_ROWS ? hi - i0 : KM_ROWS;
    // the block of x: 16 threads x 16 bytes per row, 16 rows per pass (D % 4 == 0: a float4 lies inside the row or past it)
#pragma unroll
    for (int p = 0; p < KM_ROWS / 16; ++p) {
      const int rr = p * 16 + (tid >> 4), cc = (tid & 15) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (rr < rows && col0 + cc < D) v = *reinterpret_cast<const float4*>(x + (long)(i0 + rr) * D + col0 + cc);
      *reinterpret_cast<float4*>(xs + rr * KM_COLS + cc) = v;
    }
    __syncthreads();
    for (int r = r0 + wave; r < r1; r += 4) {
      const int mine = lane < rows ? labels[(long)r * n + i0 + lane] : -1;
      float* a = acc + (r - r0) * K * KM_COLS + lane;
      for (int j = 0; j < rows; ++j) {
        const int l = __shfl(mine, j, 64);
        if ((unsigned)l < (unsigned)K) a[l * KM_COLS] += xs[j * KM_COLS + lane];
      }
      if (tally) {
        if ((unsigned)mine < (unsigned)K) atomicAdd(&cnt_s[(r - r0) * K + mine], 1);  // (integer, LDS)
        if (min_d2) {
          float m = lane < rows ? min_d2[(long)r * n + i0 + lane] : 0.f;
#pragma unroll
          for (int w = 1; w < 64; w <<= 1) m += __shfl_xor(m, w, 64);  // a fixed tree over the block's rows, blocks in order
          if (lane == 0) inert_s[r - r0] += m;
        }
      }
    }
    __syncthreads();
  }
  const int rows_out = (r1 - r0) * K;
  for (int i = tid; i < rows_out * KM_COLS; i += 256) {
    const int rr = i / KM_COLS, cc = col0 + (i % KM_COLS);
    if (cc < D) part[((long)s * RK + (long)r0 * K + rr) * D + cc] = acc[i];
  }
  if (tally) {
    for (int i = tid; i < rows_out; i += 256) part_cnt[(long)s * RK + r0 * K + i] = cnt_s[i];
    if (part_inertia)
      for (int i = tid; i < r1 - r0; i += 256) part_inertia[(long)s * d.R + r0 + i] = inert_s[i];
  }
}

// one workgroup per centroid row
__global__ __launch_bounds__(256) void kmeans_finish_kernel(const focal_kmeans_desc d, const float* __restrict__ part,
                                                            const int* __restrict__ part_cnt, const float* __restrict__ part_inertia,
                                                            float* __restrict__ c, float* __restrict__ c_sq, int* __restrict__ counts,
                                                            float* __restrict__ inertia) {
  __shared__ float red[256];
  const int tid = threadIdx.x, rk = blockIdx.x, D = d.D, RK = d.R * d.K;
  int count = 0;
#pragma unroll 8
  for (int s = 0; s < d.slices; ++s) count += part_cnt[(long)s * RK + rk];
  if (tid == 0) {
    counts[rk] = count;
    if (inertia && rk % d.K == 0) {
      const int r = rk / d.K;
      float sum = 0.f;
      for (int s = 0; s < d.slices; ++s) sum += part_inertia[(long)s * d.R + r];
      inertia[r] = sum;
    }
  }
  if (count == 0) return;  // an empty cluster keeps its centroid and its norm, bits unchanged (uniform: no barrier is skipped by a part of the workgroup)
  const float cf = (float)count;
  float sq = 0.f;
  for (int col = tid; col < D; col += 256) {
    float sum = 0.f;
#pragma unroll 8
    for (int s = 0; s < d.slices; ++s) sum += part[((long)s * RK + rk) * D + col];  // (the loads of 8 slices in flight; the adds in slice order)
    const float v = sum / cf;
    c[(long)rk * D + col] = v;
    sq = fmaf(v, v, sq);
  }
  red[tid] = sq;
  __syncthreads();
#pragma unroll
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) c_sq[rk] = red[0];
}

static int kmeans_check_desc(const focal_kmeans_desc* d, const char* who) {
  FOCAL_CHECK_ARG(d, "%s: null descriptor", who);
  FOCAL_CHECK_ARG(d->D >= 4 && d->D % 4 == 0, "%s: need D >= 4 and D %% 4 == 0 (got D=%d)", who, d->D);
  FOCAL_CHECK_ARG(d->K >= 1 && d->K <= KMEANS_MAX_K, "%s: need 1 <= K <= %d (got K=%d)", who, KMEANS_MAX_K, d->K);
  FOCAL_CHECK_ARG(d->R >= 1 && (long)d->R * d->K <= KMEANS_MAX_RK, "%s: need R >= 1 and R * K <= %d (got R=%d K=%d)", who, KMEANS_MAX_RK,
                  d->R, d->K);
  FOCAL_CHECK_ARG(d->n >= 1 && d->slices >= 1 && d->slices <= 65535, "%s: need n >= 1 and 1 <= slices <= 65535 (got n=%d slices=%d)", who,
                  d->n, d->slices);
  return FOCAL_OK;
}

extern "C" int focal_kmeans_assign(const focal_kmeans_desc* d, const float* x, const float* c, const float* c_sq, int* labels, float* min_d2,
                                   int* changed, void* stream) {
  const int rc = kmeans_check_desc(d, "kmeans_assign");
  if (rc != FOCAL_OK) return rc;
  FOCAL_CHECK_ARG(x && c && c_sq && labels, "kmeans_assign: null tensor");
  FOCAL_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)c & 15) == 0, "kmeans_assign: x and c must be 16-byte aligned");
  FOCAL_LAUNCH(kmeans_assign_kernel, dim3((unsigned)ceil_div(d->n, KNN_BQ)), dim3(256), 0, (hipStream_t)stream, *d, x, c, c_sq, labels, min_d2,
               changed);
  FOCAL_LAUNCH_CHECK();
  return FOCAL_OK;
}

static int kmeans_group(int K) { return KM_ACC_ROWS / K; }  // restarts per update workgroup (K <= 64: at least 2)

extern "C" size_t focal_kmeans_update_workspace(const focal_kmeans_desc* d) {
  if (kmeans_check_desc(d, "kmeans_update_workspace") != FOCAL_OK) return 0;
  const size_t RK = (size_t)d->R * d->K;
  return ((size_t)d->slices * RK * d->D + (size_t)d->slices * RK + (size_t)d->slices * d->R) * 4;
}

extern "C" int focal_kmeans_update(const focal_kmeans_desc* d, const float* x, const int* labels, const float* min_d2, float* c, float* c_sq,
                                   int* counts, float* inertia, void* ws, size_t ws_bytes, void* stream) {
  const int rc = kmeans_check_desc(d, "kmeans_update");
  if (rc != FOCAL_OK) return rc;
  FOCAL_CHECK_ARG(x && labels && c && c_sq && counts && ws, "kmeans_update: null tensor");
  FOCAL_CHECK_ARG(!inertia || min_d2, "kmeans_update: the inertia needs min_d2");
  FOCAL_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)c & 15) == 0, "kmeans_update: x and c must be 16-byte aligned");
  FOCAL_CHECK_ARG(ws_bytes >= focal_kmeans_update_workspace(d), "kmeans_update: workspace of %zu bytes, need %zu", ws_bytes,
                  focal_kmeans_update_workspace(d));
  const size_t RK = (size_t)d->R * d->K;
  float* part = (float*)ws;
  int* part_cnt = (int*)(part + (size_t)d->slices * RK * d->D);
  float* part_inertia = (float*)(part_cnt + (size_t)d->slices * RK);
  const int rg = kmeans_group(d->K);
  const dim3 grid((unsigned)d->slices, (unsigned)ceil_div(d->D, KM_COLS), (unsigned)ceil_div(d->R, rg));
  FOCAL_LAUNCH(kmeans_accum_kernel, grid, dim3(256), 0, (hipStream_t)stream, *d, rg, x, labels, inertia ? min_d2 : nullptr, part, part_cnt,
               inertia ? part_inertia : nullptr);
  FOCAL_LAUNCH_CHECK();
  FOCAL_LAUNCH(kmeans_finish_kernel, dim3((unsigned)RK), dim3(256), 0, (hipStream_t)stream, *d, part, part_cnt, part_inertia, c, c_sq, counts,
               inertia);
  FOCAL_LAUNCH_CHECK();
  return FOCAL_OK;
}
