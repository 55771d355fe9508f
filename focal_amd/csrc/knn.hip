// k-nearest-neighbour search and vote for scoring a pretrained backbone (train_utils/knn.py: GpuKNNClassifier.predict_fused).
//
// focal_knn_search: a workgroup owns KNN_BQ = 128 query rows and one of `slices` contiguous slices of the training rows.  It walks the slice
// in tiles of KNN_BT = 64 rows: the 128 x 64 distance tile is knn_dist.hpp's PairTile, written to LDS and no further: one thread per query
// row scans its 64 candidates against the last entry of the row's running k-best, which lives in that thread's registers.  An entry is ONE
// 64-bit word, (order-preserving key of d2) << 32 | training index, so the order (d2, index) is an integer compare, a NaN distance (key
// 0xFFFFFFFF) orders behind every number, and an empty slot (all ones) behind every candidate.  d2 of a pair is a function of the two rows
// alone (knn_dist.hpp), whatever tile, lane or slice the pair falls into: the result is bit-identical for every `slices`.
// focal_knn_vote: one thread per query merges the `slices` lists under the same order, votes (most frequent label, ties to the smallest)
// and optionally writes the neighbour lists and adds to a confusion matrix laid out as focal_eval_accumulate's.
#include "knn_dist.hpp"

#define KNN_MAX_K 16
#define KNN_MAX_C 64

// The KC best entries seen, ascending, in registers: every index below is a compile-time constant.
template <int KC> struct KnnBest {
  unsigned long long e[KC];
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int i = 0; i < KC; ++i) e[i] = KNN_EMPTY;
  }
  __device__ __forceinline__ void insert(unsigned long long c) {
    if (c < e[KC - 1]) {  // the threshold: almost every candidate ends here
#pragma unroll
      for (int i = 0; i < KC; ++i) {
        const unsigned long long lo = c < e[i] ? c : e[i], hi = c < e[i] ? e[i] : c;
        e[i] = lo;
        c = hi;
      }
    }
  }
};

template <int KC>
__global__ __launch_bounds__(256) void knn_search_kernel(const focal_knn_desc d, const float* __restrict__ q, const float* __restrict__ t,
                                                         const float* __restrict__ t_sq, float* __restrict__ part_d2,
                                                         int* __restrict__ part_idx) {
  __shared__ PairTile::Lds lds;
  constexpr int DP = PairTile::DP;

  const int tid = threadIdx.x;
  const int D = d.D, k = d.k;
  const int s = (int)(blockIdx.x % (unsigned)d.slices), q0 = (int)(blockIdx.x / (unsigned)d.slices) * KNN_BQ;
  int lo, hi;
  knn_slice(d.nt, d.slices, s, lo, hi);
  const int q_ext = d.nq - q0;
  const float* qb = q + (long)q0 * D;

  knn_row_norms(qb, D, q_ext, tid, lds.qsq);

  KnnBest<KC> best;
  best.init();

  const int nT = (hi - lo + KNN_BT - 1) / KNN_BT;
  PairTile pt(lds, qb, D, q_ext);
  auto load = [&](int ti, int ks) { pt.load(t, lo, hi, ti, ks); };
  if (nT > 0) load(0, 0);
  for (int ti = 0; ti < nT; ++ti) {
    f32x4 acc[2][4];
    pt.product(acc, ti, nT, load);
    const int t0 = lo + ti * KNN_BT;
    float ts[4];
    pt.col_norms(ts, t_sq, t0, hi);
    pt.write_d2(acc, ts);
    if (tid < KNN_BQ) {
      const int valid = hi - t0 < KNN_BT ? hi - t0 : KNN_BT;
      const float4* row = reinterpret_cast<const float4*>(lds.d2 + tid * DP);
#pragma unroll 4
      for (int c = 0; c < KNN_BT / 4; ++c) {
        const float4 v = row[c];
        const float f[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (4 * c + e < valid) best.insert(((unsigned long long)knn_key(f[e]) << 32) | (uint32_t)(t0 + 4 * c + e));
      }
    }
  }
  if (tid < KNN_BQ && tid < q_ext) {
    const long o = ((long)(q0 + tid) * d.slices + s) * k;
#pragma unroll
    for (int i = 0; i < KC; ++i)
      if (i < k) {
        const bool empty = best.e[i] == KNN_EMPTY;
        part_d2[o + i] = empty ? __uint_as_float(0x7F800000u) : knn_unkey((uint32_t)(best.e[i] >> 32));
        part_idx[o + i] = empty ? -1 : (int)(uint32_t)best.e[i];
      }
  }
}

template <int KC>
__global__ __launch_bounds__(64) void knn_vote_kernel(const focal_knn_desc d, const float* __restrict__ part_d2, const int* __restrict__ part_idx,
                                                      const long* __restrict__ t_labels, const long* __restrict__ q_labels,
                                                      long* __restrict__ preds, int* __restrict__ nbr_idx, float* __restrict__ nbr_d2,
                                                      int* __restrict__ conf) {
  const int qi = blockIdx.x * 64 + threadIdx.x;
  if (qi >= d.nq) return;
  const int k = d.k, n = d.slices * k, k_eff = k < d.nt ? k : d.nt;
  const long base = (long)qi * n;
  KnnBest<KC> best;
  best.init();
  for (int c = 0; c < n; ++c) {
    const int idx = part_idx[base + c];
    if (idx >= 0) best.insert(((unsigned long long)knn_key(part_d2[base + c]) << 32) | (uint32_t)idx);
  }
  // (every slice hands in min(k, its rows) real entries, so the first k_eff merged ones are real)
  long lab[KC];
#pragma unroll
  for (int i = 0; i < KC; ++i) lab[i] = (i < k_eff && best.e[i] != KNN_EMPTY) ? t_labels[(uint32_t)best.e[i]] : -1;
  long pred = -1;
  int top = 0;
#pragma unroll
  for (int i = 0; i < KC; ++i) {
    if (i >= k_eff) continue;
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < KC; ++j) cnt += (j < k_eff && lab[j] == lab[i]) ? 1 : 0;
    if (cnt > top || (cnt == top && lab[i] < pred)) { top = cnt; pred = lab[i]; }
  }
  preds[qi] = pred;
  if (nbr_idx || nbr_d2) {
#pragma unroll
    for (int i = 0; i < KC; ++i)
      if (i < k) {
        const bool real = i < k_eff && best.e[i] != KNN_EMPTY;
        if (nbr_idx) nbr_idx[(long)qi * k + i] = real ? (int)(uint32_t)best.e[i] : -1;
        if (nbr_d2) nbr_d2[(long)qi * k + i] = real ? knn_unkey((uint32_t)(best.e[i] >> 32)) : __uint_as_float(0x7F800000u);
      }
  }
  if (conf) {
    const int Cn = d.n_classes;
    const long y = q_labels[qi];
    const bool ok = y >= 0 && y < Cn && pred >= 0 && pred < Cn;
    atomicAdd(conf + (ok ? (int)y * Cn + (int)pred : Cn * Cn), 1);
  }
}

static int knn_check_desc(const focal_knn_desc* d, const char* who) {
  FOCAL_CHECK_ARG(d, "%s: null descriptor", who);
  FOCAL_CHECK_ARG(d->k >= 1 && d->k <= KNN_MAX_K, "%s: need 1 <= k <= %d (got k=%d)", who, KNN_MAX_K, d->k);
  FOCAL_CHECK_ARG(d->n_classes >= 1 && d->n_classes <= KNN_MAX_C, "%s: need 1 <= n_classes <= %d (got n_classes=%d)", who, KNN_MAX_C,
                  d->n_classes);
  FOCAL_CHECK_ARG(d->D >= 4 && d->D % 4 == 0, "%s: need D >= 4 and D %% 4 == 0 (got D=%d)", who, d->D);
  FOCAL_CHECK_ARG(d->nt >= 1 && d->nq >= 1 && d->slices >= 1, "%s: need nt >= 1, nq >= 1, slices >= 1 (got nt=%d nq=%d slices=%d)", who,
                  d->nt, d->nq, d->slices);
  FOCAL_CHECK_ARG((long)ceil_div(d->nq, KNN_BQ) * d->slices < (1L << 31) && (long)d->slices * d->k < (1L << 31),
                  "%s: nq / %d * slices exceeds the launch grid (nq=%d slices=%d)", who, KNN_BQ, d->nq, d->slices);
  return FOCAL_OK;
}

extern "C" int focal_knn_search(const focal_knn_desc* d, const float* q, const float* t, const float* t_sq, float* part_d2, int* part_idx,
                                void* stream) {
  const int rc = knn_check_desc(d, "knn_search");
  if (rc != FOCAL_OK) return rc;
  FOCAL_CHECK_ARG(q && t && t_sq && part_d2 && part_idx, "knn_search: null tensor");
  FOCAL_CHECK_ARG(((uintptr_t)q & 15) == 0 && ((uintptr_t)t & 15) == 0, "knn_search: q and t must be 16-byte aligned");
  const dim3 grid((unsigned)(ceil_div(d->nq, KNN_BQ) * d->slices));
  if (d->k <= 8) FOCAL_LAUNCH(knn_search_kernel<8>, grid, dim3(256), 0, (hipStream_t)stream, *d, q, t, t_sq, part_d2, part_idx);
  else FOCAL_LAUNCH(knn_search_kernel<16>, grid, dim3(256), 0, (hipStream_t)stream, *d, q, t, t_sq, part_d2, part_idx);
  FOCAL_LAUNCH_CHECK();
  return FOCAL_OK;
}

extern "C" int focal_knn_vote(const focal_knn_desc* d, const float* part_d2, const int* part_idx, const long* t_labels, const long* q_labels,
                              long* preds, int* nbr_idx, float* nbr_d2, int* conf, void* stream) {
  const int rc = knn_check_desc(d, "knn_vote");
  if (rc != FOCAL_OK) return rc;
  FOCAL_CHECK_ARG(part_d2 && part_idx && t_labels && preds, "knn_vote: null tensor");
  FOCAL_CHECK_ARG(!conf || q_labels, "knn_vote: a confusion matrix needs the queries' labels");
  const dim3 grid((unsigned)ceil_div(d->nq, 64));
  if (d->k <= 8) FOCAL_LAUNCH(knn_vote_kernel<8>, grid, dim3(64), 0, (hipStream_t)stream, *d, part_d2, part_idx, t_labels, q_labels, preds, nbr_idx, nbr_d2, conf);
  else FOCAL_LAUNCH(knn_vote_kernel<16>, grid, dim3(64), 0, (hipStream_t)stream, *d, part_d2, part_idx, t_labels, q_labels, preds, nbr_idx, nbr_d2, conf);
  FOCAL_LAUNCH_CHECK();
  return FOCAL_OK;
}
