// Rank of one named gallery row per query, for cross-modal retrieval of the projected embeddings (train_utils/retrieval.py:
// cross_modal_ranks, src/eval_retrieval.py).  The [nq, nt] distances exist in LDS tiles only.
//
// focal_rank_positive is two launches of ONE tile loop -- knn_dist.hpp's PairTile, so d2 of a pair is the bits focal_knn_search (knn.hip)
// produces for it:
// rank_kernel<true>: a workgroup owns 128 queries and runs the product against the GATHERED rows t[pos[q0 .. q0 + 127]] (tiles of 64);
// the diagonal of each tile is d2(i, pos_i).  Because d2 of a pair does not depend on the tile or lane it falls into, those are the bits
// the scan sees in column pos_i.  The launch writes pos_d2 and zeroes before / tied (-1 / -1 / NaN for a pos outside [0, nt), whose row is
// never gathered: its chunks are predicated off and arrive as zeros).
// rank_kernel<false>: a workgroup owns 128 queries and one of `slices` contiguous slices of t, walked in tiles of 64 as the search does;
// two threads per query row scan 32 candidates each of the distance tile against the row's positive, (key, index) as integer compares,
// and add their two counters to before / tied with integer atomics: order-free, so the outputs are the same bits for every `slices`.
#include "knn_dist.hpp"

template <bool GATHER>
__global__ __launch_bounds__(256) void rank_kernel(const focal_rank_desc d, const float* __restrict__ q, const float* __restrict__ t,
                                                   const float* __restrict__ t_sq, const int* __restrict__ pos, int* __restrict__ before,
                                                   int* __restrict__ tied, float* __restrict__ pos_d2) {
  using StT = PairTile::StT;
  static_assert(StT::NCH == 2 && StT::CPR == 8, "the gather below addresses the training stage's chunks");
  constexpr int DP = PairTile::DP;
  __shared__ PairTile::Lds lds;
  float* d2s = lds.d2;
  // the rows' positives, -1 where there is none (row past nq, or pos outside [0, nt)), live in the distance tile's first pad column, which
  // no distance is written to: the footprint is the search's
  auto pos_of = [&](int row) -> int& { return reinterpret_cast<int*>(d2s)[row * DP + KNN_BT]; };

  const int tid = threadIdx.x;
  const int D = d.D;
  const int q0 = (GATHER ? (int)blockIdx.x : (int)(blockIdx.x / (unsigned)d.slices)) * KNN_BQ;
  const int q_ext = d.nq - q0;
  // GATHER: the gathered rows 0 .. (the workgroup's queries) - 1; else slice blockIdx.x % slices of t
  int lo = 0, hi = q_ext < KNN_BQ ? q_ext : KNN_BQ;
  if (!GATHER) knn_slice(d.nt, d.slices, (int)(blockIdx.x % (unsigned)d.slices), lo, hi);
  const float* qb = q + (long)q0 * D;

  if (tid < KNN_BQ) {
    const int p = tid < q_ext ? pos[q0 + tid] : -1;
    pos_of(tid) = (p >= 0 && p < d.nt) ? p : -1;
  }
  knn_row_norms(qb, D, q_ext, tid, lds.qsq);
  __syncthreads();

  // scan state of thread (row = tid & 127, half = tid >> 7): the positive's key and index, and the two counters
  const int srow = tid & (KNN_BQ - 1), shalf = tid >> 7;
  const int my_p = pos_of(srow);
  uint32_t my_key = 0;
  int n_before = 0, n_tied = 0;
  if (!GATHER && my_p >= 0) my_key = knn_key(pos_d2[q0 + srow]);

  const int nT = (hi - lo + KNN_BT - 1) / KNN_BT;
  PairTile pt(lds, qb, D, q_ext);
  auto load = [&](int ti, int ks) {
    if (!GATHER) {
      pt.load(t, lo, hi, ti, ks);
      return;
    }
    // chunk j of this thread is 16 bytes of gathered row t0 + a: the row pos names, or zeros where it names none
    const int t0 = ti * KNN_BT;
    pt.load_q(ks);
#pragma unroll
    for (int j = 0; j < StT::NCH; ++j) {
      const int c = tid + 256 * j, a = c / StT::CPR, b = (c % StT::CPR) * StT::EC;
      const int p = pos_of(t0 + a), r = ks * KNN_BK + b;
      const bool ok = p >= 0 && r < D;
      raw_load(pt.st.raw[j], t + (ok ? (long)p * D + r : 0L), ok);
    }
  };
  if (nT > 0) load(0, 0);
  for (int ti = 0; ti < nT; ++ti) {
    f32x4 acc[2][4];
    pt.product(acc, ti, nT, load);
    const int t0 = lo + ti * KNN_BT;
    float ts[4];
    if (GATHER) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int p = pos_of(t0 + pt.col(j));
        ts[j] = p >= 0 ? t_sq[p] : 0.f;
      }
    } else {
      pt.col_norms(ts, t_sq, t0, hi);
    }
    pt.write_d2(acc, ts);
    if (GATHER) {
      // the diagonal: query row t0 + c against gathered row t0 + c
      if (tid < KNN_BT && t0 + tid < q_ext) {
        const int qr = t0 + tid;
        const bool ok = pos_of(qr) >= 0;
        before[q0 + qr] = ok ? 0 : -1;
        tied[q0 + qr] = ok ? 0 : -1;
        pos_d2[q0 + qr] = ok ? d2s[qr * DP + tid] : __uint_as_float(0x7FC00000u);
      }
    } else if (my_p >= 0) {
      const int c0 = shalf * (KNN_BT / 2), valid = hi - t0 < KNN_BT ? hi - t0 : KNN_BT;
      const float4* row = reinterpret_cast<const float4*>(d2s + srow * DP + c0);
#pragma unroll 4
      for (int c = 0; c < KNN_BT / 8; ++c) {
        const float4 v = row[c];
        const float f[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int col = c0 + 4 * c + e;
          // (key, index) < (key_p, p) in two 32-bit compares; the positive's own column has an equal key and is taken out below
          const uint32_t key = knn_key(f[e]);
          const bool in = col < valid, eq = in && key == my_key;
          n_before += ((in && key < my_key) || (eq && t0 + col < my_p)) ? 1 : 0;
          n_tied += eq ? 1 : 0;
        }
      }
    }
  }
  if (!GATHER && my_p >= 0) {
    // the positive itself was counted as a tie by the half whose columns hold it
    if (my_p >= lo && my_p < hi && (((my_p - lo) % KNN_BT) >> 5) == shalf) n_tied -= 1;
    if (n_before) atomicAdd(before + q0 + srow, n_before);
    if (n_tied) atomicAdd(tied + q0 + srow, n_tied);
  }
}

static int rank_check_desc(const focal_rank_desc* d, const char* who) {
  FOCAL_CHECK_ARG(d, "%s: null descriptor", who);
  const int rc = knn_check_tile_desc(who, d->D, d->slices, d->nq, "nq");
  if (rc != FOCAL_OK) return rc;
  FOCAL_CHECK_ARG(d->nq >= 1 && d->nt >= 1, "%s: need nq >= 1 and nt >= 1 (got nq=%d nt=%d)", who, d->nq, d->nt);
  return FOCAL_OK;
}

// tied [nq] and pos_d2 [nq] for a caller who passes NULL for either (the scan reads both launches' pos_d2)
extern "C" size_t focal_rank_workspace(const focal_rank_desc* d) {
  if (rank_check_desc(d, "rank_workspace") != FOCAL_OK) return 0;
  return (size_t)d->nq * (sizeof(int) + sizeof(float));
}

extern "C" int focal_rank_positive(const focal_rank_desc* d, const float* q, const float* t, const float* t_sq, const int* pos, int* before,
                                   int* tied, float* pos_d2, void* ws, size_t ws_bytes, void* stream) {
  const int rc = rank_check_desc(d, "rank_positive");
  if (rc != FOCAL_OK) return rc;
  FOCAL_CHECK_ARG(q && t && t_sq && pos && before, "rank_positive: null tensor");
  FOCAL_CHECK_ARG(((uintptr_t)q & 15) == 0 && ((uintptr_t)t & 15) == 0, "rank_positive: q and t must be 16-byte aligned");
  FOCAL_CHECK_ARG(ws && ws_bytes >= focal_rank_workspace(d), "rank_positive: workspace of %zu bytes, need %zu", ws ? ws_bytes : (size_t)0,
                  focal_rank_workspace(d));
  int* tied_w = tied ? tied : (int*)ws;
  float* d2_w = pos_d2 ? pos_d2 : (float*)ws + d->nq;
  const int q_tiles = ceil_div(d->nq, KNN_BQ);
  FOCAL_LAUNCH(rank_kernel<true>, dim3((unsigned)q_tiles), dim3(256), 0, (hipStream_t)stream, *d, q, t, t_sq, pos, before, tied_w, d2_w);
  FOCAL_LAUNCH_CHECK();
  FOCAL_LAUNCH(rank_kernel<false>, dim3((unsigned)q_tiles * (unsigned)d->slices), dim3(256), 0, (hipStream_t)stream, *d, q, t, t_sq, pos,
               before, tied_w, d2_w);
  FOCAL_LAUNCH_CHECK();
  return FOCAL_OK;
}
