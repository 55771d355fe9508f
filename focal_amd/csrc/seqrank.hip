// Sequence-to-sequence ranking counts for the temporal constraint of the FOCAL loss on a whole split (train_utils/temporal.py:
// sequence_ranking; src/eval_temporal.py).  Rows a L .. a L + L - 1 of z are sequence a; the [S, S] matrix of pooled distances
// P(a, b) = sum_{i in a, j in b} f(max(d2(i, j), 0)) exists as L x L blocks of LDS distance tiles only.
//
// focal_seq_rank walks z in knn_dist.hpp's PairTile, as focal_rank_positive's scan (rank.hip) does -- d2 of a pair is the bits
// focal_knn_search produces for it -- with another epilogue, in three launches:
// seqrank_kernel<FN, L, true>: a workgroup owns 128 rows and runs the product against ITS OWN rows (two tiles of 64); the L x L blocks on
// the diagonal are the sequences' own distances.  Because d2 of a pair does not depend on the tile or lane it falls into, those are the
// bits the scan sees.  The launch writes intra_d2 and intra_sum (one thread per sequence, row-major, i != j) and zeroes before / viol.
// seqrank_kernel<FN, L, false>: a workgroup owns 128 rows (128 / L row sequences) and one of `slices` contiguous slices of z, cut at
// multiples of 64 rows so that no block straddles a slice or a tile, walked in tiles of 64.  2 L threads serve one row sequence for the
// whole scan: each pools whole blocks, row-major from 0, compares the pooled value with the sequence's two thresholds (registers) and
// keeps two counters and two float sums in registers.  After the last tile the threads of a sequence meet through the distance tile
// in thread order 0 .. 2 L - 1; the counters go to before / viol with integer atomics (order-free: the same bits for every `slices`),
// the float sums to the slice's partial.
// seqrank_reduce_kernel: adds the slices' partials in slice order.  hinge_sum is carried times L^2 (L^2 - L), thr_v - P (L^2 - L) per
// active pair -- the two sides of viol's comparison -- and divided once after its last addition.  No floating-point atomic anywhere:
// the bits are a function of (n, D, L, slices) and the inputs alone; another `slices` is another order and may differ in the last bits.
// How the blocks are read (DP = 68 words: row r, 16-byte column slot c lies on bank slot (r + c) mod 16, and a ds_read_b128 is served in
// four fixed groups of 16 lanes, conflict-free when the group's 16 slots differ): the threads are renumbered so that each such group is
// 16 consecutive virtual threads, and a group takes
//   L = 2:  four row sequences x four threads, a thread reading the block PAIRS {0, 1, 8, 9}[sub] + 2 it: slots 2 rs + pair, all 16;
//   L = 4:  row sequences rs and rs + 2 x eight threads, blocks sub + 8 it: slots 4 rs + sub (+ 8), all 16;
//   L = 8:  one row sequence, threads 0 .. 7 on blocks 0 .. 7 (slots 2 b (+ 1)), threads 8 .. 15 idle;
//   L = 16: one row sequence, threads 0 .. 3 on blocks 0 .. 3 (slots 4 b + h), the others idle;
// every read is conflict-free.  (L = 8, 16 leave lanes idle because a block's row-major sum is one chain; the MFMA product is 16 x the
// epilogue's flops at D = 256 and the second workgroup of the CU runs under it.)
#include "knn_dist.hpp"

#include <cmath>

template <int FN, int L, bool INTRA>
__global__ __launch_bounds__(256) void seqrank_kernel(const focal_seqrank_desc d, const float* __restrict__ z, const float* __restrict__ z_sq,
                                                      float* __restrict__ intra_d2, float* __restrict__ intra_sum, int* __restrict__ before,
                                                      int* __restrict__ viol, float* __restrict__ part_hinge, float* __restrict__ part_inter) {
  static_assert(L == 2 || L == 4 || L == 8 || L == 16, "blocks never straddle a tile");
  static_assert(FN == FOCAL_PAIR_SQDIST || FN == FOCAL_PAIR_DIST, "pair_fn without a scale");
  constexpr int DP = PairTile::DP;
  constexpr int NRS = KNN_BQ / L;   // row sequences of a workgroup
  constexpr int TPS = 2 * L;        // threads per row sequence
  constexpr int NBT = KNN_BT / L;   // blocks of a tile per row sequence
  constexpr float L2 = (float)(L * L), L2L = (float)(L * L - L);
  __shared__ PairTile::Lds lds;
  float* d2s = lds.d2;
  static_assert(KNN_BQ * DP >= 4 * 256, "the join uses the distance tile");

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D = d.D, n = d.n;
  const int s = INTRA ? 0 : (int)(blockIdx.x % (unsigned)d.slices);
  const int q_tile = INTRA ? (int)blockIdx.x : (int)(blockIdx.x / (unsigned)d.slices);
  const int q0 = q_tile * KNN_BQ;
  const int q_ext = n - q0;
  // slices of whole tiles
  const long per = ((((long)n + KNN_BT - 1) / KNN_BT + d.slices - 1) / d.slices) * KNN_BT;
  const long lo_l = (long)s * per < (long)n ? (long)s * per : (long)n;
  const int lo = INTRA ? q0 : (int)lo_l;
  const int hi = INTRA ? q0 + (q_ext < KNN_BQ ? q_ext : KNN_BQ) : (int)(lo_l + per < (long)n ? lo_l + per : (long)n);
  const float* qb = z + (long)q0 * D;

  knn_row_norms(qb, D, q_ext, tid, lds.qsq);
  __syncthreads();

  // scan state: virtual thread vt (the ds_read_b128 lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} (+ 32) made consecutive),
  // its row sequence rs and its place sub among the sequence's TPS threads
  const int quad = (lane & 31) >> 2;
  const int vt = wave * 64 + ((lane >> 5) * 2 + ((quad ^ (quad >> 1) ^ (quad >> 2)) & 1)) * 16 + (quad >> 1) * 4 + (lane & 3);
  const int vg = vt >> 4, vp = vt & 15;
  int rs, sub;
  if (L == 2) { rs = 4 * vg + (vp >> 2); sub = vp & 3; }
  else if (L == 4) { rs = 8 * (vg >> 2) + (vg & 1) + 4 * ((vg >> 1) & 1) + 2 * (vp >> 3); sub = vp & 7; }
  else if (L == 8) { rs = vg; sub = vp; }
  else { rs = vg >> 1; sub = (vg & 1) * 16 + vp; }
  const bool live = !INTRA && rs * L < q_ext;  // (n % L == 0: a sequence is whole or absent)
  const int my_a = q0 / L + rs;
  float thr_b = 0.f, thr_v = 0.f;
  if (live) {
    thr_b = __fmul_rn(intra_sum[my_a], L2);
    thr_v = __fadd_rn(thr_b, __fmul_rn(d.margin, L2 * L2L));
  }
  int n_before = 0, n_viol = 0;
  float s_hinge = 0.f, s_inter = 0.f;

  const int nT = (hi - lo + KNN_BT - 1) / KNN_BT;
  PairTile pt(lds, qb, D, q_ext);
  auto load = [&](int ti, int ks) { pt.load(z, lo, hi, ti, ks); };
  if (nT > 0) load(0, 0);
  for (int ti = 0; ti < nT; ++ti) {
    // the tile's norms are asked for before the k loop, so that their latency is not paid between the loop and the epilogue
    const int t0 = lo + ti * KNN_BT;
    float ts_pre[4];
    pt.col_norms(ts_pre, z_sq, t0, hi);
    f32x4 acc[2][4];
    pt.product(acc, ti, nT, load);
    pt.write_d2(acc, ts_pre);
    if (INTRA) {
      // tile ti holds the own blocks of query rows 64 ti .. 64 ti + 63: block column = block row
      const int r0 = ti * KNN_BT;
      for (int idx = tid; idx < KNN_BT * L; idx += 256) {
        const int r = idx / L, c = idx - r * L, qr = r0 + r;
        if (qr < q_ext) intra_d2[(long)(q0 + qr) * L + c] = d2s[qr * DP + (r / L) * L + c];
      }
      if (tid < NBT && r0 + tid * L < q_ext) {
        float sum = 0.f;
        for (int i = 0; i < L; ++i)
          for (int j = 0; j < L; ++j)
            if (i != j) sum += pair_fn<FN>(d2s[(r0 + tid * L + i) * DP + tid * L + j]);
        const int a = (q0 + r0) / L + tid;
        intra_sum[a] = sum;
        before[a] = 0;
        viol[a] = 0;
      }
    } else if (live) {
      const int b_valid = (hi - t0 < KNN_BT ? hi - t0 : KNN_BT) / L;  // whole blocks: hi is n or a multiple of 64
      const int b_self = my_a - t0 / L;                               // the sequence's own block as a column of this tile, if 0 .. NBT - 1
      auto take = [&](float P, int b) {
        if (b < b_valid && b != b_self) {
          const float pl = __fmul_rn(P, L2L);
          n_before += pl < thr_b ? 1 : 0;
          n_viol += pl < thr_v ? 1 : 0;
          // the hinge times L^2 (L^2 - L): positive exactly where viol counts, exact on integer inputs; divided once, after the last sum
          const float h = __fsub_rn(thr_v, pl);
          s_hinge += (h > 0.f || h != h) ? h : 0.f;  // (a NaN pooled value is not counted and makes both sums NaN)
          s_inter += P;
        }
      };
      if (L == 2) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
          const int bp = (sub & 1) + 8 * (sub >> 1) + 2 * it;  // blocks 2 bp and 2 bp + 1: one 16-byte slot
          const float4 v0 = *reinterpret_cast<const float4*>(d2s + (rs * 2) * DP + 4 * bp);
          const float4 v1 = *reinterpret_cast<const float4*>(d2s + (rs * 2 + 1) * DP + 4 * bp);
          float Pa = 0.f, Pb = 0.f;
          Pa += pair_fn<FN>(v0.x); Pa += pair_fn<FN>(v0.y); Pa += pair_fn<FN>(v1.x); Pa += pair_fn<FN>(v1.y);
          Pb += pair_fn<FN>(v0.z); Pb += pair_fn<FN>(v0.w); Pb += pair_fn<FN>(v1.z); Pb += pair_fn<FN>(v1.w);
          take(Pa, 2 * bp);
          take(Pb, 2 * bp + 1);
        }
      } else {
#pragma unroll
        for (int it = 0; it < (NBT + TPS - 1) / TPS; ++it) {
          const int b = sub + TPS * it;
          if (b < NBT) {
            float P = 0.f;
#pragma unroll
            for (int i = 0; i < L; ++i) {
              const float4* row = reinterpret_cast<const float4*>(d2s + (rs * L + i) * DP + b * L);
#pragma unroll
              for (int c = 0; c < L / 4; ++c) {
                const float4 v = row[c];
                P += pair_fn<FN>(v.x); P += pair_fn<FN>(v.y); P += pair_fn<FN>(v.z); P += pair_fn<FN>(v.w);
              }
            }
            take(P, b);
          }
        }
      }
    }
  }
  if (!INTRA) {
    // the threads of a sequence, in the order of sub, through the distance tile's first 1024 words (every thread writes its slot: rs, sub
    // is a renumbering of the 256 threads)
    __syncthreads();
    const int slot = rs * TPS + sub;
    int* d2i = reinterpret_cast<int*>(d2s);
    d2s[slot] = s_hinge;
    d2s[256 + slot] = s_inter;
    d2i[512 + slot] = n_before;
    d2i[768 + slot] = n_viol;
    __syncthreads();
    if (tid < NRS && tid * L < q_ext) {
      float h = d2s[tid * TPS], in = d2s[256 + tid * TPS];
      int nb = d2i[512 + tid * TPS], nv = d2i[768 + tid * TPS];
      for (int k = 1; k < TPS; ++k) {
        h += d2s[tid * TPS + k];
        in += d2s[256 + tid * TPS + k];
        nb += d2i[512 + tid * TPS + k];
        nv += d2i[768 + tid * TPS + k];
      }
      const int a = q0 / L + tid;
      if (nb) atomicAdd(before + a, nb);
      if (nv) atomicAdd(viol + a, nv);
      // one slice: part_* are the outputs themselves
      const long at = d.slices == 1 ? (long)a : ((long)q_tile * d.slices + s) * KNN_BT + tid;
      part_hinge[at] = d.slices == 1 ? h / (L2 * L2L) : h;
      part_inter[at] = in;
    }
  }
}

// hinge_sum[a], inter_sum[a] = the slices' partials [q tiles, slices, 64] in slice order
__global__ __launch_bounds__(256) void seqrank_reduce_kernel(const focal_seqrank_desc d, const float* __restrict__ part_hinge,
                                                             const float* __restrict__ part_inter, float* __restrict__ hinge_sum,
                                                             float* __restrict__ inter_sum) {
  const int a = (int)(blockIdx.x * 256 + threadIdx.x);
  if (a >= d.n / d.L) return;
  const int nrs = KNN_BQ / d.L;
  const long base = (long)(a / nrs) * d.slices * KNN_BT + a % nrs;
  float h = part_hinge[base], in = part_inter[base];
  for (int s = 1; s < d.slices; ++s) {
    h += part_hinge[base + (long)s * KNN_BT];
    in += part_inter[base + (long)s * KNN_BT];
  }
  hinge_sum[a] = h / ((float)(d.L * d.L) * (float)(d.L * d.L - d.L));
  inter_sum[a] = in;
}

static int seqrank_check_desc(const focal_seqrank_desc* d, const char* who) {
  FOCAL_CHECK_ARG(d, "%s: null descriptor", who);
  const int rc = knn_check_tile_desc(who, d->D, d->slices, d->n, "n");
  if (rc != FOCAL_OK) return rc;
  FOCAL_CHECK_ARG(d->L == 2 || d->L == 4 || d->L == 8 || d->L == 16, "%s: need L in {2, 4, 8, 16} (got L=%d)", who, d->L);
  FOCAL_CHECK_ARG(d->n >= 1 && d->n % d->L == 0, "%s: need n %% L == 0 (got n=%d L=%d)", who, d->n, d->L);
  FOCAL_CHECK_ARG(d->n / d->L >= 2, "%s: need S = n / L >= 2 sequences (got n=%d L=%d)", who, d->n, d->L);
  FOCAL_CHECK_ARG(d->fn == FOCAL_PAIR_SQDIST || d->fn == FOCAL_PAIR_DIST, "%s: need fn in 0 .. 1 (sqdist, dist; got fn=%d)", who, d->fn);
  FOCAL_CHECK_ARG(std::isfinite(d->margin), "%s: need a finite margin (got margin=%g)", who, (double)d->margin);
  return FOCAL_OK;
}

// the slices' partials of the two float sums, [2][q tiles, slices, 64]; with one slice the scan writes the outputs itself
extern "C" size_t focal_seq_rank_workspace(const focal_seqrank_desc* d) {
  if (seqrank_check_desc(d, "seq_rank_workspace") != FOCAL_OK) return 0;
  if (d->slices == 1) return 16;
  return 2 * (size_t)ceil_div(d->n, KNN_BQ) * (size_t)d->slices * KNN_BT * sizeof(float);
}

typedef void (*seqrank_kern_t)(const focal_seqrank_desc, const float*, const float*, float*, float*, int*, int*, float*, float*);

template <bool INTRA>
static seqrank_kern_t seqrank_pick(int fn, int L) {
#define SEQRANK_ROW(FN) {seqrank_kernel<FN, 2, INTRA>, seqrank_kernel<FN, 4, INTRA>, seqrank_kernel<FN, 8, INTRA>, seqrank_kernel<FN, 16, INTRA>}
  static const seqrank_kern_t kerns[2][4] = {SEQRANK_ROW(FOCAL_PAIR_SQDIST), SEQRANK_ROW(FOCAL_PAIR_DIST)};
#undef SEQRANK_ROW
  return kerns[fn][L == 2 ? 0 : L == 4 ? 1 : L == 8 ? 2 : 3];
}

extern "C" int focal_seq_rank(const focal_seqrank_desc* d, const float* z, const float* z_sq, float* intra_d2, float* intra_sum, int* before,
                              int* viol, float* hinge_sum, float* inter_sum, void* ws, size_t ws_bytes, void* stream) {
  const int rc = seqrank_check_desc(d, "seq_rank");
  if (rc != FOCAL_OK) return rc;
  FOCAL_CHECK_ARG(z && z_sq && intra_d2 && intra_sum && before && viol && hinge_sum && inter_sum, "seq_rank: null tensor");
  FOCAL_CHECK_ARG(((uintptr_t)z & 15) == 0, "seq_rank: z must be 16-byte aligned");
  FOCAL_CHECK_ARG(ws && ws_bytes >= focal_seq_rank_workspace(d), "seq_rank: workspace of %zu bytes, need %zu", ws ? ws_bytes : (size_t)0,
                  focal_seq_rank_workspace(d));
  const int q_tiles = ceil_div(d->n, KNN_BQ), S = d->n / d->L;
  const size_t half = (size_t)q_tiles * (size_t)d->slices * KNN_BT;
  float* ph = d->slices == 1 ? hinge_sum : (float*)ws;
  float* pi = d->slices == 1 ? inter_sum : (float*)ws + half;
  FOCAL_LAUNCH(seqrank_pick<true>(d->fn, d->L), dim3((unsigned)q_tiles), dim3(256), 0, (hipStream_t)stream, *d, z, z_sq, intra_d2, intra_sum,
               before, viol, ph, pi);
  FOCAL_LAUNCH_CHECK();
  FOCAL_LAUNCH(seqrank_pick<false>(d->fn, d->L), dim3((unsigned)q_tiles * (unsigned)d->slices), dim3(256), 0, (hipStream_t)stream, *d, z, z_sq,
               intra_d2, intra_sum, before, viol, ph, pi);
  FOCAL_LAUNCH_CHECK();
  if (d->slices > 1) {
    FOCAL_LAUNCH(seqrank_reduce_kernel, dim3((unsigned)ceil_div(S, 256)), dim3(256), 0, (hipStream_t)stream, *d, (const float*)ph,
                 (const float*)pi, hinge_sum, inter_sum);
    FOCAL_LAUNCH_CHECK();
  }
  return FOCAL_OK;
}
