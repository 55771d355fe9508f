// What the evaluation tools' tile kernels share (knn.hip, kmeans.hip, probe.hip, tsne.hip, rank.hip, pairsum.hip, seqrank.hip), so that
// d2 of a pair of rows is the same bits in all of them BY CONSTRUCTION: the tile sizes of the exact-fp32 distance product, the
// order-preserving key of a distance, the fixed tree that takes |q|^2, and PairTile -- the staging, the k loop and the write of the
// distance tile.  d2 of a pair is a function of the two rows alone: the k-ordered fma chain of the MFMA from k = 0, |q|^2 by the fixed
// tree, |t|^2 passed in, joined by ONE fmaf -- whatever tile, lane, slice or kernel the pair falls into.
#pragma once
#include "gemm.hpp"

constexpr int KNN_BQ = 128, KNN_BT = 64, KNN_BK = 32;
constexpr unsigned long long KNN_EMPTY = ~0ull;

__device__ __forceinline__ uint32_t knn_key(float d) {
  if (d != d) return 0xFFFFFFFFu;
  const uint32_t u = __float_as_uint(d + 0.0f);  // (-0 -> +0)
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float knn_unkey(uint32_t k) {
  if (k == 0xFFFFFFFFu) return __uint_as_float(0x7FC00000u);
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// |q|^2 of the workgroup's KNN_BQ rows (256 threads): 8 lanes per row, each a k-ordered fma chain over its 16-byte chunks, joined by a
// fixed xor tree -- the same for every row
__device__ __forceinline__ void knn_row_norms(const float* __restrict__ qb, int D, int q_ext, int tid, float* __restrict__ qsq_s) {
#pragma unroll
  for (int pass = 0; pass < KNN_BQ / 32; ++pass) {
    const int row = pass * 32 + (tid >> 3), part = tid & 7;
    float sum = 0.f;
    if (row < q_ext) {
      const float4* src = reinterpret_cast<const float4*>(qb + (long)row * D);
      for (int c = part; c < D / 4; c += 8) {
        const float4 v = src[c];
        sum = fmaf(v.x, v.x, sum); sum = fmaf(v.y, v.y, sum); sum = fmaf(v.z, v.z, sum); sum = fmaf(v.w, v.w, sum);
      }
    }
    sum += __shfl_xor(sum, 1, 64);
    sum += __shfl_xor(sum, 2, 64);
    sum += __shfl_xor(sum, 4, 64);
    if (part == 0) qsq_s[row] = sum;
  }
}

// Slice s of `slices` contiguous slices of n rows: [lo, hi), empty past the last row.
__device__ __forceinline__ void knn_slice(int n, int slices, int s, int& lo, int& hi) {
  const long per = ((long)n + slices - 1) / slices;
  const long lo_l = (long)s * per < (long)n ? (long)s * per : (long)n;
  lo = (int)lo_l;
  hi = (int)(lo_l + per < (long)n ? lo_l + per : (long)n);
}

// f(max(d2, 0)) of the pooled-distance tools (FN: FOCAL_PAIR_SQDIST, FOCAL_PAIR_DIST, FOCAL_PAIR_GAUSS; scale is read by the last alone)
template <int FN>
__device__ __forceinline__ float pair_fn(float d2, float scale = 0.f) {
  const float x = d2 < 0.f ? 0.f : d2;  // (a NaN distance stays NaN)
  if (FN == FOCAL_PAIR_SQDIST) return x;
  if (FN == FOCAL_PAIR_DIST) return sqrtf(x);
  return expf(-scale * x);
}

// The 128 x 64 tile of q . t for one workgroup of 256 threads: the exact-fp32 MFMA product (v_mfma_f32_16x16x4_f32) on the fp32 GEMM
// family's staging (gemm.hpp: OperandStage / FragLoad, one LDS buffer, the next k block's global loads in registers).  Wave w owns query
// rows 32 w .. 32 w + 31: acc[i][j][r] is row row(i, r), column col(j) of the tile.
struct PairTile {
  using StQ = OperandStage<float, float, false, PRO_NONE, KNN_BQ, 1>;
  using StT = OperandStage<float, float, false, PRO_NONE, KNN_BT, 1>;
  using FQ = FragLoad<float, false, StQ::PITCH>;
  using FT = FragLoad<float, false, StT::PITCH>;
  static_assert(GemmCfg<float>::BK == KNN_BK, "k-step of the fp32 staging");
  static constexpr int DP = KNN_BT + 4;  // pitch of the distance tile (16-byte rows for the epilogues' ds_read_b128; 4 pad columns)
  struct __attribute__((aligned(16))) Lds {
    float d2[KNN_BQ * DP];  // first: the paired stores of write_d2 (ds_write2_b32) reach 1020 bytes from their base and no further
    float q[StQ::LDS_ELEMS], t[StT::LDS_ELEMS];
    float qsq[KNN_BQ];  // knn_row_norms of the query rows: the caller fills it (and decides whether a barrier follows)
  };

  Lds& s;
  const float* qb;  // the workgroup's first query row, q_ext of which exist
  const int D, q_ext, nK, tid, lane, wave;
  MaskEval me;  // (PRO_NONE: never read)
  // st before sq: in the other order the register allocator (ROCm 7.2's clang, gfx950) splits the last 16-byte chunk of the query stage
  // around the MFMAs and waits for it with s_waitcnt vmcnt(0) right behind its global load, at every one of the three load sites --
  // the prefetch then hides nothing (profiles/pair_tile_fold.txt: + 6 % at D = 128, + 9 % at D = 256)
  StT st;
  StQ sq;

  __device__ __forceinline__ PairTile(Lds& lds, const float* qb_, int D_, int q_ext_)
      : s(lds), qb(qb_), D(D_), q_ext(q_ext_), nK((D_ + KNN_BK - 1) / KNN_BK), tid(threadIdx.x), lane(threadIdx.x & 63), wave(threadIdx.x >> 6) {
    sq.init(D, 0, tid);
    st.init(D, 0, tid);
  }
  __device__ __forceinline__ int row(int i, int r) const { return wave * 32 + i * 16 + 4 * (lane >> 4) + r; }
  __device__ __forceinline__ int col(int j) const { return j * 16 + (lane & 15); }

  // Requests k block ks of the query rows, and of tile ti (KNN_BT rows) of the contiguous gallery rows t[lo .. hi).  Rows past hi (or a
  // ragged k block) arrive as zeros.  A caller with other gallery rows fills st.raw[] itself.
  __device__ __forceinline__ void load_q(int ks) { sq.load(qb, D, 0, ks * KNN_BK, q_ext, D, tid, me); }
  __device__ __forceinline__ void load(const float* __restrict__ t, int lo, int hi, int ti, int ks) {
    const int t0 = lo + ti * KNN_BT;
    load_q(ks);
    st.load(t + (long)t0 * D, D, 0, ks * KNN_BK, hi - t0, D, tid, me);
  }

  // acc = the product of tile ti of a walk of nT tiles, whose k block 0 has been requested.  load(ti, ks) requests a k block; the one
  // after (ti, ks) -- the next tile's first after this tile's last -- is requested right after the barrier that publishes (ti, ks), so
  // it is in flight under the MFMAs.  The second barrier lets the next store overwrite the stages.
  template <class Load>
  __device__ __forceinline__ void product(f32x4 (&acc)[2][4], int ti, int nT, Load&& load) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < nK; ++ks) {
      sq.template store<false>(s.q, 0, ks * KNN_BK, tid, me, nullptr);
      st.template store<false>(s.t, 0, ks * KNN_BK, tid, me, nullptr);
      __syncthreads();
      if (ks + 1 < nK) load(ti, ks + 1);
      else if (ti + 1 < nT) load(ti + 1, 0);
#pragma unroll
      for (int kk = 0; kk < KNN_BK / 4; ++kk) {
        float xq[2], xt[4];
#pragma unroll
        for (int i = 0; i < 2; ++i) xq[i] = FQ::load(s.q, wave * 32 + i * 16, kk, lane);
#pragma unroll
        for (int j = 0; j < 4; ++j) xt[j] = FT::load(s.t, j * 16, kk, lane);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = mma16(xq[i], xt[j], acc[i][j]);
      }
      __syncthreads();
    }
  }

  // |t|^2 of the lane's four columns of the tile that starts at gallery row t0 of t[.. hi): 0 past hi
  __device__ __forceinline__ void col_norms(float (&ts)[4], const float* __restrict__ t_sq, int t0, int hi) const {
#pragma unroll
    for (int j = 0; j < 4; ++j) ts[j] = t0 + col(j) < hi ? t_sq[t0 + col(j)] : 0.f;
  }

  // The distance tile d2 = (|q|^2 + |t|^2) - 2 q.t, ts[j] = |t|^2 of column col(j).  Written after the k loop's last barrier and
  // published by the barrier here; the next tile's k loop has barriers of its own before anything writes it again.
  __device__ __forceinline__ void write_d2(const f32x4 (&acc)[2][4], const float (&ts)[4]) {
    // |q|^2 of the lane's rows first: qsq and d2 are members of one object, and a load the compiler cannot move above a store to d2
    // would be repeated per column.  The lane's 16 cells of block i lie at constant offsets r DP + 16 j from one address, spelt so:
    // the stores of two rows pair (ds_write2_b32), as they did when every kernel spelt this loop itself.
    float qs[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) qs[i][r] = s.qsq[row(i, r)];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      float* cell = s.d2 + row(i, 0) * DP + col(0);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) cell[r * DP + 16 * j] = fmaf(-2.0f, acc[i][j][r], qs[i][r] + ts[j]);
    }
    __syncthreads();
  }
};

// The descriptor checks the sliced tile exports spell alike (n_name: what the descriptor calls its query rows)
static inline int knn_check_tile_desc(const char* who, int D, int slices, int n, const char* n_name) {
  FOCAL_CHECK_ARG(D >= 4 && D % 4 == 0, "%s: need D >= 4 and D %% 4 == 0 (got D=%d)", who, D);
  FOCAL_CHECK_ARG(slices >= 1 && slices <= 65535, "%s: need 1 <= slices <= 65535 (got slices=%d)", who, slices);
  FOCAL_CHECK_ARG((long)ceil_div(n, KNN_BQ) * slices < (1L << 31), "%s: %s / %d * slices exceeds the launch grid (%s=%d slices=%d)", who,
                  n_name, KNN_BQ, n_name, n, slices);
  return FOCAL_OK;
}
