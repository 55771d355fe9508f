// What focal_knn_search (knn.hip) and focal_kmeans_assign (kmeans.hip) share, so that d2 of a pair of rows is the same bits in both: the
// tile sizes of the exact-fp32 distance product, the order-preserving key of a distance and the fixed tree that takes |q|^2.
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
