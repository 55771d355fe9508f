// Location fusion of SW_Transformer on multi-location datasets (models/SW_Transformer.py:126-150 / :226-242 of the reference):
// per modality, the L location features of a sample form a sequence of L tokens that runs through `loc_block_num`
// nn.TransformerEncoderLayer (post-norm, ReLU) and one TransformerFusionBlock.  The matrix products of those layers run on the
// GEMM family, LayerNorm on norm.hip, the fusion block's attention on head.hip; this file holds what has no kernel elsewhere:
//   focal_loc_attn_fwd / _bwd   the self-attention core of the encoder layer: every token attends over the L tokens of its
//                               sequence (nn.MultiheadAttention, head_dim 64, softmax(QK^T / 8) with dropout on the weights)
//   focal_loc_stack             the L encoder outputs [N, E] -> one [N, L, E] sequence buffer (the stage's input)
//   focal_loc_unstack_add       a + b of two [N, L, E] gradients, written location-major [L, N, E]: one contiguous gradient per encoder
//   focal_loc_mean_bwd_add      dx[n, l, :] += dq[n, :] / L: the fusion block's query is the mean of the L normalised tokens
// Tensors are [N <= a few thousand, L <= 8, E <= 256] fp32: kilobytes to a few MB.  One workgroup per sequence, one wave per head
// (head_dim 64 = one lane per channel): dot products are wave reductions, the L x L softmax lives in registers.
#include "common.hpp"

#define LOC_MAX_L 8

// qkv [N*L, 3E] rows (n, i) = {q | k | v}; out [N*L, E]; probs / weights [N, H, L, L] = softmax and softmax * dropout mask
__global__ __launch_bounds__(256) void loc_attn_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                           float* __restrict__ probs, float* __restrict__ weights, int L, int E, int H,
                                                           float scale, const uint32_t* rng, uint32_t stream, float p_drop) {
  const int n = blockIdx.x, e = threadIdx.x, h = e >> 6;
  if (e >= E) return;  // (E is a multiple of 64: whole waves leave)
  const DropCtx dc = make_drop(rng, stream, p_drop);
  const long row0 = (long)n * L;
  float k[LOC_MAX_L], v[LOC_MAX_L];
#pragma unroll
  for (int j = 0; j < LOC_MAX_L; ++j) {
    if (j < L) {
      k[j] = qkv[(row0 + j) * 3 * E + E + e];
      v[j] = qkv[(row0 + j) * 3 * E + 2 * E + e];
    }
  }
  for (int i = 0; i < L; ++i) {
    const float qe = qkv[(row0 + i) * 3 * E + e] * scale;
    float s[LOC_MAX_L], mx = -3.0e38f;
#pragma unroll
    for (int j = 0; j < LOC_MAX_L; ++j) {
      if (j < L) {
        s[j] = wave_sum(qe * k[j]);
        mx = fmaxf(mx, s[j]);
      }
    }
    float den = 0.f;
#pragma unroll
    for (int j = 0; j < LOC_MAX_L; ++j) {
      if (j < L) { s[j] = expf(s[j] - mx); den += s[j]; }
    }
    const float rden = 1.0f / den;
    const long pbase = (((long)n * H + h) * L + i) * L;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < LOC_MAX_L; ++j) {
      if (j < L) {
        const float pj = s[j] * rden;
        const float wj = p_drop > 0.f ? pj * drop_mult(dc, (uint32_t)(pbase + j)) : pj;
        acc += wj * v[j];
        if ((e & 63) == j) { probs[pbase + j] = pj; weights[pbase + j] = wj; }  // (lane j of the head's wave writes entry j)
      }
    }
    out[(row0 + i) * E + e] = acc;
  }
}

// dqkv [N*L, 3E] (same packing as qkv) from dout [N*L, E]
__global__ __launch_bounds__(256) void loc_attn_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ probs,
                                                           const float* __restrict__ weights, const float* __restrict__ dout,
                                                           float* __restrict__ dqkv, int L, int E, int H, float scale) {
  const int n = blockIdx.x, e = threadIdx.x, h = e >> 6;
  if (e >= E) return;
  const long row0 = (long)n * L;
  float k[LOC_MAX_L], v[LOC_MAX_L], dk[LOC_MAX_L], dv[LOC_MAX_L];
#pragma unroll
  for (int j = 0; j < LOC_MAX_L; ++j) {
    if (j < L) {
      k[j] = qkv[(row0 + j) * 3 * E + E + e];
      v[j] = qkv[(row0 + j) * 3 * E + 2 * E + e];
    }
    dk[j] = 0.f;
    dv[j] = 0.f;
  }
  for (int i = 0; i < L; ++i) {
    const float go = dout[(row0 + i) * E + e], qi = qkv[(row0 + i) * 3 * E + e];
    const long pbase = (((long)n * H + h) * L + i) * L;
    float p[LOC_MAX_L], dp[LOC_MAX_L], dot = 0.f;
#pragma unroll
    for (int j = 0; j < LOC_MAX_L; ++j) {
      if (j < L) {
        p[j] = probs[pbase + j];
        const float wj = weights[pbase + j];
        const float mj = p[j] > 0.f ? wj / p[j] : 0.f;  // dropout multiplier (0 or 1 / (1 - p))
        dv[j] += wj * go;                                 // dV_j += w_ij dO_i
        dp[j] = wave_sum(go * v[j]) * mj;                 // dL / d p_ij
        dot += p[j] * dp[j];
      }
    }
    float dq = 0.f;
#pragma unroll
    for (int j = 0; j < LOC_MAX_L; ++j) {
      if (j < L) {
        const float ds = p[j] * (dp[j] - dot) * scale;   // dL / d(q_i . k_j), the 1/8 folded in
        dq += ds * k[j];
        dk[j] += ds * qi;
      }
    }
    dqkv[(row0 + i) * 3 * E + e] = dq;
  }
#pragma unroll
  for (int j = 0; j < LOC_MAX_L; ++j) {
    if (j < L) {
      dqkv[(row0 + j) * 3 * E + E + e] = dk[j];
      dqkv[(row0 + j) * 3 * E + 2 * E + e] = dv[j];
    }
  }
}

static int check_loc_geometry(const char* what, int N, int L, int E, int heads) {
  FOCAL_CHECK_ARG(N > 0 && L >= 2 && L <= LOC_MAX_L && heads >= 1 && E == heads * 64 && E <= 256,
                  "%s: need head_dim 64, E <= 256, 2 <= L <= %d (got N=%d L=%d E=%d heads=%d)", what, LOC_MAX_L, N, L, E, heads);
  return FOCAL_OK;
}

extern "C" int focal_loc_attn_fwd(int N, int L, int E, int heads, const float* qkv, float* out, float* probs, float* weights,
                                  const uint32_t* rng, uint32_t stream_id, float p_drop, void* stream) {
  FOCAL_CHECK_ARG(qkv && out && probs && weights, "loc_attn_fwd: null tensor");
  if (int rc = check_loc_geometry("loc_attn_fwd", N, L, E, heads)) return rc;
  FOCAL_CHECK_ARG(p_drop >= 0.f && p_drop < 1.f && (p_drop == 0.f || rng), "loc_attn_fwd: dropout needs 0 <= p < 1 and an rng state");
  FOCAL_LAUNCH(loc_attn_fwd_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, qkv, out, probs, weights, L, E, heads, 0.125f, rng,
               stream_id, p_drop);  // 1 / sqrt(64)
  FOCAL_LAUNCH_CHECK();
  return FOCAL_OK;
}

extern "C" int focal_loc_attn_bwd(int N, int L, int E, int heads, const float* qkv, const float* probs, const float* weights,
                                  const float* dout, float* dqkv, void* stream) {
  FOCAL_CHECK_ARG(qkv && probs && weights && dout && dqkv, "loc_attn_bwd: null tensor");
  if (int rc = check_loc_geometry("loc_attn_bwd", N, L, E, heads)) return rc;
  FOCAL_LAUNCH(loc_attn_bwd_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, qkv, probs, weights, dout, dqkv, L, E, heads, 0.125f);
  FOCAL_LAUNCH_CHECK();
  return FOCAL_OK;
}

// ------------------------------------------------------------------------------------------------ layout glue (element-wise, float4)
struct LocPtrs {
  const float* p[LOC_MAX_L];
};
struct LocOutPtrs {
  float* p[LOC_MAX_L];
};

// out[n][l][:] = feats[l][n][:]
__global__ __launch_bounds__(256) void loc_stack_kernel(LocPtrs feats, float4* __restrict__ out, int N, int L, int E4) {
  const long total = (long)N * L * E4;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const int c = (int)(t % E4);
    const long nl = t / E4;
    const int l = (int)(nl % L);
    const long n = nl / L;
    out[t] = reinterpret_cast<const float4*>(feats.p[l])[n * E4 + c];
  }
}

// dst[l][n][:] = a[n][l][:] + b[n][l][:]
__global__ __launch_bounds__(256) void loc_unstack_add_kernel(const float4* __restrict__ a, const float4* __restrict__ b, LocOutPtrs dst,
                                                              int N, int L, int E4) {
  const long total = (long)N * L * E4;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const int c = (int)(t % E4);
    const long nl = t / E4;
    const int l = (int)(nl % L);
    const long n = nl / L;
    const float4 x = a[t], y = b[t];
    reinterpret_cast<float4*>(dst.p[l])[n * E4 + c] = make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w);
  }
}

// dx[n][l][:] += dq[n][:] / L
__global__ __launch_bounds__(256) void loc_mean_bwd_add_kernel(const float4* __restrict__ dq, float4* __restrict__ dx, int N, int L, int E4,
                                                               float fl) {
  const long total = (long)N * L * E4;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const int c = (int)(t % E4);
    const long n = t / E4 / L;
    const float4 g = dq[n * E4 + c];
    float4 x = dx[t];
    x.x += g.x / fl; x.y += g.y / fl; x.z += g.z / fl; x.w += g.w / fl;
    dx[t] = x;
  }
}

static int loc_grid(long n4) { return (int)(n4 / 256 + 1 < 2048 ? n4 / 256 + 1 : 2048); }

static bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

extern "C" int focal_loc_stack(int N, int L, int E, const float* const* feats, float* out, void* stream) {
  FOCAL_CHECK_ARG(N > 0 && L >= 1 && L <= LOC_MAX_L && E > 0 && E % 4 == 0 && feats && out && aligned16(out),
                  "loc_stack: bad argument (N=%d L=%d E=%d)", N, L, E);
  LocPtrs f;
  for (int l = 0; l < LOC_MAX_L; ++l) f.p[l] = nullptr;
  for (int l = 0; l < L; ++l) {
    FOCAL_CHECK_ARG(feats[l] && aligned16(feats[l]), "loc_stack: feature %d null or not 16-byte aligned", l);
    f.p[l] = feats[l];
  }
  FOCAL_LAUNCH(loc_stack_kernel, dim3(loc_grid((long)N * L * E / 4)), dim3(256), 0, (hipStream_t)stream, f, reinterpret_cast<float4*>(out),
               N, L, E / 4);
  FOCAL_LAUNCH_CHECK();
  return FOCAL_OK;
}

extern "C" int focal_loc_unstack_add(int N, int L, int E, const float* a, const float* b, float* const* dst, void* stream) {
  FOCAL_CHECK_ARG(N > 0 && L >= 1 && L <= LOC_MAX_L && E > 0 && E % 4 == 0 && a && b && dst && aligned16(a) && aligned16(b),
                  "loc_unstack_add: bad argument (N=%d L=%d E=%d)", N, L, E);
  LocOutPtrs d;
  for (int l = 0; l < LOC_MAX_L; ++l) d.p[l] = nullptr;
  for (int l = 0; l < L; ++l) {
    FOCAL_CHECK_ARG(dst[l] && aligned16(dst[l]), "loc_unstack_add: output %d null or not 16-byte aligned", l);
    d.p[l] = dst[l];
  }
  FOCAL_LAUNCH(loc_unstack_add_kernel, dim3(loc_grid((long)N * L * E / 4)), dim3(256), 0, (hipStream_t)stream,
               reinterpret_cast<const float4*>(a), reinterpret_cast<const float4*>(b), d, N, L, E / 4);
  FOCAL_LAUNCH_CHECK();
  return FOCAL_OK;
}

extern "C" int focal_loc_mean_bwd_add(int N, int L, int E, const float* dq, float* dx, void* stream) {
  FOCAL_CHECK_ARG(N > 0 && L >= 1 && E > 0 && E % 4 == 0 && dq && dx && aligned16(dq) && aligned16(dx),
                  "loc_mean_bwd_add: bad argument (N=%d L=%d E=%d)", N, L, E);
  FOCAL_LAUNCH(loc_mean_bwd_add_kernel, dim3(loc_grid((long)N * L * E / 4)), dim3(256), 0, (hipStream_t)stream,
               reinterpret_cast<const float4*>(dq), reinterpret_cast<float4*>(dx), N, L, E / 4, (float)L);
  FOCAL_LAUNCH_CHECK();
  return FOCAL_OK;
}
