// Fused AdamW over the flat parameter arena + bf16 shadow refresh + device-side step / seed bookkeeping.
// HBM-bound: 16 B read + 12 B written per parameter (+2 B shadow), float4 per lane.
#include "common.hpp"

__global__ void rng_advance_kernel(uint32_t* state) {
  state[0] = focal_mix32(state[0] + 0x9E3779B9U);
  state[1] += 1u;
}

extern "C" int focal_rng_advance(uint32_t* state, void* stream) {
  FOCAL_CHECK_ARG(state != nullptr, "rng_advance: null state");
  FOCAL_LAUNCH(rng_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state);
  FOCAL_LAUNCH_CHECK();
  return FOCAL_OK;
}

// Diagnostic: slots[index] = the device's constant-rate wall clock (100 MHz) when this one-thread launch runs -- a marker that can sit INSIDE
// a captured hipGraph, where events cannot be read and rocprofv3 serialises the branches (tools/phase_marks.py).
__global__ void mark_kernel(unsigned long long* slots, int index) { slots[index] = wall_clock64(); }

extern "C" int focal_mark(unsigned long long* slots, int index, void* stream) {
  FOCAL_CHECK_ARG(slots != nullptr && index >= 0, "mark: null buffer or negative index");
  FOCAL_LAUNCH(mark_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, slots, index);
  FOCAL_LAUNCH_CHECK();
  return FOCAL_OK;
}

// torch.optim.AdamW: p *= 1 - lr*wd; m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
// p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
// advance != 0 (focal_adamw_multi_advance): the update uses step count step_state[1] + 1, and the workgroup that finishes LAST -- by
// then every workgroup has read the count -- advances step_state and seed_state the way focal_rng_advance would (tickets in
// step_state[2] and step_state[8 .. 39]: FOCAL_STEP_STATE_WORDS = 40 zero-initialised words): the step's two one-thread bookkeeping launches ride on the optimizer kernel.
// g * coef rounded ONCE (no contraction into the L2-decay term g + wd * p that follows): the clipped update is the plain update on
// torch's pre-scaled gradient, bit for bit
__device__ __forceinline__ float4 scale_rn(float4 g, float coef) {
#pragma clang fp contract(off)
  g.x = g.x * coef; g.y = g.y * coef; g.z = g.z * coef; g.w = g.w * coef;
  return g;
}

// The bookkeeping tail of an `advance` launch (adamw_body, lamb_apply_kernel): the workgroup that finishes last advances the step count
// (not on a skipped step) and the dropout seed.  `count` is the step count this workgroup read before its stores.
template <bool CLIP>
__device__ __forceinline__ void step_tail(uint32_t* rng_state, uint32_t* seed_state, uint32_t count, bool skip) {
  __syncthreads();
  if (threadIdx.x == 0) {
    // (no fence: a workgroup's read of the step count has returned -- its value went into every store above -- before it takes a
    // ticket, and the words written below are read by later kernels only.  __threadfence() here is an L2 write-back per workgroup:
    // it tripled the kernel's duration.)  Two ticket levels -- 32 groups of workgroups, then the groups -- because atomics onto ONE
    // word are a serial chain of ~10 ns links: 2048 workgroups on one ticket added 12 us to DeepSense's 26 us launch.
    const uint32_t grp = blockIdx.x & 31u, ngrp = gridDim.x < 32u ? gridDim.x : 32u;
    const uint32_t gsize = (gridDim.x - grp + 31u) >> 5;
    const uint32_t ticket_one = 1u + (count & 0u);  // == 1, computed from the count that was read
    if (atomicAdd(rng_state + 8 + grp, ticket_one) == gsize - 1u) {
      rng_state[8 + grp] = 0u;
      if (atomicAdd(rng_state + 2, 1u) == ngrp - 1u) {
        rng_state[2] = 0u;
        if (!(CLIP && skip)) {
          rng_state[0] = focal_mix32(rng_state[0] + 0x9E3779B9U);
          rng_state[1] += 1u;
        }
        if (seed_state != nullptr) {
          seed_state[0] = focal_mix32(seed_state[0] + 0x9E3779B9U);
          seed_state[1] += 1u;
        }
      }
    }
  }
}

// The update of adamw_kernel and adamw_clip_kernel.  CLIP: gradients are scaled by `coef` as they are loaded, and `skip` (uniform over the
// launch: a non-finite gradient norm) leaves p, m, v, the shadow and the step count alone -- the last workgroup still advances seed_state.
template <bool CLIP>
__device__ __forceinline__ void adamw_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                           float* __restrict__ v, bf16_t* __restrict__ shadow, long n,
                                           const float* __restrict__ lr_dev, uint32_t* rng_state, uint32_t* seed_state,
                                           int advance, const focal_adamw_desc& d, float coef, bool skip) {
  const float lr = lr_dev[0];
  // (an explicit relaxed atomic load: `count` feeds every store below and, through `ticket_base`, the ticket this workgroup takes -- a data
  // dependence, so the read cannot be ordered behind the ticket whatever the compiler does with the loop)
  const uint32_t count = __atomic_load_n(rng_state + 1, __ATOMIC_RELAXED);
  const float t = (float)(count + (advance ? 1u : 0u));
  const float bc1 = 1.0f - powf(d.beta1, t), bc2 = 1.0f - powf(d.beta2, t);
  // weight decay: decoupled (AdamW: p *= 1 - lr * wd) or, with d.l2_decay, torch.optim.Adam's L2 form (g += wd * p)
  const float step = lr / bc1, isq = rsqrtf(bc2), decay = d.l2_decay ? 1.0f : 1.0f - lr * d.weight_decay;
  const float l2 = d.l2_decay ? d.weight_decay : 0.0f;
  const long n4 = (CLIP && skip) ? 0 : n >> 2;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    float4 pp = reinterpret_cast<float4*>(p)[i];
    const float4 gg = CLIP ? scale_rn(reinterpret_cast<const float4*>(g)[i], coef) : reinterpret_cast<const float4*>(g)[i];
    float4 mm = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
#define ADAM1(c)                                              \
    const float g_##c = gg.c + l2 * pp.c;                     \
    mm.c = d.beta1 * mm.c + (1.0f - d.beta1) * g_##c;         \
    vv.c = d.beta2 * vv.c + (1.0f - d.beta2) * g_##c * g_##c; \
    pp.c = pp.c * decay - step * mm.c / (sqrtf(vv.c) * isq + d.eps);
    ADAM1(x) ADAM1(y) ADAM1(z) ADAM1(w)
#undef ADAM1
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
    if (shadow) {
      bf16x4 s;
      s[0] = (bf16_t)pp.x; s[1] = (bf16_t)pp.y; s[2] = (bf16_t)pp.z; s[3] = (bf16_t)pp.w;
      reinterpret_cast<bf16x4*>(shadow)[i] = s;
    }
  }
  if (advance == 2) step_tail<CLIP>(rng_state, seed_state, count, skip);
}

__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, bf16_t* __restrict__ shadow, long n,
                                                    const float* __restrict__ lr_dev, uint32_t* rng_state, uint32_t* seed_state,
                                                    int advance, focal_adamw_desc d) {
  adamw_body<false>(p, g, m, v, shadow, n, lr_dev, rng_state, seed_state, advance, d, 1.0f, false);
}

// ---- gradient clipping by global L2 norm: one reduction launch, then the update on g * coef
// Sum of squares of every segment: one float4 per lane and trip, ONE accumulator per lane (a chain of 4 additions per trip), then the wave
// (6 levels), then the 4 waves in order; workgroup b stores partials[b].  The slots behind the grid are stored as zero by workgroup 0, so
// the reader sums all FOCAL_CLIP_SCRATCH_WORDS words whatever grid wrote them last.  No atomics, no hand-off between workgroups: the
// kernel boundary publishes the row (the update re-sums it; ~4 KB out of L2 per workgroup).
struct GradSegs { const float* g[FOCAL_CLIP_MAX_SEGMENTS]; long n4[FOCAL_CLIP_MAX_SEGMENTS]; };

__global__ __launch_bounds__(256) void grad_norm_kernel(GradSegs segs, int nseg, float* __restrict__ partials) {
  __shared__ float wsum[4];
  float acc = 0.0f;
  for (int s = 0; s < nseg; ++s) {
    const float4* __restrict__ g = reinterpret_cast<const float4*>(segs.g[s]);
    const long n4 = segs.n4[s];
#pragma unroll 4
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
      const float4 a = g[i];
      acc += a.x * a.x; acc += a.y * a.y; acc += a.z * a.z; acc += a.w * a.w;
    }
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
  if (blockIdx.x == 0)
    for (int i = (int)gridDim.x + threadIdx.x; i < FOCAL_CLIP_SCRATCH_WORDS; i += 256) partials[i] = 0.0f;
}

extern "C" int focal_grad_norm_multi(int nseg, const float* const* g, const long* n, float* partials, int partial_words, void* stream) {
  FOCAL_CHECK_ARG(g && n && partials, "grad_norm_multi: null argument");
  FOCAL_CHECK_ARG(nseg >= 1 && nseg <= FOCAL_CLIP_MAX_SEGMENTS, "grad_norm_multi: %d segments, 1 .. %d fit one launch", nseg, FOCAL_CLIP_MAX_SEGMENTS);
  FOCAL_CHECK_ARG(partial_words >= FOCAL_CLIP_SCRATCH_WORDS, "grad_norm_multi: the scratch row holds %d words, FOCAL_CLIP_SCRATCH_WORDS = %d are written",
                  partial_words, FOCAL_CLIP_SCRATCH_WORDS);
  GradSegs segs = {};
  long total4 = 0;
  for (int s = 0; s < nseg; ++s) {
    FOCAL_CHECK_ARG(n[s] >= 0 && n[s] % 4 == 0, "grad_norm_multi: segment %d length %ld is not a multiple of 4 (arena segments are padded)", s, n[s]);
    FOCAL_CHECK_ARG(n[s] == 0 || (g[s] != nullptr && ((uintptr_t)g[s] & 15) == 0), "grad_norm_multi: segment %d is null or not 16-byte aligned", s);
    segs.g[s] = g[s];
    segs.n4[s] = n[s] / 4;
    total4 += n[s] / 4;
  }
  long blocks = (total4 + 255) / 256;
  blocks = blocks < 1 ? 1 : (blocks > FOCAL_CLIP_MAX_BLOCKS ? FOCAL_CLIP_MAX_BLOCKS : blocks);  // (no gradient at all: one workgroup stores a row of zeros)
  FOCAL_LAUNCH(grad_norm_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, segs, nseg, partials);
  FOCAL_LAUNCH_CHECK();
  return FOCAL_OK;
}

// adamw_kernel on g * coef.  Every workgroup re-sums the partial row in the same fixed order (4 slots per lane, the wave, the 4 waves): the
// same bits everywhere, so coef and the skip decision are uniform over the launch and over the launches of a step's segments without a
// second reduction launch or a fence.  `record` is non-null in ONE launch per step (the last non-empty segment's): workgroup 0's lane 0 is
// its only writer, launches are stream-ordered.
__global__ __launch_bounds__(256) void adamw_clip_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                         float* __restrict__ v, bf16_t* __restrict__ shadow, long n,
                                                         const float* __restrict__ lr_dev, uint32_t* rng_state, uint32_t* seed_state,
                                                         int advance, focal_adamw_desc d, const float* __restrict__ partials,
                                                         uint32_t* record, float max_norm) {
  static_assert(FOCAL_CLIP_SCRATCH_WORDS == 4 * 256, "four slots per lane");
  __shared__ float wsum[4];
  float s = partials[threadIdx.x];
  s += partials[threadIdx.x + 256];
  s += partials[threadIdx.x + 512];
  s += partials[threadIdx.x + 768];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
  __syncthreads();
  const float sq = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
  const float norm = sqrtf(sq);
  const bool skip = !(norm <= 3.402823466e+38f);  // NaN or +inf (a sum of squares that overflowed counts as non-finite)
  const float coef = skip ? 0.0f : fminf(1.0f, max_norm / (norm + 1e-6f));
  if (record != nullptr && blockIdx.x == 0 && threadIdx.x == 0) {
    record[0] += 1u;
    if (skip) {
      record[2] += 1u;
    } else {
      if (coef < 1.0f) record[1] += 1u;
      record[3] = __float_as_uint(__uint_as_float(record[3]) + norm);
      record[4] = __float_as_uint(fmaxf(__uint_as_float(record[4]), norm));
    }
    record[5] = __float_as_uint(norm);
    record[6] = __float_as_uint(sq);
    record[7] = __float_as_uint(coef);
  }
  adamw_body<true>(p, g, m, v, shadow, n, lr_dev, rng_state, seed_state, advance, d, coef, skip);
}

struct ClipArgs { const float* partials; uint32_t* record; float max_norm; };

static int adamw_launch(const focal_adamw_desc* d, int nseg, float* const* p, const float* const* g, float* const* m, float* const* v,
                        void* const* shadow_bf16, const long* n, const float* lr_dev, uint32_t* step_state, uint32_t* seed_state,
                        bool advance, hipStream_t st, const ClipArgs* clip = nullptr) {
  FOCAL_CHECK_ARG(d && p && g && m && v && n && lr_dev && step_state, "adamw_multi: null argument");
  int last = -1;
  for (int s = 0; s < nseg; ++s) {
    FOCAL_CHECK_ARG(n[s] % 4 == 0, "adamw_multi: segment %d length %ld is not a multiple of 4 (arena segments are padded)", s, n[s]);
    if (n[s] > 0) last = s;
  }
  FOCAL_CHECK_ARG(!advance || last >= 0, "adamw_multi_advance: no non-empty segment to carry the step-count advance");
  for (int s = 0; s < nseg; ++s) {
    if (n[s] == 0) continue;
    int blocks = ceil_div(n[s] / 4, 256);
    if (blocks > 2048) blocks = 2048;
    // segments run in stream order: every one of them reads the same step count, the last one advances it
    if (clip) {
      FOCAL_LAUNCH(adamw_clip_kernel, dim3(blocks), dim3(256), 0, st, p[s], g[s], m[s], v[s], shadow_bf16 ? (bf16_t*)shadow_bf16[s] : nullptr,
                         n[s], lr_dev, step_state, (advance && s == last) ? seed_state : nullptr, advance ? (s == last ? 2 : 1) : 0, *d,
                         clip->partials, s == last ? clip->record : nullptr, clip->max_norm);
      continue;
    }
    FOCAL_LAUNCH(adamw_kernel, dim3(blocks), dim3(256), 0, st, p[s], g[s], m[s], v[s], shadow_bf16 ? (bf16_t*)shadow_bf16[s] : nullptr,
                       n[s], lr_dev, step_state, (advance && s == last) ? seed_state : nullptr, advance ? (s == last ? 2 : 1) : 0, *d);
  }
  FOCAL_LAUNCH_CHECK();
  return FOCAL_OK;
}

extern "C" int focal_adamw_multi(const focal_adamw_desc* d, int nseg, float* const* p, const float* const* g, float* const* m,
                                 float* const* v, void* const* shadow_bf16, const long* n, const float* lr_dev,
                                 const uint32_t* rng_state, void* stream) {
  return adamw_launch(d, nseg, p, g, m, v, shadow_bf16, n, lr_dev, const_cast<uint32_t*>(rng_state), nullptr, false, (hipStream_t)stream);
}

extern "C" int focal_adamw_multi_advance(const focal_adamw_desc* d, int nseg, float* const* p, const float* const* g, float* const* m,
                                         float* const* v, void* const* shadow_bf16, const long* n, const float* lr_dev,
                                         uint32_t* step_state, int step_state_words, uint32_t* seed_state, void* stream) {
  FOCAL_CHECK_ARG(step_state_words >= FOCAL_STEP_STATE_WORDS, "adamw_multi_advance: step_state holds %d words, the tickets need FOCAL_STEP_STATE_WORDS = %d "
                  "(the 4-word state of focal_rng_advance / focal_adamw_multi is not enough)", step_state_words, FOCAL_STEP_STATE_WORDS);
  return adamw_launch(d, nseg, p, g, m, v, shadow_bf16, n, lr_dev, step_state, seed_state, true, (hipStream_t)stream);
}

// the checks both clipped entry points make before anything is launched
static int clip_check(const char* who, const float* partials, int partial_words, const uint32_t* record, int record_words, float max_norm) {
  FOCAL_CHECK_ARG(partials && record, "%s: null argument (partial row or record)", who);
  FOCAL_CHECK_ARG(partial_words >= FOCAL_CLIP_SCRATCH_WORDS, "%s: the scratch row holds %d words, FOCAL_CLIP_SCRATCH_WORDS = %d are read", who,
                  partial_words, FOCAL_CLIP_SCRATCH_WORDS);
  FOCAL_CHECK_ARG(record_words >= FOCAL_CLIP_RECORD_WORDS, "%s: the record holds %d words, FOCAL_CLIP_RECORD_WORDS = %d are written", who, record_words,
                  FOCAL_CLIP_RECORD_WORDS);
  FOCAL_CHECK_ARG(max_norm > 0.0f, "%s: max_norm = %g must be positive (+inf: clip nothing, record the norms)", who, (double)max_norm);  // (NaN fails too)
  return FOCAL_OK;
}

extern "C" int focal_adamw_clip_multi(const focal_adamw_desc* d, int nseg, float* const* p, const float* const* g, float* const* m,
                                      float* const* v, void* const* shadow_bf16, const long* n, const float* lr_dev,
                                      const uint32_t* rng_state, const float* partials, int partial_words, uint32_t* record,
                                      int record_words, float max_norm, void* stream) {
  if (int rc = clip_check("adamw_clip_multi", partials, partial_words, record, record_words, max_norm)) return rc;
  const ClipArgs clip = {partials, record, max_norm};
  return adamw_launch(d, nseg, p, g, m, v, shadow_bf16, n, lr_dev, const_cast<uint32_t*>(rng_state), nullptr, false, (hipStream_t)stream, &clip);
}

extern "C" int focal_adamw_clip_multi_advance(const focal_adamw_desc* d, int nseg, float* const* p, const float* const* g, float* const* m,
                                              float* const* v, void* const* shadow_bf16, const long* n, const float* lr_dev,
                                              uint32_t* step_state, int step_state_words, uint32_t* seed_state, const float* partials,
                                              int partial_words, uint32_t* record, int record_words, float max_norm, void* stream) {
  if (int rc = clip_check("adamw_clip_multi_advance", partials, partial_words, record, record_words, max_norm)) return rc;
  FOCAL_CHECK_ARG(step_state_words >= FOCAL_STEP_STATE_WORDS, "adamw_clip_multi_advance: step_state holds %d words, the tickets need FOCAL_STEP_STATE_WORDS = %d",
                  step_state_words, FOCAL_STEP_STATE_WORDS);
  const ClipArgs clip = {partials, record, max_norm};
  return adamw_launch(d, nseg, p, g, m, v, shadow_bf16, n, lr_dev, step_state, seed_state, true, (hipStream_t)stream, &clip);
}

// ---- LAMB (You et al. 2020, Algorithm 2) with AdamW's conventions: per-tensor trust ratios over the arena, two launches
// A trust ratio needs a whole tensor's norms before any of its weights move, so the step is cut at a launch boundary:
//   lamb_moments_kernel  one workgroup per PIECE (at most FOCAL_LAMB_PIECE elements inside one tensor's padded extent): g, m, v, w in, m, v
//                        out, u = r + lambda_T w formed in registers, the piece's sum(w^2) and sum(u^2) stored to partials[2 piece], [2 piece + 1]
//   lamb_apply_kernel    the same grid: every workgroup adds its tensor's partials in one fixed order (the same bits in each of them, no
//                        hand-off inside a launch), forms phi_T, recomputes u from the stored m, v and writes w and the bf16 shadow
// 24 + 18 B per element against AdamW's 30.  Plain stores, no atomics besides the step-count tickets: two runs give the same bits.
// The table (int4 rows, device copy of the host table the entry points check): pieces {offset, length, tensor, -} in elements from the segment's
// start, then tensors {first piece, last piece (exclusive), flags, -}.
#define LAMB_ADAPT 1
#define LAMB_DECAY 2

// The clip row turned into the coefficient and the skip decision, as adamw_clip_kernel does it (same order of additions, same bits); where
// `record` is non-null, workgroup 0's lane 0 updates the record.
__device__ __forceinline__ void lamb_clip_decide(const float* __restrict__ partials, float* wsum, uint32_t* record, float max_norm, float& coef_out,
                                                 bool& skip_out) {
  static_assert(FOCAL_CLIP_SCRATCH_WORDS == 4 * 256, "four slots per lane");
  float s = partials[threadIdx.x];
  s += partials[threadIdx.x + 256];
  s += partials[threadIdx.x + 512];
  s += partials[threadIdx.x + 768];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
  __syncthreads();
  const float sq = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
  const float norm = sqrtf(sq);
  const bool skip = !(norm <= 3.402823466e+38f);
  const float coef = skip ? 0.0f : fminf(1.0f, max_norm / (norm + 1e-6f));
  if (record != nullptr && blockIdx.x == 0 && threadIdx.x == 0) {
    record[0] += 1u;
    if (skip) {
      record[2] += 1u;
    } else {
      if (coef < 1.0f) record[1] += 1u;
      record[3] = __float_as_uint(__uint_as_float(record[3]) + norm);
      record[4] = __float_as_uint(fmaxf(__uint_as_float(record[4]), norm));
    }
    record[5] = __float_as_uint(norm);
    record[6] = __float_as_uint(sq);
    record[7] = __float_as_uint(coef);
  }
  coef_out = coef;
  skip_out = skip;
}

// Bias corrections of step count t, shared by both launches: the same expressions on the same inputs, the same bits.
struct LambStep { float ibc1, isq; };
__device__ __forceinline__ LambStep lamb_step(const focal_adamw_desc& d, uint32_t count, int advance) {
  const float t = (float)(count + (advance ? 1u : 0u));
  const float bc1 = 1.0f - powf(d.beta1, t), bc2 = 1.0f - powf(d.beta2, t);
  LambStep s;
  s.ibc1 = 1.0f / bc1;
  s.isq = rsqrtf(bc2);
  return s;
}

// u = r + lambda w, r = (m / bc1) / (sqrt(v / bc2) + eps).  Every rounding is spelled out (no contraction left to the compiler): the second
// launch must get the bits the first one summed.
__device__ __forceinline__ float lamb_u(float m, float v, float w, const LambStep& s, float eps, float lam) {
#pragma clang fp contract(off)
  const float den = sqrtf(v) * s.isq + eps;
  const float r = (m * s.ibc1) / den;
  return fmaf(lam, w, r);
}

template <bool CLIP>
__global__ __launch_bounds__(256) void lamb_moments_kernel(const float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, const int4* __restrict__ table, int npieces,
                                                           const uint32_t* __restrict__ rng_state, int advance, focal_adamw_desc d,
                                                           float* __restrict__ partials, const float* __restrict__ clip_partials, float max_norm) {
  __shared__ float wsum[4];
  __shared__ float red[8];
  float coef = 1.0f;
  if (CLIP) {
    bool skip;
    lamb_clip_decide(clip_partials, wsum, nullptr, max_norm, coef, skip);
    if (skip) return;  // (uniform over the launch: a non-finite gradient norm writes nothing)
  }
  const int4 pc = table[blockIdx.x];
  const int4 tn = table[npieces + pc.z];
  const float lam = (tn.z & LAMB_DECAY) ? d.weight_decay : 0.0f;
  const LambStep st = lamb_step(d, rng_state[1], advance);
  const float b1 = d.beta1, b2 = d.beta2, omb1 = 1.0f - d.beta1, omb2 = 1.0f - d.beta2;
  const float4* __restrict__ p4 = reinterpret_cast<const float4*>(p + pc.x);
  const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g + pc.x);
  float4* __restrict__ m4 = reinterpret_cast<float4*>(m + pc.x);
  float4* __restrict__ v4 = reinterpret_cast<float4*>(v + pc.x);
  const int n4 = pc.y >> 2;
  float sw = 0.0f, su = 0.0f;  // one accumulator each per lane: at most FOCAL_LAMB_PIECE / 256 elements in a chain
  for (int i = threadIdx.x; i < n4; i += 256) {
    const float4 ww = p4[i];
    const float4 gg = CLIP ? scale_rn(g4[i], coef) : g4[i];
    float4 mm = m4[i];
    float4 vv = v4[i];
#define LAMB1(c)                                        \
    mm.c = fmaf(b1, mm.c, omb1 * gg.c);                 \
    vv.c = fmaf(omb2 * gg.c, gg.c, b2 * vv.c);          \
    {                                                   \
      const float u = lamb_u(mm.c, vv.c, ww.c, st, d.eps, lam); \
      sw = fmaf(ww.c, ww.c, sw);                        \
      su = fmaf(u, u, su);                              \
    }
    LAMB1(x) LAMB1(y) LAMB1(z) LAMB1(w)
#undef LAMB1
    m4[i] = mm;
    v4[i] = vv;
  }
  sw = wave_sum(sw);
  su = wave_sum(su);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = sw;
    red[4 + (threadIdx.x >> 6)] = su;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    partials[2 * blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    partials[2 * blockIdx.x + 1] = (red[4] + red[5]) + (red[6] + red[7]);
  }
}

template <bool CLIP>
__global__ __launch_bounds__(256) void lamb_apply_kernel(float* __restrict__ p, const float* __restrict__ m, const float* __restrict__ v,
                                                         bf16_t* __restrict__ shadow, const int4* __restrict__ table, int npieces,
                                                         const float* __restrict__ lr_dev, uint32_t* rng_state, uint32_t* seed_state, int advance,
                                                         focal_adamw_desc d, const float* __restrict__ partials, float* __restrict__ record,
                                                         float max_trust, const float* __restrict__ clip_partials, uint32_t* clip_record,
                                                         float max_norm) {
  __shared__ float wsum[4];
  bool skip = false;
  if (CLIP) {
    float coef;
    lamb_clip_decide(clip_partials, wsum, clip_record, max_norm, coef, skip);
  }
  const uint32_t count = __atomic_load_n(rng_state + 1, __ATOMIC_RELAXED);  // (feeds every store below and the ticket: see adamw_body)
  if (!(CLIP && skip)) {
    const int4 pc = table[blockIdx.x];
    const int4 tn = table[npieces + pc.z];
    // the tensor's partials: lane l of every wave adds pieces first + l, first + l + 64, ... in a chain, then the wave (6 levels); the four
    // waves do the same work and hold the same bits, as does every other workgroup of the tensor
    float sw = 0.0f, su = 0.0f;
    for (int k = tn.x + (threadIdx.x & 63); k < tn.y; k += 64) {
      sw += partials[2 * k];
      su += partials[2 * k + 1];
    }
    sw = wave_sum(sw);
    su = wave_sum(su);
    const float nw = sqrtf(sw), nu = sqrtf(su);
    const bool ratio = (tn.z & LAMB_ADAPT) && nw > 0.0f && nu > 0.0f && nw <= 3.402823466e+38f && nu <= 3.402823466e+38f;
    const float phi = fminf(ratio ? nw / nu : 1.0f, max_trust);
    if ((int)blockIdx.x == tn.x && threadIdx.x == 0) {  // one writer per tensor
      record[3 * pc.z] = phi;
      record[3 * pc.z + 1] = nw;
      record[3 * pc.z + 2] = nu;
    }
    const float lam = (tn.z & LAMB_DECAY) ? d.weight_decay : 0.0f;
    const LambStep st = lamb_step(d, count, advance);
    const float neg_step = -(lr_dev[0] * phi);
    float4* __restrict__ p4 = reinterpret_cast<float4*>(p + pc.x);
    const float4* __restrict__ m4 = reinterpret_cast<const float4*>(m + pc.x);
    const float4* __restrict__ v4 = reinterpret_cast<const float4*>(v + pc.x);
    const int n4 = pc.y >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) {
      float4 ww = p4[i];
      const float4 mm = m4[i];
      const float4 vv = v4[i];
      ww.x = fmaf(neg_step, lamb_u(mm.x, vv.x, ww.x, st, d.eps, lam), ww.x);
      ww.y = fmaf(neg_step, lamb_u(mm.y, vv.y, ww.y, st, d.eps, lam), ww.y);
      ww.z = fmaf(neg_step, lamb_u(mm.z, vv.z, ww.z, st, d.eps, lam), ww.z);
      ww.w = fmaf(neg_step, lamb_u(mm.w, vv.w, ww.w, st, d.eps, lam), ww.w);
      p4[i] = ww;
      if (shadow) {
        bf16x4 s;
        s[0] = (bf16_t)ww.x; s[1] = (bf16_t)ww.y; s[2] = (bf16_t)ww.z; s[3] = (bf16_t)ww.w;
        reinterpret_cast<bf16x4*>(shadow + pc.x)[i] = s;
      }
    }
  }
  if (advance == 2) step_tail<CLIP>(rng_state, seed_state, count, skip);
}

// Everything the kernels index with comes from the table: it is checked here, on the host copy, before anything is launched.
static int lamb_table_check(const char* who, int s, const focal_lamb_table& tb, long n) {
  FOCAL_CHECK_ARG(tb.host && tb.dev && tb.partials && tb.record, "%s: segment %d: null table, partial row or record", who, s);
  FOCAL_CHECK_ARG(((uintptr_t)tb.dev & 15) == 0, "%s: segment %d: the device table is not 16-byte aligned", who, s);
  FOCAL_CHECK_ARG(tb.npieces >= 1 && tb.ntensors >= 1 && tb.ntensors <= tb.npieces, "%s: segment %d: %d pieces of %d tensors", who, s, tb.npieces,
                  tb.ntensors);
  FOCAL_CHECK_ARG(n <= 0x7fffffffL, "%s: segment %d length %ld does not fit the table's 32-bit offsets", who, s, n);
  FOCAL_CHECK_ARG(tb.partial_words >= 2L * tb.npieces, "%s: segment %d: the partial row holds %d words, 2 per piece = %ld are written", who, s,
                  tb.partial_words, 2L * tb.npieces);
  FOCAL_CHECK_ARG(tb.record_words >= (long)FOCAL_LAMB_RECORD_WORDS * tb.ntensors, "%s: segment %d: the record holds %d words, FOCAL_LAMB_RECORD_WORDS = %d "
                  "per tensor = %ld are written", who, s, tb.record_words, FOCAL_LAMB_RECORD_WORDS, (long)FOCAL_LAMB_RECORD_WORDS * tb.ntensors);
  const int32_t* pc = tb.host;
  const int32_t* tn = tb.host + 4L * tb.npieces;
  long end = 0;
  for (int i = 0; i < tb.npieces; ++i, pc += 4) {
    FOCAL_CHECK_ARG(pc[1] > 0 && pc[1] % 4 == 0 && pc[1] <= FOCAL_LAMB_PIECE, "%s: segment %d piece %d length %d is not a positive multiple of 4 up to "
                    "FOCAL_LAMB_PIECE = %d", who, s, i, pc[1], FOCAL_LAMB_PIECE);
    FOCAL_CHECK_ARG(pc[0] >= end && pc[0] % 4 == 0, "%s: segment %d piece %d at offset %d: pieces ascend without overlap from multiples of 4 (the "
                    "piece before it ends at %ld)", who, s, i, pc[0], end);
    end = (long)pc[0] + pc[1];
    FOCAL_CHECK_ARG(end <= n, "%s: segment %d piece %d ends at %ld, behind the segment's %ld elements", who, s, i, end, n);
    FOCAL_CHECK_ARG(pc[2] >= 0 && pc[2] < tb.ntensors, "%s: segment %d piece %d names tensor %d of %d", who, s, i, pc[2], tb.ntensors);
  }
  int next = 0;
  for (int t = 0; t < tb.ntensors; ++t, tn += 4) {
    FOCAL_CHECK_ARG(tn[0] == next && tn[1] > tn[0] && tn[1] <= tb.npieces, "%s: segment %d tensor %d owns pieces [%d, %d): the tensors' ranges partition "
                    "the %d pieces in order (expected a range from %d)", who, s, t, tn[0], tn[1], tb.npieces, next);
    FOCAL_CHECK_ARG((tn[2] & ~(LAMB_ADAPT | LAMB_DECAY)) == 0, "%s: segment %d tensor %d has flags %d (1: adapted, 2: decayed)", who, s, t, tn[2]);
    for (int i = tn[0]; i < tn[1]; ++i)
      FOCAL_CHECK_ARG(tb.host[4L * i + 2] == t, "%s: segment %d piece %d names tensor %d inside the range of tensor %d", who, s, i, tb.host[4L * i + 2], t);
    next = tn[1];
  }
  FOCAL_CHECK_ARG(next == tb.npieces, "%s: segment %d: the tensors' ranges end at piece %d of %d", who, s, next, tb.npieces);
  return FOCAL_OK;
}

static int lamb_launch(const char* who, const focal_adamw_desc* d, int nseg, float* const* p, const float* const* g, float* const* m,
                       float* const* v, void* const* shadow_bf16, const long* n, const focal_lamb_table* tables, float max_trust,
                       const float* lr_dev, uint32_t* step_state, uint32_t* seed_state, bool advance, const float* clip_partials,
                       int clip_partial_words, uint32_t* clip_record, int clip_record_words, float max_norm, hipStream_t st) {
  FOCAL_CHECK_ARG(d && p && g && m && v && n && tables && lr_dev && step_state, "%s: null argument", who);
  FOCAL_CHECK_ARG(d->l2_decay == 0, "%s: LAMB decays the weights in the update (u = r + lambda w); l2_decay = %d is AdamW's", who, d->l2_decay);
  FOCAL_CHECK_ARG(max_trust > 0.0f, "%s: max_trust = %g must be positive (+inf: no clamp)", who, (double)max_trust);  // (NaN fails too)
  const bool clip = clip_partials != nullptr || clip_record != nullptr;
  if (clip)
    if (int rc = clip_check(who, clip_partials, clip_partial_words, clip_record, clip_record_words, max_norm)) return rc;
  int last = -1;
  for (int s = 0; s < nseg; ++s) {
    FOCAL_CHECK_ARG(n[s] >= 0 && n[s] % 4 == 0, "%s: segment %d length %ld is not a multiple of 4 (arena segments are padded)", who, s, n[s]);
    if (n[s] == 0) continue;
    FOCAL_CHECK_ARG(p[s] && g[s] && m[s] && v[s] && (((uintptr_t)p[s] | (uintptr_t)g[s] | (uintptr_t)m[s] | (uintptr_t)v[s]) & 15) == 0,
                    "%s: segment %d has a null or not 16-byte aligned buffer", who, s);
    FOCAL_CHECK_ARG(!shadow_bf16 || !shadow_bf16[s] || ((uintptr_t)shadow_bf16[s] & 7) == 0, "%s: segment %d: the bf16 shadow is not 8-byte aligned", who, s);
    if (int rc = lamb_table_check(who, s, tables[s], n[s])) return rc;
    last = s;
  }
  FOCAL_CHECK_ARG(!advance || last >= 0, "%s: no non-empty segment to carry the step-count advance", who);
  for (int s = 0; s < nseg; ++s) {
    if (n[s] == 0) continue;
    const focal_lamb_table& tb = tables[s];
    const int4* table = reinterpret_cast<const int4*>(tb.dev);
    const dim3 grid((unsigned)tb.npieces), block(256);
    bf16_t* shadow = shadow_bf16 ? (bf16_t*)shadow_bf16[s] : nullptr;
    uint32_t* seed = (advance && s == last) ? seed_state : nullptr;
    const int adv = advance ? (s == last ? 2 : 1) : 0;
    // segments run in stream order: every launch reads the same step count, the last one advances it
    if (clip) {
      FOCAL_LAUNCH(lamb_moments_kernel<true>, grid, block, 0, st, p[s], g[s], m[s], v[s], table, tb.npieces, step_state, adv, *d, tb.partials,
                   clip_partials, max_norm);
      FOCAL_LAUNCH(lamb_apply_kernel<true>, grid, block, 0, st, p[s], m[s], v[s], shadow, table, tb.npieces, lr_dev, step_state, seed, adv, *d,
                   tb.partials, tb.record, max_trust, clip_partials, s == last ? clip_record : nullptr, max_norm);
    } else {
      FOCAL_LAUNCH(lamb_moments_kernel<false>, grid, block, 0, st, p[s], g[s], m[s], v[s], table, tb.npieces, step_state, adv, *d, tb.partials,
                   (const float*)nullptr, 0.0f);
      FOCAL_LAUNCH(lamb_apply_kernel<false>, grid, block, 0, st, p[s], m[s], v[s], shadow, table, tb.npieces, lr_dev, step_state, seed, adv, *d,
                   tb.partials, tb.record, max_trust, (const float*)nullptr, (uint32_t*)nullptr, 0.0f);
    }
  }
  FOCAL_LAUNCH_CHECK();
  return FOCAL_OK;
}

extern "C" int focal_lamb_multi(const focal_adamw_desc* d, int nseg, float* const* p, const float* const* g, float* const* m, float* const* v,
                                void* const* shadow_bf16, const long* n, const focal_lamb_table* tables, float max_trust, const float* lr_dev,
                                const uint32_t* rng_state, const float* clip_partials, int clip_partial_words, uint32_t* clip_record,
                                int clip_record_words, float max_norm, void* stream) {
  return lamb_launch("lamb_multi", d, nseg, p, g, m, v, shadow_bf16, n, tables, max_trust, lr_dev, const_cast<uint32_t*>(rng_state), nullptr, false,
                     clip_partials, clip_partial_words, clip_record, clip_record_words, max_norm, (hipStream_t)stream);
}

extern "C" int focal_lamb_multi_advance(const focal_adamw_desc* d, int nseg, float* const* p, const float* const* g, float* const* m,
                                        float* const* v, void* const* shadow_bf16, const long* n, const focal_lamb_table* tables, float max_trust,
                                        const float* lr_dev, uint32_t* step_state, int step_state_words, uint32_t* seed_state,
                                        const float* clip_partials, int clip_partial_words, uint32_t* clip_record, int clip_record_words,
                                        float max_norm, void* stream) {
  FOCAL_CHECK_ARG(step_state_words >= FOCAL_STEP_STATE_WORDS, "lamb_multi_advance: step_state holds %d words, the tickets need FOCAL_STEP_STATE_WORDS = %d",
                  step_state_words, FOCAL_STEP_STATE_WORDS);
  return lamb_launch("lamb_multi_advance", d, nseg, p, g, m, v, shadow_bf16, n, tables, max_trust, lr_dev, step_state, seed_state, true, clip_partials,
                     clip_partial_words, clip_record, clip_record_words, max_norm, (hipStream_t)stream);
}

__global__ __launch_bounds__(256) void cast_bf16_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, long n) {
  const long n4 = n >> 2;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const float4 a = reinterpret_cast<const float4*>(src)[i];
    bf16x4 s;
    s[0] = (bf16_t)a.x; s[1] = (bf16_t)a.y; s[2] = (bf16_t)a.z; s[3] = (bf16_t)a.w;
    reinterpret_cast<bf16x4*>(dst)[i] = s;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) dst[(n4 << 2) + threadIdx.x] = (bf16_t)src[(n4 << 2) + threadIdx.x];
}

extern "C" int focal_cast_bf16(const float* src, void* dst, long n, void* stream) {
  FOCAL_CHECK_ARG(src && dst && n >= 0, "cast_bf16: bad argument");
  if (n == 0) return FOCAL_OK;
  int blocks = ceil_div((n + 3) / 4, 256);
  if (blocks > 2048) blocks = 2048;
  FOCAL_LAUNCH(cast_bf16_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src, (bf16_t*)dst, n);
  FOCAL_LAUNCH_CHECK();
  return FOCAL_OK;
}
