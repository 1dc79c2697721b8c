// The global norm of the flat gradient, the clip factor and the non-finite guard of Trainer(max_grad_norm=...), all on the device
// (include/bist_hip.h: bist_grad_sumsq, bist_clip_hyper).
//
// The reference neither clips nor guards (train.py:29-37, optimize.py:19-26); torch.nn.utils.clip_grad_norm_ is the formula users
// expect.  Here the step is a replayed graph without a host round trip, so the norm is taken by two launches inside the step:
//
//   grad_sumsq_kernel   sum of squares of a flat range into `nslots` fp64 partial slots.  Slot s is the sum over ONE contiguous chunk
//                       whose bounds are a function of (n, nslots) alone; within a chunk every thread walks a fixed strided sequence of
//                       elements and adds their squares in fp64, and one fixed-shape tree through LDS combines the 256 threads.  No
//                       atomics, no tickets: a slot's bits depend on the data, on (n, nslots) and on where the range starts within a
//                       16-byte line (the length of the scalar head), never on the grid or on the order in which workgroups run.
//   clip_hyper_kernel   one workgroup: the slots added in index order, norm = sqrt(sum) * grad_scale, and the step's scalars rewritten
//                       in `hyper` -- slot 3 (grad_scale, which every device-side Adam multiplies the gradient by) times the clip factor,
//                       slot 5 the skip word the guarded Adam launches read, 6 the norm, 7 the factor.
//
// fp64: the square of an fp32 value is exact in fp64, so a slot is a plain sum of exact terms; the pass is HBM-bound (2 bytes per bf16
// element against one fp64 FMA), far below the chip's fp64 rate.
#include "common.hpp"

namespace {

// the value Adam will consume at element i, before grad_scale: g, or acc + g formed in fp32 as adam_accum4_kernel forms it
template <typename TG>
__device__ __forceinline__ float sumsq_value(const TG* __restrict__ g, const float* __restrict__ acc, long i) {
  const float x = to_f(g[i]);
  return acc ? acc[i] + x : x;
}

template <typename TG>
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const TG* __restrict__ g, const float* __restrict__ acc, const int* __restrict__ phase,
                                                         long n, long chunk, double* __restrict__ partials, int nslots) {
  __shared__ double red[256];
  if (phase) {                                   // one uniform load: every thread of every workgroup takes the same branch
    const int ph = phase[0];
    if (!(ph & 2)) return;                       // not the last pass of a group: nothing is measured, nothing is stored
    if (ph & 1) acc = nullptr;                   // a group of one: the accumulator holds nothing of this group
  }
  constexpr int E = 16 / (int)sizeof(TG);        // elements per 16-byte load of the gradient
  const int t = (int)threadIdx.x;
  // grid-stride over SLOTS (max_blocks bounds the resident workgroups only): the work of a slot is the same whoever does it
  for (int s = (int)blockIdx.x; s < nslots; s += (int)gridDim.x) {
    const long c0 = (long)s * chunk;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (c0 < n) {
      const long len = (n - c0 < chunk) ? n - c0 : chunk;
      const TG* __restrict__ gc = g + c0;
      const float* __restrict__ ac = acc ? acc + c0 : nullptr;
      // scalar head up to the first 16-byte line of the gradient; the accumulator must be aligned there too, else all scalar
      long head = (E - (long)(((uintptr_t)gc % 16) / sizeof(TG))) % E;
      if (head > len) head = len;
      if (ac && ((uintptr_t)(ac + head) % 16) != 0) head = len;
      const long nvec = (len - head) / E;
      const long tail0 = head + nvec * E;
      for (long i = t; i < head; i += 256) {
        const double d = (double)sumsq_value(gc, ac, i);
        a0 = __builtin_fma(d, d, a0);
      }
#pragma unroll 4
      for (long j = t; j < nvec; j += 256) {
        float f[E];
        if constexpr (sizeof(TG) == 2) {
          const uint4 q = reinterpret_cast<const uint4*>(gc + head)[j];
          f[0] = __builtin_bit_cast(float, q.x << 16); f[1] = __builtin_bit_cast(float, q.x & 0xffff0000u);
          f[2] = __builtin_bit_cast(float, q.y << 16); f[3] = __builtin_bit_cast(float, q.y & 0xffff0000u);
          f[4] = __builtin_bit_cast(float, q.z << 16); f[5] = __builtin_bit_cast(float, q.z & 0xffff0000u);
          f[6] = __builtin_bit_cast(float, q.w << 16); f[7] = __builtin_bit_cast(float, q.w & 0xffff0000u);
        } else {
          const float4 q = reinterpret_cast<const float4*>(gc + head)[j];
          f[0] = q.x; f[1] = q.y; f[2] = q.z; f[3] = q.w;
        }
        if (ac) {
#pragma unroll
          for (int k = 0; k < E / 4; ++k) {
            const float4 a = reinterpret_cast<const float4*>(ac + head)[j * (E / 4) + k];
            f[4 * k + 0] = a.x + f[4 * k + 0]; f[4 * k + 1] = a.y + f[4 * k + 1];
            f[4 * k + 2] = a.z + f[4 * k + 2]; f[4 * k + 3] = a.w + f[4 * k + 3];
          }
        }
#pragma unroll
        for (int e = 0; e < E; e += 4) {         // four independent chains, each in element order
          const double d0 = (double)f[e], d1 = (double)f[e + 1], d2 = (double)f[e + 2], d3 = (double)f[e + 3];
          a0 = __builtin_fma(d0, d0, a0); a1 = __builtin_fma(d1, d1, a1);
          a2 = __builtin_fma(d2, d2, a2); a3 = __builtin_fma(d3, d3, a3);
        }
      }
      for (long i = tail0 + t; i < len; i += 256) {
        const double d = (double)sumsq_value(gc, ac, i);
        a0 = __builtin_fma(d, d, a0);
      }
    }
    red[t] = (a0 + a1) + (a2 + a3);
    __syncthreads();
#pragma unroll
    for (int o = 128; o > 0; o >>= 1) {          // one fixed-shape tree
      if (t < o) red[t] += red[t + o];
      __syncthreads();
    }
    if (t == 0) partials[s] = red[0];            // an empty chunk writes 0.0: every slot is overwritten by every launch
  }
}

__global__ __launch_bounds__(256) void clip_hyper_kernel(const double* __restrict__ partials, int nslots, float max_norm,
                                                         float* __restrict__ hyper, long long* __restrict__ skipped,
                                                         const int* __restrict__ phase) {
  __shared__ double stage[BIST_GRAD_SUMSQ_MAX_SLOTS];
  const int t = (int)threadIdx.x;
  if (phase && !(phase[0] & 2)) {                // first / middle pass of a group: the accumulating launches must not be held back
    if (t == 0) hyper[5] = 0.f;
    return;
  }
  for (int i = t; i < nslots; i += 256) stage[i] = partials[i];
  __syncthreads();
  if (t != 0) return;
  double sum = 0.0;
  for (int i = 0; i < nslots; ++i) sum += stage[i];          // index order
  const float gscale = hyper[3];
  const float norm = (float)sqrt(sum) * gscale;              // of the gradient as Adam will consume it
  hyper[6] = norm;
  if (!__builtin_isfinite(norm)) {
    hyper[5] = 1.f;
    hyper[7] = 0.f;
    skipped[0] += 1;
    return;
  }
  const float scale = fminf(1.f, max_norm / (norm + 1e-6f));   // torch.nn.utils.clip_grad_norm_; max_norm = +inf: exactly 1
  hyper[5] = 0.f;
  hyper[7] = scale;
  hyper[3] = gscale * scale;
}

}  // namespace

extern "C" int bist_grad_sumsq(const void* g, const float* acc, const int32_t* phase, int64_t n, int32_t grad_dtype, double* partials,
                               int32_t slot_lo, int32_t nslots, int32_t max_blocks, void* stream) {
  BIST_REQUIRE(g && partials && n > 0 && slot_lo >= 0 && max_blocks >= 0, "bist_grad_sumsq: bad argument");
  BIST_REQUIRE(nslots >= 1 && nslots <= BIST_GRAD_SUMSQ_MAX_SLOTS && slot_lo <= BIST_GRAD_SUMSQ_MAX_SLOTS - nslots,
               "bist_grad_sumsq: 1 <= nslots and slot_lo + nslots <= %d", BIST_GRAD_SUMSQ_MAX_SLOTS);
  BIST_REQUIRE((acc == nullptr) == (phase == nullptr), "bist_grad_sumsq: acc and phase are given together or not at all");
  BIST_REQUIRE(grad_dtype == BIST_F32 || grad_dtype == BIST_BF16, "bist_grad_sumsq: bad dtype");
  BIST_REQUIRE((uintptr_t)g % (grad_dtype == BIST_BF16 ? 2 : 4) == 0 && (uintptr_t)acc % 4 == 0 && (uintptr_t)partials % 8 == 0,
               "bist_grad_sumsq: pointers must be aligned to their element");
  // the chunk of a slot: a function of (n, nslots) alone, a multiple of 8 elements (a bf16 chunk starts 16 bytes into the base's line)
  const long per = (long)((n + nslots - 1) / nslots);
  const long chunk = (per + 7) / 8 * 8;
  unsigned grid = (unsigned)nslots;
  if (max_blocks > 0 && grid > (unsigned)max_blocks) grid = (unsigned)max_blocks;
  hipStream_t st = (hipStream_t)stream;
  if (grad_dtype == BIST_BF16)
    hipLaunchKernelGGL(grad_sumsq_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, (const bf16_t*)g, acc, (const int*)phase, (long)n, chunk,
                       partials + slot_lo, (int)nslots);
  else
    hipLaunchKernelGGL(grad_sumsq_kernel<float>, dim3(grid), dim3(256), 0, st, (const float*)g, acc, (const int*)phase, (long)n, chunk,
                       partials + slot_lo, (int)nslots);
  BIST_LAUNCH_CHECK("bist_grad_sumsq");
  return BIST_OK;
}

extern "C" int bist_clip_hyper(const double* partials, int32_t nslots_total, float max_norm, float* hyper, int64_t* skipped_ctr,
                               const int32_t* phase, void* stream) {
  BIST_REQUIRE(partials && hyper && skipped_ctr, "bist_clip_hyper: null argument");
  BIST_REQUIRE(nslots_total >= 1 && nslots_total <= BIST_GRAD_SUMSQ_MAX_SLOTS, "bist_clip_hyper: 1 <= nslots_total <= %d",
               BIST_GRAD_SUMSQ_MAX_SLOTS);
  BIST_REQUIRE(max_norm > 0.f, "bist_clip_hyper: max_norm must be positive (+inf: measure and guard, never scale)");      // (NaN fails too)
  hipLaunchKernelGGL(clip_hyper_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, (int)nslots_total, max_norm, hyper,
                     (long long*)skipped_ctr, (const int*)phase);
  BIST_LAUNCH_CHECK("bist_clip_hyper");
  return BIST_OK;
}
