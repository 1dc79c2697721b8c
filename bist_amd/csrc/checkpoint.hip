// Trainer checkpoints: the optimiser state -- fp32 master weights and both Adam moments -- copied and digested in ONE pass
// (include/bist_hip.h: bist_state_copy).
//
// The reference writes its model after validation and keeps the best one (train.py:156-177); here the state to keep is three flat fp32
// buffers on the device, and a checkpoint wants the digest of exactly the bits it copied.  One launch reads each 16-byte group of the
// three ranges once, stores it to the destination (snapshot, restore) or nowhere (digest only), refreshes the compute-dtype working
// copy from the weights it just read (restore), and adds the group's two 64-bit words into the digest of its slot:
//
//   state_copy_kernel   slot s covers ONE contiguous chunk whose bounds are a function of (n, nslots) alone (the scheme of
//                       grad_norm.hip); within a chunk every thread walks a fixed strided sequence of 16-byte groups and adds the
//                       hashes of their words in uint64, one fixed tree through LDS combines the 256 threads.  No atomics, no tickets;
//                       every slot is written by every launch.  The sum wraps, so the total over the slots does not depend on
//                       nslots, max_blocks, the grid or the order of arrival -- the position enters through the word index j.
//
// HBM-bound like adam4_kernel: 12 bytes read and 12 written per parameter (2 more for a bf16 working copy) against two 64-bit
// multiplies per word.
#include "common.hpp"

namespace {

// h_j of the header: splitmix64's finaliser over w + j * golden (j: the word's index in the whole tensor, from 1)
__device__ __forceinline__ uint64_t word_hash(uint32_t lo, uint32_t hi, uint64_t j) {
  uint64_t z = ((uint64_t)lo | ((uint64_t)hi << 32)) + j * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// one 16-byte group of one tensor: element index e (a multiple of 4) of the whole tensor -> words e / 2 + 1 and e / 2 + 2
template <bool COPY>
__device__ __forceinline__ uint4 group(const float* __restrict__ src, float* __restrict__ dst, long e, uint64_t& acc) {
  const uint4 q = *reinterpret_cast<const uint4*>(src + e);
  if constexpr (COPY) *reinterpret_cast<uint4*>(dst + e) = q;
  const uint64_t j = (uint64_t)(e >> 1) + 1;
  acc += word_hash(q.x, q.y, j) + word_hash(q.z, q.w, j + 1);
  return q;
}

// the last 1 .. 3 elements of a tensor (element index e, a multiple of 4): scalar accesses, a missing high half reads as 0
template <bool COPY>
__device__ __forceinline__ void tail(const float* __restrict__ src, float* __restrict__ dst, long e, int k, uint64_t& acc) {
  uint32_t x[4] = {0u, 0u, 0u, 0u};
  for (int i = 0; i < k; ++i) {
    x[i] = __builtin_bit_cast(uint32_t, src[e + i]);
    if constexpr (COPY) dst[e + i] = __builtin_bit_cast(float, x[i]);
  }
  const uint64_t j = (uint64_t)(e >> 1) + 1;
  acc += word_hash(x[0], x[1], j);
  if (k > 2) acc += word_hash(x[2], x[3], j + 1);
}

// WORK: 0 = none, 1 = f32, 2 = bf16 (the casts of adam4_kernel)
template <bool COPY, int WORK>
__global__ __launch_bounds__(256) void state_copy_kernel(const float* __restrict__ sp, const float* __restrict__ sm, const float* __restrict__ sv,
                                                         float* __restrict__ dp, float* __restrict__ dm, float* __restrict__ dv,
                                                         void* __restrict__ work, long n, long chunk, uint64_t* __restrict__ digests, int nslots) {
  __shared__ uint64_t red[3][256];
  const int t = (int)threadIdx.x;
  // grid-stride over SLOTS (max_blocks bounds the resident workgroups only): the work of a slot is the same whoever does it
  for (int s = (int)blockIdx.x; s < nslots; s += (int)gridDim.x) {
    const long c0 = (long)s * chunk;                 // a multiple of 8 elements: 16-byte aligned in all three tensors and in work
    uint64_t ap = 0, am = 0, av = 0;
    if (c0 < n) {
      const long len = (n - c0 < chunk) ? n - c0 : chunk;
      const long nvec = len / 4;
#pragma unroll 2
      for (long i = t; i < nvec; i += 256) {
        const long e = c0 + 4 * i;
        const uint4 q = group<COPY>(sp, dp, e, ap);
        group<COPY>(sm, dm, e, am);
        group<COPY>(sv, dv, e, av);
        if constexpr (WORK == 1) {
          *reinterpret_cast<uint4*>((float*)work + e) = q;
        } else if constexpr (WORK == 2) {
          typedef __attribute__((ext_vector_type(2))) float f32x2_;
          typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_;
          const bf16x2_ lo = __builtin_convertvector(f32x2_{__builtin_bit_cast(float, q.x), __builtin_bit_cast(float, q.y)}, bf16x2_);
          const bf16x2_ hi = __builtin_convertvector(f32x2_{__builtin_bit_cast(float, q.z), __builtin_bit_cast(float, q.w)}, bf16x2_);
          *reinterpret_cast<uint2*>((bf16_t*)work + e) = make_uint2(__builtin_bit_cast(unsigned, lo), __builtin_bit_cast(unsigned, hi));
        }
      }
      const int k = (int)(len - 4 * nvec);           // 1 .. 3 only in the chunk that ends the tensor
      if (k > 0 && t == 0) {
        const long e = c0 + 4 * nvec;
        tail<COPY>(sp, dp, e, k, ap);
        tail<COPY>(sm, dm, e, k, am);
        tail<COPY>(sv, dv, e, k, av);
        for (int i = 0; i < k; ++i) {
          if constexpr (WORK == 1) ((float*)work)[e + i] = sp[e + i];
          if constexpr (WORK == 2) ((bf16_t*)work)[e + i] = (bf16_t)sp[e + i];
        }
      }
    }
    red[0][t] = ap; red[1][t] = am; red[2][t] = av;
    __syncthreads();
#pragma unroll
    for (int o = 128; o > 0; o >>= 1) {              // one fixed-shape tree
      if (t < o) { red[0][t] += red[0][t + o]; red[1][t] += red[1][t + o]; red[2][t] += red[2][t + o]; }
      __syncthreads();
    }
    if (t < 3) digests[(long)t * nslots + s] = red[t][0];      // an empty chunk writes 0: every slot is overwritten by every launch
    __syncthreads();                                 // (the next slot of this workgroup rewrites red)
  }
}

}  // namespace

extern "C" int bist_state_copy(const float* src_p, const float* src_m, const float* src_v, float* dst_p, float* dst_m, float* dst_v,
                               void* work, int32_t work_dtype, int64_t n, uint64_t* digests, int32_t nslots, int32_t max_blocks,
                               void* stream) {
  BIST_REQUIRE(src_p && src_m && src_v && digests, "bist_state_copy: null source or digests");
  BIST_REQUIRE(n >= 1, "bist_state_copy: n must be at least 1");
  BIST_REQUIRE(nslots >= 1 && nslots <= BIST_STATE_MAX_SLOTS, "bist_state_copy: 1 <= nslots <= %d", BIST_STATE_MAX_SLOTS);
  BIST_REQUIRE(max_blocks >= 0, "bist_state_copy: max_blocks must not be negative");
  const int given = (dst_p != nullptr) + (dst_m != nullptr) + (dst_v != nullptr);
  BIST_REQUIRE(given == 0 || given == 3, "bist_state_copy: dst_p, dst_m, dst_v are given together or not at all");
  const float* srcs[3] = {src_p, src_m, src_v};
  float* dsts[3] = {dst_p, dst_m, dst_v};
  for (int a = 0; a < 3; ++a) {
    BIST_REQUIRE((uintptr_t)srcs[a] % 16 == 0 && (uintptr_t)dsts[a] % 16 == 0, "bist_state_copy: src and dst must be 16-byte aligned");
    for (int b = 0; given && b < 3; ++b)
      BIST_REQUIRE(srcs[a] != dsts[b], "bist_state_copy: a src that is also a dst");
  }
  BIST_REQUIRE((uintptr_t)digests % 8 == 0, "bist_state_copy: digests must be 8-byte aligned");
  if (work) {
    BIST_REQUIRE(work_dtype == BIST_F32 || work_dtype == BIST_BF16, "bist_state_copy: bad work_dtype");
    BIST_REQUIRE((uintptr_t)work % (work_dtype == BIST_BF16 ? 8 : 16) == 0, "bist_state_copy: work must be aligned to 4 of its elements");
  }
  // the chunk of a slot: a function of (n, nslots) alone, a multiple of 8 elements (every chunk starts on a 16-byte line)
  const long per = (long)((n + nslots - 1) / nslots);
  const long chunk = (per + 7) / 8 * 8;
  unsigned grid = (unsigned)nslots;
  if (max_blocks > 0 && grid > (unsigned)max_blocks) grid = (unsigned)max_blocks;
  hipStream_t st = (hipStream_t)stream;
#define LAUNCH_(COPY, WORK)                                                                                                       \
  hipLaunchKernelGGL((state_copy_kernel<COPY, WORK>), dim3(grid), dim3(256), 0, st, src_p, src_m, src_v, dst_p, dst_m, dst_v, work, \
                     (long)n, chunk, digests, (int)nslots)
  const int wk = !work ? 0 : work_dtype == BIST_F32 ? 1 : 2;
  if (given) {
    if (wk == 0) LAUNCH_(true, 0); else if (wk == 1) LAUNCH_(true, 1); else LAUNCH_(true, 2);
  } else {
    if (wk == 0) LAUNCH_(false, 0); else if (wk == 1) LAUNCH_(false, 1); else LAUNCH_(false, 2);
  }
#undef LAUNCH_
  BIST_LAUNCH_CHECK("bist_state_copy");
  return BIST_OK;
}
