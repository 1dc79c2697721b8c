// Ragged audio features staged into the class-shaped static buffer of a captured step (include/bist_hip.h: bist_stage_audio).
//
// The reference pads a batch's audio to its own longest clip and masks rows whose features SUM to zero (data/dataset.py:60, 83-87:
// audio_mask = (audio_fts.sum(-1) != 0).unsqueeze(-2)).  A captured step replays one geometry, so bist_amd/train.py maps the audio
// length to a class length PTa >= Ta and this launch writes [B, Ta, Da] into [B, PTa, Da]: the rows cast to the compute dtype, the
// tail rows zero, and audio_mask [B, PTa] from the SOURCE values (a zero tail row is masked by construction: the same function of
// the real rows as the reference computes on its own padding).
//
// One wave per destination row, four rows per workgroup.  The mask bit is the sum of the source row in EXACTLY the order of
// temporal_mask_kernel (csrc/rowops.hip), which is what Batch runs on device features: there thread tid of 256 folds the 16-byte chunks
// (or, unaligned, the single elements) tid, tid + 256, ... in sequence, each of the four waves is summed by wave_sum and the four
// results are added in wave order.  Here lane l plays threads l, 64 + l, 128 + l, 192 + l one after the other, so the bit equals
// bist_temporal_mask over the padded source bit for bit, also for rows whose entries cancel.  The copy is a second walk over the row
// (a VGGish row is 512 bytes: it comes from the cache); 16-byte stores where the row width and the bases allow, single elements
// otherwise.  At 16 x 32 x 128 the launch moves 0.4 MB: it is bound by launch latency, not by bandwidth.
#include "common.hpp"

namespace {

template <typename TS>
__device__ __forceinline__ float audio_row_sum(const TS* __restrict__ p, long n, int lane) {
  constexpr int E = 16 / (int)sizeof(TS);
  const bool vec = (n % E) == 0 && ((uintptr_t)p % 16) == 0;             // temporal_mask_kernel's own test
  float tot = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    float s = 0.f;
    if (vec) {
      for (long c = w * 64 + lane; c < n / E; c += 256) {
        const uint4 q = reinterpret_cast<const uint4*>(p)[c];
        const TS* qe = reinterpret_cast<const TS*>(&q);
#pragma unroll
        for (int e = 0; e < E; ++e) s += to_f(qe[e]);
      }
    } else {
      for (long c = w * 64 + lane; c < n; c += 256) s += to_f(p[c]);
    }
    s = wave_sum(s);
    tot = w == 0 ? s : tot + s;
  }
  return tot;
}

template <typename TS, typename TD>
__global__ __launch_bounds__(256) void stage_audio_kernel(const TS* __restrict__ src, TD* __restrict__ dst, unsigned char* __restrict__ mask,
                                                          long rows, int Ta, int PTa, long n, int vec) {
  constexpr int E = 16 / (int)sizeof(TD);
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const long b = row / PTa, t = row % PTa;
  TD* d = dst + row * n;
  if (t >= Ta) {                                       // appended row: zeros, masked
    if (vec) {
      const uint4 z = make_uint4(0u, 0u, 0u, 0u);
      for (long c = lane; c < n / E; c += 64) reinterpret_cast<uint4*>(d)[c] = z;
    } else {
      for (long c = lane; c < n; c += 64) d[c] = from_f<TD>(0.f);
    }
    if (lane == 0) mask[row] = 0;
    return;
  }
  const TS* s = src + (b * Ta + t) * n;
  const float sum = audio_row_sum<TS>(s, n, lane);
  if (lane == 0) mask[row] = sum != 0.f ? 1 : 0;
  if (vec) {
    for (long c = lane; c < n / E; c += 64) {
      union { uint4 q[(E * sizeof(TS) + 15) / 16]; uint2 h; TS e[E]; } in;
      if constexpr (E * sizeof(TS) >= 16) {
#pragma unroll
        for (int k = 0; k < (int)(E * sizeof(TS) / 16); ++k) in.q[k] = reinterpret_cast<const uint4*>(s + c * E)[k];
      } else {
        in.h = *reinterpret_cast<const uint2*>(s + c * E);
      }
      union { uint4 q; TD e[E]; } o;
#pragma unroll
      for (int e = 0; e < E; ++e) o.e[e] = from_f<TD>(to_f(in.e[e]));     // bist_cast's rounding
      reinterpret_cast<uint4*>(d)[c] = o.q;
    }
  } else {
    for (long c = lane; c < n; c += 64) d[c] = from_f<TD>(to_f(s[c]));
  }
}

}  // namespace

extern "C" int bist_stage_audio(const void* src, void* dst, uint8_t* mask, int32_t B, int32_t Ta, int32_t PTa, int32_t Da,
                                int32_t src_dtype, int32_t out_dtype, void* stream) {
  BIST_REQUIRE(src && dst && mask && B >= 1 && Ta >= 1 && PTa >= Ta && Da >= 1, "bist_stage_audio: B >= 1, 1 <= Ta <= PTa, Da >= 1");
  BIST_REQUIRE((src_dtype == BIST_F32 || src_dtype == BIST_BF16) && (out_dtype == BIST_F32 || out_dtype == BIST_BF16),
               "bist_stage_audio: feature dtypes f32 / bf16");
  const long ssz = src_dtype == BIST_BF16 ? 2 : 4, dsz = out_dtype == BIST_BF16 ? 2 : 4;
  BIST_REQUIRE(((uintptr_t)src % ssz) == 0 && ((uintptr_t)dst % dsz) == 0, "bist_stage_audio: element-aligned buffers");
  const long rows = (long)B * PTa;
  BIST_REQUIRE((rows + 3) / 4 < (1L << 31), "bist_stage_audio: too many rows");
  // whole 16-byte vectors of the output AND of the source per row, from 16-byte aligned bases: every row then starts on a 16-byte boundary
  const int vec = (Da % (16 / dsz)) == 0 && (Da % (16 / ssz)) == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 g((unsigned)((rows + 3) / 4)), blk(256);
#define SA(TS, TD) hipLaunchKernelGGL((stage_audio_kernel<TS, TD>), g, blk, 0, st, (const TS*)src, (TD*)dst, (unsigned char*)mask, rows, Ta, PTa, (long)Da, vec)
  if (src_dtype == BIST_F32 && out_dtype == BIST_BF16) SA(float, bf16_t);
  else if (src_dtype == BIST_BF16 && out_dtype == BIST_BF16) SA(bf16_t, bf16_t);
  else if (src_dtype == BIST_F32) SA(float, float);
  else SA(bf16_t, float);
#undef SA
  BIST_LAUNCH_CHECK("bist_stage_audio");
  return BIST_OK;
}
