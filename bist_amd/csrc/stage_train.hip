// A ragged training batch staged into the class-shaped static batch of a captured step (include/bist_hip.h: bist_stage_train_batch).
//
// The reference's collate_fn (data/dataset.py:133-195) pads every batch to its own maximum lengths and builds the masks from the pad id
// (dataset.py:66-67, 79, 92, 96-99).  A captured training step replays one fixed geometry, so bist_amd/train.py maps each batch to a
// LENGTH CLASS and this launch writes the batch into that class's static buffers, padded further -- the same function for the real
// positions, since every consumer masks padded keys, excludes padded targets from the losses, and zero frames are excluded by
// temporal_mask exactly as the reference's own padded frames are.
//
// One launch, two kinds of workgroups (256 threads):
//   blocks [0, B*PT)        one feature row (b, t) each: the source row cast to the compute dtype (16-byte vectors, four in flight per
//                           lane) or a zero row for t >= T, and its temporal_mask bit.  The bit is a sum over the row in EXACTLY the order
//                           of temporal_mask_kernel (csrc/rowops.hip) over the written row -- thread tid folds the 16-byte output chunks
//                           tid, tid+256, ... in sequence, then the wave and workgroup sums -- so it equals bist_temporal_mask on the
//                           padded tensor bit for bit, also for rows whose features cancel;
//   blocks [B*PT, B*PT+B)   clip b's token ids (tails = pad) and every mask derived from them; block B*PT also copies the token counts.
// The features hold essentially all the bytes (B=16, T=32: 205 MB read in fp32, 103 MB written in bf16).
#include "common.hpp"

namespace {

constexpr int UNROLL = 4;

struct StageTrainK {
  const long* src[5]; long* dst[5];
  unsigned char* qm; unsigned char* qm2; unsigned char* hm; unsigned char* cm; unsigned char* tm; unsigned char* tmm; unsigned char* vm;
  const long* ntok; const long* qntok; long* d_ntok; long* d_qntok;
  const void* fts; void* d_fts;
  long src_ld[5]; long n; long pad;
  int src_len[5]; int dst_len[5];
  int B, T, PT;
};

// E output elements (16 bytes of TD) and the E source elements they come from
template <typename TS, typename TD>
struct Chunk {
  static constexpr int E = 16 / (int)sizeof(TD);
  static constexpr int SB = E * (int)sizeof(TS);       // source bytes: 32 (f32 -> bf16), 16, or 8 (bf16 -> f32)
  union { uint4 q[SB >= 16 ? SB / 16 : 1]; uint2 h; TS e[E]; } u;
  __device__ __forceinline__ void load(const TS* p) {
    if constexpr (SB >= 16) {
#pragma unroll
      for (int k = 0; k < SB / 16; ++k) u.q[k] = reinterpret_cast<const uint4*>(p)[k];
    } else {
      u.h = *reinterpret_cast<const uint2*>(p);
    }
  }
  // cast (bist_cast's rounding), store 16 bytes, and fold the stored values into s in element order (temporal_mask_kernel's order)
  __device__ __forceinline__ void store(TD* p, float& s) const {
    union { uint4 q; TD e[E]; } o;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      o.e[e] = from_f<TD>(to_f(u.e[e]));
      s += to_f(o.e[e]);
    }
    *reinterpret_cast<uint4*>(p) = o.q;
  }
};

template <typename TS, typename TD>
__device__ void stage_feature_row(const StageTrainK& a, long row) {
  __shared__ float red[4];
  using C = Chunk<TS, TD>;
  constexpr int E = C::E;
  const long b = row / a.PT, t = row % a.PT;
  const long nc = a.n / E;
  TD* dst = reinterpret_cast<TD*>(a.d_fts) + row * a.n;
  if (t >= a.T) {                                     // appended frame: zeros, excluded by its mask bit
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    for (long c = threadIdx.x; c < nc; c += 256) reinterpret_cast<uint4*>(dst)[c] = z;
    if (threadIdx.x == 0) a.vm[row] = 0;
    return;
  }
  const TS* src = reinterpret_cast<const TS*>(a.fts) + (b * a.T + t) * a.n;
  float s = 0.f;
  long c = threadIdx.x;
  for (; c + (UNROLL - 1) * 256 < nc; c += UNROLL * 256) {
    C ch[UNROLL];
#pragma unroll
    for (int k = 0; k < UNROLL; ++k) ch[k].load(src + (c + k * 256) * E);
#pragma unroll
    for (int k = 0; k < UNROLL; ++k) ch[k].store(dst + (c + k * 256) * E, s);
  }
  for (; c < nc; c += 256) {
    C ch;
    ch.load(src + c * E);
    ch.store(dst + c * E, s);
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) a.vm[row] = (red[0] + red[1] + red[2] + red[3]) != 0.f ? 1 : 0;
}

__device__ __forceinline__ long staged_id(const StageTrainK& a, int f, long b, int j) {
  return j < a.src_len[f] ? a.src[f][b * a.src_ld[f] + j] : a.pad;
}

__device__ void stage_tokens(const StageTrainK& a, long b) {
  enum { Q = 0, H = 1, CAP = 2, TRG = 3, TY = 4 };
  for (int f = 0; f < 5; ++f) {
    if (!a.src[f]) continue;
    const int P = a.dst_len[f];
    unsigned char* m = f == Q ? a.qm : f == H ? a.hm : f == CAP ? a.cm : f == TY ? a.tmm : nullptr;
    for (int j = threadIdx.x; j < P; j += 256) {
      const long v = staged_id(a, f, b, j);
      a.dst[f][b * P + j] = v;
      const unsigned char k = v != a.pad ? 1 : 0;
      if (m) m[b * P + j] = k;
      if (f == Q && a.qm2) {
        a.qm2[b * P + j] = k;
        a.qm2[(a.B + b) * P + j] = k;
      }
    }
  }
  if (a.src[TRG] && a.tm) {                           // (trg != pad).unsqueeze(-2) & subsequent_mask  (dataset.py:101-105)
    const int P = a.dst_len[TRG];
    for (int idx = threadIdx.x; idx < P * P; idx += 256) {
      const int i = idx / P, j = idx % P;
      a.tm[b * (long)P * P + idx] = (j <= i && staged_id(a, TRG, b, j) != a.pad) ? 1 : 0;
    }
  }
  if (b == 0 && threadIdx.x == 0) {
    if (a.ntok && a.d_ntok) a.d_ntok[0] = a.ntok[0];
    if (a.qntok && a.d_qntok) a.d_qntok[0] = a.qntok[0];
  }
}

template <typename TS, typename TD>
__global__ __launch_bounds__(256) void stage_train_kernel(StageTrainK a) {
  const long nrows = (long)a.B * a.PT;
  if ((long)blockIdx.x < nrows) stage_feature_row<TS, TD>(a, blockIdx.x);
  else stage_tokens(a, (long)blockIdx.x - nrows);
}

}  // namespace

extern "C" int bist_stage_train_batch(const BistTrainStage* d, void* stream) {
  BIST_REQUIRE(d, "bist_stage_train_batch: null descriptor");
  BIST_REQUIRE(d->B >= 1 && d->T >= 1 && d->PT >= d->T && d->row_elems >= 1 && d->fts && d->d_fts && d->temporal_mask,
               "bist_stage_train_batch: B >= 1, 1 <= T <= PT, features and temporal_mask required");
  BIST_REQUIRE((d->fts_dtype == BIST_F32 || d->fts_dtype == BIST_BF16) && (d->out_dtype == BIST_F32 || d->out_dtype == BIST_BF16),
               "bist_stage_train_batch: feature dtypes f32 / bf16");
  const int E = d->out_dtype == BIST_BF16 ? 8 : 4;
  BIST_REQUIRE(d->row_elems % E == 0 && (((uintptr_t)d->fts | (uintptr_t)d->d_fts) & 15) == 0,
               "bist_stage_train_batch: feature rows must be whole 16-byte vectors of the output dtype, 16-byte aligned");
  BIST_REQUIRE(d->src[0] && d->src[1] && d->src[3], "bist_stage_train_batch: query, his and trg are required");
  BIST_REQUIRE((d->src[4] == nullptr) == (d->trg_mean_mask == nullptr) && (d->src[2] == nullptr) == (d->cap_mask == nullptr),
               "bist_stage_train_batch: cap_mask / trg_mean_mask exactly when cap / trg_y are staged");
  BIST_REQUIRE(d->query_mask && d->his_mask && d->trg_mask, "bist_stage_train_batch: query_mask, his_mask and trg_mask required");
  BIST_REQUIRE(d->dst_len[3] == d->dst_len[4] || !d->src[4], "bist_stage_train_batch: trg and trg_y share one class length");
  StageTrainK a{};
  for (int f = 0; f < 5; ++f) {
    if (!d->src[f]) continue;
    BIST_REQUIRE(d->dst[f] && d->src_len[f] >= 1 && d->dst_len[f] >= d->src_len[f] && d->src_ld[f] >= d->src_len[f],
                 "bist_stage_train_batch: field %d: 1 <= length <= class length, row stride >= length", f);
    a.src[f] = (const long*)d->src[f];
    a.dst[f] = (long*)d->dst[f];
    a.src_ld[f] = (long)d->src_ld[f];
    a.src_len[f] = d->src_len[f];
    a.dst_len[f] = d->dst_len[f];
  }
  a.qm = (unsigned char*)d->query_mask; a.qm2 = (unsigned char*)d->query_mask2; a.hm = (unsigned char*)d->his_mask;
  a.cm = (unsigned char*)d->cap_mask; a.tm = (unsigned char*)d->trg_mask; a.tmm = (unsigned char*)d->trg_mean_mask;
  a.vm = (unsigned char*)d->temporal_mask;
  a.ntok = (const long*)d->ntokens; a.qntok = (const long*)d->qntokens; a.d_ntok = (long*)d->d_ntokens; a.d_qntok = (long*)d->d_qntokens;
  a.fts = d->fts; a.d_fts = d->d_fts;
  a.n = (long)d->row_elems; a.pad = (long)d->pad;
  a.B = d->B; a.T = d->T; a.PT = d->PT;
  const long blocks = (long)d->B * d->PT + d->B;
  BIST_REQUIRE(blocks < (1L << 31), "bist_stage_train_batch: too many rows");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 g((unsigned)blocks), blk(256);
  if (d->fts_dtype == BIST_F32 && d->out_dtype == BIST_BF16) hipLaunchKernelGGL((stage_train_kernel<float, bf16_t>), g, blk, 0, st, a);
  else if (d->fts_dtype == BIST_BF16 && d->out_dtype == BIST_BF16) hipLaunchKernelGGL((stage_train_kernel<bf16_t, bf16_t>), g, blk, 0, st, a);
  else if (d->fts_dtype == BIST_F32) hipLaunchKernelGGL((stage_train_kernel<float, float>), g, blk, 0, st, a);
  else hipLaunchKernelGGL((stage_train_kernel<bf16_t, float>), g, blk, 0, st, a);
  BIST_LAUNCH_CHECK("bist_stage_train_batch");
  return BIST_OK;
}
