// Deterministic forms of the row reductions of backward.hip (bias gradients, LayerNorm gain / offset gradients, the stage-2 value bias,
// the shared embedding): no float atomics.  Every (job, row chunk) writes its fp32 partial sums to a slab of a caller-provided
// workspace; a second launch sums a job's slabs in chunk-index order and does ONE plain `out += total` per element.  The chunking of a
// job is a function of the job's own shape only, so its result does not depend on which other jobs share the launch, nor on the order
// in which workgroups retire.  The embedding has no slabs: the first row that carries an id owns it and sums all rows of that id in
// ascending row order (the ordering of pointer_mix, generator.hip).
// Two jobs of one call must not overlap in their destinations (the caller puts such jobs into separate calls, in order).
#include "common.hpp"

namespace {

inline unsigned blocks_for(long n, int per) { return (unsigned)((n + per - 1) / per); }

// ---- column sums --------------------------------------------------------------------------------------------------------------------
// rows per chunk of a [M x N] job: at most 128 chunks, at least 16 rows each -- a function of M alone
inline int colsum_chunk_rows(long M) { const long r = (M + 127) / 128; return r < 16 ? 16 : (int)r; }

constexpr int DET_COLSUM_JOBS = 40;
struct DetColSumBatch {
  const void* x[DET_COLSUM_JOBS]; float* out[DET_COLSUM_JOBS];
  int M[DET_COLSUM_JOBS], N[DET_COLSUM_JOBS], ld[DET_COLSUM_JOBS], rpb[DET_COLSUM_JOBS], cb[DET_COLSUM_JOBS], nchunk[DET_COLSUM_JOBS];
  unsigned slab[DET_COLSUM_JOBS];          // first float of the job's [nchunk][N] slabs in the workspace
  unsigned char vec[DET_COLSUM_JOBS];      // 16-byte loads: N, ld whole pieces and an aligned base
  int first[DET_COLSUM_JOBS + 1];          // first block of every job in the partial launch; first[n] = total
  int cfirst[DET_COLSUM_JOBS + 1];         // ... in the combine launch (256 columns per block)
  int n;
};

// slab[chunk][n] = sum of the chunk's rows of column n.  The order of additions per column is the same on both paths: row lane rl takes
// rows m0 + rl, m0 + rl + 4, ..., then lanes 0 + 1 + 2 + 3.
template <typename T>
__global__ __launch_bounds__(256) void col_sum_partial_kernel(const DetColSumBatch b, float* __restrict__ ws) {
  constexpr int E = 16 / (int)sizeof(T);
  __shared__ float part[4][64 * E];
  int j = 0;
  while (j + 1 < b.n && (int)blockIdx.x >= b.first[j + 1]) ++j;
  const int lb = (int)blockIdx.x - b.first[j];
  const int bx = lb % b.cb[j], by = lb / b.cb[j];
  const T* x = reinterpret_cast<const T*>(b.x[j]);
  const int M = b.M[j], N = b.N[j], ld = b.ld[j], rpb = b.rpb[j];
  const int c = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int m0 = by * rpb, m1 = min(M, m0 + rpb);
  float* slab = ws + b.slab[j] + (long)by * N;
  if (b.vec[j]) {
    const int n0 = (bx * 64 + c) * E;
    float acc[E];
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = 0.f;
    if (n0 < N) {
#pragma unroll 4
      for (int m = m0 + rl; m < m1; m += 4) {
        const uint4 q = *reinterpret_cast<const uint4*>(x + (long)m * ld + n0);
        const T* qe = reinterpret_cast<const T*>(&q);
#pragma unroll
        for (int e = 0; e < E; ++e) acc[e] += to_f(qe[e]);
      }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) part[rl][c * E + e] = acc[e];
    __syncthreads();
    for (int idx = threadIdx.x; idx < 64 * E; idx += 256) {
      const int n = bx * 64 * E + idx;
      if (n < N) slab[n] = (part[0][idx] + part[1][idx]) + (part[2][idx] + part[3][idx]);
    }
    return;
  }
  const int n = bx * 64 + c;
  float acc = 0.f;
  if (n < N)
    for (int m = m0 + rl; m < m1; m += 4) acc += to_f(x[(long)m * ld + n]);
  part[rl][c] = acc;
  __syncthreads();
  if (rl == 0 && n < N) slab[n] = (part[0][c] + part[1][c]) + (part[2][c] + part[3][c]);
}

// out[n] += slab[0][n] + slab[1][n] + ... in chunk order: one thread per column, one plain read-modify-write
__global__ __launch_bounds__(256) void col_sum_combine_kernel(const DetColSumBatch b, const float* __restrict__ ws) {
  int j = 0;
  while (j + 1 < b.n && (int)blockIdx.x >= b.cfirst[j + 1]) ++j;
  const int n = ((int)blockIdx.x - b.cfirst[j]) * 256 + (int)threadIdx.x;
  const int N = b.N[j];
  if (n >= N) return;
  const float* slab = ws + b.slab[j] + n;
  float t = 0.f;
  for (int k = 0; k < b.nchunk[j]; ++k) t += slab[(long)k * N];
  b.out[j][n] += t;
}

// ---- LayerNorm gain / offset gradients ---------------------------------------------------------------------------------------------------
// rows per wave of a job: at most 512 waves, at least 4 rows each -- a function of the row count alone
inline int lngrad_wave_rows(long rows) { const long r = (rows + 511) / 512; return r < 4 ? 4 : (int)r; }

constexpr int DET_LN_JOBS = 32;
struct DetLnBatch {
  const void* dy[DET_LN_JOBS]; const void* x[DET_LN_JOBS]; float* da[DET_LN_JOBS]; float* db[DET_LN_JOBS];
  int rows[DET_LN_JOBS], lddy[DET_LN_JOBS], ldx[DET_LN_JOBS], rpw[DET_LN_JOBS], nwave[DET_LN_JOBS];
  float eps[DET_LN_JOBS];
  unsigned slab[DET_LN_JOBS];              // first float of the job's [nwave][2][d] slabs
  int first[DET_LN_JOBS + 1], cfirst[DET_LN_JOBS + 1];
  int n, d;
};

// One wave per run of rpw rows; lane l holds columns l, l + 64, ... (NC of them) of the row in registers.  slab[wave][0][c] = the wave's
// sum over its rows, in row order, of dy * (x - mean) / (std + eps); slab[wave][1][c] = of dy.
template <typename T, int NC>
__global__ __launch_bounds__(256) void ln_param_partial_kernel(const DetLnBatch b, float* __restrict__ ws) {
  int j = 0;
  while (j + 1 < b.n && (int)blockIdx.x >= b.first[j + 1]) ++j;
  const int lane = threadIdx.x & 63;
  const int wave = ((int)blockIdx.x - b.first[j]) * 4 + (int)(threadIdx.x >> 6);
  if (wave >= b.nwave[j]) return;
  const T* __restrict__ x = (const T*)b.x[j];
  const T* __restrict__ dy = (const T*)b.dy[j];
  const int d = b.d, rows = b.rows[j], rpw = b.rpw[j];
  const long ldx = b.ldx[j], lddy = b.lddy[j];
  const float eps = b.eps[j];
  const int r0 = wave * rpw, r1 = min(rows, r0 + rpw);
  float pa[NC], pb[NC];
#pragma unroll
  for (int u = 0; u < NC; ++u) { pa[u] = 0.f; pb[u] = 0.f; }
  for (int row = r0; row < r1; ++row) {
    float xv[NC], gv[NC];
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < NC; ++u) {
      const int c = lane + u * 64;
      xv[u] = c < d ? to_f(x[row * ldx + c]) : 0.f;
      gv[u] = c < d ? to_f(dy[row * lddy + c]) : 0.f;
      s += xv[u];
    }
    const float mean = wave_sum(s) / (float)d;
    float q = 0.f;
#pragma unroll
    for (int u = 0; u < NC; ++u) {
      const int c = lane + u * 64;
      xv[u] = c < d ? xv[u] - mean : 0.f;
      q += xv[u] * xv[u];
    }
    q = wave_sum(q);
    const float inv = 1.f / (sqrtf(q / (float)(d - 1)) + eps);
#pragma unroll
    for (int u = 0; u < NC; ++u) { pa[u] += gv[u] * xv[u] * inv; pb[u] += gv[u]; }
  }
  float* slab = ws + b.slab[j] + (long)wave * 2 * d;
#pragma unroll
  for (int u = 0; u < NC; ++u) {
    const int c = lane + u * 64;
    if (c < d) { slab[c] = pa[u]; slab[d + c] = pb[u]; }
  }
}

__global__ __launch_bounds__(256) void ln_param_combine_kernel(const DetLnBatch b, const float* __restrict__ ws) {
  int j = 0;
  while (j + 1 < b.n && (int)blockIdx.x >= b.cfirst[j + 1]) ++j;
  const int c = ((int)blockIdx.x - b.cfirst[j]) * 256 + (int)threadIdx.x;
  const int d = b.d;
  if (c >= d) return;
  const float* slab = ws + b.slab[j] + c;
  float ta = 0.f, tb = 0.f;
  for (int w = 0; w < b.nwave[j]; ++w) { ta += slab[(long)w * 2 * d]; tb += slab[(long)w * 2 * d + d]; }
  b.da[j][c] += ta;
  b.db[j][c] += tb;
}

// ---- stage-2 value bias ----------------------------------------------------------------------------------------------------------------
// scaled_bias_bwd_kernel of backward.hip with the block's dbias partial sums written to slab[block][h * dk] instead of added atomically;
// ds is computed by the same expressions in the same order.
template <typename T>
__global__ __launch_bounds__(256) void scaled_bias_partial_kernel(const T* __restrict__ dy, const float* __restrict__ s, const T* __restrict__ bias,
                                                                  float* __restrict__ ds, float* __restrict__ ws, long M, int h, int dk, int rpb,
                                                                  long Mset, long bias_zs) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long m0 = (long)blockIdx.x * rpb, m1 = min(M, m0 + rpb);
  bias += (m0 / Mset) * bias_zs;                     // Mset % rpb == 0: a block's rows lie in one set
  float* slab = ws + (long)blockIdx.x * h * dk;
  for (int hh = w; hh < h; hh += 4) {
    float bv[4], part[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { const int c = lane + 64 * u; bv[u] = c < dk ? to_f(bias[hh * dk + c]) : 0.f; part[u] = 0.f; }
    for (long m = m0; m < m1; ++m) {
      const T* g = dy + (m * h + hh) * dk;
      const float sv = s[m * h + hh];
      float acc = 0.f;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int c = lane + 64 * u;
        const float gv = c < dk ? to_f(g[c]) : 0.f;
        acc += gv * bv[u];
        part[u] += sv * gv;
      }
      acc = wave_sum(acc);
      if (lane == 0) ds[m * h + hh] = acc;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) { const int c = lane + 64 * u; if (c < dk) slab[hh * dk + c] = part[u]; }
  }
}

// dbias[z][c] += the slabs of set z's blocks, in block order; grid = (column blocks, sets)
__global__ __launch_bounds__(256) void scaled_bias_combine_kernel(const float* __restrict__ ws, float* __restrict__ dbias, int d, int blocks_per_set,
                                                                  long dbias_zs) {
  const int c = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (c >= d) return;
  const int z = blockIdx.y;
  const float* slab = ws + (long)z * blocks_per_set * d + c;
  float t = 0.f;
  for (int k = 0; k < blocks_per_set; ++k) t += slab[(long)k * d];
  dbias[z * dbias_zs + c] += t;
}

// ---- embedding ---------------------------------------------------------------------------------------------------------------------------
constexpr int DET_EMB_JOBS = 16;
struct DetEmbBatch {
  const long* ids[DET_EMB_JOBS]; const void* dy[DET_EMB_JOBS];
  long row0[DET_EMB_JOBS + 1];             // first global row of every job; row0[n] = all rows
  float p[DET_EMB_JOBS]; unsigned long long seed[DET_EMB_JOBS]; const unsigned long long* ctr[DET_EMB_JOBS];
  int n;
};

// One workgroup per global row r.  It walks all rows in tiles of 256 (one id per thread, the matches of a tile as four 64-bit ballots in
// LDS): a match below r means another row owns the id -- the workgroup leaves; otherwise it sums the matching rows from r on in
// ascending order (thread t: columns t, t + 256, ...; scale and regenerated dropout mask as embed_bwd_kernel, mask index = the
// element's index in its own job) and adds the total to dlut[id, :] once.
template <typename T>
__global__ __launch_bounds__(256) void embed_bwd_det_kernel(const DetEmbBatch b, float* __restrict__ dlut, long lut_rows, int d, float scale) {
  __shared__ unsigned long long smask[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long R = b.row0[b.n];
  const long r = blockIdx.x;
  int jr = 0;
  while (jr + 1 < b.n && r >= b.row0[jr + 1]) ++jr;
  const long id = b.ids[jr][r - b.row0[jr]];
  if (id < 0 || id >= lut_rows) return;              // (an id outside the table has no row to add to)
  float acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.f;
  for (long base = 0; base < R; base += 256) {
    const long g = base + tid;
    bool match = false;
    if (g < R) {
      int j = 0;
      while (j + 1 < b.n && g >= b.row0[j + 1]) ++j;
      match = b.ids[j][g - b.row0[j]] == id;
    }
    const unsigned long long bal = __ballot(match);
    __syncthreads();                                 // the previous tile's masks have been read
    if (lane == 0) smask[w] = bal;
    __syncthreads();
    for (int ww = 0; ww < 4; ++ww) {
      unsigned long long mm = smask[ww];
      while (mm) {
        const int bit = __ffsll(mm) - 1;
        mm &= mm - 1;
        const long g2 = base + ww * 64 + bit;
        if (g2 < r) return;                          // an earlier row carries this id and owns it (the same decision in every thread)
        int j2 = 0;
        while (j2 + 1 < b.n && g2 >= b.row0[j2 + 1]) ++j2;
        const long local = g2 - b.row0[j2];
        const T* src = (const T*)b.dy[j2] + local * d;
        const float p = b.p[j2];
        const unsigned long long key = p > 0.f ? b.seed[j2] + (b.ctr[j2] ? b.ctr[j2][0] * 0xD1B54A32D192ED03ULL : 0ULL) : 0ULL;
        const float ks = p > 0.f ? 1.f / (1.f - p) : 1.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int c = tid + 256 * k;
          if (c < d) {
            float gv = to_f(src[c]) * scale;
            if (p > 0.f) gv *= drop_mul(key, (unsigned long long)(local * d + c), p, ks);
            acc[k] += gv;
          }
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = tid + 256 * k;
    if (c < d) dlut[id * d + c] += acc[k];
  }
}

inline bool ws_ok(const void* ws, int64_t have, int64_t need) { return ws && ((uintptr_t)ws % 4) == 0 && have >= need; }

}  // namespace

// ---- entry points ------------------------------------------------------------------------------------------------------------------------
extern "C" int64_t bist_col_sum_multi_det_workspace(const BistColSum* jobs, int32_t njobs) {
  if (!jobs || njobs <= 0) return -1;
  int64_t floats = 0;
  for (int i = 0; i < njobs; ++i) {
    if (jobs[i].M <= 0 || jobs[i].N <= 0) return -1;
    floats += (int64_t)blocks_for(jobs[i].M, colsum_chunk_rows(jobs[i].M)) * jobs[i].N;
  }
  return floats * 4;
}

extern "C" int bist_col_sum_multi_det(const BistColSum* jobs, int32_t njobs, int32_t dtype, void* workspace, int64_t workspace_bytes,
                                      void* stream) {
  BIST_REQUIRE(jobs && njobs > 0, "bist_col_sum_multi_det: bad argument");
  BIST_REQUIRE(dtype == BIST_BF16 || dtype == BIST_F32, "bist_col_sum_multi_det: bad dtype %d", dtype);
  for (int i = 0; i < njobs; ++i) {
    const BistColSum& q = jobs[i];
    BIST_REQUIRE(q.x && q.out && q.M > 0 && q.N > 0 && q.ldx >= q.N && q.M < (1L << 31) && q.ldx < (1L << 31), "bist_col_sum_multi_det: bad job %d", i);
  }
  const int64_t need = bist_col_sum_multi_det_workspace(jobs, njobs);
  BIST_REQUIRE(need < (1LL << 33), "bist_col_sum_multi_det: the jobs' slabs exceed 8 GiB; split the call");
  BIST_REQUIRE(ws_ok(workspace, workspace_bytes, need), "bist_col_sum_multi_det: workspace of %lld bytes, %lld needed (bist_col_sum_multi_det_workspace)",
               (long long)workspace_bytes, (long long)need);
  hipStream_t st = (hipStream_t)stream;
  float* ws = (float*)workspace;
  const long esz = dtype == BIST_BF16 ? 2 : 4, piece = 16 / esz;
  long slab = 0;
  for (int base = 0; base < njobs; base += DET_COLSUM_JOBS) {
    DetColSumBatch b;
    b.n = njobs - base < DET_COLSUM_JOBS ? njobs - base : DET_COLSUM_JOBS;
    int total = 0, ctotal = 0;
    for (int i = 0; i < b.n; ++i) {
      const BistColSum& q = jobs[base + i];
      const bool vec = (q.N % piece == 0) && (q.ldx % piece == 0) && ((uintptr_t)q.x % 16 == 0);
      const long cb = vec ? blocks_for(q.N, (int)(64 * piece)) : blocks_for(q.N, 64);
      const int rpb = colsum_chunk_rows(q.M);
      const int nchunk = (int)blocks_for(q.M, rpb);
      b.vec[i] = vec ? 1 : 0;
      b.x[i] = q.x; b.out[i] = q.out; b.M[i] = (int)q.M; b.N[i] = q.N; b.ld[i] = (int)q.ldx; b.rpb[i] = rpb; b.cb[i] = (int)cb; b.nchunk[i] = nchunk;
      b.slab[i] = (unsigned)slab;
      slab += (long)nchunk * q.N;
      b.first[i] = total; b.cfirst[i] = ctotal;
      total += (int)(cb * nchunk);
      ctotal += (int)blocks_for(q.N, 256);
    }
    b.first[b.n] = total; b.cfirst[b.n] = ctotal;
    if (dtype == BIST_BF16) hipLaunchKernelGGL(col_sum_partial_kernel<bf16_t>, dim3((unsigned)total), dim3(256), 0, st, b, ws);
    else hipLaunchKernelGGL(col_sum_partial_kernel<float>, dim3((unsigned)total), dim3(256), 0, st, b, ws);
    BIST_LAUNCH_CHECK("bist_col_sum_multi_det");
    hipLaunchKernelGGL(col_sum_combine_kernel, dim3((unsigned)ctotal), dim3(256), 0, st, b, (const float*)ws);
    BIST_LAUNCH_CHECK("bist_col_sum_multi_det");
  }
  return BIST_OK;
}

extern "C" int64_t bist_layernorm_param_grad_multi_det_workspace(const BistLnGrad* jobs, int32_t njobs, int32_t d) {
  if (!jobs || njobs <= 0 || d <= 1) return -1;
  int64_t floats = 0;
  for (int i = 0; i < njobs; ++i) {
    if (jobs[i].rows <= 0) return -1;
    floats += (int64_t)blocks_for(jobs[i].rows, lngrad_wave_rows(jobs[i].rows)) * 2 * d;
  }
  return floats * 4;
}

extern "C" int bist_layernorm_param_grad_multi_det(const BistLnGrad* jobs, int32_t njobs, int32_t d, int32_t dtype, void* workspace,
                                                   int64_t workspace_bytes, void* stream) {
  BIST_REQUIRE(jobs && njobs > 0, "bist_layernorm_param_grad_multi_det: bad argument");
  BIST_REQUIRE((dtype == BIST_BF16 || dtype == BIST_F32) && d > 1 && d <= 2048, "bist_layernorm_param_grad_multi_det: bf16 / f32 rows of 2 .. 2048 columns");
  for (int i = 0; i < njobs; ++i) {
    const BistLnGrad& q = jobs[i];
    BIST_REQUIRE(q.dy && q.x && q.da && q.db && q.rows > 0 && q.rows < (1L << 31) && q.lddy >= d && q.ldx >= d && q.lddy < (1L << 31) && q.ldx < (1L << 31),
                 "bist_layernorm_param_grad_multi_det: bad job %d", i);
  }
  const int64_t need = bist_layernorm_param_grad_multi_det_workspace(jobs, njobs, d);
  BIST_REQUIRE(need < (1LL << 33), "bist_layernorm_param_grad_multi_det: the jobs' slabs exceed 8 GiB; split the call");
  BIST_REQUIRE(ws_ok(workspace, workspace_bytes, need),
               "bist_layernorm_param_grad_multi_det: workspace of %lld bytes, %lld needed (bist_layernorm_param_grad_multi_det_workspace)",
               (long long)workspace_bytes, (long long)need);
  hipStream_t st = (hipStream_t)stream;
  float* ws = (float*)workspace;
  long slab = 0;
  for (int base = 0; base < njobs; base += DET_LN_JOBS) {
    DetLnBatch b;
    b.n = njobs - base < DET_LN_JOBS ? njobs - base : DET_LN_JOBS;
    b.d = d;
    int total = 0, ctotal = 0;
    for (int i = 0; i < b.n; ++i) {
      const BistLnGrad& q = jobs[base + i];
      const int rpw = lngrad_wave_rows(q.rows);
      const int nwave = (int)blocks_for(q.rows, rpw);
      b.dy[i] = q.dy; b.x[i] = q.x; b.da[i] = q.da; b.db[i] = q.db;
      b.rows[i] = (int)q.rows; b.lddy[i] = (int)q.lddy; b.ldx[i] = (int)q.ldx; b.rpw[i] = rpw; b.nwave[i] = nwave; b.eps[i] = q.eps;
      b.slab[i] = (unsigned)slab;
      slab += (long)nwave * 2 * d;
      b.first[i] = total; b.cfirst[i] = ctotal;
      total += (int)blocks_for(nwave, 4);
      ctotal += (int)blocks_for(d, 256);
    }
    b.first[b.n] = total; b.cfirst[b.n] = ctotal;
#define LNP(TT, NC) hipLaunchKernelGGL((ln_param_partial_kernel<TT, NC>), dim3((unsigned)total), dim3(256), 0, st, b, ws)
#define LNP_D(TT)                    \
  do {                               \
    if (d <= 64) LNP(TT, 1);         \
    else if (d <= 256) LNP(TT, 4);   \
    else if (d <= 512) LNP(TT, 8);   \
    else if (d <= 1024) LNP(TT, 16); \
    else LNP(TT, 32);                \
  } while (0)
    if (dtype == BIST_BF16) LNP_D(bf16_t); else LNP_D(float);
#undef LNP_D
#undef LNP
    BIST_LAUNCH_CHECK("bist_layernorm_param_grad_multi_det");
    hipLaunchKernelGGL(ln_param_combine_kernel, dim3((unsigned)ctotal), dim3(256), 0, st, b, (const float*)ws);
    BIST_LAUNCH_CHECK("bist_layernorm_param_grad_multi_det");
  }
  return BIST_OK;
}

static int scaled_bias_rows_per_block(long Mset) {
  int rpb = 4;                                     // as bist_scaled_bias_bwd_z: a block's rows must lie in one set
  while (rpb > 1 && Mset % rpb != 0) rpb >>= 1;
  return rpb;
}

extern "C" int64_t bist_scaled_bias_bwd_det_workspace(int64_t M, int32_t h, int32_t dk, int32_t nsets) {
  if (M <= 0 || h <= 0 || dk <= 0 || nsets < 1 || M % nsets != 0) return -1;
  return (int64_t)blocks_for(M, scaled_bias_rows_per_block(M / nsets)) * h * dk * 4;
}

extern "C" int bist_scaled_bias_bwd_det(const void* dy, const float* s, const void* bias, float* ds, float* dbias, int64_t M, int32_t h,
                                        int32_t dk, int32_t nsets, int64_t bias_zs, int64_t dbias_zs, int32_t dtype, void* workspace,
                                        int64_t workspace_bytes, void* stream) {
  BIST_REQUIRE(dy && s && bias && ds && dbias && M > 0 && h > 0 && dk > 0 && nsets >= 1 && M % nsets == 0, "bist_scaled_bias_bwd_det: bad argument");
  BIST_REQUIRE(dk <= 256, "bist_scaled_bias_bwd_det: head width %d > 256", dk);
  BIST_REQUIRE(dtype == BIST_BF16 || dtype == BIST_F32, "bist_scaled_bias_bwd_det: bad dtype %d", dtype);
  BIST_REQUIRE(nsets == 1 || dbias_zs >= (int64_t)h * dk, "bist_scaled_bias_bwd_det: the sets' gradients overlap");
  const int64_t need = bist_scaled_bias_bwd_det_workspace(M, h, dk, nsets);
  BIST_REQUIRE(ws_ok(workspace, workspace_bytes, need), "bist_scaled_bias_bwd_det: workspace of %lld bytes, %lld needed (bist_scaled_bias_bwd_det_workspace)",
               (long long)workspace_bytes, (long long)need);
  hipStream_t st = (hipStream_t)stream;
  float* ws = (float*)workspace;
  const long Mset = M / nsets;
  const int rpb = scaled_bias_rows_per_block(Mset);
  const unsigned nblk = blocks_for(M, rpb);
  if (dtype == BIST_BF16)
    hipLaunchKernelGGL(scaled_bias_partial_kernel<bf16_t>, dim3(nblk), dim3(256), 0, st, (const bf16_t*)dy, s, (const bf16_t*)bias, ds, ws, (long)M, h, dk, rpb,
                       Mset, (long)bias_zs);
  else
    hipLaunchKernelGGL(scaled_bias_partial_kernel<float>, dim3(nblk), dim3(256), 0, st, (const float*)dy, s, (const float*)bias, ds, ws, (long)M, h, dk, rpb,
                       Mset, (long)bias_zs);
  BIST_LAUNCH_CHECK("bist_scaled_bias_bwd_det");
  hipLaunchKernelGGL(scaled_bias_combine_kernel, dim3(blocks_for((long)h * dk, 256), (unsigned)nsets), dim3(256), 0, st, (const float*)ws, dbias, h * dk,
                     (int)(Mset / rpb), (long)dbias_zs);
  BIST_LAUNCH_CHECK("bist_scaled_bias_bwd_det");
  return BIST_OK;
}

extern "C" int bist_embed_bwd_multi_det(const BistEmbedBwd* jobs, int32_t njobs, float* dlut, int64_t lut_rows, int32_t d, int32_t dtype,
                                        void* stream) {
  BIST_REQUIRE(jobs && njobs > 0 && njobs <= DET_EMB_JOBS && dlut && lut_rows > 0, "bist_embed_bwd_multi_det: 1 .. %d jobs over one table", DET_EMB_JOBS);
  BIST_REQUIRE(d > 0 && d <= 2048, "bist_embed_bwd_multi_det: row width %d outside 1 .. 2048", d);
  BIST_REQUIRE(dtype == BIST_BF16 || dtype == BIST_F32, "bist_embed_bwd_multi_det: bad dtype %d", dtype);
  DetEmbBatch b;
  b.n = njobs;
  long rows = 0;
  for (int i = 0; i < njobs; ++i) {
    const BistEmbedBwd& q = jobs[i];
    BIST_REQUIRE(q.ids && q.dy && q.rows > 0, "bist_embed_bwd_multi_det: bad job %d", i);
    BIST_REQUIRE(q.drop.p >= 0.f && q.drop.p < 1.f, "bist_embed_bwd_multi_det: drop p out of range (job %d)", i);
    b.ids[i] = (const long*)q.ids; b.dy[i] = q.dy; b.row0[i] = rows;
    b.p[i] = q.drop.p; b.seed[i] = q.drop.seed; b.ctr[i] = q.drop.p > 0.f ? (const unsigned long long*)q.drop.ctr : nullptr;
    rows += q.rows;
  }
  BIST_REQUIRE(rows < (1L << 31), "bist_embed_bwd_multi_det: too many rows");
  b.row0[njobs] = rows;
  hipStream_t st = (hipStream_t)stream;
  const float scale = sqrtf((float)d);
  if (dtype == BIST_BF16) hipLaunchKernelGGL(embed_bwd_det_kernel<bf16_t>, dim3((unsigned)rows), dim3(256), 0, st, b, dlut, (long)lut_rows, d, scale);
  else hipLaunchKernelGGL(embed_bwd_det_kernel<float>, dim3((unsigned)rows), dim3(256), 0, st, b, dlut, (long)lut_rows, d, scale);
  BIST_LAUNCH_CHECK("bist_embed_bwd_multi_det");
  return BIST_OK;
}
