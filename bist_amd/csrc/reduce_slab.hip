// Slab forms of the batched row reductions of backward.hip (bias gradients, LayerNorm gain / offset gradients): ONE launch per batch of
// jobs and one float atomic per destination element per job.  backward.hip ends every workgroup of a job in N (or 2 d) atomics on the
// job's one accumulator row; here every (job, row chunk) workgroup writes its fp32 partial row to a slab of a caller-provided
// workspace with 16-byte stores, releases at agent scope and takes a ticket on the job's counter word.  The workgroup that draws the
// job's last ticket acquires, sums the job's slabs in chunk-index order and adds the total to the destination (an atomic still: two
// jobs of a call may share a destination), then returns the counter to zero, so a replayed graph starts clean.  The hand-off is the one
// of t64_ring_body (gemm.hip).  No workgroup ever waits for another one.
// Workspace: [64 counter words, zero before the first call and after every call][slabs, 16-byte aligned].  Calls that share a
// workspace must be ordered on one stream.  The chunking of a job is a function of its own shape.
#include "common.hpp"

namespace {

inline unsigned blocks_for(long n, int per) { return (unsigned)((n + per - 1) / per); }

constexpr int RS_HEADER_BYTES = 256;                // the counter words of one launch (one per job)
constexpr int RS_COLSUM_JOBS = 48, RS_LN_JOBS = 40; // jobs per launch (kernel-argument tables), both below the 64 counters
constexpr int RS_MAX_CHUNKS = 128;                  // the last arriver reads at most this many slabs per job

// rows per chunk of a [M x N] column sum: at most 128 chunks, at least 16 rows (4 per row lane) each
inline int rs_colsum_chunk_rows(long M) { const long r = (M + RS_MAX_CHUNKS - 1) / RS_MAX_CHUNKS; return r < 16 ? 16 : (int)r; }
// rows per wave of a LayerNorm job: a chunk is a workgroup of 4 waves, at most 128 chunks, at least 4 rows (one trip of loads) per wave
inline int rs_ln_wave_rows(long rows) { const long r = (rows + 4 * RS_MAX_CHUNKS - 1) / (4 * RS_MAX_CHUNKS); return r < 4 ? 4 : (int)r; }
inline int rs_pad4(int n) { return (n + 3) & ~3; }  // slab rows are whole 16-byte pieces

struct RsColSumBatch {
  const void* x[RS_COLSUM_JOBS]; float* out[RS_COLSUM_JOBS];
  int M[RS_COLSUM_JOBS], N[RS_COLSUM_JOBS], ld[RS_COLSUM_JOBS], rpb[RS_COLSUM_JOBS], cb[RS_COLSUM_JOBS], nchunk[RS_COLSUM_JOBS];
  unsigned slab[RS_COLSUM_JOBS];         // first float of the job's [nchunk][pad4(N)] slabs, counted from the end of the header
  unsigned char vec[RS_COLSUM_JOBS];     // 16-byte loads: N, ld whole pieces and an aligned base
  int first[RS_COLSUM_JOBS + 1];         // first block of every job; first[n] = total
  int n;
};

struct RsLnBatch {
  const void* dy[RS_LN_JOBS]; const void* x[RS_LN_JOBS]; float* da[RS_LN_JOBS]; float* db[RS_LN_JOBS];
  int rows[RS_LN_JOBS], lddy[RS_LN_JOBS], ldx[RS_LN_JOBS], rpw[RS_LN_JOBS];
  float eps[RS_LN_JOBS];
  unsigned slab[RS_LN_JOBS];             // first float of the job's [nchunk][2][d] slabs
  int first[RS_LN_JOBS + 1];             // first block (= chunk) of every job; first[n] = total
  int n, d;
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The workgroup's slab stores are issued.  Release them, take a ticket of `total`; true (in every thread) in the workgroup that drew the
// last one, which has acquired the other workgroups' slabs and has returned the counter to zero.  Sequence as in t64_ring_body.
__device__ __forceinline__ bool rs_last_arriver(int* cnt, int total, int* flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int old = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = old == total - 1;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    *flag = last;
  }
  __syncthreads();
  return *flag != 0;
}

// Last arriver: total[n] = slab[0][n] + slab[1][n] + ... over the job's nchunk slab rows of L floats (L % 4 == 0), then add(n, total[n]).
// All 256 threads read 16-byte pieces; rows shorter than 1024 floats are summed as 256 / (L / 4) runs of consecutive chunks side by
// side, combined in run order through `lds` (1024 floats; every thread is past its earlier use of it).
template <typename F>
__device__ __forceinline__ void rs_finish(const float* slabs, int L, int nchunk, float* lds, F add) {
  const int tid = threadIdx.x;
  const int G = L >> 2;
  if (G >= 256) {
    for (int g = tid; g < G; g += 256) {
      float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
      for (int k = 0; k < nchunk; ++k) {
        const float4 v = *reinterpret_cast<const float4*>(slabs + (long)k * L + 4 * g);
        t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
      }
      add(4 * g, t.x); add(4 * g + 1, t.y); add(4 * g + 2, t.z); add(4 * g + 3, t.w);
    }
    return;
  }
  const int P = 256 / G, per = (nchunk + P - 1) / P;
  const int p = tid / G, g = tid - p * G;
  if (p < P) {
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    const int k1 = min(nchunk, (p + 1) * per);
#pragma unroll 8
    for (int k = p * per; k < k1; ++k) {
      const float4 v = *reinterpret_cast<const float4*>(slabs + (long)k * L + 4 * g);
      t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
    }
    *reinterpret_cast<float4*>(lds + p * L + 4 * g) = t;
  }
  __syncthreads();
  for (int n = tid; n < L; n += 256) {
    float t = lds[n];
    for (int q = 1; q < P; ++q) t += lds[q * L + n];
    add(n, t);
  }
}

// out[n] += sum_m x[m, n] per job.  Block = (64 columns x 16 bytes) x 4 row lanes of one row chunk, as col_sum_multi_kernel.
template <typename T>
__global__ __launch_bounds__(256) void col_sum_slab_kernel(const RsColSumBatch b, float* ws) {
  constexpr int E = 16 / (int)sizeof(T);          // columns per thread on the vector path
  __shared__ __attribute__((aligned(16))) float lds[4 * 64 * E + 4];      // [row lane][column] partial sums (>= 1024 floats), then the flag
  float (*part)[64 * E] = reinterpret_cast<float (*)[64 * E]>(lds);
  int* flag = reinterpret_cast<int*>(lds + 4 * 64 * E);
  int j = 0;
  while (j + 1 < b.n && (int)blockIdx.x >= b.first[j + 1]) ++j;
  const int lb = (int)blockIdx.x - b.first[j];
  const int bx = lb % b.cb[j], by = lb / b.cb[j];
  const T* x = reinterpret_cast<const T*>(b.x[j]);
  const int M = b.M[j], N = b.N[j], ld = b.ld[j], rpb = b.rpb[j];
  const int L = (N + 3) & ~3;
  const int tid = threadIdx.x, c = tid & 63, rl = tid >> 6;
  const int m0 = by * rpb, m1 = min(M, m0 + rpb);
  float* slabs = ws + RS_HEADER_BYTES / 4 + b.slab[j];
  float* mine = slabs + (long)by * L;
  int W;                                          // columns of this block
  if (b.vec[j]) {
    W = 64 * E;
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
  } else {
    W = 64;
    const int n = bx * 64 + c;
    float acc = 0.f;
    if (n < N)
      for (int m = m0 + rl; m < m1; m += 4) acc += to_f(x[(long)m * ld + n]);
    part[rl][c] = acc;                            // (0 beyond N: the padding columns of the slab row)
  }
  __syncthreads();
  if (tid < W / 4) {                              // row lanes 0 + 1 + 2 + 3, the order of col_sum_multi_kernel
    const int n = bx * W + 4 * tid;
    if (n < L) {
      float4 t;
      t.x = part[0][4 * tid] + part[1][4 * tid] + part[2][4 * tid] + part[3][4 * tid];
      t.y = part[0][4 * tid + 1] + part[1][4 * tid + 1] + part[2][4 * tid + 1] + part[3][4 * tid + 1];
      t.z = part[0][4 * tid + 2] + part[1][4 * tid + 2] + part[2][4 * tid + 2] + part[3][4 * tid + 2];
      t.w = part[0][4 * tid + 3] + part[1][4 * tid + 3] + part[2][4 * tid + 3] + part[3][4 * tid + 3];
      *reinterpret_cast<float4*>(mine + n) = t;
    }
  }
  if (!rs_last_arriver(reinterpret_cast<int*>(ws) + j, b.first[j + 1] - b.first[j], flag)) return;
  float* out = b.out[j];
  rs_finish(slabs, L, b.nchunk[j], lds, [&](int n, float t) { if (n < N) atomicAdd(out + n, t); });
}

// da[c] += sum_r dy[r,c] (x[r,c] - mean_r) / (std_r + eps), db[c] += sum_r dy[r,c] per job, rows of 1 KiB (d = 64 E): each lane owns one
// 16-byte piece of the row.  One workgroup per chunk of 4 * rpw rows; a wave walks its rpw rows four per trip, the loads of all four
// issued before the first is reduced.  Slab row = [da partial (d) | db partial (d)].
template <typename T>
__global__ __launch_bounds__(256) void ln_param_slab_kernel(const RsLnBatch b, float* ws) {
  constexpr int E = 16 / (int)sizeof(T), D = 64 * E;
  __shared__ __attribute__((aligned(16))) float lds[2 * 4 * D + 4];       // [da | db][wave][column], then the flag
  int* flag = reinterpret_cast<int*>(lds + 2 * 4 * D);
  int j = 0;
  while (j + 1 < b.n && (int)blockIdx.x >= b.first[j + 1]) ++j;
  const int chunk = (int)blockIdx.x - b.first[j];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const T* __restrict__ x = (const T*)b.x[j];
  const T* __restrict__ dy = (const T*)b.dy[j];
  const int rows = b.rows[j], rpw = b.rpw[j];
  const long ldx = b.ldx[j], lddy = b.lddy[j];
  const float eps = b.eps[j];
  const int r0 = (int)min((long)rows, (long)(chunk * 4 + w) * rpw), r1 = (int)min((long)rows, (long)r0 + rpw);
  float pa[E], pb[E];
#pragma unroll
  for (int e = 0; e < E; ++e) { pa[e] = 0.f; pb[e] = 0.f; }
  for (int rowb = r0; rowb < r1; rowb += 4) {
    uint4 qx[4], qg[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const long row = min(rowb + rr, r1 - 1);
      qx[rr] = *reinterpret_cast<const uint4*>(x + row * ldx + lane * E);
      qg[rr] = *reinterpret_cast<const uint4*>(dy + row * lddy + lane * E);
    }
    // The row statistics and the term dy (x - mean) / (std + eps) are formed in fp64 and rounded once: x - mean cancels, and with the
    // fp32 mean (good to ~1e-8 absolute) a column that lies near its row's mean gets a term that is wrong in its leading digits, which
    // a sum over a few rows does not average out.  (2 x 64 fp64 operations per lane per row beside a 1 KiB load: not the limit here.)
    float xv[4][E];
    double s[4], q[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const T* xe = reinterpret_cast<const T*>(&qx[rr]);
      s[rr] = 0.0;
#pragma unroll
      for (int e = 0; e < E; ++e) { xv[rr][e] = to_f(xe[e]); s[rr] += (double)xv[rr][e]; }
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) s[rr] = wave_sum_f64(s[rr]) / (double)D;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      q[rr] = 0.0;
#pragma unroll
      for (int e = 0; e < E; ++e) { const double xc = (double)xv[rr][e] - s[rr]; q[rr] += xc * xc; }
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) q[rr] = wave_sum_f64(q[rr]);
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      if (rowb + rr < r1) {                       // (wave-uniform; a trip's surplus rows repeat the last one and are dropped here)
        const double inv = 1.0 / (sqrt(q[rr] / (double)(D - 1)) + (double)eps);
        const T* ge = reinterpret_cast<const T*>(&qg[rr]);
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const float g = to_f(ge[e]);
          pa[e] += (float)((double)g * ((double)xv[rr][e] - s[rr]) * inv);
          pb[e] += g;
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < E; ++e) { lds[(0 * 4 + w) * D + lane * E + e] = pa[e]; lds[(1 * 4 + w) * D + lane * E + e] = pb[e]; }
  __syncthreads();
  const int L = 2 * D;
  float* slabs = ws + RS_HEADER_BYTES / 4 + b.slab[j];
  if (tid < L / 4) {
    const int sel = (4 * tid) / D, c0 = 4 * tid - sel * D;
    const float* r = lds + sel * 4 * D + c0;
    float4 t;
    t.x = r[0] + r[D] + r[2 * D] + r[3 * D];
    t.y = r[1] + r[D + 1] + r[2 * D + 1] + r[3 * D + 1];
    t.z = r[2] + r[D + 2] + r[2 * D + 2] + r[3 * D + 2];
    t.w = r[3] + r[D + 3] + r[2 * D + 3] + r[3 * D + 3];
    *reinterpret_cast<float4*>(slabs + (long)chunk * L + 4 * tid) = t;
  }
  const int nchunk = b.first[j + 1] - b.first[j];
  if (!rs_last_arriver(reinterpret_cast<int*>(ws) + j, nchunk, flag)) return;
  float* da = b.da[j];
  float* db = b.db[j];
  rs_finish(slabs, L, nchunk, lds, [&](int n, float t) { atomicAdd(n < D ? da + n : db + (n - D), t); });
}

inline bool rs_ws_ok(const void* ws, int64_t have, int64_t need) { return ws && ((uintptr_t)ws % 16) == 0 && have >= need; }

}  // namespace

// ---- entry points ------------------------------------------------------------------------------------------------------------------------
extern "C" int64_t bist_col_sum_multi_ws_workspace(const BistColSum* jobs, int32_t njobs) {
  if (!jobs || njobs <= 0) return -1;
  int64_t floats = 0;
  for (int i = 0; i < njobs; ++i) {
    if (jobs[i].M <= 0 || jobs[i].N <= 0) return -1;
    floats += (int64_t)blocks_for(jobs[i].M, rs_colsum_chunk_rows(jobs[i].M)) * rs_pad4(jobs[i].N);
  }
  return RS_HEADER_BYTES + floats * 4;
}

extern "C" int bist_col_sum_multi_ws(const BistColSum* jobs, int32_t njobs, int32_t dtype, void* workspace, int64_t workspace_bytes,
                                     void* stream) {
  BIST_REQUIRE(jobs && njobs > 0, "bist_col_sum_multi_ws: bad argument");
  BIST_REQUIRE(dtype == BIST_BF16 || dtype == BIST_F32, "bist_col_sum_multi_ws: bad dtype %d", dtype);
  for (int i = 0; i < njobs; ++i) {
    const BistColSum& q = jobs[i];
    BIST_REQUIRE(q.x && q.out && q.M > 0 && q.N > 0 && q.ldx >= q.N && q.M < (1L << 31) && q.ldx < (1L << 31), "bist_col_sum_multi_ws: bad job %d", i);
  }
  const int64_t need = bist_col_sum_multi_ws_workspace(jobs, njobs);
  BIST_REQUIRE(need < (1LL << 33), "bist_col_sum_multi_ws: the jobs' slabs exceed 8 GiB; split the call");
  BIST_REQUIRE(rs_ws_ok(workspace, workspace_bytes, need),
               "bist_col_sum_multi_ws: 16-byte aligned workspace of %lld bytes, %lld needed (bist_col_sum_multi_ws_workspace)",
               (long long)workspace_bytes, (long long)need);
  hipStream_t st = (hipStream_t)stream;
  float* ws = (float*)workspace;
  const long esz = dtype == BIST_BF16 ? 2 : 4, piece = 16 / esz;
  long slab = 0;
  for (int base = 0; base < njobs; base += RS_COLSUM_JOBS) {
    RsColSumBatch b;
    b.n = njobs - base < RS_COLSUM_JOBS ? njobs - base : RS_COLSUM_JOBS;
    int total = 0;
    for (int i = 0; i < b.n; ++i) {
      const BistColSum& q = jobs[base + i];
      const bool vec = (q.N % piece == 0) && (q.ldx % piece == 0) && ((uintptr_t)q.x % 16 == 0);
      const long cb = vec ? blocks_for(q.N, (int)(64 * piece)) : blocks_for(q.N, 64);
      const int rpb = rs_colsum_chunk_rows(q.M);
      const int nchunk = (int)blocks_for(q.M, rpb);
      b.vec[i] = vec ? 1 : 0;
      b.x[i] = q.x; b.out[i] = q.out; b.M[i] = (int)q.M; b.N[i] = q.N; b.ld[i] = (int)q.ldx; b.rpb[i] = rpb; b.cb[i] = (int)cb; b.nchunk[i] = nchunk;
      b.slab[i] = (unsigned)slab;
      slab += (long)nchunk * rs_pad4(q.N);
      b.first[i] = total;
      total += (int)(cb * nchunk);
    }
    b.first[b.n] = total;
    if (dtype == BIST_BF16) hipLaunchKernelGGL(col_sum_slab_kernel<bf16_t>, dim3((unsigned)total), dim3(256), 0, st, b, ws);
    else hipLaunchKernelGGL(col_sum_slab_kernel<float>, dim3((unsigned)total), dim3(256), 0, st, b, ws);
    BIST_LAUNCH_CHECK("bist_col_sum_multi_ws");
  }
  return BIST_OK;
}

extern "C" int64_t bist_layernorm_param_grad_multi_ws_workspace(const BistLnGrad* jobs, int32_t njobs, int32_t d) {
  if (!jobs || njobs <= 0 || d <= 1) return -1;
  int64_t floats = 0;
  for (int i = 0; i < njobs; ++i) {
    if (jobs[i].rows <= 0) return -1;
    floats += (int64_t)blocks_for(jobs[i].rows, 4 * rs_ln_wave_rows(jobs[i].rows)) * 2 * d;
  }
  return RS_HEADER_BYTES + floats * 4;
}

extern "C" int bist_layernorm_param_grad_multi_ws(const BistLnGrad* jobs, int32_t njobs, int32_t d, int32_t dtype, void* workspace,
                                                  int64_t workspace_bytes, void* stream) {
  BIST_REQUIRE(jobs && njobs > 0, "bist_layernorm_param_grad_multi_ws: bad argument");
  const long sz = dtype == BIST_BF16 ? 2 : 4;
  BIST_REQUIRE((dtype == BIST_BF16 || dtype == BIST_F32) && d * sz == 1024, "bist_layernorm_param_grad_multi_ws: rows must be 1 KiB (d = 512 bf16 / 256 f32)");
  for (int i = 0; i < njobs; ++i) {
    const BistLnGrad& q = jobs[i];
    BIST_REQUIRE(q.dy && q.x && q.da && q.db && q.rows > 0 && q.rows < (1L << 31) && q.lddy >= d && q.ldx >= d && q.lddy < (1L << 31) && q.ldx < (1L << 31),
                 "bist_layernorm_param_grad_multi_ws: bad job %d", i);
    BIST_REQUIRE((((uintptr_t)q.dy | (uintptr_t)q.x) % 16 == 0) && (q.lddy * sz) % 16 == 0 && (q.ldx * sz) % 16 == 0,
                 "bist_layernorm_param_grad_multi_ws: job %d is not 16-byte aligned", i);
  }
  const int64_t need = bist_layernorm_param_grad_multi_ws_workspace(jobs, njobs, d);
  BIST_REQUIRE(need < (1LL << 33), "bist_layernorm_param_grad_multi_ws: the jobs' slabs exceed 8 GiB; split the call");
  BIST_REQUIRE(rs_ws_ok(workspace, workspace_bytes, need),
               "bist_layernorm_param_grad_multi_ws: 16-byte aligned workspace of %lld bytes, %lld needed (bist_layernorm_param_grad_multi_ws_workspace)",
               (long long)workspace_bytes, (long long)need);
  hipStream_t st = (hipStream_t)stream;
  float* ws = (float*)workspace;
  long slab = 0;
  for (int base = 0; base < njobs; base += RS_LN_JOBS) {
    RsLnBatch b;
    b.n = njobs - base < RS_LN_JOBS ? njobs - base : RS_LN_JOBS;
    b.d = d;
    int total = 0;
    for (int i = 0; i < b.n; ++i) {
      const BistLnGrad& q = jobs[base + i];
      const int rpw = rs_ln_wave_rows(q.rows);
      const int nchunk = (int)blocks_for(q.rows, 4 * rpw);
      b.dy[i] = q.dy; b.x[i] = q.x; b.da[i] = q.da; b.db[i] = q.db;
      b.rows[i] = (int)q.rows; b.lddy[i] = (int)q.lddy; b.ldx[i] = (int)q.ldx; b.rpw[i] = rpw; b.eps[i] = q.eps;
      b.slab[i] = (unsigned)slab;
      slab += (long)nchunk * 2 * d;
      b.first[i] = total;
      total += nchunk;
    }
    b.first[b.n] = total;
    if (dtype == BIST_BF16) hipLaunchKernelGGL(ln_param_slab_kernel<bf16_t>, dim3((unsigned)total), dim3(256), 0, st, b, ws);
    else hipLaunchKernelGGL(ln_param_slab_kernel<float>, dim3((unsigned)total), dim3(256), 0, st, b, ws);
    BIST_LAUNCH_CHECK("bist_layernorm_param_grad_multi_ws");
  }
  return BIST_OK;
}
