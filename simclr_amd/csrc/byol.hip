// BYOL (Grill et al. 2020, Bootstrap Your Own Latent) on a momentum target network, gfx950.
//
// Two bandwidth-bound kernel families, no atomics, fixed summation orders (two runs are bitwise equal):
//   * simclr_ema_multi_tensor: t = t + omt * (o - t) over every (target, online) tensor pair in ONE launch, on the descriptor / chunk
//     tables of simclr_lars_multi_tensor (csrc/lars.hip): one workgroup per 8192-element chunk, 16-byte accesses where both pointers
//     of the chunk allow them.
//   * simclr_byol_fwd / simclr_byol_bwd: loss = (1 / b) sum_r |l2n(q_r) - l2n(t_{(r + b) mod 2b})|^2 and its gradient wrt q.
//     The squared DIFFERENCE is summed, never 2 - 2 cos: near convergence the cosine is 1 - 1e-7 and fp32 would keep no digit of the
//     loss.  All per-row arithmetic is double (two fp64 multiplies, a subtract and an fma per element pair: far below the HBM time of
//     the 8 bytes they read); rows are read once, as 16-byte chunks, and stay in registers between the norm and the difference pass.
#include "common.h"
#include <math.h>

namespace {

constexpr int kChunk = 8192;       // simclr_lars_chunk_elems()
constexpr double kEps = 1e-12;     // tf.math.l2_normalize: x * rsqrt(max(sum x^2, epsilon))

// ---------------------------------------------------------------------------------------------------------------- EMA
// The three roundings are separate (no contraction into an fma), so float32 numpy restates the update bit for bit.  The values are
// pinned in registers between the operations: __fsub_rn / __fmul_rn alone are plain operators to the compiler and contract.
__device__ __forceinline__ float ema_one(float t, float o, float omt) {
  float d = o - t;
  asm volatile("" : "+v"(d));
  float p = omt * d;
  asm volatile("" : "+v"(p));
  return t + p;
}

// table[0*T + k] = target pointer, table[1*T + k] = online pointer, table[2*T + k] = element count; chunks as csrc/lars.hip.
__global__ __launch_bounds__(256) void ema_update(const long long* __restrict__ table, int T, const long long* __restrict__ chunks,
                                                  float omt) {
  const int k = (int)chunks[2 * blockIdx.x];
  const long long off = chunks[2 * blockIdx.x + 1];
  float* t = (float*)table[0 * T + k];
  const float* o = (const float*)table[1 * T + k];
  const long long numel = table[2 * T + k];
  if (off >= numel) return;
  const int n = (int)min((long long)kChunk, numel - off);
  t += off;
  o += off;
  // off is a multiple of 8192 elements: a chunk is 16-byte aligned exactly when its tensor is
  if ((((uintptr_t)t | (uintptr_t)o) & 15) == 0) {
    const int n4 = n >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) {
      f32x4 tv = ((const f32x4*)t)[i];
      const f32x4 ov = ((const f32x4*)o)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) tv[j] = ema_one(tv[j], ov[j], omt);
      ((f32x4*)t)[i] = tv;
    }
    for (int i = (n4 << 2) + threadIdx.x; i < n; i += 256) t[i] = ema_one(t[i], o[i], omt);     // tail of 1..3 elements
  } else {
    for (int i = threadIdx.x; i < n; i += 256) t[i] = ema_one(t[i], o[i], omt);
  }
}

// ---------------------------------------------------------------------------------------------------------------- loss
// A row is D / 4 16-byte chunks, D a multiple of 64 in [64, 8192].  WPR waves share a row (1: D <= 1024, a workgroup holds four rows;
// 4: one row per workgroup); a lane holds up to VPT chunks of the q row and of its partner t row.
// row_stats[r] = {1 / max-clamped norm of q_r, 1 / norm of t_p, s_r = sum_j qhat_rj * 2 (qhat_rj - that_pj), eps flag of q_r};
// row_out[r] = {l_r, qhat_r . that_p}.
template <int WPR> __device__ __forceinline__ void row_sum3(double& a, double& b, double& c, double (*sh)[3]) {
  a = wave_sum_d(a); b = wave_sum_d(b); c = wave_sum_d(c);
  if constexpr (WPR > 1) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();                       // the previous use of sh is over
    if (lane == 0) { sh[wave][0] = a; sh[wave][1] = b; sh[wave][2] = c; }
    __syncthreads();
    a = b = c = 0.0;
#pragma unroll
    for (int w = 0; w < WPR; ++w) { a += sh[w][0]; b += sh[w][1]; c += sh[w][2]; }     // wave order: fixed
  }
}

template <int WPR, int VPT>
__global__ __launch_bounds__(256) void byol_rows(const float* __restrict__ q, const float* __restrict__ t, int b, int D,
                                                 double* __restrict__ row_stats, double* __restrict__ row_out) {
  __shared__ double sh[4][3];
  constexpr int TPR = 64 * WPR;                       // threads per row
  const int rows = 2 * b;
  const int r = blockIdx.x * (4 / WPR) + (WPR == 1 ? (int)(threadIdx.x >> 6) : 0);
  const int tr = WPR == 1 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
  const bool live = r < rows;                         // WPR == 4: always; WPR == 1: the last workgroup may hold idle waves
  const int p = live ? (r + b) % rows : 0;
  const int nv = D >> 2;
  const f32x4* qr = (const f32x4*)(q + (size_t)(live ? r : 0) * D);
  const f32x4* tp = (const f32x4*)(t + (size_t)p * D);
  f32x4 qv[VPT], tv[VPT];
  double sq = 0.0, st = 0.0, unused = 0.0;
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    const int c = tr + i * TPR;
    const bool in = live && c < nv;
    qv[i] = in ? qr[c] : f32x4{0.f, 0.f, 0.f, 0.f};
    tv[i] = in ? tp[c] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) { sq += (double)qv[i][j] * qv[i][j]; st += (double)tv[i][j] * tv[i][j]; }
  }
  row_sum3<WPR>(sq, st, unused, sh);
  const double iq = 1.0 / sqrt(fmax(sq, kEps)), it = 1.0 / sqrt(fmax(st, kEps));
  double l = 0.0, dot = 0.0, s = 0.0;
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {                     // zero-filled chunks add exact zeros
      const double a = (double)qv[i][j] * iq, c = (double)tv[i][j] * it, d = a - c;
      l += d * d;
      dot += a * c;
      s += a * (2.0 * d);
    }
  }
  row_sum3<WPR>(l, dot, s, sh);
  if (live && tr == 0) {
    row_stats[4 * (size_t)r + 0] = iq;
    row_stats[4 * (size_t)r + 1] = it;
    row_stats[4 * (size_t)r + 2] = s;
    row_stats[4 * (size_t)r + 3] = sq < kEps ? 1.0 : 0.0;
    row_out[2 * (size_t)r + 0] = l;
    row_out[2 * (size_t)r + 1] = dot;
  }
}

// out[0] = (1 / b) sum_r l_r, out[1] = (1 / 2b) sum_r cos_r: thread i adds rows i, i + 256, ... in double, then a fixed binary tree.
__global__ __launch_bounds__(256) void byol_finish(const double* __restrict__ row_out, int b, float* __restrict__ out) {
  __shared__ double red[2][256];
  const int rows = 2 * b;
  double a = 0.0, c = 0.0;
  for (int r = threadIdx.x; r < rows; r += 256) { a += row_out[2 * (size_t)r]; c += row_out[2 * (size_t)r + 1]; }
  red[0][threadIdx.x] = a;
  red[1][threadIdx.x] = c;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) { red[0][threadIdx.x] += red[0][threadIdx.x + s]; red[1][threadIdx.x] += red[1][threadIdx.x + s]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = (float)(red[0][0] / (double)b);
    out[1] = (float)(red[1][0] / (double)rows);
  }
}

// dq_r = (grad_scale / b) * dl_r / dq_r.  With g = 2 (qhat - that):  sum q^2 >= eps: (g - qhat (qhat . g)) / |q|;
// sum q^2 < eps: the norm is the constant sqrt(eps) = 1e-6 (the gradient of tf.maximum goes to epsilon), g / 1e-6.
// One pass, one 16-byte chunk per thread: chunk i of the [2b, D / 4] chunk matrix, so narrow rows leave no lane idle.
__global__ __launch_bounds__(256) void byol_grad(const float* __restrict__ q, const float* __restrict__ t, int b, int D,
                                                 const double* __restrict__ row_stats, double scale, float* __restrict__ dq) {
  const int rows = 2 * b, nv = D >> 2;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)rows * nv) return;
  const int r = (int)(i / nv), c = (int)(i - (long long)r * nv);
  const int p = (r + b) % rows;
  const double iq = row_stats[4 * (size_t)r], it = row_stats[4 * (size_t)r + 1];
  const double s = row_stats[4 * (size_t)r + 3] != 0.0 ? 0.0 : row_stats[4 * (size_t)r + 2];
  const f32x4 qv = ((const f32x4*)(q + (size_t)r * D))[c];
  const f32x4 tv = ((const f32x4*)(t + (size_t)p * D))[c];
  const double f = scale * iq;
  f32x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double a = (double)qv[j] * iq, d = a - (double)tv[j] * it;
    o[j] = (float)(f * (2.0 * d - a * s));
  }
  ((f32x4*)(dq + (size_t)r * D))[c] = o;
}

bool byol_args_ok(const void* q, const void* t, int b, int D) {
  return q && t && b >= 1 && b <= (1 << 29) && D >= 64 && D <= 8192 && D % 64 == 0 && (((uintptr_t)q | (uintptr_t)t) & 15) == 0;
}

}  // namespace

extern "C" {

// One launch; table / chunks: device int64, rows of the table = target pointer, online pointer, element count (fp32 tensors, a target
// never aliases its online tensor); chunks[2c] = tensor id, chunks[2c + 1] = element offset, a multiple of simclr_lars_chunk_elems().
int simclr_ema_multi_tensor(const long long* table, int num_tensors, const long long* chunks, int num_chunks, float one_minus_tau,
                            hipStream_t stream) {
  SIMCLR_CHECK_ARG(num_tensors > 0 && num_chunks > 0, "ema: empty tensor list");
  SIMCLR_CHECK_ARG(table && chunks, "ema: null table/chunks");
  SIMCLR_CHECK_ARG(one_minus_tau >= 0.f && one_minus_tau <= 1.f, "ema: 1 - tau = %g is outside [0, 1]", (double)one_minus_tau);
  hipLaunchKernelGGL(ema_update, dim3(num_chunks), dim3(256), 0, stream, table, num_tensors, chunks, one_minus_tau);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

// q [2b, D] (online predictor output), t [2b, D] (target projection), fp32, 16-byte aligned; row r of q pairs with row (r + b) mod 2b
// of t.  out: device float[2] = {loss, cosine}; row_stats: device double[2b * 4] (kept for simclr_byol_bwd); row_out: device
// double[2b * 2] scratch.
int simclr_byol_fwd(const float* q, const float* t, int b, int D, float* out, double* row_stats, double* row_out, hipStream_t stream) {
  SIMCLR_CHECK_ARG(byol_args_ok(q, t, b, D), "byol_fwd: need 16-byte aligned q, t [2b, D] with b >= 1 and D a multiple of 64 in [64, 8192] "
                                             "(got b = %d, D = %d, q = %p, t = %p)", b, D, (const void*)q, (const void*)t);
  SIMCLR_CHECK_ARG(out && row_stats && row_out, "byol_fwd: null out / row_stats / row_out");
  const int rows = 2 * b;
  if (D <= 1024)
    hipLaunchKernelGGL((byol_rows<1, 4>), dim3((rows + 3) / 4), dim3(256), 0, stream, q, t, b, D, row_stats, row_out);
  else
    hipLaunchKernelGGL((byol_rows<4, 8>), dim3(rows), dim3(256), 0, stream, q, t, b, D, row_stats, row_out);
  SIMCLR_CHECK_LAUNCH();
  hipLaunchKernelGGL(byol_finish, dim3(1), dim3(256), 0, stream, row_out, b, out);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

// dq [2b, D] fp32 = (grad_scale / b) * d(sum_r l_r) / dq from the row_stats simclr_byol_fwd wrote for the same q, t.  No gradient for t.
int simclr_byol_bwd(const float* q, const float* t, int b, int D, const double* row_stats, float grad_scale, float* dq,
                    hipStream_t stream) {
  SIMCLR_CHECK_ARG(byol_args_ok(q, t, b, D), "byol_bwd: need 16-byte aligned q, t [2b, D] with b >= 1 and D a multiple of 64 in [64, 8192] "
                                             "(got b = %d, D = %d, q = %p, t = %p)", b, D, (const void*)q, (const void*)t);
  SIMCLR_CHECK_ARG(row_stats && dq && ((uintptr_t)dq & 15) == 0, "byol_bwd: null row_stats / dq, or dq not 16-byte aligned");
  const long long chunks = 2LL * b * (D >> 2);
  SIMCLR_CHECK_ARG((chunks + 255) / 256 <= 0x7fffffffLL, "byol_bwd: %lld chunks exceed one grid", chunks);
  hipLaunchKernelGGL(byol_grad, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, stream, q, t, b, D, row_stats,
                     (double)grad_scale / (double)b, dq);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
