// Barlow Twins loss (Zbontar et al. 2021, "Barlow Twins: Self-Supervised Learning via Redundancy Reduction") in its Gram form.
//
//   zhat   = per-view, per-dimension standardisation of the gathered block over the GLOBAL batch (biased variance, eps inside the root)
//   C      = zhat1^T zhat2 / N                      [D, D] -- NEVER formed (256 MB at D = 8192) and never communicated
//   c_i    = C_ii = (1 / N) sum_a zhat1_ai zhat2_ai [D]
//   on     = sum_i (1 - c_i)^2
//   off    = sum_{i != j} C_ij^2 = (1 / N^2) sum_{a, b} G1_ab G2_ab - sum_i c_i^2,   G1 = zhat1 zhat1^T, G2 = zhat2 zhat2^T  [N, N]
//   L      = loss_scaling * (on + lambda * off)
// (sum_ij C_ij^2 = tr(C^T C) = tr(zhat2^T zhat1 zhat1^T zhat2) / N^2 = sum_ab G1_ab G2_ab / N^2; the diagonal a = b is part of it.)
// A replica owns the rows a in [rank n, (rank + 1) n) of both Gram matrices against all N columns and reports
//   loss_scaling * (on + lambda * (R / N^2 * sum_{a local, b} G1_ab G2_ab - sum_i c_i^2)),
// whose mean over the replicas is L.  With d_i = -2 (1 - c_i) - 2 lambda c_i the gradient through a local row is
//   dL/dzhat1_a = loss_scaling * (lambda * (2 / N^2) * sum_b G2_ab zhat1_b + d o zhat2_a / N)      (view 2: G1, zhat2_b, zhat1_a)
// and only local rows get one, so no reduce-scatter follows; the standardisation backward needs the column sums of g and g o zhat
// over the global batch, which the caller all-reduces between simclr_bt_bwd and simclr_bt_apply.
//
// Matrix products run on the exact fp32-input MFMA (v_mfma_f32_16x16x4_f32) as the staged-k Gram tile of csrc/gram_tile.h, which the
// wide NT-Xent kernels share: a workgroup of 4 waves (2 x 2) owns an E x E output tile, E = 32 W, operands are staged
// global -> registers -> LDS one k-chunk ahead, and loads past the logical extents read zeros.  Every sum over rows, columns or tiles
// runs in a fixed order (the column statistics, the tile sums and the subtraction of sum c_i^2 in double): no atomics, results are
// bitwise repeatable and, for everything computed from the gathered block alone, identical on every replica.
#include "gram_tile.h"

#include <math.h>

namespace {

// Standardise: blockIdx.y = view, blockIdx.x = 32-column group.  Two passes for the statistics (mean, then centred squares), a third
// writes zhat = (h - mu) * rstd.  N = 1 gives var = 0 and zhat = 0.
__global__ __launch_bounds__(256) void bt_standardize(const float* __restrict__ h_all, int N, int D, double eps, float* __restrict__ zhat_all,
                                                      float* __restrict__ rstd) {
  __shared__ double sh[32 * gram_tile::kCols];
  __shared__ double res[gram_tile::kCols];
  const int tid = threadIdx.x, q = tid & 7, rg = tid >> 3;
  const int j0 = blockIdx.x * gram_tile::kCols + 4 * q;
  const float* h = h_all + (size_t)blockIdx.y * N * D + j0;
  float* z = zhat_all + (size_t)blockIdx.y * N * D + j0;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int a = rg; a < N; a += 32) {
    const float4 x = *(const float4*)(h + (size_t)a * D);
    v[0] += (double)x.x; v[1] += (double)x.y; v[2] += (double)x.z; v[3] += (double)x.w;
  }
  gram_tile::col_reduce(v, sh, res);
  double mu[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { mu[k] = res[4 * q + k] / (double)N; v[k] = 0.0; }
  for (int a = rg; a < N; a += 32) {
    const float4 x = *(const float4*)(h + (size_t)a * D);
    const double d0 = (double)x.x - mu[0], d1 = (double)x.y - mu[1], d2 = (double)x.z - mu[2], d3 = (double)x.w - mu[3];
    v[0] += d0 * d0; v[1] += d1 * d1; v[2] += d2 * d2; v[3] += d3 * d3;
  }
  gram_tile::col_reduce(v, sh, res);
  double rs[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) rs[k] = 1.0 / sqrt(res[4 * q + k] / (double)N + eps);
  if (rg == 0) *(float4*)(rstd + (size_t)blockIdx.y * D + j0) = make_float4((float)rs[0], (float)rs[1], (float)rs[2], (float)rs[3]);
  for (int a = rg; a < N; a += 32) {
    const float4 x = *(const float4*)(h + (size_t)a * D);
    *(float4*)(z + (size_t)a * D) = make_float4((float)(((double)x.x - mu[0]) * rs[0]), (float)(((double)x.y - mu[1]) * rs[1]),
                                                (float)(((double)x.z - mu[2]) * rs[2]), (float)(((double)x.w - mu[3]) * rs[3]));
  }
}

// c[j] = (1 / N) sum_a zhat1[a, j] zhat2[a, j] over all N rows: blockIdx.x = 32-column group.
__global__ __launch_bounds__(256) void bt_cdiag(const float* __restrict__ zhat_all, int N, int D, double* __restrict__ c) {
  __shared__ double sh[32 * gram_tile::kCols];
  __shared__ double res[gram_tile::kCols];
  const int tid = threadIdx.x, q = tid & 7, rg = tid >> 3;
  const int j0 = blockIdx.x * gram_tile::kCols + 4 * q;
  const float* z1 = zhat_all + j0;
  const float* z2 = zhat_all + (size_t)N * D + j0;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int a = rg; a < N; a += 32) {
    const float4 x = *(const float4*)(z1 + (size_t)a * D), y = *(const float4*)(z2 + (size_t)a * D);
    v[0] += (double)x.x * (double)y.x; v[1] += (double)x.y * (double)y.y;
    v[2] += (double)x.z * (double)y.z; v[3] += (double)x.w * (double)y.w;
  }
  gram_tile::col_reduce(v, sh, res);
  if (tid < gram_tile::kCols) c[blockIdx.x * gram_tile::kCols + tid] = res[tid] / (double)N;
}

// Gram forward: blockIdx.x = tile of global columns b (MFMA rows: four consecutive b per lane -> 16-byte stores), blockIdx.y = tile
// of local rows a (lane columns).  Both views' tiles run through the same LDS one after the other into two accumulator sets;
// gram[v][a][b] goes to the workspace ([2, rows_pad, ldg], padded to the tile, the padding holds the zeros the masked loads give) and
// the tile's sum of G1 o G2 to tilesum[blockIdx.y * gridDim.x + blockIdx.x].
template <int W>
__global__ __launch_bounds__(256) void bt_gram(const float* __restrict__ zhat_all, int n, int N, int D, int rank, int vec,
                                               float* __restrict__ gram, int ldg, int rows_pad, double* __restrict__ tilesum) {
  __shared__ __attribute__((aligned(16))) float lds[2 * gram_tile::op_floats<32 * W>()];
  __shared__ double wsum[4];
  constexpr int E = 32 * W;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, fl = lane & 15, wm = wave & 1, wn = wave >> 1;
  const int m0 = blockIdx.x * E, n0 = blockIdx.y * E;
  f32x4 acc1[W][W], acc2[W][W];
  gram_tile::tile<W, false, false>(lds, zhat_all, D, N, vec, zhat_all + (size_t)rank * n * D, D, n, vec, 0, D, m0, n0, acc1);
  gram_tile::tile<W, false, false>(lds, zhat_all + (size_t)N * D, D, N, vec, zhat_all + ((size_t)N + (size_t)rank * n) * D, D, n, vec, 0, D,
                                   m0, n0, acc2);
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < W; ++w) {
    const int a = n0 + 16 * W * wn + 16 * w + fl;
#pragma unroll
    for (int i = 0; i < W; ++i) {
      const int c0 = m0 + 16 * W * wm + 16 * i + 4 * g;
      *(float4*)(gram + (size_t)a * ldg + c0) = make_float4(acc1[i][w][0], acc1[i][w][1], acc1[i][w][2], acc1[i][w][3]);
      *(float4*)(gram + ((size_t)rows_pad + a) * ldg + c0) = make_float4(acc2[i][w][0], acc2[i][w][1], acc2[i][w][2], acc2[i][w][3]);
#pragma unroll
      for (int r = 0; r < 4; ++r) s += (double)acc1[i][w][r] * (double)acc2[i][w][r];
    }
  }
  s = wave_sum_d(s);
  if (lane == 0) wsum[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) tilesum[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// out = [loss, on_diag, off_diag] of this replica: one workgroup; every thread sums a strided share, the 256 shares are added in order.
__global__ __launch_bounds__(256) void bt_finish(const double* __restrict__ c, int D, const double* __restrict__ tilesum, int ntiles,
                                                 double frob_scale, double lambda, double loss_scaling, float* __restrict__ out) {
  __shared__ double sh[3][256];
  const int tid = threadIdx.x;
  double on = 0.0, c2 = 0.0, fr = 0.0;
  for (int j = tid; j < D; j += 256) {
    const double cj = c[j];
    on += (1.0 - cj) * (1.0 - cj);
    c2 += cj * cj;
  }
  for (int t = tid; t < ntiles; t += 256) fr += tilesum[t];
  sh[0][tid] = on; sh[1][tid] = c2; sh[2][tid] = fr;
  __syncthreads();
  if (tid == 0) {
    on = c2 = fr = 0.0;
    for (int t = 0; t < 256; ++t) { on += sh[0][t]; c2 += sh[1][t]; fr += sh[2][t]; }
    const double off = fr * frob_scale - c2;
    out[0] = (float)(loss_scaling * (on + lambda * off));
    out[1] = (float)on;
    out[2] = (float)off;
  }
}

// Backward GEMM: blockIdx.z = view v, blockIdx.x = tile of the D columns (MFMA rows: 16-byte stores), blockIdx.y = tile of local rows.
//   g[v][a][j] = alpha * sum_b G_{other view}[a][b] zhat_v[b][j] + beta * d_j * zhat_{other view}[rank n + a][j]
template <int W>
__global__ __launch_bounds__(256) void bt_bwd_gemm(const float* __restrict__ zhat_all, const float* __restrict__ gram, int ldg, int rows_pad,
                                                   const double* __restrict__ c, int n, int N, int D, int rank, int vec, float alpha,
                                                   float beta, float lambda, float* __restrict__ g_local) {
  __shared__ __attribute__((aligned(16))) float lds[2 * gram_tile::op_floats<32 * W>()];
  constexpr int E = 32 * W;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, fl = lane & 15, wm = wave & 1, wn = wave >> 1;
  const int v = blockIdx.z;
  const int m0 = blockIdx.x * E, n0 = blockIdx.y * E;
  f32x4 acc[W][W];
  gram_tile::tile<W, true, false>(lds, zhat_all + (size_t)v * N * D, D, D, vec, gram + (size_t)(1 - v) * rows_pad * ldg, ldg, n, true, 0, N,
                                  m0, n0, acc);
  const float* zo = zhat_all + ((size_t)(1 - v) * N + (size_t)rank * n) * D;
  float* out = g_local + (size_t)v * n * D;
#pragma unroll
  for (int i = 0; i < W; ++i) {
    const int c0 = m0 + 16 * W * wm + 16 * i + 4 * g;
    if (c0 >= D) continue;
    float dj[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float cj = (float)c[c0 + r];
      dj[r] = beta * (-2.f * (1.f - cj) - 2.f * lambda * cj);
    }
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const int a = n0 + 16 * W * wn + 16 * w + fl;
      if (a >= n) continue;
      const float4 z = *(const float4*)(zo + (size_t)a * D + c0);
      *(float4*)(out + (size_t)a * D + c0) = make_float4(alpha * acc[i][w][0] + dj[0] * z.x, alpha * acc[i][w][1] + dj[1] * z.y,
                                                         alpha * acc[i][w][2] + dj[2] * z.z, alpha * acc[i][w][3] + dj[3] * z.w);
    }
  }
}

// colsums[v][0][j] = sum_{a local} g[v][a][j], colsums[v][1][j] = sum_{a local} g[v][a][j] zhat_v[rank n + a][j]
__global__ __launch_bounds__(256) void bt_colsums(const float* __restrict__ g_local, const float* __restrict__ zhat_all, int n, int N, int D,
                                                  int rank, double* __restrict__ colsums) {
  __shared__ double sh[32 * gram_tile::kCols];
  __shared__ double res[gram_tile::kCols];
  const int tid = threadIdx.x, q = tid & 7, rg = tid >> 3;
  const int v = blockIdx.y;
  const int j0 = blockIdx.x * gram_tile::kCols + 4 * q;
  const float* gp = g_local + (size_t)v * n * D + j0;
  const float* zp = zhat_all + ((size_t)v * N + (size_t)rank * n) * D + j0;
  double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
  for (int a = rg; a < n; a += 32) {
    const float4 x = *(const float4*)(gp + (size_t)a * D), z = *(const float4*)(zp + (size_t)a * D);
    s1[0] += (double)x.x; s1[1] += (double)x.y; s1[2] += (double)x.z; s1[3] += (double)x.w;
    s2[0] += (double)x.x * (double)z.x; s2[1] += (double)x.y * (double)z.y;
    s2[2] += (double)x.z * (double)z.z; s2[3] += (double)x.w * (double)z.w;
  }
  gram_tile::col_reduce(s1, sh, res);
  if (tid < gram_tile::kCols) colsums[((size_t)v * 2 + 0) * D + blockIdx.x * gram_tile::kCols + tid] = res[tid];
  gram_tile::col_reduce(s2, sh, res);
  if (tid < gram_tile::kCols) colsums[((size_t)v * 2 + 1) * D + blockIdx.x * gram_tile::kCols + tid] = res[tid];
}

// Standardisation backward: dh[v][a][j] = (g - s1_j / N - zhat_v[rank n + a][j] * s2_j / N) * rstd[v][j]; one float4 per thread.
__global__ __launch_bounds__(256) void bt_apply(const float* __restrict__ g_local, const float* __restrict__ zhat_all,
                                                const float* __restrict__ rstd, const double* __restrict__ colsums, int n, int N, int D,
                                                int rank, float* __restrict__ dh) {
  const int dq = D / 4;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)2 * n * dq) return;
  const int j = (int)(idx % dq) * 4;
  const long long row = idx / dq;
  const int v = (int)(row / n), a = (int)(row % n);
  const float4 x = *(const float4*)(g_local + (size_t)row * D + j);
  const float4 z = *(const float4*)(zhat_all + ((size_t)v * N + (size_t)rank * n + a) * D + j);
  const float4 rs = *(const float4*)(rstd + (size_t)v * D + j);
  const double* s1 = colsums + ((size_t)v * 2 + 0) * D + j;
  const double* s2 = colsums + ((size_t)v * 2 + 1) * D + j;
  const double inv = 1.0 / (double)N;
  float m1[4], m2[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { m1[k] = (float)(s1[k] * inv); m2[k] = (float)(s2[k] * inv); }
  *(float4*)(dh + (size_t)row * D + j) = make_float4((x.x - m1[0] - z.x * m2[0]) * rs.x, (x.y - m1[1] - z.y * m2[1]) * rs.y,
                                                     (x.z - m1[2] - z.z * m2[2]) * rs.z, (x.w - m1[3] - z.w * m2[3]) * rs.w);
}

// Tile edge of an M x Nc output: 128 where that still gives the chip >= 256 workgroups, else 64 (the rule of the wide NT-Xent GEMMs).
int bt_edge(long long M, long long Nc) { return (long long)ceil_div(M, 128) * ceil_div(Nc, 128) >= 256 ? 128 : 64; }
bool bt_dim_ok(int D) { return D >= 64 && D <= 8192 && D % 64 == 0; }
bool bt_shape_ok(int n, int N, int D) { return bt_dim_ok(D) && n >= 1 && N >= n && N % n == 0; }
// workspace layout: [c: D doubles | tile sums: doubles | Gram blocks: 2 x rows_pad x ldg floats]
struct BtPlan { int E, rows_pad, ldg, ntiles; size_t off_tiles, off_gram, bytes; };
BtPlan bt_plan(int n, int N, int D) {
  BtPlan p;
  p.E = bt_edge(N, n);
  p.rows_pad = ceil_div(n, p.E) * p.E;
  p.ldg = ceil_div(N, p.E) * p.E;
  p.ntiles = (p.rows_pad / p.E) * (p.ldg / p.E);
  p.off_tiles = (size_t)D * sizeof(double);
  p.off_gram = (p.off_tiles + (size_t)p.ntiles * sizeof(double) + 255) / 256 * 256;
  p.bytes = p.off_gram + (size_t)2 * p.rows_pad * p.ldg * sizeof(float);
  return p;
}
int bt_vec_ok(const void* p) { return (uintptr_t)p % 16 == 0 ? 1 : 0; }

}  // namespace

extern "C" {

size_t simclr_bt_workspace_bytes(int n, int N, int D) { return bt_shape_ok(n, N, D) ? bt_plan(n, N, D).bytes : 0; }
size_t simclr_bt_gram_offset_bytes(int n, int N, int D) { return bt_shape_ok(n, N, D) ? bt_plan(n, N, D).off_gram : 0; }
size_t simclr_bt_gram_rows(int n, int N, int D) { return bt_shape_ok(n, N, D) ? (size_t)bt_plan(n, N, D).rows_pad : 0; }
size_t simclr_bt_gram_pitch(int n, int N, int D) { return bt_shape_ok(n, N, D) ? (size_t)bt_plan(n, N, D).ldg : 0; }

int simclr_bt_standardize(const float* h_all, int N, int D, float eps, float* zhat_all, float* rstd, hipStream_t stream) {
  SIMCLR_CHECK_ARG(bt_dim_ok(D), "bt_standardize: the width must be a multiple of 64 in [64, 8192] (got %d)", D);
  SIMCLR_CHECK_ARG(N >= 1, "bt_standardize: need N >= 1 (got %d)", N);
  SIMCLR_CHECK_ARG(eps >= 0.f, "bt_standardize: eps must be >= 0");
  SIMCLR_CHECK_ARG(h_all && zhat_all && rstd, "bt_standardize: null argument");
  SIMCLR_CHECK_ARG(bt_vec_ok(h_all) && bt_vec_ok(zhat_all) && bt_vec_ok(rstd), "bt_standardize: tensors must be 16-byte aligned");
  hipLaunchKernelGGL(bt_standardize, dim3(D / gram_tile::kCols, 2), dim3(256), 0, stream, h_all, N, D, (double)eps, zhat_all, rstd);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

int simclr_bt_fwd(const float* zhat_all, int n, int N, int D, int rank, float lambda_weight, float loss_scaling, float* out,
                  void* workspace, hipStream_t stream) {
  SIMCLR_CHECK_ARG(bt_dim_ok(D), "bt_fwd: the width must be a multiple of 64 in [64, 8192] (got %d)", D);
  SIMCLR_CHECK_ARG(n >= 1 && N >= n && N % n == 0, "bt_fwd: need N = R*n (n=%d N=%d)", n, N);
  SIMCLR_CHECK_ARG(rank >= 0 && rank < N / n, "bt_fwd: rank %d out of range", rank);
  SIMCLR_CHECK_ARG(zhat_all && out && workspace, "bt_fwd: null argument");
  SIMCLR_CHECK_ARG(bt_vec_ok(zhat_all) && (uintptr_t)workspace % 16 == 0, "bt_fwd: tensors must be 16-byte aligned");
  const BtPlan p = bt_plan(n, N, D);
  double* c = (double*)workspace;
  double* tilesum = (double*)((char*)workspace + p.off_tiles);
  float* gram = (float*)((char*)workspace + p.off_gram);
  dim3 grid(p.ldg / p.E, p.rows_pad / p.E);
  if (p.E == 128)
    hipLaunchKernelGGL(bt_gram<4>, grid, dim3(256), 0, stream, zhat_all, n, N, D, rank, 1, gram, p.ldg, p.rows_pad, tilesum);
  else
    hipLaunchKernelGGL(bt_gram<2>, grid, dim3(256), 0, stream, zhat_all, n, N, D, rank, 1, gram, p.ldg, p.rows_pad, tilesum);
  SIMCLR_CHECK_LAUNCH();
  hipLaunchKernelGGL(bt_cdiag, dim3(D / gram_tile::kCols), dim3(256), 0, stream, zhat_all, N, D, c);
  SIMCLR_CHECK_LAUNCH();
  // R / N^2 = 1 / (n N)
  hipLaunchKernelGGL(bt_finish, dim3(1), dim3(256), 0, stream, c, D, tilesum, p.ntiles, 1.0 / ((double)n * (double)N), (double)lambda_weight,
                     (double)loss_scaling, out);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

int simclr_bt_bwd(const float* zhat_all, int n, int N, int D, int rank, float lambda_weight, float loss_scaling, float grad_scale,
                  void* workspace, float* g_local, double* colsums, hipStream_t stream) {
  SIMCLR_CHECK_ARG(bt_dim_ok(D), "bt_bwd: the width must be a multiple of 64 in [64, 8192] (got %d)", D);
  SIMCLR_CHECK_ARG(n >= 1 && N >= n && N % n == 0, "bt_bwd: need N = R*n (n=%d N=%d)", n, N);
  SIMCLR_CHECK_ARG(rank >= 0 && rank < N / n, "bt_bwd: rank %d out of range", rank);
  SIMCLR_CHECK_ARG(zhat_all && workspace && g_local && colsums, "bt_bwd: null argument");
  SIMCLR_CHECK_ARG(bt_vec_ok(zhat_all) && bt_vec_ok(g_local) && (uintptr_t)workspace % 16 == 0, "bt_bwd: tensors must be 16-byte aligned");
  const BtPlan p = bt_plan(n, N, D);
  const double* c = (const double*)workspace;
  const float* gram = (const float*)((const char*)workspace + p.off_gram);
  // the factor R of the returned gradient: R = N / n
  const double scale = (double)loss_scaling * (double)grad_scale * (double)(N / n);
  const float alpha = (float)(scale * (double)lambda_weight * 2.0 / ((double)N * (double)N));
  const float beta = (float)(scale / (double)N);
  const int E = bt_edge(D, n);
  dim3 grid(ceil_div(D, E), ceil_div(n, E), 2);
  if (E == 128)
    hipLaunchKernelGGL(bt_bwd_gemm<4>, grid, dim3(256), 0, stream, zhat_all, gram, p.ldg, p.rows_pad, c, n, N, D, rank, 1, alpha, beta,
                       lambda_weight, g_local);
  else
    hipLaunchKernelGGL(bt_bwd_gemm<2>, grid, dim3(256), 0, stream, zhat_all, gram, p.ldg, p.rows_pad, c, n, N, D, rank, 1, alpha, beta,
                       lambda_weight, g_local);
  SIMCLR_CHECK_LAUNCH();
  hipLaunchKernelGGL(bt_colsums, dim3(D / gram_tile::kCols, 2), dim3(256), 0, stream, g_local, zhat_all, n, N, D, rank, colsums);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

int simclr_bt_apply(const float* g_local, const float* zhat_all, const float* rstd, const double* colsums, int n, int N, int D, int rank,
                    float* dh, hipStream_t stream) {
  SIMCLR_CHECK_ARG(bt_dim_ok(D), "bt_apply: the width must be a multiple of 64 in [64, 8192] (got %d)", D);
  SIMCLR_CHECK_ARG(n >= 1 && N >= n && N % n == 0, "bt_apply: need N = R*n (n=%d N=%d)", n, N);
  SIMCLR_CHECK_ARG(rank >= 0 && rank < N / n, "bt_apply: rank %d out of range", rank);
  SIMCLR_CHECK_ARG(g_local && zhat_all && rstd && colsums && dh, "bt_apply: null argument");
  SIMCLR_CHECK_ARG(bt_vec_ok(g_local) && bt_vec_ok(zhat_all) && bt_vec_ok(rstd) && bt_vec_ok(colsums) && bt_vec_ok(dh),
                   "bt_apply: tensors must be 16-byte aligned");
  const long long quads = (long long)2 * n * (D / 4);
  hipLaunchKernelGGL(bt_apply, dim3(ceil_div(quads, 256)), dim3(256), 0, stream, g_local, zhat_all, rstd, colsums, n, N, D, rank, dh);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
