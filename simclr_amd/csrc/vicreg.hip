// VICReg loss (Bardes, Ponce, LeCun 2022, "VICReg: Variance-Invariance-Covariance Regularization for Self-Supervised Learning") in its
// Gram form.  Per view v of the gathered global batch, h [N, D]:
//
//   xc     = h - colmean(h),   var_i = sum_a xc_ai^2 / (N - 1),   std_i = sqrt(var_i + eps)
//   Cov    = xc^T xc / (N - 1)                      [D, D] -- NEVER formed (256 MB at D = 8192) and never communicated
//   inv    = (1 / (N D)) sum_{a,i} (h1_ai - h2_ai)^2
//   var    = (1/2) sum_v (1 / D) sum_i max(0, gamma - std_vi)
//   cov    = sum_v (1 / D) sum_{i != j} Cov_v,ij^2
//          = sum_v (1 / D) ((1 / (N-1)^2) sum_ab G_v,ab^2 - sum_i var_vi^2),   G_v = xc_v xc_v^T   [N, N]
//   L      = sim_coeff * inv + std_coeff * var + cov_coeff * cov
// (sum_ij Cov_ij^2 = tr(Cov^T Cov) = tr(xc^T xc xc^T xc) / (N-1)^2 = sum_ab G_ab^2 / (N-1)^2, and Cov_ii = var_i.)
// A replica owns the rows a in [rank n, (rank + 1) n) of each view's Gram matrix against all N columns and reports
//   inv over its own rows (1 / (n D)), the global var, and cov with R / (N-1)^2 * sum_{a local, b} G_ab^2 in place of the full sum;
// the mean over the replicas is L.  Every term but inv depends on h through xc only, and its gradient with respect to xc is a
// combination of rows of xc, whose column sums vanish: the centring has no backward.  With x, o the raw rows of this view and of the
// other one,
//   dL/dh_a = cov_coeff * (4 / ((N-1)^2 D) * sum_b G_ab xc_b - 4 / ((N-1) D) * var o xc_a)
//           - std_coeff * (1 / (2 D)) * [std < gamma] o xc_a / ((N-1) std)
//           + sim_coeff * (2 / (N D)) * (x_a - o_a)
// and only local rows get one (G is symmetric: the factor 4 holds the (a, b) and the (b, a) terms), so nothing is reduce-scattered
// and the backward has no collective.
//
// The minuend and the subtrahend of cov are formed from the SAME stored fp32 centred rows, the subtrahend from their column sums of
// squares in double: the rounding of the centring is common to both.  The sums and the subtraction run in double in a fixed order and
// cov is reported as computed, never clamped.
//
// Matrix products run on the exact fp32-input MFMA (v_mfma_f32_16x16x4_f32) as the staged-k Gram tile of csrc/gram_tile.h: a workgroup
// of 4 waves (2 x 2) owns an E x E output tile, E = 32 W, operands are staged global -> registers -> LDS one k-chunk of 32 ahead, and
// loads past the logical extents read zeros.  Unlike Barlow's Gram launch a workgroup carries ONE view (grid z), so one accumulator
// set, and where the grid of both views' tiles has fewer than 256 workgroups the k range (D) is split into S parts at multiples of
// the 32-wide stage: every part writes its partial tile, and a merge launch adds them in the order ((p0 + p1) + p2) + ... in fp32.
// No atomics anywhere: a second call is bitwise the first, and everything computed from the gathered block alone is identical on
// every replica.
#include "gram_tile.h"

#include <math.h>

#include <algorithm>

namespace {

// Centre: blockIdx.y = view, blockIdx.x = 32-column group.  Pass 1 the mean; pass 2 writes xc = fl32(h - mu) and sums the squares of
// the ROUNDED value it stored, so var is the variance of what the Gram launch reads.  stats[v][0][j] = var, stats[v][1][j] = std.
__global__ __launch_bounds__(256) void vr_center(const float* __restrict__ h_all, int N, int D, double eps, float* __restrict__ xc_all,
                                                 double* __restrict__ stats) {
  __shared__ double sh[32 * gram_tile::kCols];
  __shared__ double res[gram_tile::kCols];
  const int tid = threadIdx.x, q = tid & 7, rg = tid >> 3;
  const int j0 = blockIdx.x * gram_tile::kCols + 4 * q;
  const float* h = h_all + (size_t)blockIdx.y * N * D + j0;
  float* xc = xc_all + (size_t)blockIdx.y * N * D + j0;
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
    const float4 c = make_float4((float)((double)x.x - mu[0]), (float)((double)x.y - mu[1]), (float)((double)x.z - mu[2]),
                                 (float)((double)x.w - mu[3]));
    *(float4*)(xc + (size_t)a * D) = c;
    v[0] += (double)c.x * (double)c.x; v[1] += (double)c.y * (double)c.y;
    v[2] += (double)c.z * (double)c.z; v[3] += (double)c.w * (double)c.w;
  }
  gram_tile::col_reduce(v, sh, res);
  if (tid < gram_tile::kCols) {
    const double var = res[tid] / (double)(N - 1);
    const int j = blockIdx.x * gram_tile::kCols + tid;
    stats[((size_t)blockIdx.y * 2 + 0) * D + j] = var;
    stats[((size_t)blockIdx.y * 2 + 1) * D + j] = sqrt(var + eps);
  }
}

// invpart[blockIdx.x] = sum over the local rows and this workgroup's 32 columns of (h1 - h2)^2, in double.
__global__ __launch_bounds__(256) void vr_inv(const float* __restrict__ h_all, int n, int N, int D, int rank, double* __restrict__ invpart) {
  __shared__ double sh[32 * gram_tile::kCols];
  __shared__ double res[gram_tile::kCols];
  const int tid = threadIdx.x, q = tid & 7, rg = tid >> 3;
  const int j0 = blockIdx.x * gram_tile::kCols + 4 * q;
  const float* h1 = h_all + (size_t)rank * n * D + j0;
  const float* h2 = h_all + ((size_t)N + (size_t)rank * n) * D + j0;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int a = rg; a < n; a += 32) {
    const float4 x = *(const float4*)(h1 + (size_t)a * D), y = *(const float4*)(h2 + (size_t)a * D);
    const double d0 = (double)x.x - (double)y.x, d1 = (double)x.y - (double)y.y, d2 = (double)x.z - (double)y.z,
                 d3 = (double)x.w - (double)y.w;
    v[0] += d0 * d0; v[1] += d1 * d1; v[2] += d2 * d2; v[3] += d3 * d3;
  }
  gram_tile::col_reduce(v, sh, res);
  if (tid == 0) {
    double s = 0.0;
    for (int k = 0; k < gram_tile::kCols; ++k) s += res[k];
    invpart[blockIdx.x] = s;
  }
}

// Gram forward: blockIdx.z = view, blockIdx.x = tile of global columns b (MFMA rows: four consecutive b per lane -> 16-byte stores),
// blockIdx.y = (tile of local rows a) * S + part.  Part p covers k in [p * kchunk, min(D, (p + 1) * kchunk)).
//   SPLIT = false (S = 1): G[v][a][b] goes to the Gram blocks ([2, rows_pad, ldg], padded to the tile; the padding holds the zeros the
//     masked loads give) and the tile's sum of G^2 to sums[v * ntiles + tile].
//   SPLIT = true: the partial tile goes to parts[p][v][a][b] of the same layout; vr_merge adds the parts.
template <int W, bool SPLIT>
__global__ __launch_bounds__(256) void vr_gram(const float* __restrict__ xc_all, int n, int N, int D, int rank, int S, int kchunk,
                                               float* __restrict__ dst, int ldg, int rows_pad, double* __restrict__ sums) {
  __shared__ __attribute__((aligned(16))) float lds[2 * gram_tile::op_floats<32 * W>()];
  __shared__ double wsum[4];
  constexpr int E = 32 * W;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, fl = lane & 15, wm = wave & 1, wn = wave >> 1;
  const int v = blockIdx.z;
  const int ty = SPLIT ? blockIdx.y / S : blockIdx.y, p = SPLIT ? blockIdx.y % S : 0;
  const int m0 = blockIdx.x * E, n0 = ty * E;
  const int kbeg = p * kchunk, kend = min(D, kbeg + kchunk);
  const float* x = xc_all + (size_t)v * N * D;
  f32x4 acc[W][W];
  gram_tile::tile<W, false, false>(lds, x, D, N, true, x + (size_t)rank * n * D, D, n, true, kbeg, kend, m0, n0, acc);
  float* out = dst + ((size_t)p * 2 + v) * rows_pad * ldg;
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < W; ++w) {
    const int a = n0 + 16 * W * wn + 16 * w + fl;
#pragma unroll
    for (int i = 0; i < W; ++i) {
      const int c0 = m0 + 16 * W * wm + 16 * i + 4 * g;
      *(float4*)(out + (size_t)a * ldg + c0) = make_float4(acc[i][w][0], acc[i][w][1], acc[i][w][2], acc[i][w][3]);
      if (!SPLIT) {
#pragma unroll
        for (int r = 0; r < 4; ++r) s += (double)acc[i][w][r] * (double)acc[i][w][r];
      }
    }
  }
  if (!SPLIT) {
    s = wave_sum_d(s);
    if (lane == 0) wsum[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0)
      sums[(size_t)v * gridDim.y * gridDim.x + (size_t)blockIdx.y * gridDim.x + blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
  }
}

// Merge of the S partial Gram blocks: blockIdx.y = view, a workgroup owns 1024 consecutive float4s of that view's [rows_pad, ldg] block
// (thread t the quads t, t + 256, t + 512, t + 768).  gram = ((p0 + p1) + p2) + ... in fp32; sums[v * gridDim.x + blockIdx.x] = the
// sum of the merged G^2 over the workgroup's share, in double.
__global__ __launch_bounds__(256) void vr_merge(const float* __restrict__ parts, int S, size_t view_quads, float* __restrict__ gram,
                                                double* __restrict__ sums) {
  __shared__ double wsum[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int v = blockIdx.y;
  const float4* src = (const float4*)parts + (size_t)v * view_quads;
  float4* dst = (float4*)gram + (size_t)v * view_quads;
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const size_t q = (size_t)blockIdx.x * 1024 + j * 256 + threadIdx.x;
    float4 t = src[q];
    for (int p = 1; p < S; ++p) {
      const float4 u = src[(size_t)p * 2 * view_quads + q];
      t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
    }
    dst[q] = t;
    s += (double)t.x * (double)t.x + (double)t.y * (double)t.y + (double)t.z * (double)t.z + (double)t.w * (double)t.w;
  }
  s = wave_sum_d(s);
  if (lane == 0) wsum[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) sums[(size_t)v * gridDim.x + blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// out = [loss, inv, var, cov] of this replica: one workgroup; every thread sums a strided share, the 256 shares are added in order.
__global__ __launch_bounds__(256) void vr_finish(const double* __restrict__ stats, int D, const double* __restrict__ sums, int nsums,
                                                 const double* __restrict__ invpart, int ninv, double frob_scale, double inv_scale,
                                                 double gamma, double sim_coeff, double std_coeff, double cov_coeff,
                                                 float* __restrict__ out) {
  __shared__ double sh[4][256];
  const int tid = threadIdx.x;
  double hinge = 0.0, v2 = 0.0, fr = 0.0, iv = 0.0;
  for (int v = 0; v < 2; ++v)
    for (int j = tid; j < D; j += 256) {
      const double var = stats[((size_t)v * 2 + 0) * D + j], sd = stats[((size_t)v * 2 + 1) * D + j];
      hinge += fmax(0.0, gamma - sd);
      v2 += var * var;
    }
  for (int t = tid; t < 2 * nsums; t += 256) fr += sums[t];
  for (int t = tid; t < ninv; t += 256) iv += invpart[t];
  sh[0][tid] = hinge; sh[1][tid] = v2; sh[2][tid] = fr; sh[3][tid] = iv;
  __syncthreads();
  if (tid == 0) {
    hinge = v2 = fr = iv = 0.0;
    for (int t = 0; t < 256; ++t) { hinge += sh[0][t]; v2 += sh[1][t]; fr += sh[2][t]; iv += sh[3][t]; }
    const double inv = iv * inv_scale;
    const double var = 0.5 * hinge / (double)D;
    const double cov = (fr * frob_scale - v2) / (double)D;      // both views' sums share the scales; reported as computed
    out[0] = (float)(sim_coeff * inv + std_coeff * var + cov_coeff * cov);
    out[1] = (float)inv;
    out[2] = (float)var;
    out[3] = (float)cov;
  }
}

// Backward GEMM: blockIdx.z = view v, blockIdx.x = tile of the D columns (MFMA rows: 16-byte stores), blockIdx.y = tile of local rows.
//   dh[v][a][j] = c_gram * sum_b G_v[a][b] xc_v[b][j] + (c_var * var_vj + [0 < std_vj < gamma] * c_std / std_vj) * xc_v[rank n + a][j]
//               + c_inv * (h_v[rank n + a][j] - h_{other view}[rank n + a][j])
template <int W>
__global__ __launch_bounds__(256) void vr_bwd_gemm(const float* __restrict__ h_all, const float* __restrict__ xc_all,
                                                   const double* __restrict__ stats, const float* __restrict__ gram, int ldg, int rows_pad,
                                                   int n, int N, int D, int rank, float c_gram, float c_var, float c_std, float c_inv,
                                                   float gamma, float* __restrict__ dh_local) {
  __shared__ __attribute__((aligned(16))) float lds[2 * gram_tile::op_floats<32 * W>()];
  constexpr int E = 32 * W;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, fl = lane & 15, wm = wave & 1, wn = wave >> 1;
  const int v = blockIdx.z;
  const int m0 = blockIdx.x * E, n0 = blockIdx.y * E;
  f32x4 acc[W][W];
  gram_tile::tile<W, true, false>(lds, xc_all + (size_t)v * N * D, D, D, true, gram + (size_t)v * rows_pad * ldg, ldg, n, true, 0, N, m0, n0,
                                  acc);
  const size_t own = ((size_t)v * N + (size_t)rank * n) * D, other = ((size_t)(1 - v) * N + (size_t)rank * n) * D;
  float* out = dh_local + (size_t)v * n * D;
#pragma unroll
  for (int i = 0; i < W; ++i) {
    const int c0 = m0 + 16 * W * wm + 16 * i + 4 * g;
    if (c0 >= D) continue;
    float cj[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float var = (float)stats[((size_t)v * 2 + 0) * D + c0 + r], sd = (float)stats[((size_t)v * 2 + 1) * D + c0 + r];
      cj[r] = c_var * var + ((sd < gamma && sd > 0.f) ? c_std / sd : 0.f);
    }
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const int a = n0 + 16 * W * wn + 16 * w + fl;
      if (a >= n) continue;
      const float4 z = *(const float4*)(xc_all + own + (size_t)a * D + c0);
      const float4 x = *(const float4*)(h_all + own + (size_t)a * D + c0);
      const float4 o = *(const float4*)(h_all + other + (size_t)a * D + c0);
      *(float4*)(out + (size_t)a * D + c0) =
          make_float4(c_gram * acc[i][w][0] + cj[0] * z.x + c_inv * (x.x - o.x), c_gram * acc[i][w][1] + cj[1] * z.y + c_inv * (x.y - o.y),
                      c_gram * acc[i][w][2] + cj[2] * z.z + c_inv * (x.z - o.z), c_gram * acc[i][w][3] + cj[3] * z.w + c_inv * (x.w - o.w));
    }
  }
}

constexpr int kVrFillWgs = 256;      // a grid below this many workgroups (one per compute unit) splits the k range
constexpr int kVrTargetWgs = 1024;   // ... towards this many (four resident workgroups per compute unit)
constexpr int kVrMinStages = 4;      // ... with at least this many 32-wide stages (128 k) per part
constexpr int kVrMaxSplits = 16;

// Tile edge of an M x Nc output computed once per view: 128 where both views' tiles still give the chip >= 256 workgroups, else 64.
int vr_edge(long long M, long long Nc) { return 2LL * ceil_div(M, 128) * ceil_div(Nc, 128) >= kVrFillWgs ? 128 : 64; }
bool vr_dim_ok(int D) { return D >= 64 && D <= 8192 && D % 64 == 0; }
bool vr_shape_ok(int n, int N, int D) { return vr_dim_ok(D) && n >= 1 && N >= 2 && N >= n && N % n == 0; }
bool vr_coeff_ok(float c) { return c >= 0.f && isfinite(c); }      // NaN fails the comparison
int vr_vec_ok(const void* p) { return (uintptr_t)p % 16 == 0 ? 1 : 0; }
// workspace layout: [inv partials: D / 32 doubles | G^2 partials: 2 x nsums doubles | Gram blocks: 2 x rows_pad x ldg floats |
//                    S > 1: partial Gram blocks: S x 2 x rows_pad x ldg floats]
struct VrPlan { int E, rows_pad, ldg, ntiles, S, kchunk, nsums; size_t off_sums, off_gram, off_parts, bytes; };
VrPlan vr_plan(int n, int N, int D) {
  VrPlan p;
  p.E = vr_edge(N, n);
  p.rows_pad = ceil_div(n, p.E) * p.E;
  p.ldg = ceil_div(N, p.E) * p.E;
  p.ntiles = (p.rows_pad / p.E) * (p.ldg / p.E);
  const int wgs = 2 * p.ntiles, stages = D / gram_tile::kKc;
  int S = 1;
  if (wgs < kVrFillWgs) S = std::max(1, std::min(std::min(ceil_div(kVrTargetWgs, wgs), stages / kVrMinStages), kVrMaxSplits));
  const int chunk_stages = ceil_div(stages, S);
  p.S = ceil_div(stages, chunk_stages);          // no empty part; the last one may be shorter
  p.kchunk = chunk_stages * gram_tile::kKc;
  // S = 1: one sum per tile; S > 1: one per merge workgroup (1024 float4s of a view's block)
  p.nsums = p.S == 1 ? p.ntiles : (int)((size_t)p.rows_pad * p.ldg / 4096);
  p.off_sums = (size_t)(D / gram_tile::kCols) * sizeof(double);
  p.off_gram = (p.off_sums + (size_t)2 * p.nsums * sizeof(double) + 255) / 256 * 256;
  p.off_parts = p.off_gram + (size_t)2 * p.rows_pad * p.ldg * sizeof(float);
  p.bytes = p.off_parts + (p.S > 1 ? (size_t)p.S * 2 * p.rows_pad * p.ldg * sizeof(float) : 0);
  return p;
}

}  // namespace

extern "C" {

size_t simclr_vicreg_workspace_bytes(int n, int N, int D) { return vr_shape_ok(n, N, D) ? vr_plan(n, N, D).bytes : 0; }
size_t simclr_vicreg_gram_offset_bytes(int n, int N, int D) { return vr_shape_ok(n, N, D) ? vr_plan(n, N, D).off_gram : 0; }
size_t simclr_vicreg_gram_rows(int n, int N, int D) { return vr_shape_ok(n, N, D) ? (size_t)vr_plan(n, N, D).rows_pad : 0; }
size_t simclr_vicreg_gram_pitch(int n, int N, int D) { return vr_shape_ok(n, N, D) ? (size_t)vr_plan(n, N, D).ldg : 0; }
int simclr_vicreg_k_splits(int n, int N, int D) { return vr_shape_ok(n, N, D) ? vr_plan(n, N, D).S : 0; }
int simclr_vicreg_fwd_workgroups(int n, int N, int D) {
  if (!vr_shape_ok(n, N, D)) return 0;
  const VrPlan p = vr_plan(n, N, D);
  return 2 * p.ntiles * p.S;
}

int simclr_vicreg_center(const float* h_all, int N, int D, float eps, float* xc_all, double* stats, hipStream_t stream) {
  SIMCLR_CHECK_ARG(vr_dim_ok(D), "vicreg_center: the width must be a multiple of 64 in [64, 8192] (got %d)", D);
  SIMCLR_CHECK_ARG(N >= 2, "vicreg_center: the unbiased variance needs N >= 2 (got %d)", N);
  SIMCLR_CHECK_ARG(eps >= 0.f, "vicreg_center: eps must be >= 0");
  SIMCLR_CHECK_ARG(h_all && xc_all && stats, "vicreg_center: null argument");
  SIMCLR_CHECK_ARG(vr_vec_ok(h_all) && vr_vec_ok(xc_all) && vr_vec_ok(stats), "vicreg_center: tensors must be 16-byte aligned");
  hipLaunchKernelGGL(vr_center, dim3(D / gram_tile::kCols, 2), dim3(256), 0, stream, h_all, N, D, (double)eps, xc_all, stats);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

int simclr_vicreg_fwd(const float* h_all, const float* xc_all, const double* stats, int n, int N, int D, int rank, float sim_coeff,
                      float std_coeff, float cov_coeff, float gamma, float* out, void* workspace, hipStream_t stream) {
  SIMCLR_CHECK_ARG(vr_dim_ok(D), "vicreg_fwd: the width must be a multiple of 64 in [64, 8192] (got %d)", D);
  SIMCLR_CHECK_ARG(n >= 1 && N >= 2 && N >= n && N % n == 0, "vicreg_fwd: need N = R*n with n >= 1 and N >= 2 (n=%d N=%d)", n, N);
  SIMCLR_CHECK_ARG(rank >= 0 && rank < N / n, "vicreg_fwd: rank %d out of range", rank);
  SIMCLR_CHECK_ARG(vr_coeff_ok(sim_coeff) && vr_coeff_ok(std_coeff) && vr_coeff_ok(cov_coeff),
                   "vicreg_fwd: the coefficients must be finite and >= 0 (got %g, %g, %g)", sim_coeff, std_coeff, cov_coeff);
  SIMCLR_CHECK_ARG(isfinite(gamma), "vicreg_fwd: gamma must be finite");
  SIMCLR_CHECK_ARG(h_all && xc_all && stats && out && workspace, "vicreg_fwd: null argument");
  SIMCLR_CHECK_ARG(vr_vec_ok(h_all) && vr_vec_ok(xc_all) && vr_vec_ok(stats) && vr_vec_ok(workspace),
                   "vicreg_fwd: tensors must be 16-byte aligned");
  const VrPlan p = vr_plan(n, N, D);
  double* invpart = (double*)workspace;
  double* sums = (double*)((char*)workspace + p.off_sums);
  float* gram = (float*)((char*)workspace + p.off_gram);
  float* parts = (float*)((char*)workspace + p.off_parts);
  hipLaunchKernelGGL(vr_inv, dim3(D / gram_tile::kCols), dim3(256), 0, stream, h_all, n, N, D, rank, invpart);
  SIMCLR_CHECK_LAUNCH();
  if (p.S == 1) {
    dim3 grid(p.ldg / p.E, p.rows_pad / p.E, 2);
    if (p.E == 128)
      hipLaunchKernelGGL((vr_gram<4, false>), grid, dim3(256), 0, stream, xc_all, n, N, D, rank, 1, p.kchunk, gram, p.ldg, p.rows_pad, sums);
    else
      hipLaunchKernelGGL((vr_gram<2, false>), grid, dim3(256), 0, stream, xc_all, n, N, D, rank, 1, p.kchunk, gram, p.ldg, p.rows_pad, sums);
    SIMCLR_CHECK_LAUNCH();
  } else {
    // a split grid has fewer than 256 tiles, so its edge is 64
    dim3 grid(p.ldg / p.E, (p.rows_pad / p.E) * p.S, 2);
    hipLaunchKernelGGL((vr_gram<2, true>), grid, dim3(256), 0, stream, xc_all, n, N, D, rank, p.S, p.kchunk, parts, p.ldg, p.rows_pad,
                       (double*)nullptr);
    SIMCLR_CHECK_LAUNCH();
    const size_t view_quads = (size_t)p.rows_pad * p.ldg / 4;
    hipLaunchKernelGGL(vr_merge, dim3(p.nsums, 2), dim3(256), 0, stream, parts, p.S, view_quads, gram, sums);
    SIMCLR_CHECK_LAUNCH();
  }
  // R / (N-1)^2 with R = N / n; inv over the local rows
  const double frob_scale = (double)(N / n) / ((double)(N - 1) * (double)(N - 1));
  hipLaunchKernelGGL(vr_finish, dim3(1), dim3(256), 0, stream, stats, D, sums, p.nsums, invpart, D / gram_tile::kCols, frob_scale,
                     1.0 / ((double)n * (double)D), (double)gamma, (double)sim_coeff, (double)std_coeff, (double)cov_coeff, out);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

int simclr_vicreg_bwd(const float* h_all, const float* xc_all, const double* stats, int n, int N, int D, int rank, float sim_coeff,
                      float std_coeff, float cov_coeff, float gamma, float grad_scale, void* workspace, float* dh_local,
                      hipStream_t stream) {
  SIMCLR_CHECK_ARG(vr_dim_ok(D), "vicreg_bwd: the width must be a multiple of 64 in [64, 8192] (got %d)", D);
  SIMCLR_CHECK_ARG(n >= 1 && N >= 2 && N >= n && N % n == 0, "vicreg_bwd: need N = R*n with n >= 1 and N >= 2 (n=%d N=%d)", n, N);
  SIMCLR_CHECK_ARG(rank >= 0 && rank < N / n, "vicreg_bwd: rank %d out of range", rank);
  SIMCLR_CHECK_ARG(vr_coeff_ok(sim_coeff) && vr_coeff_ok(std_coeff) && vr_coeff_ok(cov_coeff),
                   "vicreg_bwd: the coefficients must be finite and >= 0 (got %g, %g, %g)", sim_coeff, std_coeff, cov_coeff);
  SIMCLR_CHECK_ARG(isfinite(gamma) && isfinite(grad_scale), "vicreg_bwd: gamma and grad_scale must be finite");
  SIMCLR_CHECK_ARG(h_all && xc_all && stats && workspace && dh_local, "vicreg_bwd: null argument");
  SIMCLR_CHECK_ARG(vr_vec_ok(h_all) && vr_vec_ok(xc_all) && vr_vec_ok(stats) && vr_vec_ok(workspace) && vr_vec_ok(dh_local),
                   "vicreg_bwd: tensors must be 16-byte aligned");
  const VrPlan p = vr_plan(n, N, D);
  const float* gram = (const float*)((const char*)workspace + p.off_gram);
  // the factor R of the returned gradient: R = N / n
  const double s = (double)grad_scale * (double)(N / n), nm1 = (double)(N - 1), d = (double)D;
  const float c_gram = (float)(s * (double)cov_coeff * 4.0 / (nm1 * nm1 * d));
  const float c_var = (float)(-s * (double)cov_coeff * 4.0 / (nm1 * d));
  const float c_std = (float)(-s * (double)std_coeff / (2.0 * d * nm1));
  const float c_inv = (float)(s * (double)sim_coeff * 2.0 / ((double)N * d));
  // one view per workgroup (grid z): the edge rule counts both views' tiles
  const int E = vr_edge(D, n);
  dim3 grid(ceil_div(D, E), ceil_div(n, E), 2);
  if (E == 128)
    hipLaunchKernelGGL(vr_bwd_gemm<4>, grid, dim3(256), 0, stream, h_all, xc_all, stats, gram, p.ldg, p.rows_pad, n, N, D, rank, c_gram,
                       c_var, c_std, c_inv, gamma, dh_local);
  else
    hipLaunchKernelGGL(vr_bwd_gemm<2>, grid, dim3(256), 0, stream, h_all, xc_all, stats, gram, p.ldg, p.rows_pad, n, N, D, rank, c_gram,
                       c_var, c_std, c_inv, gamma, dh_local);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
