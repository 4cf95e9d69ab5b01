// Eigen-spectrum evaluation of the frozen encoder (simclr_amd/spectrum.py): the column sums and the centred covariance of a slab of
// unnormalised features.  x [n, D] fp32 = a slab of rows, weights [n] fp32; a row is COUNTED when its weight is > 0 and not at all
// otherwise -- the kernels select, they never multiply, so a weight-0 row is not even read (a NaN or inf in it changes no output bit).
//   sums [D + 1] double (+)= {sum_counted x_n, number of counted rows}
//   cov [D, D]   double (+)= sum_counted (x_n - mu32)(x_n - mu32)^T,   mu32 [D] fp32 = the caller's rounded mean
// The host subtracts S delta delta^T, delta = mu - mu32, in float64 afterwards (sum (x - mu32) = S delta): centring with the rounded
// mean costs nothing, while "accumulate X^T X, subtract n mu mu^T" loses the covariance of features whose means are as large as their
// standard deviations.
//
// Column sums, two launches:
//   sp_colsum   blockIdx.x = 32-column group, blockIdx.y = row part of kSpSumRows rows: the walk of gram_tile::col_reduce (thread (q, rg)
//               adds rows rg, rg + 32, ... of a column quad in double, the 32 row groups in the order 0 .. 31); group 0 also counts
//   sp_sumfin   one thread per column: the row parts in ascending order, then the add to what sums holds
// Covariance, three launches:
//   sp_center   xc = counted ? fl32(x - mu32) : 0 into a slab-sized fp32 scratch in the workspace (as rp_center of csrc/repr.hip): the
//               product then runs on gram_tile::tile as it stands, with both operands in their global orientation (KR: k = the row)
//   sp_cov      blockIdx.x = tile pair (ti <= tj) of the upper triangle, blockIdx.y = row part: one E x E tile of xc^T xc over the part's
//               rows on the exact fp32-input MFMA, accumulated in the MFMA's fp32 and stored in the accumulators' own layout (one
//               float4 per thread and 16x16 block: fully coalesced)
//   sp_covfin   blockIdx.x = tile pair, blockIdx.y = 16x16 block slot: a thread adds its float4 over the row parts in ascending order in
//               double and writes the element and its mirror FROM THE SAME REGISTER: cov[a, b] and cov[b, a] are the same bits.  A
//               16-lane group writes 16 consecutive doubles (one 128-byte line) in the tile; in the mirror the 4 lane groups' double4s
//               of one row are again 128 consecutive bytes: no LDS transpose, no partly written line.  In a diagonal tile only the
//               elements a <= b are taken.
// D is a multiple of the tile edge (the 128-wide tile is chosen only for D a multiple of 128), so no tile is ragged in D; the rows past
// a part's end are read as zeros by the tile.  No atomics, every order fixed: repeat calls are bitwise equal.
#include "gram_tile.h"

namespace {

constexpr int kSpSumRows = 2048;      // rows per workgroup of sp_colsum
constexpr int kSpMaxPartRows = 8192;  // longest fp32 accumulation of sp_cov
constexpr int kSpWorkgroups = 256;    // workgroups that leave no CU idle

__global__ __launch_bounds__(256) void sp_colsum(const float* __restrict__ x, const float* __restrict__ weights, int n, int D,
                                                 double* __restrict__ part) {
  __shared__ double sh[32 * gram_tile::kCols];
  __shared__ double res[gram_tile::kCols];
  const int tid = threadIdx.x, q = tid & 7, rg = tid >> 3;
  const int j0 = blockIdx.x * gram_tile::kCols + 4 * q;
  const int rbeg = blockIdx.y * kSpSumRows, rend = min(n, rbeg + kSpSumRows);
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  double cnt = 0.0;
  for (int a = rbeg + rg; a < rend; a += 32) {
    if (weights[a] > 0.f) {                       // a NaN weight fails the comparison; an uncounted row is not read
      const float4 t = *(const float4*)(x + (size_t)a * D + j0);
      v[0] += (double)t.x; v[1] += (double)t.y; v[2] += (double)t.z; v[3] += (double)t.w;
      cnt += 1.0;
    }
  }
  double* out = part + (size_t)blockIdx.y * (D + 1);
  gram_tile::col_reduce(v, sh, res);
  if (tid < gram_tile::kCols) out[blockIdx.x * gram_tile::kCols + tid] = res[tid];
  if (blockIdx.x == 0) {
    const double c[4] = {q == 0 ? cnt : 0.0, 0.0, 0.0, 0.0};
    gram_tile::col_reduce(c, sh, res);
    if (tid == 0) out[D] = res[0];
  }
}

__global__ __launch_bounds__(256) void sp_sumfin(const double* __restrict__ part, int nparts, int D, double* __restrict__ sums,
                                                 int accumulate) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j > D) return;
  double s = 0.0;
  for (int p = 0; p < nparts; ++p) s += part[(size_t)p * (D + 1) + j];
  sums[j] = accumulate ? sums[j] + s : s;
}

// One float4 (4 consecutive columns of one row) per thread.
__global__ __launch_bounds__(256) void sp_center(const float* __restrict__ x, const float* __restrict__ weights,
                                                 const float* __restrict__ mu32, int n, int D, float* __restrict__ xc) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const int q = D / 4;
  if (idx >= (long long)n * q) return;
  const int row = (int)(idx / q), j = (int)(idx % q) * 4;
  float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
  if (weights[row] > 0.f) {
    const float4 t = *(const float4*)(x + (size_t)row * D + j);
    const float4 m = *(const float4*)(mu32 + j);
    c = make_float4(t.x - m.x, t.y - m.y, t.z - m.z, t.w - m.w);
  }
  *(float4*)(xc + (size_t)row * D + j) = c;
}

// pair p of the upper triangle of T x T tiles, row by row: (0,0) (0,1) .. (0,T-1) (1,1) ..
__device__ __forceinline__ void sp_pair(int p, int T, int& ti, int& tj) {
  ti = 0;
  while (p >= T - ti) { p -= T - ti; ++ti; }
  tj = ti + p;
}

template <int W>
__global__ __launch_bounds__(256) void sp_cov(const float* __restrict__ xc, int n, int D, int part_rows, float4* __restrict__ part) {
  constexpr int E = 32 * W;
  __shared__ __attribute__((aligned(16))) float lds[2 * gram_tile::op_floats<E>()];
  int ti, tj;
  sp_pair(blockIdx.x, D / E, ti, tj);
  const int kbeg = blockIdx.y * part_rows, kend = min(n, kbeg + part_rows);
  f32x4 acc[W][W];
  gram_tile::tile<W, true, true>(lds, xc, D, D, true, xc, D, D, true, kbeg, kend, ti * E, tj * E, acc);
  float4* out = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (W * W * 256) + threadIdx.x;
#pragma unroll
  for (int i = 0; i < W; ++i)
#pragma unroll
    for (int w = 0; w < W; ++w) out[(i * W + w) * 256] = make_float4(acc[i][w][0], acc[i][w][1], acc[i][w][2], acc[i][w][3]);
}

template <int W>
__global__ __launch_bounds__(256) void sp_covfin(const float4* __restrict__ part, int nparts, int D, double* __restrict__ cov,
                                                 int accumulate) {
  constexpr int E = 32 * W;
  int ti, tj;
  sp_pair(blockIdx.x, D / E, ti, tj);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, fl = lane & 15, wm = wave & 1, wn = wave >> 1;
  const int i = blockIdx.y / W, w = blockIdx.y % W;
  const size_t stride = (size_t)gridDim.x * (W * W * 256);
  const float4* src = part + (size_t)blockIdx.x * (W * W * 256) + blockIdx.y * 256 + tid;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int p = 0; p < nparts; ++p) {
    const float4 t = src[(size_t)p * stride];
    s[0] += (double)t.x; s[1] += (double)t.y; s[2] += (double)t.z; s[3] += (double)t.w;
  }
  const int a0 = ti * E + 16 * W * wm + 16 * i + 4 * g;      // rows a0 .. a0 + 3
  const int b = tj * E + 16 * W * wn + 16 * w + fl;          // column
  const bool diag = ti == tj;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int a = a0 + r;
    if (diag && a > b) continue;
    double* up = cov + (size_t)a * D + b;
    const double v = accumulate ? *up + s[r] : s[r];      // cov is symmetric on entry: the mirror holds the same bits
    *up = v;
    s[r] = v;
  }
  double* lo = cov + (size_t)b * D + a0;
  if (!diag) {
    *(double2*)lo = make_double2(s[0], s[1]);
    *(double2*)(lo + 2) = make_double2(s[2], s[3]);
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (a0 + r < b) lo[r] = s[r];
  }
}

bool sp_dim_ok(int D) { return D >= 64 && D <= 8192 && D % 64 == 0; }
bool sp_shape_ok(int n, int D) { return sp_dim_ok(D) && n >= 1 && n <= 65536; }
int sp_pairs(int D, int e) { const int T = D / e; return T * (T + 1) / 2; }
// Tile edge: 128 where D is a multiple of 128 and the 128-wide triangle, cut into row parts of at least one 32-row stage, still gives
// the chip kSpWorkgroups workgroups; else 64
int sp_edge(int n, int D) {
  return D % 128 == 0 && (long long)sp_pairs(D, 128) * ceil_div(n, gram_tile::kKc) >= kSpWorkgroups ? 128 : 64;
}
// workspace: [xc: n D floats (its head doubles as the column-sum parts: ceil(n / kSpSumRows) x (D + 1) doubles) | part: parts x pairs x E x E floats]
struct SpPlan {
  int e, pairs, part_rows, parts, sum_parts;
  size_t off_part, bytes;
};
SpPlan sp_plan(int n, int D) {
  SpPlan p;
  p.e = sp_edge(n, D);
  p.pairs = sp_pairs(D, p.e);
  // parts: enough that pairs x parts workgroups leave no CU idle, and no part longer than kSpMaxPartRows; a multiple of the stage each
  const int want = ceil_div(kSpWorkgroups, p.pairs) > ceil_div(n, kSpMaxPartRows) ? ceil_div(kSpWorkgroups, p.pairs) : ceil_div(n, kSpMaxPartRows);
  p.part_rows = ceil_div(n, want) / gram_tile::kKc * gram_tile::kKc;      // rounded DOWN to whole stages: never fewer parts than wanted
  if (p.part_rows < gram_tile::kKc) p.part_rows = gram_tile::kKc;
  p.parts = ceil_div(n, p.part_rows);
  p.sum_parts = ceil_div(n, kSpSumRows);
  const size_t xc = (size_t)n * D * sizeof(float), sums = (size_t)p.sum_parts * (D + 1) * sizeof(double);
  p.off_part = ((xc > sums ? xc : sums) + 255) / 256 * 256;
  p.bytes = p.off_part + (size_t)p.parts * p.pairs * p.e * p.e * sizeof(float);
  return p;
}
bool sp_al16(const void* p) { return (uintptr_t)p % 16 == 0; }

}  // namespace

extern "C" {

int simclr_spectrum_dim_ok(int D) { return sp_dim_ok(D) ? 1 : 0; }
size_t simclr_spectrum_workspace_bytes(int n, int D) { return sp_shape_ok(n, D) ? sp_plan(n, D).bytes : 0; }
// the column sums use the head of the workspace alone: a stand-alone call needs no more than its row parts
size_t simclr_spectrum_colsum_workspace_bytes(int n, int D) {
  return sp_shape_ok(n, D) ? ((size_t)sp_plan(n, D).sum_parts * (D + 1) * sizeof(double) + 15) / 16 * 16 : 0;
}
int simclr_spectrum_tile_edge(int n, int D) { return sp_shape_ok(n, D) ? sp_plan(n, D).e : 0; }
int simclr_spectrum_row_parts(int n, int D) { return sp_shape_ok(n, D) ? sp_plan(n, D).parts : 0; }

#define SP_CHECK_SHAPE(name)                                                                                                    \
  SIMCLR_CHECK_ARG(sp_dim_ok(D), name ": the width must be a multiple of 64 in [64, 8192] (got %d)", D);                        \
  SIMCLR_CHECK_ARG(n >= 1 && n <= 65536, name ": need 1 <= n <= 65536 rows per call (got %d)", n)

int simclr_spectrum_colsum(const float* x, const float* weights, int n, int D, double* sums, int accumulate, void* workspace,
                           hipStream_t stream) {
  SP_CHECK_SHAPE("spectrum_colsum");
  SIMCLR_CHECK_ARG(x && weights && sums && workspace, "spectrum_colsum: null argument");
  SIMCLR_CHECK_ARG(sp_al16(x) && sp_al16(weights) && sp_al16(sums) && sp_al16(workspace), "spectrum_colsum: every pointer must be 16-byte aligned");
  const SpPlan p = sp_plan(n, D);
  double* part = (double*)workspace;
  hipLaunchKernelGGL(sp_colsum, dim3(D / gram_tile::kCols, p.sum_parts), dim3(256), 0, stream, x, weights, n, D, part);
  SIMCLR_CHECK_LAUNCH();
  hipLaunchKernelGGL(sp_sumfin, dim3(ceil_div(D + 1, 256)), dim3(256), 0, stream, (const double*)part, p.sum_parts, D, sums,
                     accumulate ? 1 : 0);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

int simclr_spectrum_cov(const float* x, const float* weights, const float* mu32, int n, int D, double* cov, int accumulate, void* workspace,
                        hipStream_t stream) {
  SP_CHECK_SHAPE("spectrum_cov");
  SIMCLR_CHECK_ARG(x && weights && mu32 && cov && workspace, "spectrum_cov: null argument");
  SIMCLR_CHECK_ARG(sp_al16(x) && sp_al16(weights) && sp_al16(mu32) && sp_al16(cov) && sp_al16(workspace),
                   "spectrum_cov: every pointer must be 16-byte aligned");
  const SpPlan p = sp_plan(n, D);
  float* xc = (float*)workspace;
  float4* part = (float4*)((char*)workspace + p.off_part);
  hipLaunchKernelGGL(sp_center, dim3(ceil_div((long long)n * (D / 4), 256)), dim3(256), 0, stream, x, weights, mu32, n, D, xc);
  SIMCLR_CHECK_LAUNCH();
  const dim3 grid(p.pairs, p.parts);
  if (p.e == 128) {
    hipLaunchKernelGGL(sp_cov<4>, grid, dim3(256), 0, stream, (const float*)xc, n, D, p.part_rows, part);
    SIMCLR_CHECK_LAUNCH();
    hipLaunchKernelGGL(sp_covfin<4>, dim3(p.pairs, 16), dim3(256), 0, stream, (const float4*)part, p.parts, D, cov, accumulate ? 1 : 0);
  } else {
    hipLaunchKernelGGL(sp_cov<2>, grid, dim3(256), 0, stream, (const float*)xc, n, D, p.part_rows, part);
    SIMCLR_CHECK_LAUNCH();
    hipLaunchKernelGGL(sp_covfin<2>, dim3(p.pairs, 4), dim3(256), 0, stream, (const float4*)part, p.parts, D, cov, accumulate ? 1 : 0);
  }
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
