// Label-free diagnostics of an embedding batch, the same four numbers under every pretraining loss.  z_all [2N, D] holds the
// l2-normalised online projections of the gathered global batch, view a in rows [0, N), view b in rows [N, 2N).  Per view v:
//   m_v = colmean(z_v),  xc = z_v - m_v,  G = xc xc^T  [N, N] -- NEVER written,  r_a = G_aa
//   align   = (1 / N) sum_i |z_a,i - z_b,i|^2                                                     in [0, 4]
//   uniform = (1/2) sum_v log((1 / (N (N-1))) sum_{a != b} exp(-t max(r_a + r_b - 2 G_ab, 0)))    in [-4t, 0]; 0 = one point
//   std     = (1/2) sum_v sqrt(D) (1 / D) sum_k sqrt(sum_a xc_ak^2 / (N-1))                       about 1 healthy, 0 collapsed
//   rank    = (1/2) sum_v PR_v,  PR_v = (sum_a G_aa)^2 / sum_ab G_ab^2 (diagonal included); 0 when sum_a G_aa / (N-1) <= 1e-12
// (alignment and uniformity after Wang & Isola 2020; the standard deviation of the normalised output is the collapse check of the BYOL
// and SimSiam papers; PR is the participation ratio (sum lambda)^2 / sum lambda^2 of the spectrum of C = xc^T xc / (N-1).)  Three
// identities carry it: |z_a - z_b|^2 = r_a + r_b - 2 G_ab (the mean cancels), tr C = sum_a G_aa / (N-1), and
// |C|_F^2 = sum_ab G_ab^2 / (N-1)^2 -- the identity of csrc/vicreg.hip -- so nothing [D, D] and no spectrum is formed.
//
// Four launches:
//   rp_center  per view and 32-column group: the mean in double, xc = fl32(z - m) stored, the column sums of squares of the ROUNDED xc
//              in double (as vr_center of csrc/vicreg.hip)
//   rp_rows    one wave per row: r_a = sum_k xc_ak^2 of the stored xc in double, and for a row of view a the squared distance to its
//              partner row of view b, summed in double from the differences (never 2 - 2 cos)
//   rp_pairs   one view per grid z, one E x E tile of G per workgroup on the exact fp32-input MFMA (csrc/gram_tile.h); the epilogue reads
//              the accumulators: every in-range element adds g^2, every in-range off-diagonal one exp2(-t log2(e) max(r_a + r_b - 2 g,
//              0)); two doubles per workgroup go to a slot of its own
//   rp_finish  one workgroup adds the slots, the rows and the columns in a fixed order in double and writes the four fp32 values
// The distance, the exponent and exp2 itself (a short polynomial after splitting off the nearest integer) are formed in double, so the
// only float32 roundings between the stored xc and the result are those of the MFMA accumulation and the final store.
// With t <= 16 the smallest term is exp(-64): a plain sum does.  No atomics, every order is fixed: a second call is bitwise the first,
// and every replica computes the same bits from the same gathered block.
#include "gram_tile.h"

#include <math.h>

namespace {

constexpr double kRpCollapse = 1e-12;     // tr C at or below this: the view has collapsed to a point, PR = 0 (a definition)

// Centre: blockIdx.y = view, blockIdx.x = 32-column group.  colsq[v][j] = sum_a xc_aj^2 of the stored values.
__global__ __launch_bounds__(256) void rp_center(const float* __restrict__ z_all, int N, int D, float* __restrict__ xc_all,
                                                 double* __restrict__ colsq) {
  __shared__ double sh[32 * gram_tile::kCols];
  __shared__ double res[gram_tile::kCols];
  const int tid = threadIdx.x, q = tid & 7, rg = tid >> 3;
  const int j0 = blockIdx.x * gram_tile::kCols + 4 * q;
  const float* z = z_all + (size_t)blockIdx.y * N * D + j0;
  float* xc = xc_all + (size_t)blockIdx.y * N * D + j0;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int a = rg; a < N; a += 32) {
    const float4 x = *(const float4*)(z + (size_t)a * D);
    v[0] += (double)x.x; v[1] += (double)x.y; v[2] += (double)x.z; v[3] += (double)x.w;
  }
  gram_tile::col_reduce(v, sh, res);
  double mu[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { mu[k] = res[4 * q + k] / (double)N; v[k] = 0.0; }
  for (int a = rg; a < N; a += 32) {
    const float4 x = *(const float4*)(z + (size_t)a * D);
    const float4 c = make_float4((float)((double)x.x - mu[0]), (float)((double)x.y - mu[1]), (float)((double)x.z - mu[2]),
                                 (float)((double)x.w - mu[3]));
    *(float4*)(xc + (size_t)a * D) = c;
    v[0] += (double)c.x * (double)c.x; v[1] += (double)c.y * (double)c.y;
    v[2] += (double)c.z * (double)c.z; v[3] += (double)c.w * (double)c.w;
  }
  gram_tile::col_reduce(v, sh, res);
  if (tid < gram_tile::kCols) colsq[(size_t)blockIdx.y * D + blockIdx.x * gram_tile::kCols + tid] = res[tid];
}

// Rows: wave w of workgroup b owns row 4 b + w of the [2N, D] block.  Lane l adds the quads l, l + 64, ... in order, the 64 lanes are
// added by the butterfly of wave_sum_d: one fixed order.  r[row] for every row; pairdist[i] for the rows i < N of view a.
__global__ __launch_bounds__(256) void rp_rows(const float* __restrict__ z_all, const float* __restrict__ xc_all, int N, int D,
                                               double* __restrict__ r, double* __restrict__ pairdist) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= 2LL * N) return;
  const float4* x = (const float4*)(xc_all + (size_t)row * D);
  double s = 0.0;
  for (int k = lane; k < D / 4; k += 64) {
    const float4 c = x[k];
    s += (double)c.x * (double)c.x + (double)c.y * (double)c.y + (double)c.z * (double)c.z + (double)c.w * (double)c.w;
  }
  s = wave_sum_d(s);
  if (lane == 0) r[row] = s;
  if (row < N) {
    const float4* za = (const float4*)(z_all + (size_t)row * D);
    const float4* zb = (const float4*)(z_all + ((size_t)N + (size_t)row) * D);
    double d = 0.0;
    for (int k = lane; k < D / 4; k += 64) {
      const float4 p = za[k], o = zb[k];
      const double d0 = (double)p.x - (double)o.x, d1 = (double)p.y - (double)o.y, d2 = (double)p.z - (double)o.z,
                   d3 = (double)p.w - (double)o.w;
      d += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
    }
    d = wave_sum_d(d);
    if (lane == 0) pairdist[row] = d;
  }
}

// exp2(e) for e <= 0 in double: e = n + f with n the nearest integer; 2^f = exp(f ln 2) by its Taylor polynomial of degree 11 in Horner
// form (|f ln 2| <= 0.347: the first dropped term, x^12 / 12!, is at most 6.3e-15, below 1e-14 of the value), then the exact scaling by 2^n.  exp2(0) is exactly 1.
__device__ __forceinline__ double rp_exp2(double e) {
  const double n = rint(e);
  const double x = (e - n) * 0.6931471805599453;
  double p = 1.0 / 39916800.0;
  p = fma(p, x, 1.0 / 3628800.0);
  p = fma(p, x, 1.0 / 362880.0);
  p = fma(p, x, 1.0 / 40320.0);
  p = fma(p, x, 1.0 / 5040.0);
  p = fma(p, x, 1.0 / 720.0);
  p = fma(p, x, 1.0 / 120.0);
  p = fma(p, x, 1.0 / 24.0);
  p = fma(p, x, 1.0 / 6.0);
  p = fma(p, x, 0.5);
  p = fma(p, x, 1.0);
  p = fma(p, x, 1.0);
  return ldexp(p, (int)n);
}

// Pairs: blockIdx.z = view, (blockIdx.x, blockIdx.y) = tile of G.  part[2 * slot] = the tile's sum of g^2 over its in-range elements,
// part[2 * slot + 1] = its sum of exp2(c max(r_a + r_b - 2 g, 0)) over the in-range off-diagonal ones, c = -t log2(e);
// slot = (view * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x.  Nothing else is written.
template <int W>
__global__ __launch_bounds__(256) void rp_pairs(const float* __restrict__ xc_all, const double* __restrict__ r_all, int N, int D, double c,
                                                double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float lds[2 * gram_tile::op_floats<32 * W>()];
  __shared__ double wsum[2][4];
  constexpr int E = 32 * W;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, fl = lane & 15, wm = wave & 1, wn = wave >> 1;
  const int v = blockIdx.z;
  const int m0 = blockIdx.x * E, n0 = blockIdx.y * E;
  const float* x = xc_all + (size_t)v * N * D;
  const double* r = r_all + (size_t)v * N;
  f32x4 acc[W][W];
  gram_tile::tile<W, false, false>(lds, x, D, N, true, x, D, N, true, 0, D, m0, n0, acc);
  // the 4 W row norms of this lane, loaded once (0 past the last row: those elements are skipped below)
  double ra[W][4];
#pragma unroll
  for (int i = 0; i < W; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int a = m0 + 16 * W * wm + 16 * i + 4 * g + k;
      ra[i][k] = a < N ? r[a] : 0.0;
    }
  double sq = 0.0, ex = 0.0;
#pragma unroll
  for (int w = 0; w < W; ++w) {
    const int b = n0 + 16 * W * wn + 16 * w + fl;
    if (b >= N) continue;
    const double rb = r[b];
#pragma unroll
    for (int i = 0; i < W; ++i) {
      const int a0 = m0 + 16 * W * wm + 16 * i + 4 * g;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int a = a0 + k;
        if (a >= N) continue;
        const double gab = (double)acc[i][w][k];
        sq += gab * gab;
        if (a != b) ex += rp_exp2(c * fmax(ra[i][k] + rb - 2.0 * gab, 0.0));
      }
    }
  }
  sq = wave_sum_d(sq);
  ex = wave_sum_d(ex);
  if (lane == 0) { wsum[0][wave] = sq; wsum[1][wave] = ex; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const size_t slot = ((size_t)v * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    part[2 * slot] = ((wsum[0][0] + wsum[0][1]) + wsum[0][2]) + wsum[0][3];
    part[2 * slot + 1] = ((wsum[1][0] + wsum[1][1]) + wsum[1][2]) + wsum[1][3];
  }
}

// out = {align, uniform, std, rank}: one workgroup; every thread sums a strided share of each list, the 256 shares are added in order.
// Sums 0..3 belong to view a and 4..7 to view b: {sum g^2, sum exp, sum r, sum of the column standard deviations}; 8 = pair distances.
__global__ __launch_bounds__(256) void rp_finish(const double* __restrict__ part, int ntiles, const double* __restrict__ r,
                                                 const double* __restrict__ pairdist, const double* __restrict__ colsq, int N, int D,
                                                 float* __restrict__ out) {
  __shared__ double sh[9][256];
  const int tid = threadIdx.x;
  double s[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) s[k] = 0.0;
#pragma unroll
  for (int v = 0; v < 2; ++v) {
    for (int t = tid; t < ntiles; t += 256) {
      s[4 * v + 0] += part[2 * ((size_t)v * ntiles + t)];
      s[4 * v + 1] += part[2 * ((size_t)v * ntiles + t) + 1];
    }
    for (int a = tid; a < N; a += 256) s[4 * v + 2] += r[(size_t)v * N + a];
    for (int j = tid; j < D; j += 256) s[4 * v + 3] += sqrt(colsq[(size_t)v * D + j] / (double)(N - 1));
  }
  for (int a = tid; a < N; a += 256) s[8] += pairdist[a];
#pragma unroll
  for (int k = 0; k < 9; ++k) sh[k][tid] = s[k];
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      double t = 0.0;
      for (int i = 0; i < 256; ++i) t += sh[k][i];
      s[k] = t;
    }
    const double n = (double)N, nm1 = (double)(N - 1);
    double uniform = 0.0, sd = 0.0, rank = 0.0;
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const double g2 = s[4 * v], ex = s[4 * v + 1], tr = s[4 * v + 2], cs = s[4 * v + 3];
      uniform += log(ex / (n * nm1));
      sd += sqrt((double)D) * cs / (double)D;
      rank += (tr / nm1 <= kRpCollapse || !(g2 > 0.0)) ? 0.0 : tr * tr / g2;
    }
    out[0] = (float)(s[8] / n);
    out[1] = (float)(0.5 * uniform);
    out[2] = (float)(0.5 * sd);
    out[3] = (float)(0.5 * rank);
  }
}

// Tile edge: 128 where both views' tiles still give the chip >= 256 workgroups, else 64 (the rule of csrc/vicreg.hip)
int rp_edge(long long N) { return 2LL * ceil_div(N, 128) * ceil_div(N, 128) >= 256 ? 128 : 64; }
bool rp_shape_ok(int N, int D) { return D >= 64 && D <= 8192 && D % 64 == 0 && N >= 2 && N <= 65536; }
bool rp_t_ok(float t) { return t > 0.f && t <= 16.f; }      // NaN fails the comparison
// workspace layout: [xc: 2 N D floats | colsq: 2 D doubles | r: 2 N doubles | pairdist: N doubles | part: 2 views x ntiles x 2 doubles]
struct RpPlan { int E, tiles_edge, ntiles; size_t off_colsq, off_r, off_pair, off_part, bytes; };
RpPlan rp_plan(int N, int D) {
  RpPlan p;
  p.E = rp_edge(N);
  p.tiles_edge = ceil_div(N, p.E);
  p.ntiles = p.tiles_edge * p.tiles_edge;
  p.off_colsq = (size_t)2 * N * D * sizeof(float);      // a multiple of 512: D is one of 64
  p.off_r = p.off_colsq + (size_t)2 * D * sizeof(double);
  p.off_pair = p.off_r + (size_t)2 * N * sizeof(double);
  p.off_part = p.off_pair + (size_t)N * sizeof(double);
  p.bytes = p.off_part + (size_t)4 * p.ntiles * sizeof(double);
  return p;
}

}  // namespace

extern "C" {

size_t simclr_repr_workspace_bytes(int N, int D) { return rp_shape_ok(N, D) ? rp_plan(N, D).bytes : 0; }
int simclr_repr_tile_edge(int N, int D) { return rp_shape_ok(N, D) ? rp_plan(N, D).E : 0; }

int simclr_repr_stats(const float* z_all, int N, int D, float t, void* ws, float* out4, hipStream_t stream) {
  SIMCLR_CHECK_ARG(D >= 64 && D <= 8192 && D % 64 == 0, "repr_stats: the width must be a multiple of 64 in [64, 8192] (got %d)", D);
  SIMCLR_CHECK_ARG(N >= 2 && N <= 65536, "repr_stats: need 2 <= N <= 65536 rows per view (got %d)", N);
  SIMCLR_CHECK_ARG(rp_t_ok(t), "repr_stats: t must lie in (0, 16] (got %g)", (double)t);
  SIMCLR_CHECK_ARG(z_all && ws && out4, "repr_stats: null argument");
  SIMCLR_CHECK_ARG((uintptr_t)z_all % 16 == 0 && (uintptr_t)ws % 16 == 0, "repr_stats: z_all and the workspace must be 16-byte aligned");
  const RpPlan p = rp_plan(N, D);
  float* xc = (float*)ws;
  double* colsq = (double*)((char*)ws + p.off_colsq);
  double* r = (double*)((char*)ws + p.off_r);
  double* pairdist = (double*)((char*)ws + p.off_pair);
  double* part = (double*)((char*)ws + p.off_part);
  hipLaunchKernelGGL(rp_center, dim3(D / gram_tile::kCols, 2), dim3(256), 0, stream, z_all, N, D, xc, colsq);
  SIMCLR_CHECK_LAUNCH();
  hipLaunchKernelGGL(rp_rows, dim3(ceil_div(2LL * N, 4)), dim3(256), 0, stream, z_all, (const float*)xc, N, D, r, pairdist);
  SIMCLR_CHECK_LAUNCH();
  const double c = -(double)t * 1.4426950408889634;      // -t log2(e)
  dim3 grid(p.tiles_edge, p.tiles_edge, 2);
  if (p.E == 128)
    hipLaunchKernelGGL(rp_pairs<4>, grid, dim3(256), 0, stream, (const float*)xc, (const double*)r, N, D, c, part);
  else
    hipLaunchKernelGGL(rp_pairs<2>, grid, dim3(256), 0, stream, (const float*)xc, (const double*)r, N, D, c, part);
  SIMCLR_CHECK_LAUNCH();
  hipLaunchKernelGGL(rp_finish, dim3(1), dim3(256), 0, stream, (const double*)part, p.ntiles, (const double*)r, (const double*)pairdist,
                     (const double*)colsq, N, D, out4);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
