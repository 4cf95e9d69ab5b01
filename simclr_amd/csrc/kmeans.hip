// Spherical k-means on frozen encoder features (simclr_amd/kmeans.py): the two hot paths of a Lloyd iteration and the centroid finish.
// x [n, D] = a slab of unit rows, c [K, D] = unit centroids, weights w_n (0 = padding):
//   a_n = argmax_k x_n . c_k   (ties to the lowest k, a NaN score below every number)
//   s_k = sum_{n: a_n = k} w_n x_n  in double,   c_k <- fp32(s_k / |s_k|)
//
// Assign, three launches:
//   km_assign  one E x E tile of C X^T per workgroup on the exact fp32-input MFMA (csrc/gram_tile.h): centroids on the MFMA's A side,
//              rows on the lane, so a lane owns W rows and walks 4 W centroids of each in ascending order, keeping the running pair
//              (max, lowest index).  The 8 lane states of a row (2 waves x 4 lane groups) are merged through LDS in one fixed order and
//              go to slot [centroid tile][row].  Centroids k >= K never enter a pair.  A score is a function of its two rows alone
//              (k in the fixed order of the tile, whatever the tile's position or edge): sharding or reordering the rows changes no bit.
//   km_merge   one thread per row: the centroid tiles in ascending order -> assign, best; the row's previous assignment is read first.
//              256 rows are summed per workgroup in a fixed order: {w (1 - best), w, [w > 0 and the assignment changed]} in double
//   km_out     adds the workgroups' triples in ascending order
// Update, one launch:
//   km_update  blockIdx.x = cluster, blockIdx.y = chunk of 256 columns; a lane owns 4 columns and adds the segment's weighted rows in
//              ascending segment position in double (the product w x is exact in double).  Every index read from memory is checked:
//              an order entry outside [0, n) is skipped, an offset is clamped to [0, n].
// Finish, two launches:
//   km_norm    one workgroup per cluster: |s_k|^2 in double in a fixed order, the keep-previous rule, c_new, 1 - c_new . c_prev
//   km_fin     {kept clusters, max_k (1 - c_new_k . c_prev_k)} in ascending cluster order
// No atomics, every order fixed: repeat calls are bitwise equal.
#include "gram_tile.h"
#include "sweep_tile.h"

#include <math.h>

namespace {

constexpr int kKmMergeRows = 256;     // rows per workgroup of km_merge
constexpr int kKmCols = 256;          // columns per workgroup of km_update (64 lanes x 4)
constexpr int kKmNoIndex = 0x7fffffff;
constexpr double kKmTinyNorm2 = 1e-24;

// (bv, bi) <- the better of (bv, bi) and (v, ix): the larger value, the lower index of equals; a NaN v never enters
__device__ __forceinline__ void km_take(float& bv, int& bi, float v, int ix) {
  if (v > bv || (v == bv && ix < bi)) { bv = v; bi = ix; }
}

// blockIdx.x = centroid tile, blockIdx.y = row tile.  Slot arrays are [centroid tiles][n].
template <int W>
__global__ __launch_bounds__(256) void km_assign(const float* __restrict__ x, const float* __restrict__ c, int n, int D, int K,
                                                 float* __restrict__ pv, int* __restrict__ pi) {
  constexpr int E = 32 * W;
  __shared__ __attribute__((aligned(16))) float lds[2 * gram_tile::op_floats<E>()];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, fl = lane & 15, wm = wave & 1, wn = wave >> 1;
  const int c0 = blockIdx.x * E, r0 = blockIdx.y * E;
  f32x4 acc[W][W];
  gram_tile::tile<W, false, false>(lds, c, D, K, true, x, D, n, true, 0, D, c0, r0, acc);
  __syncthreads();      // every wave is past its last fragment read: the operand LDS becomes the 8 lane states of each row
  float* sv = lds;
  int* si = (int*)(lds + 8 * E);
#pragma unroll
  for (int w = 0; w < W; ++w) {
    const int rl = 16 * W * wn + 16 * w + fl;
    float bv = -INFINITY;
    int bi = kKmNoIndex;
#pragma unroll
    for (int i = 0; i < W; ++i) {
      const int cb = c0 + 16 * W * wm + 16 * i + 4 * g;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (cb + k < K) km_take(bv, bi, acc[i][w][k], cb + k);
    }
    const int slot = rl * 8 + wm * 4 + g;
    sv[slot] = bv; si[slot] = bi;
  }
  __syncthreads();
  if (tid < E && r0 + tid < n) {
    float bv = -INFINITY;
    int bi = kKmNoIndex;
#pragma unroll
    for (int s = 0; s < 8; ++s) km_take(bv, bi, sv[tid * 8 + s], si[tid * 8 + s]);
    const size_t o = (size_t)blockIdx.x * n + r0 + tid;
    pv[o] = bv; pi[o] = bi;
  }
}

// Sum of one double per thread over the workgroup: the butterfly of wave_sum_d, then the 4 waves in ascending order.
__device__ __forceinline__ double km_block_sum(double v, double* sh4) {
  v = wave_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh4[0] + sh4[1]) + sh4[2]) + sh4[3];
}

__global__ __launch_bounds__(256) void km_merge(const float* __restrict__ pv, const int* __restrict__ pi, int ntc,
                                                const float* __restrict__ weights, int n, int* __restrict__ assign,
                                                float* __restrict__ best, double* __restrict__ blk) {
  __shared__ double sh4[4];
  const int row = blockIdx.x * kKmMergeRows + threadIdx.x;
  double cost = 0.0, wd = 0.0, changed = 0.0;
  if (row < n) {
    float bv = -INFINITY;
    int bi = kKmNoIndex;
    for (int t = 0; t < ntc; ++t) {
      const size_t o = (size_t)t * n + row;
      km_take(bv, bi, pv[o], pi[o]);
    }
    if (bi == kKmNoIndex) { bi = 0; bv = NAN; }      // every score of the row is a NaN
    const int before = assign[row];
    assign[row] = bi;
    best[row] = bv;
    const float w = weights[row];
    if (w > 0.f) {
      wd = (double)w;
      cost = wd * (1.0 - (double)bv);
      changed = before != bi ? 1.0 : 0.0;
    }
  }
  cost = km_block_sum(cost, sh4);
  wd = km_block_sum(wd, sh4);
  changed = km_block_sum(changed, sh4);
  if (threadIdx.x == 0) {
    blk[3 * (size_t)blockIdx.x] = cost;
    blk[3 * (size_t)blockIdx.x + 1] = wd;
    blk[3 * (size_t)blockIdx.x + 2] = changed;
  }
}

__global__ __launch_bounds__(64) void km_out(const double* __restrict__ blk, int nblk, double* __restrict__ out) {
  if (threadIdx.x < 3) {
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += blk[3 * (size_t)b + threadIdx.x];
    out[threadIdx.x] = s;
  }
}

// blockIdx.x = cluster, blockIdx.y = column chunk.  The lane's quad lies inside the row: D is a multiple of 64.
__global__ __launch_bounds__(64) void km_update(const float* __restrict__ x, const float* __restrict__ weights, const int* __restrict__ order,
                                                const int* __restrict__ offsets, int n, int D, int K, double* __restrict__ sums,
                                                double* __restrict__ wsum, int accumulate) {
  const int k = blockIdx.x, col = blockIdx.y * kKmCols + 4 * threadIdx.x;
  const int beg = min(max(offsets[k], 0), n), end = min(max(offsets[k + 1], 0), n);
  const bool live = col < D;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, ws = 0.0;
  for (int j = beg; j < end; j += 4) {
    float4 v[4];
    float w[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      w[u] = 0.f;
      if (j + u < end) {
        const int r = order[j + u];
        if ((unsigned)r < (unsigned)n) {         // an entry outside [0, n) is skipped
          w[u] = weights[r];
          if (live && w[u] != 0.f) v[u] = *(const float4*)(x + (size_t)r * D + col);      // a weight-0 row is not read
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {                // ascending segment position; a skipped entry adds an exact zero
      const double wd = (double)w[u];
      s0 += wd * (double)v[u].x; s1 += wd * (double)v[u].y; s2 += wd * (double)v[u].z; s3 += wd * (double)v[u].w;
      ws += wd;
    }
  }
  if (live) {
    double* p = sums + (size_t)k * D + col;
    if (accumulate) { p[0] += s0; p[1] += s1; p[2] += s2; p[3] += s3; }
    else { p[0] = s0; p[1] = s1; p[2] = s2; p[3] = s3; }
  }
  if (blockIdx.y == 0 && threadIdx.x == 0) wsum[k] = accumulate ? wsum[k] + ws : ws;
}

// One workgroup per cluster.  fin [2 K] = {kept flag, 1 - c_new . c_prev} per cluster.
__global__ __launch_bounds__(256) void km_norm(const double* __restrict__ sums, const double* __restrict__ wsum, const float* __restrict__ c_prev,
                                               int D, float* __restrict__ c_new, double* __restrict__ fin) {
  __shared__ double sh4[4];
  const int k = blockIdx.x;
  const double* s = sums + (size_t)k * D;
  const float* cp = c_prev + (size_t)k * D;
  float* cn = c_new + (size_t)k * D;
  double q = 0.0;
  for (int d = threadIdx.x; d < D; d += 256) q += s[d] * s[d];
  q = km_block_sum(q, sh4);
  const bool keep = !(wsum[k] > 0.0) || !(q > kKmTinyNorm2) || !(q < INFINITY);      // a NaN sum keeps the centroid too
  const double inv = keep ? 0.0 : 1.0 / sqrt(q);
  double dot = 0.0;
  for (int d = threadIdx.x; d < D; d += 256) {
    const float p = cp[d];
    const float v = keep ? p : (float)(s[d] * inv);
    cn[d] = v;
    dot += (double)v * (double)p;
  }
  dot = km_block_sum(dot, sh4);
  if (threadIdx.x == 0) {
    fin[2 * (size_t)k] = keep ? 1.0 : 0.0;
    fin[2 * (size_t)k + 1] = 1.0 - dot;
  }
}

// One workgroup: thread t takes clusters t, t + 256, ...; a count of flags and a maximum depend on no order.
__global__ __launch_bounds__(256) void km_fin(const double* __restrict__ fin, int K, double* __restrict__ out2) {
  __shared__ double sh4[4];
  __shared__ double shm[256];
  double s = 0.0, m = -INFINITY;
  for (int k = threadIdx.x; k < K; k += 256) {
    s += fin[2 * (size_t)k];
    m = fmax(m, fin[2 * (size_t)k + 1]);
  }
  s = km_block_sum(s, sh4);
  shm[threadIdx.x] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int t = 1; t < 256; ++t) m = fmax(m, shm[t]);
    out2[0] = s;
    out2[1] = m;
  }
}

bool km_shape_ok(int n, int D, int K) {
  return D >= 64 && D <= 8192 && D % 64 == 0 && K >= 2 && K <= 16384 && n >= 1 && n <= 65536;
}
// Tile edge: 128 where the 128-wide grid alone gives the chip >= 256 workgroups, else 64 (the rule of csrc/logreg.hip)
int km_edge(int n, int K) { return (long long)ceil_div(n, 128) * ceil_div(K, 128) >= 256 ? 128 : 64; }
// workspace: [fin: 2 K doubles][pv | pi: ntc x n x 4 bytes each][blk: 3 doubles per merge workgroup]
struct KmPlan {
  int e, ntc, nblk;
  size_t off_pv, slots, off_blk, bytes;
};
KmPlan km_plan(int n, int D, int K) {
  KmPlan p;
  p.e = km_edge(n, K);
  p.ntc = ceil_div(K, p.e);
  p.nblk = ceil_div(n, kKmMergeRows);
  p.off_pv = (size_t)2 * K * sizeof(double);
  p.slots = ((size_t)p.ntc * n * sizeof(float) + 15) / 16 * 16;
  p.off_blk = p.off_pv + 2 * p.slots;
  p.bytes = p.off_blk + (size_t)3 * p.nblk * sizeof(double);
  return p;
}

}  // namespace

extern "C" {

size_t simclr_kmeans_workspace_bytes(int n, int D, int K) { return km_shape_ok(n, D, K) ? km_plan(n, D, K).bytes : 0; }
int simclr_kmeans_tile_edge(int n, int D, int K) { return km_shape_ok(n, D, K) ? km_plan(n, D, K).e : 0; }

#define KM_CHECK_DK(name)                                                                                                       \
  SIMCLR_CHECK_ARG(D >= 64 && D <= 8192 && D % 64 == 0, name ": the width must be a multiple of 64 in [64, 8192] (got %d)", D); \
  SIMCLR_CHECK_ARG(K >= 2 && K <= 16384, name ": need 2 <= K <= 16384 centroids (got %d)", K)
#define KM_CHECK_N(name) SIMCLR_CHECK_ARG(n >= 1 && n <= 65536, name ": need 1 <= n <= 65536 rows per call (got %d)", n)

int simclr_kmeans_assign(const float* x, const float* c, const float* weights, int n, int D, int K, int* assign, float* best, double* out3,
                         void* workspace, hipStream_t stream) {
  KM_CHECK_DK("kmeans_assign");
  KM_CHECK_N("kmeans_assign");
  SIMCLR_CHECK_ARG(x && c && weights && assign && best && out3 && workspace, "kmeans_assign: null argument");
  SIMCLR_CHECK_ARG(sweep::al16(x) && sweep::al16(c) && sweep::al16(weights) && sweep::al16(assign) && sweep::al16(best) && sweep::al16(out3) &&
                       sweep::al16(workspace),
                   "kmeans_assign: every pointer must be 16-byte aligned");
  const KmPlan p = km_plan(n, D, K);
  char* ws = (char*)workspace;
  float* pv = (float*)(ws + p.off_pv);
  int* pi = (int*)(ws + p.off_pv + p.slots);
  double* blk = (double*)(ws + p.off_blk);
  dim3 grid(p.ntc, ceil_div(n, p.e));
  if (p.e == 128) hipLaunchKernelGGL(km_assign<4>, grid, dim3(256), 0, stream, x, c, n, D, K, pv, pi);
  else hipLaunchKernelGGL(km_assign<2>, grid, dim3(256), 0, stream, x, c, n, D, K, pv, pi);
  SIMCLR_CHECK_LAUNCH();
  hipLaunchKernelGGL(km_merge, dim3(p.nblk), dim3(256), 0, stream, (const float*)pv, (const int*)pi, p.ntc, weights, n, assign, best, blk);
  SIMCLR_CHECK_LAUNCH();
  hipLaunchKernelGGL(km_out, dim3(1), dim3(64), 0, stream, (const double*)blk, p.nblk, out3);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

int simclr_kmeans_update(const float* x, const float* weights, const int* order, const int* offsets, int n, int D, int K, double* sums,
                         double* wsum, int accumulate, hipStream_t stream) {
  KM_CHECK_DK("kmeans_update");
  KM_CHECK_N("kmeans_update");
  SIMCLR_CHECK_ARG(x && weights && order && offsets && sums && wsum, "kmeans_update: null argument");
  SIMCLR_CHECK_ARG(sweep::al16(x) && sweep::al16(weights) && sweep::al16(order) && sweep::al16(offsets) && sweep::al16(sums) && sweep::al16(wsum),
                   "kmeans_update: every pointer must be 16-byte aligned");
  hipLaunchKernelGGL(km_update, dim3(K, ceil_div(D, kKmCols)), dim3(64), 0, stream, x, weights, order, offsets, n, D, K, sums, wsum,
                     accumulate ? 1 : 0);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

int simclr_kmeans_finish(const double* sums, const double* wsum, const float* c_prev, int K, int D, float* c_new, double* out2, void* workspace,
                         hipStream_t stream) {
  KM_CHECK_DK("kmeans_finish");
  SIMCLR_CHECK_ARG(sums && wsum && c_prev && c_new && out2 && workspace, "kmeans_finish: null argument");
  SIMCLR_CHECK_ARG(sweep::al16(sums) && sweep::al16(wsum) && sweep::al16(c_prev) && sweep::al16(c_new) && sweep::al16(out2) && sweep::al16(workspace),
                   "kmeans_finish: every pointer must be 16-byte aligned");
  double* fin = (double*)workspace;
  hipLaunchKernelGGL(km_norm, dim3(K), dim3(256), 0, stream, sums, wsum, c_prev, D, c_new, fin);
  SIMCLR_CHECK_LAUNCH();
  hipLaunchKernelGGL(km_fin, dim3(1), dim3(256), 0, stream, (const double*)fin, K, out2);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
