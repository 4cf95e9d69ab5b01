// Generalized contrastive loss (Intriguing Properties of Contrastive Losses) for gfx950:
//   loss = loss_scaling * (align + lambda_weight * dist_match)
// replacing the un-fused graph of the reference's colabs/intriguing_properties/generalized_contrastive_loss.ipynb.
//
// 1. Decoupled NT-Xent (dist='logsumexp').  align = mean((z1 - z2)^2) / 2 over the replica's rows, dist_match = mean over the replica's
//    2n rows of logsumexp over ALL 2N gathered columns of z_i.z_j / T, minus log D.  Nothing is masked (the self column counts) and no
//    column is a positive, so the sweep is the NT-Xent one (csrc/ntxent.hip) without its row_cols() bookkeeping: S = Q K^T tile by tile
//    on v_mfma_f32_16x16x4_f32 (exact f32), reduced online with the running row maximum subtracted (correct for un-normalised rows,
//    where S / T is unbounded), key splits merged in a fixed order, the [2n, 2N] matrix never written.  The backward recomputes S:
//    dS = softmax * coeff, dz_local = dS K, dz_all = dS^T Q as two sweeps in one launch, the per-split partial gradients summed in split
//    order by the combine kernel, which also adds the alignment gradient.  No atomics: bitwise run-to-run deterministic.
//    For l2-normalised rows the self column's term of the gradient, 2 coeff P_ii z_i, is purely radial and can be left out (skip_self):
//    the normalisation backward removes it anyway, but at T = 0.1 it is ~10^3 times the tangential rest, whose low bits it would cost.
//
// 2. Sliced-Wasserstein match (dist='normal' / 'uniform').  The caller projects the gathered rows and the prior on a random orthogonal
//    basis (simclr_gcl_gemm_nt); simclr_swd_sort_match sorts every projected dimension over the M = 2N rows -- one workgroup per
//    dimension, keys + row indices + prior keys in LDS (12 bytes per row: 96 KB at M = 8192), one bitonic network for both -- and writes
//    the matched differences back in ROW order: the gradient of mean((Q_sorted - P_sorted)^2) wrt the projections.  Equal keys are
//    ordered by row index (numpy.argsort(kind='stable')): the network compares (key, index) pairs.
//
// MFMA mapping, tile stager, S fragment and online (max, sum): csrc/sweep_tile.h.
#include "sweep_tile.h"

namespace {

using namespace sweep;

constexpr int kSortThreads = 1024;
constexpr int kSortMaxM = 8192;

// ---- forward: part[split][row] = {running max, sum of exp2} of the logits * log2(e) over the split's key columns -------------------
template <int D>
__global__ __launch_bounds__(256) void gcl_lse_fwd_partial(const float* __restrict__ zq, const float* __restrict__ zk, int two_n,
                                                           int two_N, float scale2 /* log2(e) / T */, int tiles_per_split,
                                                           float* __restrict__ part, int rows_pad) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, fl = lane & 15;
  const int q = blockIdx.x * kTile + wave * 16 + fl;
  float4 ff[D / 16];
#pragma unroll
  for (int s = 0; s < D / 16; ++s)
    ff[s] = (q < two_n) ? *(const float4*)(zq + (size_t)q * D + 16 * s + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
  float m = -INFINITY, l = 0.f;
  const int ntiles = (two_N + kTile - 1) / kTile;
  const int tile_begin = blockIdx.y * tiles_per_split;
  const int tile_end = min(ntiles, tile_begin + tiles_per_split);
  for (int kt = tile_begin; kt < tile_end; ++kt) {
    __syncthreads();
    load_tile<D>(lds, zk, kt * kTile, two_N, tid);
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      const f32x4 acc = s_frag<D>(lds, sub, fl, g, ff);
      const int col0 = kt * kTile + sub * 16 + g * 4;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (col0 + r < two_N) {
          float t = acc[r] * scale2;
          asm volatile("" : "+v"(t));      // the ROUNDED logit everywhere: fused into t - mn the product would keep its low bits and exp2(t - t) != 1
          const float mn = fmaxf(m, t);
          l = l * exp2f(m - mn) + exp2f(t - mn);
          m = mn;
        }
      }
    }
  }
  // the 4 lane groups that share this fixed row, in a fixed order
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {
    const float om = __shfl_xor(m, o, 64), ol = __shfl_xor(l, o, 64);
    ml_merge(m, l, om, ol);
  }
  if (g == 0 && q < two_n) {
    float* p = part + ((size_t)blockIdx.y * rows_pad + q) * 2;
    p[0] = m; p[1] = l;
  }
}

// merge the key splits of every query row (16 lanes per row, fixed xor tree): row_stats[row] = logsumexp in the base-2 domain,
// rowterm[row] = logsumexp - log D
__global__ __launch_bounds__(256) void gcl_lse_finalize_rows(const float* __restrict__ part, int nsplit, int rows_pad, int two_n,
                                                             double log_d, float* __restrict__ row_stats,
                                                             float* __restrict__ rowterm) {
  const int q = blockIdx.x * 16 + (threadIdx.x >> 4);
  const int j = threadIdx.x & 15;
  float m = -INFINITY, l = 0.f;
  if (q < two_n) {
    for (int s = j; s < nsplit; s += 16) {
      const float2 a = *(const float2*)(part + ((size_t)s * rows_pad + q) * 2);
      ml_merge(m, l, a.x, a.y);
    }
  }
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) {
    const float om = __shfl_xor(m, o, 64), ol = __shfl_xor(l, o, 64);
    ml_merge(m, l, om, ol);
  }
  if (j == 0 && q < two_n) {
    row_stats[q] = m + log2f(l);
    rowterm[q] = (float)(((double)m + log2((double)l)) * kLn2d - log_d);
  }
}

// out[0] = loss_scaling * (align + lambda * dist), out[1] = align = mean((z1 - z2)^2) / 2, out[2] = dist = sum(terms) / denom -- one
// workgroup, fixed summation order.  terms = the row terms of the decoupled sweep (denom 2n) or the column losses of the SWD match (D M).
__global__ __launch_bounds__(256) void gcl_reduce_out(const float* __restrict__ terms, int nterms, double denom,
                                                      const float* __restrict__ z, int n, int D, float lambda_weight,
                                                      float loss_scaling, float* __restrict__ out) {
  __shared__ double sh_d[256];
  __shared__ double sh_a[256];
  double dist = 0.0, al = 0.0;
  for (int q = threadIdx.x; q < nterms; q += 256) dist += (double)terms[q];
  const long long half = (long long)n * D;
  for (long long i = threadIdx.x; i < half; i += 256) {
    const double d = (double)z[i] - (double)z[half + i];
    al += d * d;
  }
  sh_d[threadIdx.x] = dist;
  sh_a[threadIdx.x] = al;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      sh_d[threadIdx.x] += sh_d[threadIdx.x + s];
      sh_a[threadIdx.x] += sh_a[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double align = sh_a[0] / (2.0 * (double)half), dm = sh_d[0] / denom;
    out[0] = (float)((double)loss_scaling * (align + (double)lambda_weight * dm));
    out[1] = (float)align;
    out[2] = (float)dm;
  }
}

// SWD backward tail: dz_local[r] = scale * g_all[own row of r] +- (z1 - z2) * acoeff, own row = rank * n + r (view 1), N + rank * n + r - n (view 2)
__global__ __launch_bounds__(256) void gcl_swd_combine(const float* __restrict__ g_all, const float* __restrict__ z_local, int n, int N,
                                                       int D, int rank, float scale, float acoeff, float* __restrict__ dz_local) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * n * (D / 4)) return;
  const int r = i / (D / 4), c = i % (D / 4);
  const int r1 = r < n ? r : r - n;
  const size_t own = r < n ? (size_t)rank * n + r1 : (size_t)N + (size_t)rank * n + r1;
  const float4 gv = *(const float4*)(g_all + own * D + c * 4);
  const float4 a = *(const float4*)(z_local + (size_t)r1 * D + c * 4);
  const float4 b = *(const float4*)(z_local + (size_t)(r1 + n) * D + c * 4);
  const float sg = r < n ? acoeff : -acoeff;
  *(float4*)(dz_local + (size_t)r * D + c * 4) =
      make_float4(gv.x * scale + (a.x - b.x) * sg, gv.y * scale + (a.y - b.y) * sg, gv.z * scale + (a.z - b.z) * sg,
                  gv.w * scale + (a.w - b.w) * sg);
}

// ---- backward sweeps (recompute S).  QUERY_FIXED: fixed rows = queries, streamed = keys, gpart[split][q] = sum_keys softmax[q, key] K[key];
// otherwise fixed rows = keys, streamed = queries, gpart[split][key] = sum_q softmax[q, key] Q[q].  The coefficient is applied by the combine.
template <int D, bool QUERY_FIXED>
__device__ __forceinline__ void gcl_bwd_sweep_body(float* lds, const float* __restrict__ fixed_mat, int fixed_rows,
                                                   const float* __restrict__ stream_mat, int stream_rows, float scale2,
                                                   const float* __restrict__ row_stats, int tiles_per_split,
                                                   float* __restrict__ gpart, int rows_pad, int n, int N, int self_rank) {
  float* stats_s = lds + kTile * D;  // [64] logsumexp of the streamed queries (key-fixed mode)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, fl = lane & 15;
  const int f = blockIdx.x * kTile + wave * 16 + fl;
  float4 ff[D / 16];
#pragma unroll
  for (int s = 0; s < D / 16; ++s)
    ff[s] = (f < fixed_rows) ? *(const float4*)(fixed_mat + (size_t)f * D + 16 * s + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
  const float f_lse = (QUERY_FIXED && f < fixed_rows) ? row_stats[f] : 0.f;
  f32x4 dacc[D / 16];
#pragma unroll
  for (int i = 0; i < D / 16; ++i) dacc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int ntiles = (stream_rows + kTile - 1) / kTile;
  const int tile_begin = blockIdx.y * tiles_per_split;
  const int tile_end = min(ntiles, tile_begin + tiles_per_split);
  for (int kt = tile_begin; kt < tile_end; ++kt) {
    __syncthreads();
    load_tile<D>(lds, stream_mat, kt * kTile, stream_rows, tid);
    if (!QUERY_FIXED && tid < kTile) {
      const int qq = kt * kTile + tid;
      stats_s[tid] = (qq < stream_rows) ? row_stats[qq] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      const f32x4 acc = s_frag<D>(lds, sub, fl, g, ff);
      const int s0 = kt * kTile + sub * 16 + g * 4;  // streamed row of acc[0]
      float ds[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float lse = QUERY_FIXED ? f_lse : stats_s[sub * 16 + g * 4 + r];
        const int q = QUERY_FIXED ? f : s0 + r, col = QUERY_FIXED ? s0 + r : f;
        // the query's own column (self_rank >= 0: its term is left out, see simclr_gcl_lse_bwd)
        const int own = q < n ? self_rank * n + q : N + self_rank * n + (q - n);
        float t = acc[r] * scale2;
        asm volatile("" : "+v"(t));        // the forward's rounded logit, not fma(acc, scale2, -lse): |S / T| may be 10^4, its ulp 10^-3
        ds[r] = (f < fixed_rows && s0 + r < stream_rows && !(self_rank >= 0 && col == own)) ? exp2f(t - lse) : 0.f;
      }
      // dF^T[d][fixed] += sum_streamed T[streamed][d] * dS[streamed][fixed]
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int srow = sub * 16 + 4 * g + u;
          const int dcol = dt * 16 + fl;
          const float a = lds[srow * D + ((((dcol >> 2) ^ (srow & 15)) << 2) | (dcol & 3))];
          dacc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, ds[u], dacc[dt], 0, 0, 0);
        }
      }
    }
  }
  if (f < fixed_rows) {
    float* gp = gpart + ((size_t)blockIdx.y * rows_pad + f) * D;
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt)
      *(float4*)(gp + dt * 16 + 4 * g) = make_float4(dacc[dt][0], dacc[dt][1], dacc[dt][2], dacc[dt][3]);
  }
}

// both sweeps in one launch: blockIdx.z = 0 query-fixed, 1 key-fixed
template <int D>
__global__ __launch_bounds__(256) void gcl_lse_bwd_sweeps(const float* __restrict__ z_local, const float* __restrict__ z_all, int two_n,
                                                          int two_N, float scale2, const float* __restrict__ row_stats, int tiles_k,
                                                          int tiles_q, float* __restrict__ gq, int rows_pad_q, float* __restrict__ gk,
                                                          int rows_pad_k, int gxq, int gyq, int gxk, int gyk, int n, int N,
                                                          int self_rank) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  if (blockIdx.z == 0) {
    if ((int)blockIdx.x >= gxq || (int)blockIdx.y >= gyq) return;
    gcl_bwd_sweep_body<D, true>(lds, z_local, two_n, z_all, two_N, scale2, row_stats, tiles_k, gq, rows_pad_q, n, N, self_rank);
  } else {
    if ((int)blockIdx.x >= gxk || (int)blockIdx.y >= gyk) return;
    gcl_bwd_sweep_body<D, false>(lds, z_all, two_N, z_local, two_n, scale2, row_stats, tiles_q, gk, rows_pad_k, n, N, self_rank);
  }
}

// dz_local = coeff * sum_split gq  +-  (z1 - z2) * acoeff   (the alignment gradient: + on view-1 rows, - on view-2 rows),
// dz_all = coeff * sum_split gk; fixed split order
__global__ __launch_bounds__(256) void gcl_lse_combine(const float* __restrict__ gq, int ksplit, int rows_pad_q, int rows_q,
                                                       const float* __restrict__ gk, int qsplit, int rows_pad_k, int rows_k, int D,
                                                       float coeff, float acoeff, const float* __restrict__ z_local,
                                                       float* __restrict__ dz_local, float* __restrict__ dz_all, int blocks_q) {
  const int b = blockIdx.x;
  const bool isq = b < blocks_q;
  const float* gp = isq ? gq : gk;
  const int nsplit = isq ? ksplit : qsplit, rows_pad = isq ? rows_pad_q : rows_pad_k, rows = isq ? rows_q : rows_k;
  float* dst = isq ? dz_local : dz_all;
  const int i = (isq ? b : b - blocks_q) * 256 + threadIdx.x;
  if (i >= rows * (D / 4)) return;
  const int r = i / (D / 4), c = i % (D / 4);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int s = 0; s < nsplit; ++s) {
    const float4 v = *(const float4*)(gp + ((size_t)s * rows_pad + r) * D + c * 4);
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  acc.x *= coeff; acc.y *= coeff; acc.z *= coeff; acc.w *= coeff;
  if (isq) {
    const int n = rows_q / 2;
    const int r1 = r < n ? r : r - n;
    const float4 a = *(const float4*)(z_local + (size_t)r1 * D + c * 4);
    const float4 bb = *(const float4*)(z_local + (size_t)(r1 + n) * D + c * 4);
    const float sg = r < n ? acoeff : -acoeff;
    acc.x += (a.x - bb.x) * sg; acc.y += (a.y - bb.y) * sg; acc.z += (a.z - bb.z) * sg; acc.w += (a.w - bb.w) * sg;
  }
  *(float4*)(dst + (size_t)r * D + c * 4) = acc;
}

// fks / ftiles_k: key split of the forward sweep (~512 workgroups); ksplit / qsplit: splits of the two backward sweeps (~256 each),
// the targets csrc/ntxent.hip measured for the same sweeps
struct Plan { int rows_pad_q, rows_pad_k, qsplit, ksplit, tiles_q, tiles_k, fks, ftiles_k; };
Plan make_plan(int n, int N) {
  Plan p;
  const int qtiles = ceil_div(2LL * n, kTile), ktiles = ceil_div(2LL * N, kTile);
  p.rows_pad_q = qtiles * kTile;
  p.rows_pad_k = ktiles * kTile;
  constexpr int wgs_f = 512, wgs_b = 256;
  const int fs = max(1, min(ktiles, wgs_f / max(1, qtiles)));
  p.ftiles_k = ceil_div(ktiles, fs);
  p.fks = ceil_div(ktiles, p.ftiles_k);
  const int ks = max(1, min(ktiles, wgs_b / max(1, qtiles)));
  p.tiles_k = ceil_div(ktiles, ks);
  p.ksplit = ceil_div(ktiles, p.tiles_k);
  const int qs = max(1, min(qtiles, wgs_b / max(1, ktiles)));
  p.tiles_q = ceil_div(qtiles, qs);
  p.qsplit = ceil_div(qtiles, p.tiles_q);
  return p;
}
// workspace layout (floats): [forward partials | gq | gk | row terms]
size_t off_gq(const Plan& p) { return (size_t)p.fks * p.rows_pad_q * 2; }
size_t off_gk(const Plan& p, int D) { return off_gq(p) + (size_t)p.ksplit * p.rows_pad_q * D; }
size_t off_rowterm(const Plan& p, int D) { return off_gk(p, D) + (size_t)p.qsplit * p.rows_pad_k * D; }
size_t ws_floats(int n, int N, int D) {
  const Plan p = make_plan(n, N);
  return off_rowterm(p, D) + (size_t)p.rows_pad_q;
}

// ---- sliced-Wasserstein sort-and-match: one workgroup per projected dimension -------------------------------------------------------
// LDS: kp[Mp] keys of P, ip[Mp] their row indices, kq[Mp] keys of the prior; Mp = M rounded up to a power of two, the tail padded with
// (+inf, index >= M), which sorts behind every real row.  The network's compare-exchange sequence does not depend on the data, so the
// kernel terminates on any input; a row index is only ever moved, so ip stays a permutation of 0 .. Mp-1 whatever the keys are, and
// the scatter below is guarded by index < M on top of that.
__global__ __launch_bounds__(kSortThreads) void swd_sort_match_kernel(const float* __restrict__ Pt, const float* __restrict__ Qt, int M,
                                                                      int Mp, int D, float coeff, float* __restrict__ dP,
                                                                      float* __restrict__ col_loss, int* __restrict__ perm) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ double red[kSortThreads];
  float* kp = lds;
  int* ip = (int*)(lds + Mp);
  float* kq = lds + 2 * (size_t)Mp;
  const int c = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < Mp; i += kSortThreads) {
    kp[i] = i < M ? Pt[(size_t)c * M + i] : INFINITY;
    kq[i] = i < M ? Qt[(size_t)c * M + i] : INFINITY;
    ip[i] = i;
  }
  __syncthreads();
  for (int k = 2; k <= Mp; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (Mp >> 1); t += kSortThreads) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));   // bit j clear
        const int p = i | j;
        const bool up = (i & k) == 0;
        const float a = kp[i], b = kp[p];
        const int ia = ip[i], ib = ip[p];
        const bool a_after_b = (a > b) || (a == b && ia > ib);
        const bool b_after_a = (b > a) || (a == b && ib > ia);
        if (up ? a_after_b : b_after_a) { kp[i] = b; kp[p] = a; ip[i] = ib; ip[p] = ia; }
        const float qa = kq[i], qb = kq[p];
        if (up ? (qa > qb) : (qb > qa)) { kq[i] = qb; kq[p] = qa; }
      }
      __syncthreads();
    }
  }
  double acc = 0.0;
  for (int k = tid; k < M; k += kSortThreads) {
    const float diff = kp[k] - kq[k];
    const int id = ip[k];
    if ((unsigned)id < (unsigned)M) dP[(size_t)id * D + c] = coeff * diff;
    if (perm != nullptr) perm[(size_t)c * M + k] = id;
    acc += (double)diff * (double)diff;
  }
  red[tid] = acc;
  __syncthreads();
  for (int s = kSortThreads / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) col_loss[c] = (float)red[0];
}

// C[m][n] = sum_k A[m][k] * B[n][k], fp32 row-major, any M and N, K a multiple of 16; exact f32 MFMA.  The projections of the SWD loss
// (M or N = the global row count, which need not be a multiple of 16; K = D <= 256): a wave owns a 32 x 32 tile and reads its operand
// rows straight from global memory (both operands sit in L2: at most 8192 x 256 floats).
__global__ __launch_bounds__(256) void gcl_gemm_nt_kernel(const float* __restrict__ A, const float* __restrict__ B, float* __restrict__ C,
                                                          int M, int N, int K) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, fl = lane & 15;
  const int m0 = blockIdx.y * 64 + (wave >> 1) * 32, n0 = blockIdx.x * 64 + (wave & 1) * 32;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += 16) {
    float4 a[2], b[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int m = m0 + i * 16 + fl, nn = n0 + i * 16 + fl;
      a[i] = m < M ? *(const float4*)(A + (size_t)m * K + k0 + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
      b[i] = nn < N ? *(const float4*)(B + (size_t)nn * K + k0 + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].x, b[j].x, acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].y, b[j].y, acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].z, b[j].z, acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].w, b[j].w, acc[i][j], 0, 0, 0);
      }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + i * 16 + 4 * g + r, nn = n0 + j * 16 + fl;
        if (m < M && nn < N) C[(size_t)m * N + nn] = acc[i][j][r];
      }
}

}  // namespace

extern "C" {

size_t simclr_gcl_lse_workspace_bytes(int n, int N, int D) {
  if (n <= 0 || N < n || N % n != 0 || !(D == 64 || D == 128 || D == 256)) return 0;
  return ws_floats(n, N, D) * sizeof(float);
}

int simclr_gcl_lse_fwd(const float* z_local, const float* z_all, int n, int N, int D, float temperature, float lambda_weight,
                       float loss_scaling, float* out, float* row_stats, void* workspace, hipStream_t stream) {
  SIMCLR_CHECK_ARG(D == 64 || D == 128 || D == 256, "gcl_lse_fwd: D must be 64/128/256 (got %d)", D);
  SIMCLR_CHECK_ARG(n > 0 && N >= n && N % n == 0, "gcl_lse_fwd: need N = R*n (n=%d N=%d)", n, N);
  SIMCLR_CHECK_ARG(temperature > 0.f, "gcl_lse_fwd: temperature must be > 0");
  SIMCLR_CHECK_ARG(z_local && z_all && out && row_stats && workspace, "gcl_lse_fwd: null argument");
  const Plan p = make_plan(n, N);
  float* part = (float*)workspace;
  const float scale2 = kLog2e / temperature;
  const dim3 grid(p.rows_pad_q / kTile, p.fks);
  const size_t lds = (size_t)kTile * D * sizeof(float);
#define LAUNCH_FWD(DD) \
  hipLaunchKernelGGL((gcl_lse_fwd_partial<DD>), grid, dim3(256), lds, stream, z_local, z_all, 2 * n, 2 * N, scale2, p.ftiles_k, part, p.rows_pad_q)
  if (D == 64) LAUNCH_FWD(64); else if (D == 128) LAUNCH_FWD(128); else LAUNCH_FWD(256);
#undef LAUNCH_FWD
  SIMCLR_CHECK_LAUNCH();
  float* rowterm = part + off_rowterm(p, D);
  hipLaunchKernelGGL(gcl_lse_finalize_rows, dim3(ceil_div(2LL * n, 16)), dim3(256), 0, stream, part, p.fks, p.rows_pad_q, 2 * n,
                     log((double)D), row_stats, rowterm);
  hipLaunchKernelGGL(gcl_reduce_out, dim3(1), dim3(256), 0, stream, rowterm, 2 * n, 2.0 * n, z_local, n, D, lambda_weight, loss_scaling, out);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

int simclr_gcl_lse_bwd(const float* z_local, const float* z_all, int n, int N, int D, float temperature, float lambda_weight,
                       float loss_scaling, int rank, int skip_self, const float* row_stats, float grad_scale, float* dz_local,
                       float* dz_all, void* workspace, hipStream_t stream) {
  SIMCLR_CHECK_ARG(D == 64 || D == 128 || D == 256, "gcl_lse_bwd: D must be 64/128/256 (got %d)", D);
  SIMCLR_CHECK_ARG(n > 0 && N >= n && N % n == 0, "gcl_lse_bwd: need N = R*n (n=%d N=%d)", n, N);
  SIMCLR_CHECK_ARG(temperature > 0.f, "gcl_lse_bwd: temperature must be > 0");
  SIMCLR_CHECK_ARG(rank >= 0 && rank < N / n, "gcl_lse_bwd: rank %d out of range", rank);
  SIMCLR_CHECK_ARG(z_local && z_all && row_stats && dz_local && dz_all && workspace, "gcl_lse_bwd: null argument");
  const Plan p = make_plan(n, N);
  float* part = (float*)workspace;
  float* gq = part + off_gq(p);
  float* gk = part + off_gk(p, D);
  const float scale2 = kLog2e / temperature;
  const size_t lds = (size_t)(kTile * D + kTile) * sizeof(float);
  const dim3 gridq(p.rows_pad_q / kTile, p.ksplit), gridk(p.rows_pad_k / kTile, p.qsplit);
  const dim3 gridb(max(gridq.x, gridk.x), max(gridq.y, gridk.y), 2);
#define LAUNCH_BWD(DD)                                                                                                               \
  hipLaunchKernelGGL((gcl_lse_bwd_sweeps<DD>), gridb, dim3(256), lds, stream, z_local, z_all, 2 * n, 2 * N, scale2, row_stats, p.tiles_k, \
                     p.tiles_q, gq, p.rows_pad_q, gk, p.rows_pad_k, (int)gridq.x, (int)gridq.y, (int)gridk.x, (int)gridk.y, n, N, skip_self ? rank : -1)
  if (D == 64) LAUNCH_BWD(64); else if (D == 128) LAUNCH_BWD(128); else LAUNCH_BWD(256);
#undef LAUNCH_BWD
  SIMCLR_CHECK_LAUNCH();
  // d(loss_scaling * lambda * mean_{2n rows} lse(S / T)) / dS = softmax / (2n T); d align / dz1 = (z1 - z2) / (n D)
  const float coeff = loss_scaling * lambda_weight * grad_scale / (temperature * 2.0f * (float)n);
  const float acoeff = loss_scaling * grad_scale / ((float)n * (float)D);
  const int blocks_q = ceil_div(2LL * n * (D / 4), 256), blocks_k = ceil_div(2LL * N * (D / 4), 256);
  hipLaunchKernelGGL(gcl_lse_combine, dim3(blocks_q + blocks_k), dim3(256), 0, stream, gq, p.ksplit, p.rows_pad_q, 2 * n, gk, p.qsplit,
                     p.rows_pad_k, 2 * N, D, coeff, acoeff, z_local, dz_local, dz_all, blocks_q);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

int simclr_swd_sort_match(const float* Pt, const float* Qt, int M, int D, float coeff, float* dP, float* col_loss, int* perm,
                          hipStream_t stream) {
  SIMCLR_CHECK_ARG(M >= 1 && M <= kSortMaxM, "swd_sort_match: M must be 1..%d rows (got %d): a column is sorted in LDS", kSortMaxM, M);
  SIMCLR_CHECK_ARG(D >= 1, "swd_sort_match: bad D=%d", D);
  SIMCLR_CHECK_ARG(Pt && Qt && dP && col_loss, "swd_sort_match: null argument");
  int Mp = 2;
  while (Mp < M) Mp <<= 1;
  const size_t lds = (size_t)Mp * 12;
  hipLaunchKernelGGL(swd_sort_match_kernel, dim3(D), dim3(kSortThreads), lds, stream, Pt, Qt, M, Mp, D, coeff, dP, col_loss, perm);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

int simclr_gcl_swd_out(const float* col_loss, const float* z_local, int n, int M, int D, float lambda_weight, float loss_scaling, float* out,
                       hipStream_t stream) {
  SIMCLR_CHECK_ARG(n >= 1 && M >= 1 && D >= 4 && D % 4 == 0, "gcl_swd_out: bad shape n=%d M=%d D=%d", n, M, D);
  SIMCLR_CHECK_ARG(col_loss && z_local && out, "gcl_swd_out: null argument");
  hipLaunchKernelGGL(gcl_reduce_out, dim3(1), dim3(256), 0, stream, col_loss, D, (double)D * (double)M, z_local, n, D, lambda_weight,
                     loss_scaling, out);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

int simclr_gcl_swd_bwd(const float* g_all, const float* z_local, int n, int N, int D, int rank, float lambda_weight, float loss_scaling,
                       float grad_scale, float* dz_local, hipStream_t stream) {
  SIMCLR_CHECK_ARG(n > 0 && N >= n && N % n == 0 && D >= 4 && D % 4 == 0, "gcl_swd_bwd: need N = R*n, D a multiple of 4 (n=%d N=%d D=%d)", n, N, D);
  SIMCLR_CHECK_ARG(rank >= 0 && rank < N / n, "gcl_swd_bwd: rank %d out of range", rank);
  SIMCLR_CHECK_ARG(g_all && z_local && dz_local, "gcl_swd_bwd: null argument");
  // every replica computes the same global term: the replica's share (1 / R through grad_scale) of R identical terms is the term itself
  const float scale = lambda_weight * loss_scaling * grad_scale * (float)(N / n);
  const float acoeff = loss_scaling * grad_scale / ((float)n * (float)D);
  hipLaunchKernelGGL(gcl_swd_combine, dim3(ceil_div(2LL * n * (D / 4), 256)), dim3(256), 0, stream, g_all, z_local, n, N, D, rank, scale,
                     acoeff, dz_local);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

int simclr_gcl_gemm_nt(const float* A, const float* B, float* C, int M, int N, int K, hipStream_t stream) {
  SIMCLR_CHECK_ARG(M > 0 && N > 0 && K > 0 && K % 16 == 0, "gcl_gemm_nt: M=%d N=%d must be positive, K=%d a multiple of 16", M, N, K);
  SIMCLR_CHECK_ARG(A && B && C, "gcl_gemm_nt: null argument");
  hipLaunchKernelGGL(gcl_gemm_nt_kernel, dim3(ceil_div(N, 64), ceil_div(M, 64)), dim3(256), 0, stream, A, B, C, M, N, K);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
