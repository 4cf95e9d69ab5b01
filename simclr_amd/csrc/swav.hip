// SwAV (Caron et al. 2020, Unsupervised Learning of Visual Features by Contrasting Cluster Assignments) for gfx950: the cross-entropy of
// the student's K-way softmax over trained prototypes against the equipartitioned Sinkhorn-Knopp CODE of the OTHER view.
//
//   q [2b, D] = l2-normalised online projections, [view-a rows; view-b rows];  w [K, D] = the row-normalised prototypes;
//   z_all [2N, D] = the gathered global batch, view-major;  p(r) = (r + b) mod 2b;  v(r) = the view of row r (r >= b)
//   Sinkhorn as scaling potentials, L_gj = z_g . w_j / eps, beta^(0) = 0, it = 1 .. I:
//     alpha^v_j = -ln K - logsumexp_{g in view v}(L_gj + beta_g)            (the column step, per view)
//     beta_g    = -ln N - logsumexp_j(L_gj + alpha^{v(g)}_j)   for it < I    (the row step)
//   the code of row g is softmax_j(L_gj + alpha^{v(g)}_j): no [2N, K] matrix ever exists.
//   s_rj = q_r . w_j / T,  t_rj = q_r . w_j / eps + alpha^{v(r)}_j,  Ps = softmax_j(s_r),  Pt = softmax_j(t_r)  (the code: no gradient)
//   l_r = logsumexp_j(s_r) - sum_j Pt[p(r), j] s_rj = logsumexp_j(s_r) - q_r . u_p(r) / T,   u_p = sum_j Pt[p, j] w_j
//   loss = (1 / 2b) sum_r l_r,  code entropy = (1 / 2b) sum_r H(Pt[r])
//   d loss / d q_r = (1 / (2b T)) (sum_j Ps[r, j] w_j - u_p(r)),   d loss / d w_j = (1 / (2b T)) sum_r (Ps[r, j] - Pt[p(r), j]) q_r
//
// The sweeps are csrc/moco.hip's and csrc/dino.hip's -- S = X W^T tile by tile on v_mfma_f32_16x16x4_f32 (exact f32), 64 fixed rows per
// workgroup held as MFMA fragments, 64-row XOR-swizzled LDS tiles, online statistics in the base-2 domain on the ROUNDED logit, splits
// merged in a fixed order, no atomics: two calls are bitwise equal.  s and t are ONE dot product at two scales: the forward's statistics
// sweep pushes both statistics from one fragment.  The per-view offset alpha stands where csrc/dino.hip reads its centre:
//   * a query-side sweep stages the 64 alpha entries of BOTH views beside the key tile and a lane reads the ones of its own row's view
//     (a 64-row workgroup may straddle the view boundary);
//   * the Sinkhorn's column sweep streams rows, and every element counts for the view of ITS row (a tile may straddle the boundary);
//   * the key-side backward reads alpha for the view of the PAIRED row.
// Cancellations avoided as in csrc/dino.hip: the non-maximum mass stays apart (log1p in the double finalize), the entropy is formed from
// two non-negative terms, Ps - Pt is formed per element.
//
// MFMA mapping, tile stager (plain and PAIRED rows), S fragment, rounded logit and the three online row statistics: csrc/sweep_tile.h.
#include "sweep_tile.h"

namespace {

using namespace sweep;

constexpr int kPart = 8;       // floats per (split, row) forward partial: {code max, non-maximum mass, sum exp2(t - m)(t - m), -, student max, non-maximum mass, -, -}
constexpr int kMaxK = 1 << 20;

// ======================================================= Sinkhorn-Knopp ==============================================================
// ---- column sweep: a workgroup owns 64 prototypes and streams 64-row tiles of z_all with their beta; cpart[split][view][prototype] =
// the online (max, sum) of L2_gj + beta2_g over the split's rows g of that view.  beta2 = nullptr: beta = 0 (the first iteration).
template <int D>
__global__ __launch_bounds__(256) void swav_col_sweep(const float* __restrict__ z, const float* __restrict__ w,
                                                      const float* __restrict__ beta2, int rows_all, int K, float scale2,
                                                      int tiles_per_split, float* __restrict__ cpart, int k_pad) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* ldb = lds + kTile * D;        // beta2 of the 64 streamed rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, fl = lane & 15;
  const int proto = blockIdx.x * kTile + wave * 16 + fl;
  const bool pv = proto < K;
  const int n = rows_all >> 1;
  float4 ff[D / 16];
  load_frag<D>(ff, w, proto, pv, g);
  float m0 = -INFINITY, l0 = 0.f, m1 = -INFINITY, l1 = 0.f;
  const int ntiles = (rows_all + kTile - 1) / kTile;
  const int tile_begin = blockIdx.y * tiles_per_split;
  const int tile_end = min(ntiles, tile_begin + tiles_per_split);
  for (int rt = tile_begin; rt < tile_end; ++rt) {
    __syncthreads();
    load_tile<D>(lds, z, rt * kTile, rows_all, tid);
    if (tid < kTile) ldb[tid] = (beta2 != nullptr && rt * kTile + tid < rows_all) ? beta2[rt * kTile + tid] : 0.f;
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      const f32x4 acc = s_frag<D>(lds, sub, fl, g, ff);
      const int row0 = rt * kTile + sub * 16 + g * 4;    // streamed row of acc[0]
      const float4 b4 = *(const float4*)(ldb + sub * 16 + g * 4);
      const float bb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = row0 + i;
        if (row < rows_all) {                // rows past the batch count nowhere
          const float x = logit2(acc[i], scale2, bb[i]);
          if (row < n) ml_push(m0, l0, x); else ml_push(m1, l1, x);   // every element counts for ITS row's view
        }
      }
    }
  }
  // the 4 lane groups that share this prototype, in a fixed order
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {
    const float om0 = __shfl_xor(m0, o, 64), ol0 = __shfl_xor(l0, o, 64);
    const float om1 = __shfl_xor(m1, o, 64), ol1 = __shfl_xor(l1, o, 64);
    ml_merge(m0, l0, om0, ol0);
    ml_merge(m1, l1, om1, ol1);
  }
  if (g == 0 && pv) {
    *(float2*)(cpart + (((size_t)blockIdx.y * 2 + 0) * k_pad + proto) * 2) = make_float2(m0, l0);
    *(float2*)(cpart + (((size_t)blockIdx.y * 2 + 1) * k_pad + proto) * 2) = make_float2(m1, l1);
  }
}

// Merge the row splits of every (view, prototype) in the order 0, 1, ... in double:
//   alpha[v][j] = -ln K - logsumexp (nats, what the caller sees),  alpha2[v][j] = the same in the base-2 domain (what the row sweep reads)
__global__ __launch_bounds__(256) void swav_col_finalize(const float* __restrict__ cpart, int nsplit, int k_pad, int K,
                                                         float* __restrict__ alpha, float* __restrict__ alpha2) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= 2LL * K) return;
  const int v = (int)(idx / K), j = (int)(idx % K);
  double M = -INFINITY;
  for (int s = 0; s < nsplit; ++s) M = fmax(M, (double)cpart[(((size_t)s * 2 + v) * k_pad + j) * 2]);
  double sum = 0.0;
  for (int s = 0; s < nsplit; ++s) {
    const float2 ml = *(const float2*)(cpart + (((size_t)s * 2 + v) * k_pad + j) * 2);
    if (ml.x != -INFINITY) sum += (double)ml.y * exp2((double)ml.x - M);
  }
  const double lse2 = M + log2(sum);
  alpha[(size_t)v * K + j] = (float)(-log((double)K) - lse2 * kLn2d);
  alpha2[(size_t)v * k_pad + j] = (float)(-log2((double)K) - lse2);
}

// ---- row sweep: csrc/moco.hip's statistics sweep with the alpha2 entries of both views staged beside the key tile; a lane reads the
// ones of its own row's view.  rpart[split][row] = the online (max, sum) of L2_gj + alpha2^{v(g)}_j over the split's prototypes.
template <int D>
__global__ __launch_bounds__(256) void swav_row_sweep(const float* __restrict__ z, const float* __restrict__ w,
                                                      const float* __restrict__ alpha2, int rows_all, int K, float scale2,
                                                      int tiles_per_split, float* __restrict__ rpart, int rows_pad, int k_pad) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* lda = lds + kTile * D;        // alpha2[view][the tile's 64 prototypes]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, fl = lane & 15;
  const int row = blockIdx.x * kTile + wave * 16 + fl;
  const bool rv = row < rows_all;
  const int view = row >= (rows_all >> 1) ? 1 : 0;
  float4 ff[D / 16];
  load_frag<D>(ff, z, row, rv, g);
  float m = -INFINITY, l = 0.f;
  const int ntiles = (K + kTile - 1) / kTile;
  const int tile_begin = blockIdx.y * tiles_per_split;
  const int tile_end = min(ntiles, tile_begin + tiles_per_split);
  for (int kt = tile_begin; kt < tile_end; ++kt) {
    __syncthreads();
    load_tile<D>(lds, w, kt * kTile, K, tid);
    if (tid < 2 * kTile) {
      const int col = kt * kTile + (tid & 63);
      lda[tid] = col < K ? alpha2[(size_t)(tid >> 6) * k_pad + col] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      const f32x4 acc = s_frag<D>(lds, sub, fl, g, ff);
      const int col0 = kt * kTile + sub * 16 + g * 4;
      const float4 a4 = *(const float4*)(lda + view * kTile + sub * 16 + g * 4);
      const float aa[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (col0 + i < K) ml_push(m, l, logit2(acc[i], scale2, aa[i]));   // the ragged last tile: rows past the table count nowhere
      }
    }
  }
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {
    const float om = __shfl_xor(m, o, 64), ol = __shfl_xor(l, o, 64);
    ml_merge(m, l, om, ol);
  }
  if (g == 0 && rv) *(float2*)(rpart + ((size_t)blockIdx.y * rows_pad + row) * 2) = make_float2(m, l);
}

// beta2[g] = -log2 N - logsumexp2 over the key splits merged in the order 0, 1, ... in double
__global__ __launch_bounds__(256) void swav_row_finalize(const float* __restrict__ rpart, int nsplit, int rows_pad, int rows_all,
                                                         float* __restrict__ beta2) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= rows_all) return;
  double M = -INFINITY;
  for (int s = 0; s < nsplit; ++s) M = fmax(M, (double)rpart[((size_t)s * rows_pad + row) * 2]);
  double sum = 0.0;
  for (int s = 0; s < nsplit; ++s) {
    const float2 ml = *(const float2*)(rpart + ((size_t)s * rows_pad + row) * 2);
    if (ml.x != -INFINITY) sum += (double)ml.y * exp2((double)ml.x - M);
  }
  beta2[row] = (float)(-log2((double)(rows_all >> 1)) - (M + log2(sum)));
}

// ======================================================= the loss ====================================================================
// ---- statistics sweep: ONE dot product, two scales -- the code logit t (with alpha of the row's own view) and the student logit s
template <int D>
__global__ __launch_bounds__(256) void swav_stats_sweep(const float* __restrict__ q, const float* __restrict__ w,
                                                        const float* __restrict__ alpha, int two_n, int K, float scale2s, float scale2t,
                                                        int tiles_per_split, float* __restrict__ part, int rows_pad) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* lda = lds + kTile * D;        // alpha[view][the tile's 64 prototypes] in the base-2 domain
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, fl = lane & 15;
  const int row = blockIdx.x * kTile + wave * 16 + fl;
  const bool rv = row < two_n;
  const int view = row >= (two_n >> 1) ? 1 : 0;
  float4 ff[D / 16];
  load_frag<D>(ff, q, row, rv, g);
  float mt = -INFINITY, rt = 0.f, at = 0.f, ms = -INFINITY, rs = 0.f;
  const int ntiles = (K + kTile - 1) / kTile;
  const int tile_begin = blockIdx.y * tiles_per_split;
  const int tile_end = min(ntiles, tile_begin + tiles_per_split);
  for (int kt = tile_begin; kt < tile_end; ++kt) {
    __syncthreads();
    load_tile<D>(lds, w, kt * kTile, K, tid);
    if (tid < 2 * kTile) {
      const int col = kt * kTile + (tid & 63);
      lda[tid] = col < K ? alpha[(size_t)(tid >> 6) * K + col] * kLog2e : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      const f32x4 acc = s_frag<D>(lds, sub, fl, g, ff);
      const int col0 = kt * kTile + sub * 16 + g * 4;
      const float4 a4 = *(const float4*)(lda + view * kTile + sub * 16 + g * 4);
      const float aa[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (col0 + i < K) {                // the ragged last tile: rows past the table count nowhere
          mra_push(mt, rt, at, logit2(acc[i], scale2t, aa[i]));
          mr_push(ms, rs, logit2(acc[i], scale2s, 0.f));
        }
      }
    }
  }
  // the 4 lane groups that share this row, in a fixed order
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {
    const float omt = __shfl_xor(mt, o, 64), ort = __shfl_xor(rt, o, 64), oat = __shfl_xor(at, o, 64);
    const float oms = __shfl_xor(ms, o, 64), ors = __shfl_xor(rs, o, 64);
    mra_merge(mt, rt, at, omt, ort, oat);
    mr_merge(ms, rs, oms, ors);
  }
  if (g == 0 && rv) {
    float* pp = part + ((size_t)blockIdx.y * rows_pad + row) * kPart;
    *(float4*)pp = make_float4(mt, rt, at, 0.f);
    *(float4*)(pp + 4) = make_float4(ms, rs, 0.f, 0.f);
  }
}

// Merge the key splits of every row (16 lanes per row, fixed xor trees), then in double:
//   row_stats[r] = {lse_s, lse_t} in the base-2 domain (m + log2(1 + r) via log1p),  lse_s_d[r] = the student's, kept in double
//   rowent[r] = H(Pt[r]) = log1p(r) - ln 2 * a / (1 + r)   (a <= 0: two non-negative terms)
__global__ __launch_bounds__(256) void swav_merge_rows(const float* __restrict__ part, int nsplit, int rows_pad, int two_n,
                                                       float* __restrict__ row_stats, double* __restrict__ lse_s_d,
                                                       double* __restrict__ rowent) {
  const int row = blockIdx.x * 16 + (threadIdx.x >> 4);
  const int j = threadIdx.x & 15;
  float mt = -INFINITY, rt = 0.f, at = 0.f, ms = -INFINITY, rs = 0.f;
  if (row < two_n) {
    for (int s = j; s < nsplit; s += 16) {
      const float* pp = part + ((size_t)s * rows_pad + row) * kPart;
      const float4 vt = *(const float4*)pp, vs = *(const float4*)(pp + 4);
      mra_merge(mt, rt, at, vt.x, vt.y, vt.z);
      mr_merge(ms, rs, vs.x, vs.y);
    }
  }
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) {
    const float omt = __shfl_xor(mt, o, 64), ort = __shfl_xor(rt, o, 64), oat = __shfl_xor(at, o, 64);
    const float oms = __shfl_xor(ms, o, 64), ors = __shfl_xor(rs, o, 64);
    mra_merge(mt, rt, at, omt, ort, oat);
    mr_merge(ms, rs, oms, ors);
  }
  if (j == 0 && row < two_n) {
    const double lt = log1p((double)rt), ls = log1p((double)rs);
    const double lse_s = (double)ms + ls * kLog2ed;
    row_stats[2 * row] = (float)lse_s;
    row_stats[2 * row + 1] = (float)((double)mt + lt * kLog2ed);
    lse_s_d[row] = lse_s;
    rowent[row] = lt - kLn2d * (double)at / (1.0 + (double)rt);
  }
}

// ---- probability sweep (recomputes the logits): gpart[split][row] = sum over the split's prototypes j of P[row, j] w_j ----------------
// CODE = false: P = Ps = exp2(s - lse_s): the query-side backward.   CODE = true: P = Pt = exp2(t - lse_t), t with alpha of the row's own
// view: the forward's u.  One prototype table: the tile that gives the logits is the tile that is averaged.
template <int D, bool CODE>
__global__ __launch_bounds__(256) void swav_prob_sweep(const float* __restrict__ q, const float* __restrict__ w,
                                                       const float* __restrict__ alpha, int two_n, int K, float scale2,
                                                       const float* __restrict__ row_stats, int tiles_per_split,
                                                       float* __restrict__ gpart, int rows_pad) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* lda = lds + kTile * D;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, fl = lane & 15;
  const int row = blockIdx.x * kTile + wave * 16 + fl;
  const bool rv = row < two_n;
  const int view = row >= (two_n >> 1) ? 1 : 0;
  float4 ff[D / 16];
  load_frag<D>(ff, q, row, rv, g);
  const float lse = rv ? row_stats[2 * row + (CODE ? 1 : 0)] : 0.f;
  f32x4 dacc[D / 16];
#pragma unroll
  for (int i = 0; i < D / 16; ++i) dacc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int ntiles = (K + kTile - 1) / kTile;
  const int tile_begin = blockIdx.y * tiles_per_split;
  const int tile_end = min(ntiles, tile_begin + tiles_per_split);
  for (int kt = tile_begin; kt < tile_end; ++kt) {
    __syncthreads();
    load_tile<D>(lds, w, kt * kTile, K, tid);
    if (CODE && tid < 2 * kTile) {
      const int col = kt * kTile + (tid & 63);
      lda[tid] = col < K ? alpha[(size_t)(tid >> 6) * K + col] * kLog2e : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      const f32x4 acc = s_frag<D>(lds, sub, fl, g, ff);
      const int col0 = kt * kTile + sub * 16 + g * 4;  // prototype of acc[0]
      float aa[4] = {0.f, 0.f, 0.f, 0.f};
      if (CODE) {
        const float4 a4 = *(const float4*)(lda + view * kTile + sub * 16 + g * 4);
        aa[0] = a4.x; aa[1] = a4.y; aa[2] = a4.z; aa[3] = a4.w;
      }
      float ds[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float t = logit2(acc[i], scale2, aa[i]);   // the statistics sweep's rounded logit
        ds[i] = (rv && col0 + i < K) ? exp2f(t - lse) : 0.f;
      }
      // G^T[d][fixed row] += sum_proto w[proto][d] * P[proto][fixed row]
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int srow = sub * 16 + 4 * g + u;
          const int dcol = dt * 16 + fl;
          const float av = lds[srow * D + ((((dcol >> 2) ^ (srow & 15)) << 2) | (dcol & 3))];
          dacc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, ds[u], dacc[dt], 0, 0, 0);
        }
      }
    }
  }
  if (rv) {
    float* gp = gpart + ((size_t)blockIdx.y * rows_pad + row) * D;
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt)
      *(float4*)(gp + dt * 16 + 4 * g) = make_float4(dacc[dt][0], dacc[dt][1], dacc[dt][2], dacc[dt][3]);
  }
}

// dst_r = coeff * (sum_split gpart[split][r] - sub_p(r)) in a fixed split order; one 16-byte chunk per thread.  sub = nullptr: the plain
// sum (the forward's u, and the key-side backward's dw with rows = K)
__global__ __launch_bounds__(256) void swav_combine(const float* __restrict__ gpart, int nsplit, int rows_pad, int rows, int D,
                                                    const float* __restrict__ sub, float coeff, float* __restrict__ dst) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int C = D / 4;
  if (i >= (long long)rows * C) return;
  const int r = (int)(i / C), c = (int)(i % C);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int s = 0; s < nsplit; ++s) {
    const float4 v = *(const float4*)(gpart + ((size_t)s * rows_pad + r) * D + c * 4);
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  if (sub) {
    const int n = rows >> 1;
    const int p = r < n ? r + n : r - n;
    const float4 u = *(const float4*)(sub + (size_t)p * D + c * 4);
    acc.x -= u.x; acc.y -= u.y; acc.z -= u.z; acc.w -= u.w;
  }
  *(float4*)(dst + (size_t)r * D + c * 4) = make_float4(coeff * acc.x, coeff * acc.y, coeff * acc.z, coeff * acc.w);
}

// rowterm[r] = l_r = lse_s ln 2 - (q_r . u_p(r)) / T in double (D fp32 products, 16 lanes per row, fixed xor tree)
template <int D>
__global__ __launch_bounds__(256) void swav_finalize_rows(const float* __restrict__ q, const float* __restrict__ u,
                                                          const double* __restrict__ lse_s_d, int two_n, double inv_t,
                                                          double* __restrict__ rowterm) {
  const int r = blockIdx.x * 16 + (threadIdx.x >> 4);
  const int j = threadIdx.x & 15;
  double dot = 0.0;
  if (r < two_n) {
    const int n = two_n >> 1;
    const int p = r < n ? r + n : r - n;
    const float4* qr = (const float4*)(q + (size_t)r * D);
    const float4* up = (const float4*)(u + (size_t)p * D);
#pragma unroll
    for (int i = 0; i < D / 64; ++i) {
      const float4 a = qr[j + 16 * i], b = up[j + 16 * i];
      dot += (double)a.x * b.x + (double)a.y * b.y + (double)a.z * b.z + (double)a.w * b.w;
    }
  }
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) dot += __shfl_xor(dot, o, 64);
  if (j == 0 && r < two_n) rowterm[r] = lse_s_d[r] * kLn2d - dot * inv_t;
}

// out[0] = loss = sum(l_r) / 2b, out[1] = mean code entropy -- one workgroup: thread i adds rows i, i + 256, ... in double, then a
// fixed binary tree
__global__ __launch_bounds__(256) void swav_reduce_out(const double* __restrict__ rowterm, const double* __restrict__ rowent, int two_n,
                                                       float* __restrict__ out) {
  __shared__ double sh_l[256];
  __shared__ double sh_h[256];
  double ls = 0.0, hs = 0.0;
  for (int r = threadIdx.x; r < two_n; r += 256) {
    ls += rowterm[r];
    hs += rowent[r];
  }
  sh_l[threadIdx.x] = ls; sh_h[threadIdx.x] = hs;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      sh_l[threadIdx.x] += sh_l[threadIdx.x + s];
      sh_h[threadIdx.x] += sh_h[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = (float)(sh_l[0] / (double)two_n);
    out[1] = (float)(sh_h[0] / (double)two_n);
  }
}

// ---- key-side backward sweep: wpart[split][j] = sum over the split's rows r of (Ps[r, j] - Pt[p(r), j]) q_r ---------------------------
// A workgroup owns 64 prototypes (ONE fragment set: there is one table) and streams 64-row tiles of q and of the PAIRED rows q_p(r);
// the code logit takes alpha of the paired row's view: v(p(r)) = 1 for r < b.
template <int D>
__global__ __launch_bounds__(256) void swav_bwd_w_sweep(const float* __restrict__ q, const float* __restrict__ w,
                                                        const float* __restrict__ alpha, int two_n, int K, float scale2s, float scale2t,
                                                        const float* __restrict__ row_stats, int tiles_per_split,
                                                        float* __restrict__ wpart, int k_pad) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* ldk = lds + kTile * D;          // the paired rows
  float* lst = lds + 2 * kTile * D;      // {lse_s[r], lse_t[p(r)]} of the 64 streamed rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, fl = lane & 15;
  const int proto = blockIdx.x * kTile + wave * 16 + fl;
  const bool pv = proto < K;
  const int n = two_n >> 1;
  float4 ff[D / 16];
  load_frag<D>(ff, w, proto, pv, g);
  // alpha of this prototype for a paired row of view a / view b, in the base-2 domain (the statistics sweep's product)
  const float a2a = pv ? alpha[proto] * kLog2e : 0.f;
  const float a2b = pv ? alpha[(size_t)K + proto] * kLog2e : 0.f;
  f32x4 dacc[D / 16];
#pragma unroll
  for (int i = 0; i < D / 16; ++i) dacc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int ntiles = (two_n + kTile - 1) / kTile;
  const int tile_begin = blockIdx.y * tiles_per_split;
  const int tile_end = min(ntiles, tile_begin + tiles_per_split);
  for (int rt = tile_begin; rt < tile_end; ++rt) {
    __syncthreads();
    load_tile<D>(lds, q, rt * kTile, two_n, tid);
    load_tile<D, RowMap::kPaired>(ldk, q, rt * kTile, two_n, tid);
    if (tid < kTile) {
      const int row = rt * kTile + tid;
      const bool ok = row < two_n;
      lst[2 * tid] = ok ? row_stats[2 * row] : 0.f;
      lst[2 * tid + 1] = ok ? row_stats[2 * (row < n ? row + n : row - n) + 1] : 0.f;
    }
    __syncthreads();
#pragma unroll 1                           // a fragment set and an accumulator set live: keep the loop rolled as csrc/dino.hip does
    for (int sub = 0; sub < 4; ++sub) {
      const f32x4 as = s_frag<D>(lds, sub, fl, g, ff);
      const f32x4 at = s_frag<D>(ldk, sub, fl, g, ff);
      const int row0 = rt * kTile + sub * 16 + g * 4;  // streamed row of as[0]
      float ds[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = row0 + i;
        const float s = logit2(as[i], scale2s, 0.f);                    // the statistics sweep's rounded logits
        const float t = logit2(at[i], scale2t, row < n ? a2b : a2a);    // the PAIRED row's view
        const float2 st = *(const float2*)(lst + 2 * (sub * 16 + 4 * g + i));
        ds[i] = (pv && row < two_n) ? exp2f(s - st.x) - exp2f(t - st.y) : 0.f;
      }
      // dW^T[d][prototype] += sum_row q[row][d] * (Ps - Pt)[row][prototype]
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int srow = sub * 16 + 4 * g + u;
          const int dcol = dt * 16 + fl;
          const float av = lds[srow * D + ((((dcol >> 2) ^ (srow & 15)) << 2) | (dcol & 3))];
          dacc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, ds[u], dacc[dt], 0, 0, 0);
        }
      }
    }
  }
  if (pv) {
    float* gp = wpart + ((size_t)blockIdx.y * k_pad + proto) * D;
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt)
      *(float4*)(gp + dt * 16 + 4 * g) = make_float4(dacc[dt][0], dacc[dt][1], dacc[dt][2], dacc[dt][3]);
  }
}

// fks / ftiles: key split of the statistics and row sweeps (~512 workgroups); bks / btiles: of the probability sweeps (~256), the
// targets csrc/moco.hip uses for the same sweeps; rs / rtiles: row split of the key-side and column sweeps (~256 workgroups)
struct Plan { int rows_pad, k_pad, fks, ftiles, bks, btiles, rs, rtiles; };
Plan make_plan(int rows, int K) {
  Plan p;
  const int qtiles = ceil_div(rows, kTile), ktiles = ceil_div(K, kTile);
  p.rows_pad = qtiles * kTile;
  p.k_pad = ktiles * kTile;
  constexpr int wgs_f = 512, wgs_b = 256;
  const int fs = max(1, min(ktiles, wgs_f / max(1, qtiles)));
  p.ftiles = ceil_div(ktiles, fs);
  p.fks = ceil_div(ktiles, p.ftiles);
  const int bs = max(1, min(ktiles, wgs_b / max(1, qtiles)));
  p.btiles = ceil_div(ktiles, bs);
  p.bks = ceil_div(ktiles, p.btiles);
  const int rs = max(1, min(qtiles, wgs_b / max(1, ktiles)));
  p.rtiles = ceil_div(qtiles, rs);
  p.rs = ceil_div(qtiles, p.rtiles);
  return p;
}
// workspace of the loss (4-byte words): [row terms (double) | row entropies (double) | student lse (double) | statistics partials |
// probability-sweep partials | key-side partials]
size_t off_ent(const Plan& p) { return 2 * (size_t)p.rows_pad; }
size_t off_lse(const Plan& p) { return 4 * (size_t)p.rows_pad; }
size_t off_part(const Plan& p) { return 6 * (size_t)p.rows_pad; }
size_t off_gpart(const Plan& p) { return off_part(p) + (size_t)p.fks * p.rows_pad * kPart; }
size_t off_wpart(const Plan& p, int D) { return off_gpart(p) + (size_t)p.bks * p.rows_pad * D; }
size_t loss_words(const Plan& p, int D) { return off_wpart(p, D) + (size_t)p.rs * p.k_pad * D; }
// workspace of the Sinkhorn (4-byte words): [beta2 | alpha2 of both views | column partials | row partials]
size_t off_alpha2(const Plan& p) { return (size_t)p.rows_pad; }
size_t off_cpart(const Plan& p) { return off_alpha2(p) + 2 * (size_t)p.k_pad; }
size_t off_rpart(const Plan& p) { return off_cpart(p) + (size_t)p.rs * 2 * p.k_pad * 2; }
size_t sink_words(const Plan& p) { return off_rpart(p) + (size_t)p.fks * p.rows_pad * 2; }

bool shape_ok(int rows, int K) { return rows >= 2 && rows % 2 == 0 && rows <= (1 << 22) && K >= 2 && K <= kMaxK; }

template <int D>
int sinkhorn_launch(const float* z, const float* w, int rows_all, int K, float scale2, int iters, float* alpha, float* wsp,
                    const Plan& p, hipStream_t stream) {
  float* beta2 = wsp;
  float* alpha2 = wsp + off_alpha2(p);
  float* cpart = wsp + off_cpart(p);
  float* rpart = wsp + off_rpart(p);
  const size_t lds_c = ((size_t)kTile * D + kTile) * sizeof(float), lds_r = ((size_t)kTile * D + 2 * kTile) * sizeof(float);
  SIMCLR_CHECK_ARG(raise_lds(swav_col_sweep<D>, lds_c) && raise_lds(swav_row_sweep<D>, lds_r), "swav_sinkhorn: %d bytes of LDS refused",
                   (int)lds_r);
  const dim3 grid_c(p.k_pad / kTile, p.rs), grid_r(p.rows_pad / kTile, p.fks);
  for (int it = 1; it <= iters; ++it) {
    hipLaunchKernelGGL((swav_col_sweep<D>), grid_c, dim3(256), lds_c, stream, z, w, it == 1 ? (const float*)nullptr : beta2, rows_all, K,
                       scale2, p.rtiles, cpart, p.k_pad);
    SIMCLR_CHECK_LAUNCH();
    hipLaunchKernelGGL(swav_col_finalize, dim3((unsigned)((2LL * K + 255) / 256)), dim3(256), 0, stream, cpart, p.rs, p.k_pad, K, alpha,
                       alpha2);
    SIMCLR_CHECK_LAUNCH();
    if (it == iters) break;
    hipLaunchKernelGGL((swav_row_sweep<D>), grid_r, dim3(256), lds_r, stream, z, w, alpha2, rows_all, K, scale2, p.ftiles, rpart,
                       p.rows_pad, p.k_pad);
    SIMCLR_CHECK_LAUNCH();
    hipLaunchKernelGGL(swav_row_finalize, dim3(ceil_div(rows_all, 256)), dim3(256), 0, stream, rpart, p.fks, p.rows_pad, rows_all, beta2);
    SIMCLR_CHECK_LAUNCH();
  }
  return 0;
}

}  // namespace

extern "C" {

size_t simclr_swav_workspace_bytes(int rows, int K, int D) {
  if (!shape_ok(rows, K) || !dim_ok(D)) return 0;
  const Plan p = make_plan(rows, K);
  const size_t a = loss_words(p, D), b = sink_words(p);
  return (a > b ? a : b) * sizeof(float);
}

int simclr_swav_key_splits(int rows, int K) {
  if (!shape_ok(rows, K)) return 0;
  return make_plan(rows, K).fks;
}

int simclr_swav_row_splits(int rows, int K) {
  if (!shape_ok(rows, K)) return 0;
  return make_plan(rows, K).rs;
}

int simclr_swav_sinkhorn(const float* z_all, const float* w, int rows_all, int K, int D, float epsilon, int iters, float* alpha,
                         void* workspace, hipStream_t stream) {
  SIMCLR_CHECK_ARG(dim_ok(D), "swav_sinkhorn: D must be 64/128/256 (got %d)", D);
  SIMCLR_CHECK_ARG(shape_ok(rows_all, K), "swav_sinkhorn: need an even rows_all >= 2 and K in [2, 1048576] (rows_all=%d K=%d)", rows_all,
                   K);
  SIMCLR_CHECK_ARG(pos_finite(epsilon), "swav_sinkhorn: epsilon must be > 0 and finite");
  SIMCLR_CHECK_ARG(iters >= 1 && iters <= 16, "swav_sinkhorn: iters must lie in [1, 16] (got %d)", iters);
  SIMCLR_CHECK_ARG(al16(z_all) && al16(w) && al16(workspace) && al4(alpha),
                   "swav_sinkhorn: null argument, or z_all / w / workspace not 16-byte aligned");
  const Plan p = make_plan(rows_all, K);
  const float scale2 = kLog2e / epsilon;
  float* wsp = (float*)workspace;
  if (D == 64) return sinkhorn_launch<64>(z_all, w, rows_all, K, scale2, iters, alpha, wsp, p, stream);
  if (D == 128) return sinkhorn_launch<128>(z_all, w, rows_all, K, scale2, iters, alpha, wsp, p, stream);
  return sinkhorn_launch<256>(z_all, w, rows_all, K, scale2, iters, alpha, wsp, p, stream);
}

int simclr_swav_fwd(const float* q, const float* w, const float* alpha, int two_n, int K, int D, float temperature, float epsilon,
                    float* out, float* row_stats, float* u, void* workspace, hipStream_t stream) {
  SIMCLR_CHECK_ARG(dim_ok(D), "swav_fwd: D must be 64/128/256 (got %d)", D);
  SIMCLR_CHECK_ARG(shape_ok(two_n, K), "swav_fwd: need an even two_n >= 2 and K in [2, 1048576] (two_n=%d K=%d)", two_n, K);
  SIMCLR_CHECK_ARG(pos_finite(temperature) && pos_finite(epsilon), "swav_fwd: the temperature and epsilon must be > 0 and finite");
  SIMCLR_CHECK_ARG(al16(q) && al16(w) && al16(u) && al16(workspace) && al4(alpha) && al4(out) && al8(row_stats),
                   "swav_fwd: null argument, or q / w / u / workspace not 16-byte aligned");
  const Plan p = make_plan(two_n, K);
  float* wsp = (float*)workspace;
  double* rowterm = (double*)wsp;
  double* rowent = (double*)(wsp + off_ent(p));
  double* lse_s_d = (double*)(wsp + off_lse(p));
  float* part = wsp + off_part(p);
  float* gpart = wsp + off_gpart(p);
  const float scale2s = kLog2e / temperature, scale2t = kLog2e / epsilon;
  const size_t lds1 = ((size_t)kTile * D + 2 * kTile) * sizeof(float);
  const dim3 grid_s(p.rows_pad / kTile, p.fks), grid_p(p.rows_pad / kTile, p.bks), gridr(ceil_div(two_n, 16));
  const long long chunks = (long long)two_n * (D / 4);
#define LAUNCH_FWD(DD)                                                                                                                \
  do {                                                                                                                                \
    SIMCLR_CHECK_ARG(raise_lds(swav_stats_sweep<DD>, lds1) && raise_lds(swav_prob_sweep<DD, true>, lds1),                             \
                     "swav_fwd: %d bytes of LDS refused", (int)lds1);                                                                 \
    hipLaunchKernelGGL((swav_stats_sweep<DD>), grid_s, dim3(256), lds1, stream, q, w, alpha, two_n, K, scale2s, scale2t, p.ftiles,    \
                       part, p.rows_pad);                                                                                             \
    SIMCLR_CHECK_LAUNCH();                                                                                                            \
    hipLaunchKernelGGL(swav_merge_rows, gridr, dim3(256), 0, stream, part, p.fks, p.rows_pad, two_n, row_stats, lse_s_d, rowent);     \
    SIMCLR_CHECK_LAUNCH();                                                                                                            \
    hipLaunchKernelGGL((swav_prob_sweep<DD, true>), grid_p, dim3(256), lds1, stream, q, w, alpha, two_n, K, scale2t, row_stats,       \
                       p.btiles, gpart, p.rows_pad);                                                                                  \
    SIMCLR_CHECK_LAUNCH();                                                                                                            \
    hipLaunchKernelGGL(swav_combine, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, stream, gpart, p.bks, p.rows_pad, two_n,   \
                       DD, (const float*)nullptr, 1.f, u);                                                                            \
    SIMCLR_CHECK_LAUNCH();                                                                                                            \
    hipLaunchKernelGGL((swav_finalize_rows<DD>), gridr, dim3(256), 0, stream, q, u, lse_s_d, two_n, 1.0 / (double)temperature,        \
                       rowterm);                                                                                                      \
  } while (0)
  if (D == 64) LAUNCH_FWD(64); else if (D == 128) LAUNCH_FWD(128); else LAUNCH_FWD(256);
#undef LAUNCH_FWD
  SIMCLR_CHECK_LAUNCH();
  hipLaunchKernelGGL(swav_reduce_out, dim3(1), dim3(256), 0, stream, rowterm, rowent, two_n, out);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

int simclr_swav_bwd_q(const float* q, const float* w, const float* u, int two_n, int K, int D, float temperature,
                      const float* row_stats, float grad_scale, float* dq, void* workspace, hipStream_t stream) {
  SIMCLR_CHECK_ARG(dim_ok(D), "swav_bwd_q: D must be 64/128/256 (got %d)", D);
  SIMCLR_CHECK_ARG(shape_ok(two_n, K), "swav_bwd_q: need an even two_n >= 2 and K in [2, 1048576] (two_n=%d K=%d)", two_n, K);
  SIMCLR_CHECK_ARG(pos_finite(temperature), "swav_bwd_q: the temperature must be > 0 and finite");
  SIMCLR_CHECK_ARG(al16(q) && al16(w) && al16(u) && al16(dq) && al16(workspace) && al8(row_stats),
                   "swav_bwd_q: null argument, or q / w / u / dq / workspace not 16-byte aligned");
  const Plan p = make_plan(two_n, K);
  float* gpart = (float*)workspace + off_gpart(p);
  const float scale2s = kLog2e / temperature;
  const size_t lds1 = ((size_t)kTile * D + 2 * kTile) * sizeof(float);
  const dim3 grid_p(p.rows_pad / kTile, p.bks);
#define LAUNCH_BWD(DD)                                                                                                               \
  do {                                                                                                                               \
    SIMCLR_CHECK_ARG(raise_lds(swav_prob_sweep<DD, false>, lds1), "swav_bwd_q: %d bytes of LDS refused", (int)lds1);                 \
    hipLaunchKernelGGL((swav_prob_sweep<DD, false>), grid_p, dim3(256), lds1, stream, q, w, (const float*)nullptr, two_n, K, scale2s, \
                       row_stats, p.btiles, gpart, p.rows_pad);                                                                      \
  } while (0)
  if (D == 64) LAUNCH_BWD(64); else if (D == 128) LAUNCH_BWD(128); else LAUNCH_BWD(256);
#undef LAUNCH_BWD
  SIMCLR_CHECK_LAUNCH();
  // d((1 / 2b) sum_r l_r) / dq_r = (1 / (2b T)) (sum_j Ps[r, j] w_j - u_p(r))
  const float coeff = grad_scale / (temperature * (float)two_n);
  const long long chunks = (long long)two_n * (D / 4);
  hipLaunchKernelGGL(swav_combine, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, stream, gpart, p.bks, p.rows_pad, two_n, D, u,
                     coeff, dq);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

int simclr_swav_bwd_w(const float* q, const float* w, const float* alpha, int two_n, int K, int D, float temperature, float epsilon,
                      const float* row_stats, float grad_scale, float* dw, void* workspace, hipStream_t stream) {
  SIMCLR_CHECK_ARG(dim_ok(D), "swav_bwd_w: D must be 64/128/256 (got %d)", D);
  SIMCLR_CHECK_ARG(shape_ok(two_n, K), "swav_bwd_w: need an even two_n >= 2 and K in [2, 1048576] (two_n=%d K=%d)", two_n, K);
  SIMCLR_CHECK_ARG(pos_finite(temperature) && pos_finite(epsilon), "swav_bwd_w: the temperature and epsilon must be > 0 and finite");
  SIMCLR_CHECK_ARG(al16(q) && al16(w) && al16(dw) && al16(workspace) && al4(alpha) && al8(row_stats),
                   "swav_bwd_w: null argument, or q / w / dw / workspace not 16-byte aligned");
  const Plan p = make_plan(two_n, K);
  float* wpart = (float*)workspace + off_wpart(p, D);
  const float scale2s = kLog2e / temperature, scale2t = kLog2e / epsilon;
  const size_t lds2 = ((size_t)2 * kTile * D + 2 * kTile) * sizeof(float);
  const dim3 grid_w(p.k_pad / kTile, p.rs);
#define LAUNCH_BWD(DD)                                                                                                              \
  do {                                                                                                                              \
    SIMCLR_CHECK_ARG(raise_lds(swav_bwd_w_sweep<DD>, lds2), "swav_bwd_w: %d bytes of LDS refused", (int)lds2);                      \
    hipLaunchKernelGGL((swav_bwd_w_sweep<DD>), grid_w, dim3(256), lds2, stream, q, w, alpha, two_n, K, scale2s, scale2t, row_stats, \
                       p.rtiles, wpart, p.k_pad);                                                                                   \
  } while (0)
  if (D == 64) LAUNCH_BWD(64); else if (D == 128) LAUNCH_BWD(128); else LAUNCH_BWD(256);
#undef LAUNCH_BWD
  SIMCLR_CHECK_LAUNCH();
  // d((1 / 2b) sum_r l_r) / dw_j = (1 / (2b T)) sum_r (Ps[r, j] - Pt[p(r), j]) q_r
  const float coeff = grad_scale / (temperature * (float)two_n);
  const long long chunks = (long long)K * (D / 4);
  hipLaunchKernelGGL(swav_combine, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, stream, wpart, p.rs, p.k_pad, K, D,
                     (const float*)nullptr, coeff, dw);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
