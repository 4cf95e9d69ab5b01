// DINO self-distillation (Caron et al. 2021, Emerging Properties in Self-Supervised Vision Transformers) for gfx950: the cross-entropy
// of the student's K-way softmax against the centred, sharpened K-way softmax the teacher gives the OTHER view.
//
//   q [2b, D] = l2-normalised online projections, [view-a rows; view-b rows];  k [2b, D] = l2-normalised target projections of the same
//   rows;  ws / wt [K, D] = the row-normalised prototypes of the online / the target network;  c [K] = the centre;  p(r) = (r + b) mod 2b
//   (BYOL's pairing, formed HERE);  s_rj = q_r . ws_j / Ts,  t_rj = (k_r . wt_j - c_j) / Tt,  Ps = softmax_j(s_r),  Pt = softmax_j(t_r)
//   l_r = logsumexp_j(s_r) - sum_j Pt[p(r), j] s_rj = logsumexp_j(s_r) - q_r . u_p(r) / Ts,   u_p = sum_j Pt[p, j] ws_j  ([2b, D])
//   loss = (1 / 2b) sum_r l_r  (the paper's mean over the two cross-view terms),  teacher entropy = (1 / 2b) sum_r H(Pt[r])
//   d loss / d q_r  = (1 / (2b Ts)) (sum_j Ps[r, j] ws_j - u_p(r)),   d loss / d ws_j = (1 / (2b Ts)) sum_r (Ps[r, j] - Pt[p(r), j]) q_r
//
// The sweeps are csrc/moco.hip's -- S = X W^T tile by tile on v_mfma_f32_16x16x4_f32 (exact f32), 64 fixed rows per workgroup held as
// MFMA fragments, 64-row XOR-swizzled LDS tiles, online statistics in the base-2 domain on the ROUNDED logit, splits merged in a fixed
// order, none of the four [2b, K] matrices ever written, no atomics: two calls are bitwise equal.  The forward is the TWO-PASS form:
// a statistics sweep of each side (one launch), then the teacher expectation sweep, which recomputes t from the wt tile, forms
// Pt = exp2(t - lse_t) and accumulates Pt . ws from a SECOND LDS tile.  The key-side backward fixes 64 prototypes (both tables'
// fragments in registers) and streams 64-row tiles of q and of the PAIRED rows k_p(r).
//
// Cancellations avoided:
//   * a near-one-hot teacher row: the statistics keep the NON-maximum mass r = sum_{others} exp2(t - m) apart from the maximum's own 1,
//     and a = sum exp2(t - m) (t - m) with every term <= 0; the row finalize forms lse = m + log1p(r) and the entropy
//     H = log1p(r) - ln 2 * a / (1 + r) in double.  logsumexp - E[t] is never formed;
//   * Ps - Pt is formed per element from the two rounded logits and the two saved log-sum-exps, never as 1 - ...
//
// MFMA mapping, tile stager (plain and PAIRED rows), S fragment and the (m, r, a) row statistics: csrc/sweep_tile.h.
#include "sweep_tile.h"

namespace {

using namespace sweep;

constexpr int kPart = 4;       // floats per (side, split, row) statistics partial: {max, non-maximum mass, sum exp2(t - m)(t - m), -}

// ---- statistics sweep: blockIdx.z = 0 the teacher (k rows against wt, centred), 1 the student (q rows against ws) ---------------------
template <int D>
__global__ __launch_bounds__(256) void dino_stats_sweep(const float* __restrict__ q, const float* __restrict__ k,
                                                        const float* __restrict__ ws, const float* __restrict__ wt,
                                                        const float* __restrict__ center, int two_n, int K, float scale2s, float scale2t,
                                                        int tiles_per_split, float* __restrict__ part, int rows_pad, int nsplit) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* ldc = lds + kTile * D;        // the 64 centre entries of the tile (zeros for the student)
  const bool teacher = blockIdx.z == 0;
  const float* __restrict__ x = teacher ? k : q;
  const float* __restrict__ w = teacher ? wt : ws;
  const float scale2 = teacher ? scale2t : scale2s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, fl = lane & 15;
  const int row = blockIdx.x * kTile + wave * 16 + fl;
  const bool rv = row < two_n;
  float4 ff[D / 16];
#pragma unroll
  for (int s = 0; s < D / 16; ++s)
    ff[s] = rv ? *(const float4*)(x + (size_t)row * D + 16 * s + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
  float m = -INFINITY, r = 0.f, a = 0.f;
  const int ntiles = (K + kTile - 1) / kTile;
  const int tile_begin = blockIdx.y * tiles_per_split;
  const int tile_end = min(ntiles, tile_begin + tiles_per_split);
  for (int kt = tile_begin; kt < tile_end; ++kt) {
    __syncthreads();
    load_tile<D>(lds, w, kt * kTile, K, tid);
    if (tid < kTile) ldc[tid] = (teacher && kt * kTile + tid < K) ? center[kt * kTile + tid] : 0.f;
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      const f32x4 acc = s_frag<D>(lds, sub, fl, g, ff);
      const int col0 = kt * kTile + sub * 16 + g * 4;
      const float4 c4 = *(const float4*)(ldc + sub * 16 + g * 4);
      const float cc[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (col0 + i < K) {                // the ragged last tile: rows past the table count nowhere
          float t = (acc[i] - cc[i]) * scale2;
          asm volatile("" : "+v"(t));      // the ROUNDED logit everywhere: the later sweeps recompute exactly this number
          mra_push(m, r, a, t);
        }
      }
    }
  }
  // the 4 lane groups that share this row, in a fixed order
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {
    const float om = __shfl_xor(m, o, 64), orr = __shfl_xor(r, o, 64), oa = __shfl_xor(a, o, 64);
    mra_merge(m, r, a, om, orr, oa);
  }
  if (g == 0 && rv)
    *(float4*)(part + (((size_t)blockIdx.z * nsplit + blockIdx.y) * rows_pad + row) * kPart) = make_float4(m, r, a, 0.f);
}

// Merge the key splits of every row on both sides (16 lanes per row, fixed xor trees), then in double:
//   row_stats[r] = {lse_s, lse_t} in the base-2 domain (m + log2(1 + r) via log1p),  lse_s_d[r] = the student's, kept in double
//   rowent[r] = H(Pt[r]) = log1p(r) - ln 2 * a / (1 + r)   (a <= 0: two non-negative terms)
__global__ __launch_bounds__(256) void dino_merge_rows(const float* __restrict__ part, int nsplit, int rows_pad, int two_n,
                                                       float* __restrict__ row_stats, double* __restrict__ lse_s_d,
                                                       double* __restrict__ rowent) {
  const int row = blockIdx.x * 16 + (threadIdx.x >> 4);
  const int j = threadIdx.x & 15;
  float m[2] = {-INFINITY, -INFINITY}, r[2] = {0.f, 0.f}, a[2] = {0.f, 0.f};
  if (row < two_n) {
#pragma unroll
    for (int z = 0; z < 2; ++z)
      for (int s = j; s < nsplit; s += 16) {
        const float4 v = *(const float4*)(part + (((size_t)z * nsplit + s) * rows_pad + row) * kPart);
        mra_merge(m[z], r[z], a[z], v.x, v.y, v.z);
      }
  }
#pragma unroll
  for (int z = 0; z < 2; ++z)
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      const float om = __shfl_xor(m[z], o, 64), orr = __shfl_xor(r[z], o, 64), oa = __shfl_xor(a[z], o, 64);
      mra_merge(m[z], r[z], a[z], om, orr, oa);
    }
  if (j == 0 && row < two_n) {
    const double lt = log1p((double)r[0]), ls = log1p((double)r[1]);
    const double lse_s = (double)m[1] + ls * kLog2ed;
    row_stats[2 * row] = (float)lse_s;
    row_stats[2 * row + 1] = (float)((double)m[0] + lt * kLog2ed);
    lse_s_d[row] = lse_s;
    rowent[row] = lt - kLn2d * (double)a[0] / (1.0 + (double)r[0]);
  }
}

// ---- probability sweep (recomputes the logits): gpart[split][row] = sum over the split's prototypes j of P[row, j] v_j ------------------
// TEACHER = false: fixed rows q, P = exp2(s - lse_s) from the ws tile, v = ws (the same tile): the query-side backward.
// TEACHER = true:  fixed rows k, P = exp2(t - lse_t) from the wt tile and the centre, v = ws from a SECOND tile: the forward's u.
template <int D, bool TEACHER>
__global__ __launch_bounds__(256) void dino_prob_sweep(const float* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ v, const float* __restrict__ center, int two_n, int K,
                                                       float scale2, const float* __restrict__ row_stats, int tiles_per_split,
                                                       float* __restrict__ gpart, int rows_pad) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* ldv = TEACHER ? lds + kTile * D : lds;
  float* ldc = lds + (TEACHER ? 2 : 1) * kTile * D;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, fl = lane & 15;
  const int row = blockIdx.x * kTile + wave * 16 + fl;
  const bool rv = row < two_n;
  float4 ff[D / 16];
#pragma unroll
  for (int s = 0; s < D / 16; ++s)
    ff[s] = rv ? *(const float4*)(x + (size_t)row * D + 16 * s + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
  const float lse = rv ? row_stats[2 * row + (TEACHER ? 1 : 0)] : 0.f;
  f32x4 dacc[D / 16];
#pragma unroll
  for (int i = 0; i < D / 16; ++i) dacc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int ntiles = (K + kTile - 1) / kTile;
  const int tile_begin = blockIdx.y * tiles_per_split;
  const int tile_end = min(ntiles, tile_begin + tiles_per_split);
  for (int kt = tile_begin; kt < tile_end; ++kt) {
    __syncthreads();
    load_tile<D>(lds, w, kt * kTile, K, tid);
    if (TEACHER) {
      load_tile<D>(ldv, v, kt * kTile, K, tid);
      if (tid < kTile) ldc[tid] = (kt * kTile + tid < K) ? center[kt * kTile + tid] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      const f32x4 acc = s_frag<D>(lds, sub, fl, g, ff);
      const int col0 = kt * kTile + sub * 16 + g * 4;  // prototype of acc[0]
      float cc[4] = {0.f, 0.f, 0.f, 0.f};
      if (TEACHER) {
        const float4 c4 = *(const float4*)(ldc + sub * 16 + g * 4);
        cc[0] = c4.x; cc[1] = c4.y; cc[2] = c4.z; cc[3] = c4.w;
      }
      float ds[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float t = (acc[i] - cc[i]) * scale2;
        asm volatile("" : "+v"(t));        // the statistics sweep's rounded logit
        ds[i] = (rv && col0 + i < K) ? exp2f(t - lse) : 0.f;
      }
      // G^T[d][fixed row] += sum_proto v[proto][d] * P[proto][fixed row]
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int srow = sub * 16 + 4 * g + u;
          const int dcol = dt * 16 + fl;
          const float av = ldv[srow * D + ((((dcol >> 2) ^ (srow & 15)) << 2) | (dcol & 3))];
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
// sum (the forward's u, and the key-side backward's dws with rows = K)
__global__ __launch_bounds__(256) void dino_combine(const float* __restrict__ gpart, int nsplit, int rows_pad, int rows, int D,
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

// rowterm[r] = l_r = lse_s ln 2 - (q_r . u_p(r)) / Ts in double (D fp32 products, 16 lanes per row, fixed xor tree)
template <int D>
__global__ __launch_bounds__(256) void dino_finalize_rows(const float* __restrict__ q, const float* __restrict__ u,
                                                          const double* __restrict__ lse_s_d, int two_n, double inv_ts,
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
  if (j == 0 && r < two_n) rowterm[r] = lse_s_d[r] * kLn2d - dot * inv_ts;
}

// out[0] = loss = sum(l_r) / 2b, out[1] = mean teacher entropy -- one workgroup: thread i adds rows i, i + 256, ... in double, then a
// fixed binary tree
__global__ __launch_bounds__(256) void dino_reduce_out(const double* __restrict__ rowterm, const double* __restrict__ rowent, int two_n,
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

// ---- key-side backward sweep: wpart[split][j] = sum over the split's rows r of (Ps[r, j] - Pt[p(r), j]) q_r -----------------------------
// A workgroup owns 64 prototypes (the fragments of ws_j AND wt_j fixed in registers) and streams 64-row tiles of q and of k_p(r).
template <int D>
__global__ __launch_bounds__(256) void dino_bwd_w_sweep(const float* __restrict__ q, const float* __restrict__ k,
                                                        const float* __restrict__ ws, const float* __restrict__ wt,
                                                        const float* __restrict__ center, int two_n, int K, float scale2s, float scale2t,
                                                        const float* __restrict__ row_stats, int tiles_per_split,
                                                        float* __restrict__ wpart, int k_pad) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* ldk = lds + kTile * D;          // the paired key rows
  float* lst = lds + 2 * kTile * D;      // {lse_s[r], lse_t[p(r)]} of the 64 streamed rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, fl = lane & 15;
  const int proto = blockIdx.x * kTile + wave * 16 + fl;
  const bool pv = proto < K;
  const int n = two_n >> 1;
  float4 fs[D / 16], ft[D / 16];
#pragma unroll
  for (int s = 0; s < D / 16; ++s) {
    fs[s] = pv ? *(const float4*)(ws + (size_t)proto * D + 16 * s + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
    ft[s] = pv ? *(const float4*)(wt + (size_t)proto * D + 16 * s + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const float cj = pv ? center[proto] : 0.f;
  f32x4 dacc[D / 16];
#pragma unroll
  for (int i = 0; i < D / 16; ++i) dacc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int ntiles = (two_n + kTile - 1) / kTile;
  const int tile_begin = blockIdx.y * tiles_per_split;
  const int tile_end = min(ntiles, tile_begin + tiles_per_split);
  for (int rt = tile_begin; rt < tile_end; ++rt) {
    __syncthreads();
    load_tile<D>(lds, q, rt * kTile, two_n, tid);
    load_tile<D, RowMap::kPaired>(ldk, k, rt * kTile, two_n, tid);
    if (tid < kTile) {
      const int row = rt * kTile + tid;
      const bool ok = row < two_n;
      lst[2 * tid] = ok ? row_stats[2 * row] : 0.f;
      lst[2 * tid + 1] = ok ? row_stats[2 * (row < n ? row + n : row - n) + 1] : 0.f;
    }
    __syncthreads();
#pragma unroll 1                           // two fragment sets and an accumulator set live: unrolled, D = 256 spills
    for (int sub = 0; sub < 4; ++sub) {
      const f32x4 as = s_frag<D>(lds, sub, fl, g, fs);
      const f32x4 at = s_frag<D>(ldk, sub, fl, g, ft);
      const int row0 = rt * kTile + sub * 16 + g * 4;  // streamed row of as[0]
      float ds[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float s = as[i] * scale2s;
        asm volatile("" : "+v"(s));        // the statistics sweeps' rounded logits
        float t = (at[i] - cj) * scale2t;
        asm volatile("" : "+v"(t));
        const float2 st = *(const float2*)(lst + 2 * (sub * 16 + 4 * g + i));
        ds[i] = (pv && row0 + i < two_n) ? exp2f(s - st.x) - exp2f(t - st.y) : 0.f;
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

// ---- the centre: c_j <- c_j + (1 - m) (wt_j . kbar - c_j) -----------------------------------------------------------------------------
// The dot product accumulates in double (16 lanes per prototype, fixed xor tree) and is rounded to fp32 once; the three roundings of
// the blend are separate (no contraction into an fma), so float32 numpy restates it bit for bit (csrc/byol.hip ema_one).
template <int D>
__global__ __launch_bounds__(256) void dino_center_kernel(const float* __restrict__ wt, const double* __restrict__ kbar,
                                                          float* __restrict__ center, int K, float omm) {
  const int j = blockIdx.x * 16 + (threadIdx.x >> 4);
  const int i = threadIdx.x & 15;
  double dot = 0.0;
  if (j < K) {
    const float4* wr = (const float4*)(wt + (size_t)j * D);
#pragma unroll
    for (int c = 0; c < D / 64; ++c) {
      const float4 w = wr[i + 16 * c];
      const double* kb = kbar + 4 * (i + 16 * c);
      dot += (double)w.x * kb[0] + (double)w.y * kb[1] + (double)w.z * kb[2] + (double)w.w * kb[3];
    }
  }
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) dot += __shfl_xor(dot, o, 64);
  if (i == 0 && j < K) {
    const float c = center[j];
    float d = (float)dot - c;
    asm volatile("" : "+v"(d));
    float p = omm * d;
    asm volatile("" : "+v"(p));
    center[j] = c + p;
  }
}

// kbar[d] = scale * sum_r k[r][d] in double, in a fixed order: a workgroup owns 64 columns, its 4 waves take the rows r = w, w + 4, ...
// and are merged 0 + 1 + 2 + 3
__global__ __launch_bounds__(256) void dino_key_mean_kernel(const float* __restrict__ k, int rows, int D, double scale,
                                                            double* __restrict__ kbar) {
  __shared__ double sh[256];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), w = threadIdx.x >> 6;
  double acc = 0.0;
  for (int r = w; r < rows; r += 4) acc += (double)k[(size_t)r * D + c];
  sh[threadIdx.x] = acc;
  __syncthreads();
  if (w == 0) kbar[c] = (((sh[threadIdx.x] + sh[threadIdx.x + 64]) + sh[threadIdx.x + 128]) + sh[threadIdx.x + 192]) * scale;
}

// fks / ftiles: key split of the statistics sweeps (~512 workgroups a side); bks / btiles: of the probability sweeps (~256), the
// targets csrc/moco.hip uses for the same sweeps; rs / rtiles: row split of the key-side sweep (~256 workgroups)
struct Plan { int rows_pad, k_pad, fks, ftiles, bks, btiles, rs, rtiles; };
Plan make_plan(int two_n, int K) {
  Plan p;
  const int qtiles = ceil_div(two_n, kTile), ktiles = ceil_div(K, kTile);
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
// workspace layout (4-byte words): [row terms (double) | row entropies (double) | student lse (double) | statistics partials of both
// sides | probability-sweep partials | key-side partials]
size_t off_ent(const Plan& p) { return 2 * (size_t)p.rows_pad; }
size_t off_lse(const Plan& p) { return 4 * (size_t)p.rows_pad; }
size_t off_part(const Plan& p) { return 6 * (size_t)p.rows_pad; }
size_t off_gpart(const Plan& p) { return off_part(p) + 2 * (size_t)p.fks * p.rows_pad * kPart; }
size_t off_wpart(const Plan& p, int D) { return off_gpart(p) + (size_t)p.bks * p.rows_pad * D; }
size_t ws_words(const Plan& p, int D) { return off_wpart(p, D) + (size_t)p.rs * p.k_pad * D; }

bool shape_ok(int two_n, int K) { return two_n >= 2 && two_n % 2 == 0 && two_n <= (1 << 22) && K >= 2 && K <= (1 << 22); }

}  // namespace

extern "C" {

size_t simclr_dino_workspace_bytes(int two_n, int K, int D) {
  if (!shape_ok(two_n, K) || !dim_ok(D)) return 0;
  return ws_words(make_plan(two_n, K), D) * sizeof(float);
}

int simclr_dino_key_splits(int two_n, int K) {
  if (!shape_ok(two_n, K)) return 0;
  return make_plan(two_n, K).fks;
}

int simclr_dino_row_splits(int two_n, int K) {
  if (!shape_ok(two_n, K)) return 0;
  return make_plan(two_n, K).rs;
}

int simclr_dino_fwd(const float* q, const float* k, const float* ws, const float* wt, const float* center, int two_n, int K, int D,
                    float student_temp, float teacher_temp, float* out, float* row_stats, float* u, void* workspace,
                    hipStream_t stream) {
  SIMCLR_CHECK_ARG(dim_ok(D), "dino_fwd: D must be 64/128/256 (got %d)", D);
  SIMCLR_CHECK_ARG(shape_ok(two_n, K), "dino_fwd: need an even two_n >= 2 and K >= 2 (two_n=%d K=%d)", two_n, K);
  SIMCLR_CHECK_ARG(student_temp > 0.f && teacher_temp > 0.f && student_temp <= 3.0e38f && teacher_temp <= 3.0e38f,
                   "dino_fwd: the temperatures must be > 0 and finite");          // (NaN fails the comparison)
  SIMCLR_CHECK_ARG(al16(q) && al16(k) && al16(ws) && al16(wt) && al16(u) && al16(workspace) && al4(center) && al4(out) && row_stats &&
                       ((uintptr_t)row_stats & 7) == 0,
                   "dino_fwd: null argument, or q / k / ws / wt / u / workspace not 16-byte aligned");
  const Plan p = make_plan(two_n, K);
  float* wsp = (float*)workspace;
  double* rowterm = (double*)wsp;
  double* rowent = (double*)(wsp + off_ent(p));
  double* lse_s_d = (double*)(wsp + off_lse(p));
  float* part = wsp + off_part(p);
  float* gpart = wsp + off_gpart(p);
  const float scale2s = kLog2e / student_temp, scale2t = kLog2e / teacher_temp;
  const size_t lds1 = ((size_t)kTile * D + kTile) * sizeof(float), lds2 = ((size_t)2 * kTile * D + kTile) * sizeof(float);
  const dim3 grid_s(p.rows_pad / kTile, p.fks, 2), grid_p(p.rows_pad / kTile, p.bks), gridr(ceil_div(two_n, 16));
  const long long chunks = (long long)two_n * (D / 4);
#define LAUNCH_FWD(DD)                                                                                                                \
  do {                                                                                                                                \
    SIMCLR_CHECK_ARG(raise_lds(dino_stats_sweep<DD>, lds1) && raise_lds(dino_prob_sweep<DD, true>, lds2),                             \
                     "dino_fwd: %d bytes of LDS refused", (int)lds2);                                                                 \
    hipLaunchKernelGGL((dino_stats_sweep<DD>), grid_s, dim3(256), lds1, stream, q, k, ws, wt, center, two_n, K, scale2s, scale2t,     \
                       p.ftiles, part, p.rows_pad, p.fks);                                                                            \
    SIMCLR_CHECK_LAUNCH();                                                                                                            \
    hipLaunchKernelGGL(dino_merge_rows, gridr, dim3(256), 0, stream, part, p.fks, p.rows_pad, two_n, row_stats, lse_s_d, rowent);     \
    SIMCLR_CHECK_LAUNCH();                                                                                                            \
    hipLaunchKernelGGL((dino_prob_sweep<DD, true>), grid_p, dim3(256), lds2, stream, k, wt, ws, center, two_n, K, scale2t, row_stats, \
                       p.btiles, gpart, p.rows_pad);                                                                                  \
    SIMCLR_CHECK_LAUNCH();                                                                                                            \
    hipLaunchKernelGGL(dino_combine, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, stream, gpart, p.bks, p.rows_pad, two_n,   \
                       DD, (const float*)nullptr, 1.f, u);                                                                            \
    SIMCLR_CHECK_LAUNCH();                                                                                                            \
    hipLaunchKernelGGL((dino_finalize_rows<DD>), gridr, dim3(256), 0, stream, q, u, lse_s_d, two_n, 1.0 / (double)student_temp,       \
                       rowterm);                                                                                                      \
  } while (0)
  if (D == 64) LAUNCH_FWD(64); else if (D == 128) LAUNCH_FWD(128); else LAUNCH_FWD(256);
#undef LAUNCH_FWD
  SIMCLR_CHECK_LAUNCH();
  hipLaunchKernelGGL(dino_reduce_out, dim3(1), dim3(256), 0, stream, rowterm, rowent, two_n, out);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

int simclr_dino_bwd_q(const float* q, const float* ws, const float* u, int two_n, int K, int D, float student_temp,
                      const float* row_stats, float grad_scale, float* dq, void* workspace, hipStream_t stream) {
  SIMCLR_CHECK_ARG(dim_ok(D), "dino_bwd_q: D must be 64/128/256 (got %d)", D);
  SIMCLR_CHECK_ARG(shape_ok(two_n, K), "dino_bwd_q: need an even two_n >= 2 and K >= 2 (two_n=%d K=%d)", two_n, K);
  SIMCLR_CHECK_ARG(student_temp > 0.f && student_temp <= 3.0e38f, "dino_bwd_q: the temperature must be > 0 and finite");
  SIMCLR_CHECK_ARG(al16(q) && al16(ws) && al16(u) && al16(dq) && al16(workspace) && row_stats && ((uintptr_t)row_stats & 7) == 0,
                   "dino_bwd_q: null argument, or q / ws / u / dq / workspace not 16-byte aligned");
  const Plan p = make_plan(two_n, K);
  float* gpart = (float*)workspace + off_gpart(p);
  const float scale2s = kLog2e / student_temp;
  const size_t lds1 = ((size_t)kTile * D + kTile) * sizeof(float);
  const dim3 grid_p(p.rows_pad / kTile, p.bks);
#define LAUNCH_BWD(DD)                                                                                                               \
  do {                                                                                                                               \
    SIMCLR_CHECK_ARG(raise_lds(dino_prob_sweep<DD, false>, lds1), "dino_bwd_q: %d bytes of LDS refused", (int)lds1);                 \
    hipLaunchKernelGGL((dino_prob_sweep<DD, false>), grid_p, dim3(256), lds1, stream, q, ws, ws, (const float*)nullptr, two_n, K,    \
                       scale2s, row_stats, p.btiles, gpart, p.rows_pad);                                                             \
  } while (0)
  if (D == 64) LAUNCH_BWD(64); else if (D == 128) LAUNCH_BWD(128); else LAUNCH_BWD(256);
#undef LAUNCH_BWD
  SIMCLR_CHECK_LAUNCH();
  // d((1 / 2b) sum_r l_r) / dq_r = (1 / (2b Ts)) (sum_j Ps[r, j] ws_j - u_p(r))
  const float coeff = grad_scale / (student_temp * (float)two_n);
  const long long chunks = (long long)two_n * (D / 4);
  hipLaunchKernelGGL(dino_combine, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, stream, gpart, p.bks, p.rows_pad, two_n, D, u,
                     coeff, dq);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

int simclr_dino_bwd_w(const float* q, const float* k, const float* ws, const float* wt, const float* center, int two_n, int K, int D,
                      float student_temp, float teacher_temp, const float* row_stats, float grad_scale, float* dws, void* workspace,
                      hipStream_t stream) {
  SIMCLR_CHECK_ARG(dim_ok(D), "dino_bwd_w: D must be 64/128/256 (got %d)", D);
  SIMCLR_CHECK_ARG(shape_ok(two_n, K), "dino_bwd_w: need an even two_n >= 2 and K >= 2 (two_n=%d K=%d)", two_n, K);
  SIMCLR_CHECK_ARG(student_temp > 0.f && teacher_temp > 0.f && student_temp <= 3.0e38f && teacher_temp <= 3.0e38f,
                   "dino_bwd_w: the temperatures must be > 0 and finite");
  SIMCLR_CHECK_ARG(al16(q) && al16(k) && al16(ws) && al16(wt) && al16(dws) && al16(workspace) && al4(center) && row_stats &&
                       ((uintptr_t)row_stats & 7) == 0,
                   "dino_bwd_w: null argument, or q / k / ws / wt / dws / workspace not 16-byte aligned");
  const Plan p = make_plan(two_n, K);
  float* wpart = (float*)workspace + off_wpart(p, D);
  const float scale2s = kLog2e / student_temp, scale2t = kLog2e / teacher_temp;
  const size_t lds2 = ((size_t)2 * kTile * D + 2 * kTile) * sizeof(float);
  const dim3 grid_w(p.k_pad / kTile, p.rs);
#define LAUNCH_BWD(DD)                                                                                                              \
  do {                                                                                                                              \
    SIMCLR_CHECK_ARG(raise_lds(dino_bwd_w_sweep<DD>, lds2), "dino_bwd_w: %d bytes of LDS refused", (int)lds2);                      \
    hipLaunchKernelGGL((dino_bwd_w_sweep<DD>), grid_w, dim3(256), lds2, stream, q, k, ws, wt, center, two_n, K, scale2s, scale2t,   \
                       row_stats, p.rtiles, wpart, p.k_pad);                                                                        \
  } while (0)
  if (D == 64) LAUNCH_BWD(64); else if (D == 128) LAUNCH_BWD(128); else LAUNCH_BWD(256);
#undef LAUNCH_BWD
  SIMCLR_CHECK_LAUNCH();
  // d((1 / 2b) sum_r l_r) / dws_j = (1 / (2b Ts)) sum_r (Ps[r, j] - Pt[p(r), j]) q_r
  const float coeff = grad_scale / (student_temp * (float)two_n);
  const long long chunks = (long long)K * (D / 4);
  hipLaunchKernelGGL(dino_combine, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, stream, wpart, p.rs, p.k_pad, K, D,
                     (const float*)nullptr, coeff, dws);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

int simclr_dino_key_mean(const float* k, int rows, int D, double scale, double* kbar, hipStream_t stream) {
  SIMCLR_CHECK_ARG(dim_ok(D), "dino_key_mean: D must be 64/128/256 (got %d)", D);
  SIMCLR_CHECK_ARG(rows >= 1 && rows <= (1 << 22), "dino_key_mean: need rows >= 1 (got %d)", rows);
  SIMCLR_CHECK_ARG(al4(k) && kbar && ((uintptr_t)kbar & 7) == 0, "dino_key_mean: null or misaligned argument");
  hipLaunchKernelGGL(dino_key_mean_kernel, dim3(D / 64), dim3(256), 0, stream, k, rows, D, scale, kbar);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

int simclr_dino_center(const float* wt, const double* kbar, float* center, int K, int D, float momentum, hipStream_t stream) {
  SIMCLR_CHECK_ARG(dim_ok(D), "dino_center: D must be 64/128/256 (got %d)", D);
  SIMCLR_CHECK_ARG(K >= 2 && K <= (1 << 22), "dino_center: need K >= 2 (got %d)", K);
  SIMCLR_CHECK_ARG(momentum >= 0.f && momentum <= 1.f, "dino_center: the momentum must lie in [0, 1]");   // (NaN fails both)
  SIMCLR_CHECK_ARG(al16(wt) && kbar && ((uintptr_t)kbar & 7) == 0 && al4(center),
                   "dino_center: null argument, or wt not 16-byte aligned, or kbar not 8-byte aligned");
  const float omm = (float)(1.0 - (double)momentum);
  const dim3 grid(ceil_div(K, 16));
  if (D == 64) hipLaunchKernelGGL((dino_center_kernel<64>), grid, dim3(256), 0, stream, wt, kbar, center, K, omm);
  else if (D == 128) hipLaunchKernelGGL((dino_center_kernel<128>), grid, dim3(256), 0, stream, wt, kbar, center, K, omm);
  else hipLaunchKernelGGL((dino_center_kernel<256>), grid, dim3(256), 0, stream, wt, kbar, center, K, omm);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
