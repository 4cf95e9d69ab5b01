// Supervised contrastive loss (Khosla et al. 2020, Supervised Contrastive Learning, the L_out^sup form) for gfx950: NT-Xent with every
// same-class row of the GLOBAL batch as a positive.
//
// Layout as NT-Xent's (csrc/ntxent.hip): z_local [2n, D] = [view-1 rows; view-2 rows] of this replica, z_all [2N, D] = every replica's
// view-1 rows, then every replica's view-2 rows, N = R n.  labels_all [N] int32: column j has label labels_all[j mod N]; local row i
// (view v = i / n, sample s = i % n) is global column self(i) = v N + rank n + s and has label labels_all[rank n + s].
//   A(i) = all 2N columns except self(i),  P(i) = {p in A(i): label(p) == label(i)}  (the other view of the image is in it: |P(i)| >= 1)
//   l_i  = logsumexp_{a in A(i)}(z_i.z_a / T) - (1 / |P(i)|) sum_{p in P(i)} z_i.z_p / T
//   loss = (1 / n) sum_{i < 2n} l_i      (the sum of the two per-view means, as NT-Xent; no temperature / base_temperature factor)
//   dS_ia = (g / n) (1 / T) (softmax_{A(i)}(s_i)_a - [a in P(i)] / |P(i)|),  dS_{i, self(i)} = 0,  dz_local = dS z_all,  dz_all = dS^T z_local
//
// The sweep is csrc/gcl.hip's decoupled one -- S = Q K^T tile by tile on v_mfma_f32_16x16x4_f32 (exact f32), 64-row swizzled LDS key
// tiles, online log-sum-exp on the ROUNDED logit with the running maximum subtracted, key splits merged in a fixed order, the [2n, 2N]
// matrix never written, the backward recomputing S with both sweeps in one launch and a fixed-order combine -- plus a per-element
// predicate: the tile's 64 labels are staged next to the key tile; the self column is left out of the maximum, the sum and the gradient;
// a same-label column adds to the positive sum, to an INTEGER positive count (merged by integer adds) and to the positive maximum.
// No atomics: bitwise run-to-run deterministic.  Labels are only ever compared for equality, so renaming the classes changes no bit.
//
// MFMA mapping, tile stager, S fragment and online (max, sum): csrc/sweep_tile.h.
#include "sweep_tile.h"

namespace {

using namespace sweep;

constexpr int kPart = 8;       // floats per (split, row) forward partial: {max, sum, positive sum, positive count (int), positive max, other max, -, -}

// label of global column col (< 2N) / of local row q (< 2n), global column of local row q
__device__ __forceinline__ int col_label(const int* __restrict__ labels, int col, int N) { return labels[col < N ? col : col - N]; }
__device__ __forceinline__ int row_label(const int* __restrict__ labels, int q, int n, int rank) { return labels[rank * n + (q < n ? q : q - n)]; }
__device__ __forceinline__ int row_self(int q, int n, int N, int rank) { return q < n ? rank * n + q : N + rank * n + (q - n); }

// ---- forward: one partial per (key split, query row) over the split's columns of A(row) ----------------------------------------------
// {running max, sum of exp2} of the logits * log2(e); sum of the positives' logits * log2(e); |P|; max raw dot product over P and over A \ P
template <int D>
__global__ __launch_bounds__(256) void supcon_fwd_partial(const float* __restrict__ zq, const float* __restrict__ zk,
                                                          const int* __restrict__ labels, int two_n, int two_N, int n, int N, int rank,
                                                          float scale2 /* log2(e) / T */, int tiles_per_split, float* __restrict__ part,
                                                          int rows_pad) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  int* lab_s = (int*)(lds + kTile * D);   // [64] labels of the tile's key columns
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, fl = lane & 15;
  const int q = blockIdx.x * kTile + wave * 16 + fl;
  const bool qv = q < two_n;
  float4 ff[D / 16];
#pragma unroll
  for (int s = 0; s < D / 16; ++s)
    ff[s] = qv ? *(const float4*)(zq + (size_t)q * D + 16 * s + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
  const int qlab = qv ? row_label(labels, q, n, rank) : 0;
  const int self = qv ? row_self(q, n, N, rank) : -1;
  float m = -INFINITY, l = 0.f, psum = 0.f, pmax = -INFINITY, omax = -INFINITY;
  int pcnt = 0;
  const int ntiles = (two_N + kTile - 1) / kTile;
  const int tile_begin = blockIdx.y * tiles_per_split;
  const int tile_end = min(ntiles, tile_begin + tiles_per_split);
  for (int kt = tile_begin; kt < tile_end; ++kt) {
    __syncthreads();
    load_tile<D>(lds, zk, kt * kTile, two_N, tid);
    if (tid < kTile) {
      const int col = kt * kTile + tid;
      lab_s[tid] = (col < two_N) ? col_label(labels, col, N) : 0;
    }
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      const f32x4 acc = s_frag<D>(lds, sub, fl, g, ff);
      const int col0 = kt * kTile + sub * 16 + g * 4;
      const int4 lb = *(const int4*)(lab_s + sub * 16 + g * 4);
      const int lbv[4] = {lb.x, lb.y, lb.z, lb.w};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int col = col0 + r;
        if (col < two_N && col != self) {   // a column of A(q): the self column counts nowhere
          float t = acc[r] * scale2;
          asm volatile("" : "+v"(t));      // the ROUNDED logit everywhere: fused into t - mn the product would keep its low bits and exp2(t - t) != 1
          const float mn = fmaxf(m, t);
          l = l * exp2f(m - mn) + exp2f(t - mn);
          m = mn;
          const bool pos = lbv[r] == qlab;
          psum += pos ? t : 0.f;
          pcnt += pos ? 1 : 0;
          pmax = pos ? fmaxf(pmax, acc[r]) : pmax;
          omax = pos ? omax : fmaxf(omax, acc[r]);
        }
      }
    }
  }
  // the 4 lane groups that share this fixed row, in a fixed order
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {
    const float om = __shfl_xor(m, o, 64), ol = __shfl_xor(l, o, 64);
    ml_merge(m, l, om, ol);
    psum += __shfl_xor(psum, o, 64);
    pcnt += __shfl_xor(pcnt, o, 64);
    pmax = fmaxf(pmax, __shfl_xor(pmax, o, 64));
    omax = fmaxf(omax, __shfl_xor(omax, o, 64));
  }
  if (g == 0 && qv) {
    float* p = part + ((size_t)blockIdx.y * rows_pad + q) * kPart;
    *(float4*)p = make_float4(m, l, psum, __int_as_float(pcnt));
    *(float4*)(p + 4) = make_float4(pmax, omax, 0.f, 0.f);
  }
}

// merge the key splits of every query row (16 lanes per row, fixed xor tree): row_stats[row] = {logsumexp in the base-2 domain, |P|},
// rowterm[row] = l_row, hit[row] = (max over P >= max over A \ P; a row without a non-positive column is a hit)
__global__ __launch_bounds__(256) void supcon_finalize_rows(const float* __restrict__ part, int nsplit, int rows_pad, int two_n,
                                                            float* __restrict__ row_stats, float* __restrict__ rowterm,
                                                            int* __restrict__ hit) {
  const int q = blockIdx.x * 16 + (threadIdx.x >> 4);
  const int j = threadIdx.x & 15;
  float m = -INFINITY, l = 0.f, pmax = -INFINITY, omax = -INFINITY;
  double psum = 0.0;
  int pcnt = 0;
  if (q < two_n) {
    for (int s = j; s < nsplit; s += 16) {
      const float* p = part + ((size_t)s * rows_pad + q) * kPart;
      const float4 a = *(const float4*)p;
      const float2 b = *(const float2*)(p + 4);
      ml_merge(m, l, a.x, a.y);
      psum += (double)a.z;
      pcnt += __float_as_int(a.w);
      pmax = fmaxf(pmax, b.x);
      omax = fmaxf(omax, b.y);
    }
  }
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) {
    const float om = __shfl_xor(m, o, 64), ol = __shfl_xor(l, o, 64);
    ml_merge(m, l, om, ol);
    psum += __shfl_xor(psum, o, 64);
    pcnt += __shfl_xor(pcnt, o, 64);
    pmax = fmaxf(pmax, __shfl_xor(pmax, o, 64));
    omax = fmaxf(omax, __shfl_xor(omax, o, 64));
  }
  if (j == 0 && q < two_n) {
    row_stats[2 * q] = m + log2f(l);
    row_stats[2 * q + 1] = (float)pcnt;
    rowterm[q] = (float)(((double)m + log2((double)l) - psum / (double)max(pcnt, 1)) * kLn2d);
    hit[q] = pmax >= omax ? 1 : 0;
  }
}

// out[0] = loss = sum(l_i) / n, out[1] = contrast_acc = hits / 2n, out[2] = contrast_positives = sum |P(i)| / 2n -- one workgroup,
// fixed summation order, the two counts summed as integers
__global__ __launch_bounds__(256) void supcon_reduce_out(const float* __restrict__ rowterm, const int* __restrict__ hit,
                                                         const float* __restrict__ row_stats, int two_n, float* __restrict__ out) {
  __shared__ double sh_l[256];
  __shared__ long long sh_h[256];
  __shared__ long long sh_p[256];
  double ls = 0.0;
  long long hs = 0, pc = 0;
  for (int q = threadIdx.x; q < two_n; q += 256) {
    ls += (double)rowterm[q];
    hs += hit[q];
    pc += (long long)row_stats[2 * q + 1];
  }
  sh_l[threadIdx.x] = ls; sh_h[threadIdx.x] = hs; sh_p[threadIdx.x] = pc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      sh_l[threadIdx.x] += sh_l[threadIdx.x + s];
      sh_h[threadIdx.x] += sh_h[threadIdx.x + s];
      sh_p[threadIdx.x] += sh_p[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = (float)(sh_l[0] / (0.5 * (double)two_n));
    out[1] = (float)((double)sh_h[0] / (double)two_n);
    out[2] = (float)((double)sh_p[0] / (double)two_n);
  }
}

// ---- backward sweeps (recompute S).  QUERY_FIXED: fixed rows = queries, streamed = keys,
// gpart[split][q] = sum_keys (softmax[q, key] - [key in P(q)] / |P(q)|) K[key]; otherwise fixed rows = keys, streamed = queries,
// gpart[split][key] = sum_q (softmax[q, key] - [key in P(q)] / |P(q)|) Q[q].  The coefficient is applied by the combine.
template <int D, bool QUERY_FIXED>
__device__ __forceinline__ void supcon_bwd_sweep_body(float* lds, const float* __restrict__ fixed_mat, int fixed_rows,
                                                      const float* __restrict__ stream_mat, int stream_rows,
                                                      const int* __restrict__ labels, float scale2, const float* __restrict__ row_stats,
                                                      int tiles_per_split, float* __restrict__ gpart, int rows_pad, int n, int N,
                                                      int rank) {
  int* lab_s = (int*)(lds + kTile * D);   // [64] labels of the streamed rows
  float* lse_s = lds + kTile * D + kTile; // [64] logsumexp / [64] 1 / |P| of the streamed queries (key-fixed mode)
  float* inv_s = lse_s + kTile;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, fl = lane & 15;
  const int f = blockIdx.x * kTile + wave * 16 + fl;
  const bool fv = f < fixed_rows;
  float4 ff[D / 16];
#pragma unroll
  for (int s = 0; s < D / 16; ++s)
    ff[s] = fv ? *(const float4*)(fixed_mat + (size_t)f * D + 16 * s + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
  const int flab = fv ? (QUERY_FIXED ? row_label(labels, f, n, rank) : col_label(labels, f, N)) : 0;
  const float f_lse = (QUERY_FIXED && fv) ? row_stats[2 * f] : 0.f;
  const float f_inv = (QUERY_FIXED && fv) ? 1.0f / fmaxf(row_stats[2 * f + 1], 1.0f) : 0.f;
  const int f_self = (QUERY_FIXED && fv) ? row_self(f, n, N, rank) : -1;
  f32x4 dacc[D / 16];
#pragma unroll
  for (int i = 0; i < D / 16; ++i) dacc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int ntiles = (stream_rows + kTile - 1) / kTile;
  const int tile_begin = blockIdx.y * tiles_per_split;
  const int tile_end = min(ntiles, tile_begin + tiles_per_split);
  for (int kt = tile_begin; kt < tile_end; ++kt) {
    __syncthreads();
    load_tile<D>(lds, stream_mat, kt * kTile, stream_rows, tid);
    if (tid < kTile) {
      const int sr = kt * kTile + tid;
      const bool sv = sr < stream_rows;
      if (QUERY_FIXED) {
        lab_s[tid] = sv ? col_label(labels, sr, N) : 0;
      } else {
        lab_s[tid] = sv ? row_label(labels, sr, n, rank) : 0;
        lse_s[tid] = sv ? row_stats[2 * sr] : 0.f;
        inv_s[tid] = sv ? 1.0f / fmaxf(row_stats[2 * sr + 1], 1.0f) : 0.f;
      }
    }
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      const f32x4 acc = s_frag<D>(lds, sub, fl, g, ff);
      const int s0 = kt * kTile + sub * 16 + g * 4;  // streamed row of acc[0]
      float ds[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int si = sub * 16 + g * 4 + r;
        const float lse = QUERY_FIXED ? f_lse : lse_s[si];
        const float inv = QUERY_FIXED ? f_inv : inv_s[si];
        // the query's own column: no gradient flows through it
        const int own = QUERY_FIXED ? f_self : row_self(s0 + r, n, N, rank);
        const int col = QUERY_FIXED ? s0 + r : f;
        float t = acc[r] * scale2;
        asm volatile("" : "+v"(t));        // the forward's rounded logit, not fma(acc, scale2, -lse): |S / T| may be 10^4, its ulp 10^-3
        const bool live = fv && s0 + r < stream_rows && col != own;
        const float pterm = (lab_s[si] == flab) ? inv : 0.f;
        ds[r] = live ? exp2f(t - lse) - pterm : 0.f;
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
  if (fv) {
    float* gp = gpart + ((size_t)blockIdx.y * rows_pad + f) * D;
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt)
      *(float4*)(gp + dt * 16 + 4 * g) = make_float4(dacc[dt][0], dacc[dt][1], dacc[dt][2], dacc[dt][3]);
  }
}

// both sweeps in one launch: blockIdx.z = 0 query-fixed, 1 key-fixed
template <int D>
__global__ __launch_bounds__(256) void supcon_bwd_sweeps(const float* __restrict__ z_local, const float* __restrict__ z_all,
                                                         const int* __restrict__ labels, int two_n, int two_N, float scale2,
                                                         const float* __restrict__ row_stats, int tiles_k, int tiles_q,
                                                         float* __restrict__ gq, int rows_pad_q, float* __restrict__ gk, int rows_pad_k,
                                                         int gxq, int gyq, int gxk, int gyk, int n, int N, int rank) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  if (blockIdx.z == 0) {
    if ((int)blockIdx.x >= gxq || (int)blockIdx.y >= gyq) return;
    supcon_bwd_sweep_body<D, true>(lds, z_local, two_n, z_all, two_N, labels, scale2, row_stats, tiles_k, gq, rows_pad_q, n, N, rank);
  } else {
    if ((int)blockIdx.x >= gxk || (int)blockIdx.y >= gyk) return;
    supcon_bwd_sweep_body<D, false>(lds, z_all, two_N, z_local, two_n, labels, scale2, row_stats, tiles_q, gk, rows_pad_k, n, N, rank);
  }
}

// dz_local = coeff * sum_split gq, dz_all = coeff * sum_split gk; fixed split order
__global__ __launch_bounds__(256) void supcon_combine(const float* __restrict__ gq, int ksplit, int rows_pad_q, int rows_q,
                                                      const float* __restrict__ gk, int qsplit, int rows_pad_k, int rows_k, int D,
                                                      float coeff, float* __restrict__ dz_local, float* __restrict__ dz_all, int blocks_q) {
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
  *(float4*)(dst + (size_t)r * D + c * 4) = make_float4(acc.x * coeff, acc.y * coeff, acc.z * coeff, acc.w * coeff);
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
// workspace layout (4-byte words): [forward partials | gq | gk | row terms | row hits]
size_t off_gq(const Plan& p) { return (size_t)p.fks * p.rows_pad_q * kPart; }
size_t off_gk(const Plan& p, int D) { return off_gq(p) + (size_t)p.ksplit * p.rows_pad_q * D; }
size_t off_rowterm(const Plan& p, int D) { return off_gk(p, D) + (size_t)p.qsplit * p.rows_pad_k * D; }
size_t off_hit(const Plan& p, int D) { return off_rowterm(p, D) + (size_t)p.rows_pad_q; }
size_t ws_words(int n, int N, int D) {
  const Plan p = make_plan(n, N);
  return off_hit(p, D) + (size_t)p.rows_pad_q;
}

bool shape_ok(int n, int N, int D) {
  return n > 0 && N >= n && N % n == 0 && N <= (1 << 29) && (D == 64 || D == 128 || D == 256);
}

}  // namespace

extern "C" {

size_t simclr_supcon_workspace_bytes(int n, int N, int D) {
  if (!shape_ok(n, N, D)) return 0;
  return ws_words(n, N, D) * sizeof(float);
}

int simclr_supcon_fwd(const float* z_local, const float* z_all, const int* labels_all, int n, int N, int D, int rank, float temperature,
                      float* out, float* row_stats, void* workspace, hipStream_t stream) {
  SIMCLR_CHECK_ARG(D == 64 || D == 128 || D == 256, "supcon_fwd: D must be 64/128/256 (got %d)", D);
  SIMCLR_CHECK_ARG(shape_ok(n, N, D), "supcon_fwd: need n >= 1 and N = R*n (n=%d N=%d)", n, N);
  SIMCLR_CHECK_ARG(rank >= 0 && rank < N / n, "supcon_fwd: rank %d out of range", rank);
  SIMCLR_CHECK_ARG(temperature > 0.f, "supcon_fwd: temperature must be > 0");
  SIMCLR_CHECK_ARG(z_local && z_all && labels_all && out && row_stats && workspace, "supcon_fwd: null argument");
  const Plan p = make_plan(n, N);
  float* part = (float*)workspace;
  const float scale2 = kLog2e / temperature;
  const dim3 grid(p.rows_pad_q / kTile, p.fks);
  const size_t lds = (size_t)(kTile * D + kTile) * sizeof(float);
#define LAUNCH_FWD(DD)                                                                                                                \
  hipLaunchKernelGGL((supcon_fwd_partial<DD>), grid, dim3(256), lds, stream, z_local, z_all, labels_all, 2 * n, 2 * N, n, N, rank, scale2, \
                     p.ftiles_k, part, p.rows_pad_q)
  if (D == 64) LAUNCH_FWD(64); else if (D == 128) LAUNCH_FWD(128); else LAUNCH_FWD(256);
#undef LAUNCH_FWD
  SIMCLR_CHECK_LAUNCH();
  float* rowterm = part + off_rowterm(p, D);
  int* hit = (int*)(part + off_hit(p, D));
  hipLaunchKernelGGL(supcon_finalize_rows, dim3(ceil_div(2LL * n, 16)), dim3(256), 0, stream, part, p.fks, p.rows_pad_q, 2 * n, row_stats,
                     rowterm, hit);
  hipLaunchKernelGGL(supcon_reduce_out, dim3(1), dim3(256), 0, stream, rowterm, hit, row_stats, 2 * n, out);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

int simclr_supcon_bwd(const float* z_local, const float* z_all, const int* labels_all, int n, int N, int D, int rank, float temperature,
                      const float* row_stats, float grad_scale, float* dz_local, float* dz_all, void* workspace, hipStream_t stream) {
  SIMCLR_CHECK_ARG(D == 64 || D == 128 || D == 256, "supcon_bwd: D must be 64/128/256 (got %d)", D);
  SIMCLR_CHECK_ARG(shape_ok(n, N, D), "supcon_bwd: need n >= 1 and N = R*n (n=%d N=%d)", n, N);
  SIMCLR_CHECK_ARG(rank >= 0 && rank < N / n, "supcon_bwd: rank %d out of range", rank);
  SIMCLR_CHECK_ARG(temperature > 0.f, "supcon_bwd: temperature must be > 0");
  SIMCLR_CHECK_ARG(z_local && z_all && labels_all && row_stats && dz_local && dz_all && workspace, "supcon_bwd: null argument");
  const Plan p = make_plan(n, N);
  float* part = (float*)workspace;
  float* gq = part + off_gq(p);
  float* gk = part + off_gk(p, D);
  const float scale2 = kLog2e / temperature;
  const size_t lds = (size_t)(kTile * D + 3 * kTile) * sizeof(float);
  const dim3 gridq(p.rows_pad_q / kTile, p.ksplit), gridk(p.rows_pad_k / kTile, p.qsplit);
  const dim3 gridb(max(gridq.x, gridk.x), max(gridq.y, gridk.y), 2);
#define LAUNCH_BWD(DD)                                                                                                                  \
  hipLaunchKernelGGL((supcon_bwd_sweeps<DD>), gridb, dim3(256), lds, stream, z_local, z_all, labels_all, 2 * n, 2 * N, scale2, row_stats, \
                     p.tiles_k, p.tiles_q, gq, p.rows_pad_q, gk, p.rows_pad_k, (int)gridq.x, (int)gridq.y, (int)gridk.x, (int)gridk.y, n, N, rank)
  if (D == 64) LAUNCH_BWD(64); else if (D == 128) LAUNCH_BWD(128); else LAUNCH_BWD(256);
#undef LAUNCH_BWD
  SIMCLR_CHECK_LAUNCH();
  // d((1 / n) sum_i l_i) / dS_ia = (1 / (n T)) (softmax_a - [a in P(i)] / |P(i)|)
  const float coeff = grad_scale / (temperature * (float)n);
  const int blocks_q = ceil_div(2LL * n * (D / 4), 256), blocks_k = ceil_div(2LL * N * (D / 4), 256);
  hipLaunchKernelGGL(supcon_combine, dim3(blocks_q + blocks_k), dim3(256), 0, stream, gq, p.ksplit, p.rows_pad_q, 2 * n, gk, p.qsplit,
                     p.rows_pad_k, 2 * N, D, coeff, dz_local, dz_all, blocks_q);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
