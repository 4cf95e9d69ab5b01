// Hard-negative and debiased NT-Xent for gfx950: NT-Xent whose negative term is re-weighted towards the negatives close to the anchor
// (Robinson et al. 2021, Contrastive Learning with Hard Negative Samples: beta) and corrected for the expected share of false negatives
// (Chuang et al. 2020, Debiased Contrastive Learning: tau_plus).  The formulas below are this project's definition, not a parity claim.
//
// Layout as NT-Xent's (csrc/ntxent.hip): z_local [2n, D] = [view-a rows; view-b rows] of this replica, z_all [2N, D] = every replica's
// view-a rows, then every replica's view-b rows, N = R n.  Local row i (view v = i / n, sample s = i % n) has the own column
// self(i) = v N + rank n + s and the positive column pos(i) = (1 - v) N + rank n + s; Neg(i) = the other M = 2N - 2 columns.
// With a = 1 / T and s_ik = z_i . z_k:
//   p_i     = exp(a s_i,pos)
//   A_i     = sum_{k in Neg(i)} exp((1 + beta) a s_ik),   B_i = sum_{k in Neg(i)} exp(beta a s_ik)
//   G_raw_i = (M A_i / B_i - tau_plus M p_i) / (1 - tau_plus),   G_i = max(G_raw_i, M exp(-a))            (the floor)
//   l_i     = log(p_i + G_i) - a s_i,pos,   loss = (1 / n) sum_{i < 2n} l_i
// Gradient (the re-weighting is NOT stop-gradient), P1 / P0 the softmaxes over Neg(i) at scales (1 + beta) a / beta a:
//   above the floor: dl_i/ds_ik = a w_i ((1 + beta) P1_ik - beta P0_ik),  w_i = (M A_i / B_i) / ((1 - tau_plus)(p_i + G_i)),
//                    dl_i/ds_i,pos = a (p_i (1 - tau_plus M / (1 - tau_plus)) / (p_i + G_i) - 1)
//   on the floor:    dl_i/ds_ik = 0,  dl_i/ds_i,pos = a (p_i / (p_i + G_i) - 1)
//   dS_{i, self(i)} = 0,  dz_local = dS z_all,  dz_all = dS^T z_local
//
// The sweeps are csrc/supcon.hip's -- S = Q K^T tile by tile on v_mfma_f32_16x16x4_f32 (exact f32), 64-row swizzled LDS key tiles,
// key splits merged in a fixed order, the [2n, 2N] matrix never written, both backward sweeps in one launch, no atomics -- with one
// dot product pushing TWO online (max, sum) pairs, at the scales (1 + beta) a and beta a, each on its own rounded base-2 logit
// (sweep::logit2).  The beta a pair is skipped at beta == 0, where B_i = M exactly.  The positive's dot product is kept apart.
// The row finalize works in double and relative to c = max(log(M A / B), log p): G_raw cancels near the floor (fp32 would lose it
// there) and exp(a s) overflows fp32 at small T.  It decides whether the row is on the floor and stores the decision as the row's
// two gradient coefficients; the backward reads them and never re-decides.
//
// MFMA mapping, tile stager, S fragment and online (max, sum): csrc/sweep_tile.h.
#include "sweep_tile.h"

namespace {

using namespace sweep;

constexpr int kPart = 8;       // floats per (split, row) forward partial: {max1, sum1, max0, sum0, positive's dot product, -, -, -}

// own / positive global column of local row q (< 2n)
__device__ __forceinline__ int row_self(int q, int n, int N, int rank) { return q < n ? rank * n + q : N + rank * n + (q - n); }
__device__ __forceinline__ int row_pos(int q, int n, int N, int rank) { return q < n ? N + rank * n + q : rank * n + (q - n); }

// ---- forward: one partial per (key split, query row) over the split's columns of Neg(row) --------------------------------------------
// {running max, sum of exp2} of the logits at scale1 = (1 + beta) a log2(e) and (HARD) at scale0 = beta a log2(e); the positive's dot
template <int D, bool HARD>
__global__ __launch_bounds__(256) void hcl_fwd_partial(const float* __restrict__ zq, const float* __restrict__ zk, int two_n, int two_N,
                                                       int n, int N, int rank, float scale1, float scale0, int tiles_per_split,
                                                       float* __restrict__ part, int rows_pad) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, fl = lane & 15;
  const int q = blockIdx.x * kTile + wave * 16 + fl;
  const bool qv = q < two_n;
  float4 ff[D / 16];
  load_frag<D>(ff, zq, q, qv, g);
  const int self = qv ? row_self(q, n, N, rank) : -1;
  const int posc = qv ? row_pos(q, n, N, rank) : -1;
  float m1 = -INFINITY, l1 = 0.f, m0 = -INFINITY, l0 = 0.f, pdot = -INFINITY;
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
        const int col = col0 + r;
        if (col == posc) pdot = acc[r];
        if (col < two_N && col != self && col != posc) {   // a column of Neg(q)
          ml_push(m1, l1, logit2(acc[r], scale1, 0.f));
          if (HARD) ml_push(m0, l0, logit2(acc[r], scale0, 0.f));
        }
      }
    }
  }
  // the 4 lane groups that share this fixed row, in a fixed order
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {
    const float om1 = __shfl_xor(m1, o, 64), ol1 = __shfl_xor(l1, o, 64);
    const float om0 = __shfl_xor(m0, o, 64), ol0 = __shfl_xor(l0, o, 64);
    ml_merge(m1, l1, om1, ol1);
    ml_merge(m0, l0, om0, ol0);
    pdot = fmaxf(pdot, __shfl_xor(pdot, o, 64));          // one lane of one split holds it, the others -inf
  }
  if (g == 0 && qv) {
    float* p = part + ((size_t)blockIdx.y * rows_pad + q) * kPart;
    *(float4*)p = make_float4(m1, l1, m0, l0);
    *(float4*)(p + 4) = make_float4(pdot, 0.f, 0.f, 0.f);
  }
}

// merge the key splits of every query row (16 lanes per row, fixed xor tree), then the row's finalize in double:
// row_stats[row] = {lse1, lse0 (base 2), negative coefficient a w (0 on the floor), positive coefficient}, rowterm[row] = l_row,
// onfloor[row] = the floor decision
__global__ __launch_bounds__(256) void hcl_finalize_rows(const float* __restrict__ part, int nsplit, int rows_pad, int two_n, double M,
                                                         double a, double tau, int hard, float* __restrict__ row_stats,
                                                         double* __restrict__ rowterm, int* __restrict__ onfloor) {
  const int q = blockIdx.x * 16 + (threadIdx.x >> 4);
  const int j = threadIdx.x & 15;
  float m1 = -INFINITY, l1 = 0.f, m0 = -INFINITY, l0 = 0.f, pdot = -INFINITY;
  if (q < two_n) {
    for (int s = j; s < nsplit; s += 16) {
      const float* p = part + ((size_t)s * rows_pad + q) * kPart;
      const float4 v = *(const float4*)p;
      ml_merge(m1, l1, v.x, v.y);
      ml_merge(m0, l0, v.z, v.w);
      pdot = fmaxf(pdot, p[4]);
    }
  }
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) {
    const float om1 = __shfl_xor(m1, o, 64), ol1 = __shfl_xor(l1, o, 64);
    const float om0 = __shfl_xor(m0, o, 64), ol0 = __shfl_xor(l0, o, 64);
    ml_merge(m1, l1, om1, ol1);
    ml_merge(m0, l0, om0, ol0);
    pdot = fmaxf(pdot, __shfl_xor(pdot, o, 64));
  }
  if (j == 0 && q < two_n) {
    const double lse1 = (double)m1 + log2((double)l1);
    const double lse0 = hard ? (double)m0 + log2((double)l0) : log2(M);
    const double logr = log(M) + (lse1 - lse0) * kLn2d;       // log(M A / B)
    const double logp = a * (double)pdot;
    const double c = fmax(logr, logp);
    const double er = exp(logr - c), ep = exp(logp - c);      // everything below is relative to exp(c): nothing overflows
    const double graw = (er - tau * M * ep) / (1.0 - tau);    // cancels near the floor: double only
    const double flo = M * exp(-a - c);
    const bool fl = !(graw > flo);
    const double G = fl ? flo : graw;
    const double den = ep + G;
    rowterm[q] = c + log(den) - logp;
    onfloor[q] = fl ? 1 : 0;
    const double cneg = fl ? 0.0 : a * er / ((1.0 - tau) * den);
    const double cpos = fl ? a * (ep / den - 1.0) : a * (ep * (1.0 - tau * M / (1.0 - tau)) / den - 1.0);
    *(float4*)(row_stats + 4 * (size_t)q) = make_float4((float)lse1, (float)lse0, (float)cneg, (float)cpos);
  }
}

// out[0] = loss = sum(l_i) / n, out[1] = the share of the 2n rows on the floor -- one workgroup, fixed summation order, the count
// summed as integers
__global__ __launch_bounds__(256) void hcl_reduce_out(const double* __restrict__ rowterm, const int* __restrict__ onfloor, int two_n,
                                                      float* __restrict__ out) {
  __shared__ double sh_l[256];
  __shared__ int sh_f[256];
  double ls = 0.0;
  int fs = 0;
  for (int q = threadIdx.x; q < two_n; q += 256) {
    ls += rowterm[q];
    fs += onfloor[q];
  }
  sh_l[threadIdx.x] = ls; sh_f[threadIdx.x] = fs;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      sh_l[threadIdx.x] += sh_l[threadIdx.x + s];
      sh_f[threadIdx.x] += sh_f[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = (float)(sh_l[0] / (0.5 * (double)two_n));
    out[1] = (float)((double)sh_f[0] / (double)two_n);
  }
}

// ---- backward sweeps (recompute S).  QUERY_FIXED: fixed rows = queries, streamed = keys, gpart[split][q] = sum_keys dS[q, key] K[key];
// otherwise fixed rows = keys, streamed = queries, gpart[split][key] = sum_q dS[q, key] Q[q].
// dS[q, key] = cpos_q at key = pos(q), 0 at key = self(q), cneg_q ((1 + beta) exp2(t1 - lse1_q) - beta exp2(t0 - lse0_q)) elsewhere,
// t1 / t0 the forward's two rounded logits; the grad_scale / n factor is applied by the combine.
template <int D, bool QUERY_FIXED, bool HARD>
__device__ __forceinline__ void hcl_bwd_sweep_body(float* lds, const float* __restrict__ fixed_mat, int fixed_rows,
                                                   const float* __restrict__ stream_mat, int stream_rows, float scale1, float scale0,
                                                   float beta, const float* __restrict__ row_stats, int tiles_per_split,
                                                   float* __restrict__ gpart, int rows_pad, int n, int N, int rank) {
  float4* st_s = (float4*)(lds + kTile * D);   // [64] row_stats of the streamed queries (key-fixed mode)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, fl = lane & 15;
  const int f = blockIdx.x * kTile + wave * 16 + fl;
  const bool fv = f < fixed_rows;
  float4 ff[D / 16];
  load_frag<D>(ff, fixed_mat, f, fv, g);
  const float4 f_st = (QUERY_FIXED && fv) ? *(const float4*)(row_stats + 4 * (size_t)f) : make_float4(0.f, 0.f, 0.f, 0.f);
  const int f_self = (QUERY_FIXED && fv) ? row_self(f, n, N, rank) : -1;
  const int f_pos = (QUERY_FIXED && fv) ? row_pos(f, n, N, rank) : -1;
  const float beta1 = 1.f + beta;
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
      const int sr = kt * kTile + tid;
      st_s[tid] = sr < stream_rows ? *(const float4*)(row_stats + 4 * (size_t)sr) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      const f32x4 acc = s_frag<D>(lds, sub, fl, g, ff);
      const int s0 = kt * kTile + sub * 16 + g * 4;  // streamed row of acc[0]
      float ds[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float4 st = QUERY_FIXED ? f_st : st_s[sub * 16 + g * 4 + r];
        const int own = QUERY_FIXED ? f_self : row_self(s0 + r, n, N, rank);
        const int pc = QUERY_FIXED ? f_pos : row_pos(s0 + r, n, N, rank);
        const int col = QUERY_FIXED ? s0 + r : f;
        const bool live = fv && s0 + r < stream_rows && col != own;       // the query's own column: no gradient flows through it
        float w = st.z * beta1 * exp2f(logit2(acc[r], scale1, 0.f) - st.x);
        if (HARD) w -= st.z * beta * exp2f(logit2(acc[r], scale0, 0.f) - st.y);
        ds[r] = live ? (col == pc ? st.w : w) : 0.f;
      }
      // dF^T[d][fixed] += sum_streamed T[streamed][d] * dS[streamed][fixed]
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
  if (fv) {
    float* gp = gpart + ((size_t)blockIdx.y * rows_pad + f) * D;
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt)
      *(float4*)(gp + dt * 16 + 4 * g) = make_float4(dacc[dt][0], dacc[dt][1], dacc[dt][2], dacc[dt][3]);
  }
}

// both sweeps in one launch: blockIdx.z = 0 query-fixed, 1 key-fixed
template <int D, bool HARD>
__global__ __launch_bounds__(256) void hcl_bwd_sweeps(const float* __restrict__ z_local, const float* __restrict__ z_all, int two_n,
                                                      int two_N, float scale1, float scale0, float beta,
                                                      const float* __restrict__ row_stats, int tiles_k, int tiles_q,
                                                      float* __restrict__ gq, int rows_pad_q, float* __restrict__ gk, int rows_pad_k,
                                                      int gxq, int gyq, int gxk, int gyk, int n, int N, int rank) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  if (blockIdx.z == 0) {
    if ((int)blockIdx.x >= gxq || (int)blockIdx.y >= gyq) return;
    hcl_bwd_sweep_body<D, true, HARD>(lds, z_local, two_n, z_all, two_N, scale1, scale0, beta, row_stats, tiles_k, gq, rows_pad_q, n, N,
                                      rank);
  } else {
    if ((int)blockIdx.x >= gxk || (int)blockIdx.y >= gyk) return;
    hcl_bwd_sweep_body<D, false, HARD>(lds, z_all, two_N, z_local, two_n, scale1, scale0, beta, row_stats, tiles_q, gk, rows_pad_k, n, N,
                                       rank);
  }
}

// dz_local = coeff * sum_split gq, dz_all = coeff * sum_split gk; fixed split order
__global__ __launch_bounds__(256) void hcl_combine(const float* __restrict__ gq, int ksplit, int rows_pad_q, int rows_q,
                                                   const float* __restrict__ gk, int qsplit, int rows_pad_k, int rows_k, int D, float coeff,
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
// workspace layout (4-byte words, every offset a multiple of 64): [forward partials | gq | gk | row terms (double) | floor decisions]
size_t off_gq(const Plan& p) { return (size_t)p.fks * p.rows_pad_q * kPart; }
size_t off_gk(const Plan& p, int D) { return off_gq(p) + (size_t)p.ksplit * p.rows_pad_q * D; }
size_t off_rowterm(const Plan& p, int D) { return off_gk(p, D) + (size_t)p.qsplit * p.rows_pad_k * D; }
size_t off_floor(const Plan& p, int D) { return off_rowterm(p, D) + 2 * (size_t)p.rows_pad_q; }
size_t ws_words(int n, int N, int D) {
  const Plan p = make_plan(n, N);
  return off_floor(p, D) + (size_t)p.rows_pad_q;
}

bool shape_ok(int n, int N, int D) { return n > 0 && N >= 2 && N >= n && N % n == 0 && N <= (1 << 29) && dim_ok(D); }
// (NaN fails every comparison)
bool beta_ok(float beta) { return beta >= 0.f && beta <= 3.0e38f; }
bool tau_ok(float tau) { return tau >= 0.f && tau < 1.f; }

// base-2 logit scales of the two statistics, formed in double and rounded once
float scale_of(double factor, float temperature) { return (float)(factor * kLog2ed / (double)temperature); }

}  // namespace

extern "C" {

size_t simclr_hcl_workspace_bytes(int n, int N, int D) {
  if (!shape_ok(n, N, D)) return 0;
  return ws_words(n, N, D) * sizeof(float);
}

int simclr_hcl_fwd(const float* z_local, const float* z_all, int n, int N, int D, int rank, float temperature, float beta, float tau_plus,
                   float* out, float* row_stats, void* workspace, hipStream_t stream) {
  SIMCLR_CHECK_ARG(dim_ok(D), "hcl_fwd: D must be 64/128/256 (got %d)", D);
  SIMCLR_CHECK_ARG(shape_ok(n, N, D), "hcl_fwd: need n >= 1, N >= 2 and N = R*n (n=%d N=%d)", n, N);
  SIMCLR_CHECK_ARG(rank >= 0 && rank < N / n, "hcl_fwd: rank %d out of range", rank);
  SIMCLR_CHECK_ARG(pos_finite(temperature), "hcl_fwd: temperature must be > 0 and finite");
  SIMCLR_CHECK_ARG(beta_ok(beta), "hcl_fwd: beta must be >= 0 and finite");
  SIMCLR_CHECK_ARG(tau_ok(tau_plus), "hcl_fwd: tau_plus must lie in [0, 1)");
  SIMCLR_CHECK_ARG(al16(z_local) && al16(z_all) && al4(out) && al16(row_stats) && al16(workspace),
                   "hcl_fwd: null or misaligned argument");
  const Plan p = make_plan(n, N);
  float* part = (float*)workspace;
  const bool hard = beta != 0.f;
  const float scale1 = scale_of(1.0 + (double)beta, temperature), scale0 = scale_of((double)beta, temperature);
  const dim3 grid(p.rows_pad_q / kTile, p.fks);
  const size_t lds = (size_t)kTile * D * sizeof(float);
#define LAUNCH_FWD(DD, HH)                                                                                                              \
  hipLaunchKernelGGL((hcl_fwd_partial<DD, HH>), grid, dim3(256), lds, stream, z_local, z_all, 2 * n, 2 * N, n, N, rank, scale1, scale0, \
                     p.ftiles_k, part, p.rows_pad_q)
#define LAUNCH_FWD_D(DD) do { if (hard) LAUNCH_FWD(DD, true); else LAUNCH_FWD(DD, false); } while (0)
  if (D == 64) LAUNCH_FWD_D(64); else if (D == 128) LAUNCH_FWD_D(128); else LAUNCH_FWD_D(256);
#undef LAUNCH_FWD_D
#undef LAUNCH_FWD
  SIMCLR_CHECK_LAUNCH();
  double* rowterm = (double*)(part + off_rowterm(p, D));
  int* onfloor = (int*)(part + off_floor(p, D));
  hipLaunchKernelGGL(hcl_finalize_rows, dim3(ceil_div(2LL * n, 16)), dim3(256), 0, stream, part, p.fks, p.rows_pad_q, 2 * n,
                     2.0 * (double)N - 2.0, 1.0 / (double)temperature, (double)tau_plus, hard ? 1 : 0, row_stats, rowterm, onfloor);
  hipLaunchKernelGGL(hcl_reduce_out, dim3(1), dim3(256), 0, stream, rowterm, onfloor, 2 * n, out);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

int simclr_hcl_bwd(const float* z_local, const float* z_all, int n, int N, int D, int rank, float temperature, float beta, float tau_plus,
                   const float* row_stats, float grad_scale, float* dz_local, float* dz_all, void* workspace, hipStream_t stream) {
  SIMCLR_CHECK_ARG(dim_ok(D), "hcl_bwd: D must be 64/128/256 (got %d)", D);
  SIMCLR_CHECK_ARG(shape_ok(n, N, D), "hcl_bwd: need n >= 1, N >= 2 and N = R*n (n=%d N=%d)", n, N);
  SIMCLR_CHECK_ARG(rank >= 0 && rank < N / n, "hcl_bwd: rank %d out of range", rank);
  SIMCLR_CHECK_ARG(pos_finite(temperature), "hcl_bwd: temperature must be > 0 and finite");
  SIMCLR_CHECK_ARG(beta_ok(beta), "hcl_bwd: beta must be >= 0 and finite");
  SIMCLR_CHECK_ARG(tau_ok(tau_plus), "hcl_bwd: tau_plus must lie in [0, 1)");
  SIMCLR_CHECK_ARG(al16(z_local) && al16(z_all) && al16(row_stats) && al16(dz_local) && al16(dz_all) && al16(workspace),
                   "hcl_bwd: null or misaligned argument");
  const Plan p = make_plan(n, N);
  float* part = (float*)workspace;
  float* gq = part + off_gq(p);
  float* gk = part + off_gk(p, D);
  const bool hard = beta != 0.f;
  const float scale1 = scale_of(1.0 + (double)beta, temperature), scale0 = scale_of((double)beta, temperature);
  const size_t lds = (size_t)(kTile * D + 4 * kTile) * sizeof(float);
  const dim3 gridq(p.rows_pad_q / kTile, p.ksplit), gridk(p.rows_pad_k / kTile, p.qsplit);
  const dim3 gridb(max(gridq.x, gridk.x), max(gridq.y, gridk.y), 2);
#define LAUNCH_BWD(DD, HH)                                                                                                            \
  do {                                                                                                                                \
    SIMCLR_CHECK_ARG(raise_lds(hcl_bwd_sweeps<DD, HH>, lds), "hcl_bwd: %d bytes of LDS refused", (int)lds);                           \
    hipLaunchKernelGGL((hcl_bwd_sweeps<DD, HH>), gridb, dim3(256), lds, stream, z_local, z_all, 2 * n, 2 * N, scale1, scale0, beta,   \
                       row_stats, p.tiles_k, p.tiles_q, gq, p.rows_pad_q, gk, p.rows_pad_k, (int)gridq.x, (int)gridq.y, (int)gridk.x, \
                       (int)gridk.y, n, N, rank);                                                                                     \
  } while (0)
#define LAUNCH_BWD_D(DD) do { if (hard) LAUNCH_BWD(DD, true); else LAUNCH_BWD(DD, false); } while (0)
  if (D == 64) LAUNCH_BWD_D(64); else if (D == 128) LAUNCH_BWD_D(128); else LAUNCH_BWD_D(256);
#undef LAUNCH_BWD_D
#undef LAUNCH_BWD
  SIMCLR_CHECK_LAUNCH();
  // d((1 / n) sum_i l_i) / dS: the row coefficients carry a = 1 / T already
  const float coeff = grad_scale / (float)n;
  const int blocks_q = ceil_div(2LL * n * (D / 4), 256), blocks_k = ceil_div(2LL * N * (D / 4), 256);
  hipLaunchKernelGGL(hcl_combine, dim3(blocks_q + blocks_k), dim3(256), 0, stream, gq, p.ksplit, p.rows_pad_q, 2 * n, gk, p.qsplit,
                     p.rows_pad_k, 2 * N, D, coeff, dz_local, dz_all, blocks_q);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
