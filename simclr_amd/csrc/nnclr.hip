// NNCLR for gfx950 (after Dwibedi et al. 2021, With a Little Help from My Friends: Nearest-Neighbor Contrastive Learning of Visual
// Representations): NT-Xent whose anchor is not the row itself but its nearest neighbour in a support queue of past embeddings.  The
// form below is this project's definition, written from memory of the paper, not a parity claim.
//
// Layout: nn_local [2n, D] = the neighbour row of every local row (view-a rows, then view-b rows; constants: no gradient), z_all [2N, D]
// = every replica's view-a rows, then every replica's view-b rows, N = R n.  Local row r (view v = r / n, sample s = r % n) contrasts
// its neighbour against the N columns of the OTHER view, C(r) = [(1 - v) N, (1 - v) N + N), with the positive p(r) = (1 - v) N + rank n + s.
// With a = 1 / T:
//   l_r  = logsumexp_{c in C(r)}(a nn_r . z_all[c]) - a nn_r . z_all[p(r)],   loss = (1 / n) sum_{r < 2n} l_r
//   d loss / d z_all[c] = (a / n) sum_{r : c in C(r)} (P_rc - [c = p(r)]) nn_r,   P_r = the softmax over C(r)
// Rows and columns are different matrices and only the columns carry gradient, so the backward is ONE sweep (the key-fixed one of
// csrc/hcl.hip): a workgroup owns 64 columns and streams the neighbour rows of the opposite view.
//
// The sweeps are csrc/supcon.hip's -- S tile by tile on v_mfma_f32_16x16x4_f32 (exact f32), 64-row swizzled LDS tiles, online (max, sum)
// on the rounded base-2 logit (sweep::logit2), splits merged in a fixed order, nothing of the [2n, N] matrix written, no atomics.  A
// 64-row workgroup may straddle the view boundary: it then streams both views' tiles and every row masks by its own view; a workgroup
// inside one view streams that view's candidate tiles only.  The row finalize works in double.
//
// MFMA mapping, tile stager, S fragment and online (max, sum): csrc/sweep_tile.h.
#include "sweep_tile.h"
#include <limits.h>

namespace {

using namespace sweep;

// floats per (split, row) forward partial: {max, sum but one maximum, positive's dot product, best logit, its column, -, -, -}
constexpr int kPart = 8;

// first candidate column / positive column of local row q (< 2n)
__device__ __forceinline__ int row_lo(int q, int n, int N) { return q < n ? N : 0; }
__device__ __forceinline__ int row_pos(int q, int n, int N, int rank) { return q < n ? N + rank * n + q : rank * n + (q - n); }

// (value, column) of the maximum, ties to the lowest column
__device__ __forceinline__ void best_merge(float& bv, int& bi, float ov, int oi) {
  if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
}

// the tiles [begin, end) of the streamed side this workgroup's split sweeps: the rows [lo, hi) cut into `nsplit` runs of whole tiles
__device__ __forceinline__ void split_tiles(int lo, int hi, int nsplit, int split, int& begin, int& end) {
  const int t0 = lo / kTile, t1 = (hi + kTile - 1) / kTile;
  const int per = (t1 - t0 + nsplit - 1) / nsplit;
  begin = t0 + split * per;
  end = min(t1, begin + per);
}

// ---- forward: one partial per (column split, neighbour row) over the split's columns of C(row) -----------------------------------------
template <int D>
__global__ __launch_bounds__(256) void nnclr_fwd_partial(const float* __restrict__ nn, const float* __restrict__ zk, int two_n, int two_N,
                                                         int n, int N, int rank, float scale2, float* __restrict__ part, int rows_pad) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, fl = lane & 15;
  const int q = blockIdx.x * kTile + wave * 16 + fl;
  const bool qv = q < two_n;
  float4 ff[D / 16];
  load_frag<D>(ff, nn, q, qv, g);
  const int lo = qv ? row_lo(q, n, N) : 0;
  const int hi = qv ? lo + N : 0;                              // an invalid row has no candidate
  const int posc = qv ? row_pos(q, n, N, rank) : -1;
  // the workgroup's columns: one view's when all its rows lie in one view, both otherwise
  const int q_first = blockIdx.x * kTile, q_last = min(q_first + kTile, two_n) - 1;
  const bool one_view = (q_first < n) == (q_last < n);
  const int wg_lo = one_view ? row_lo(q_first, n, N) : 0, wg_hi = one_view ? wg_lo + N : two_N;
  int tile_begin, tile_end;
  split_tiles(wg_lo, wg_hi, gridDim.y, blockIdx.y, tile_begin, tile_end);
  float m = -INFINITY, l = 0.f, pdot = -INFINITY, bv = -INFINITY;
  int bi = INT_MAX;
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
        if (col >= lo && col < hi) {                           // a column of C(q): the row's own view mask
          const float t = logit2(acc[r], scale2, 0.f);
          mr_push(m, l, t);
          if (t > bv) { bv = t; bi = col; }                    // a lane meets its columns in ascending order
          if (col == posc) pdot = acc[r];
        }
      }
    }
  }
  // the 4 lane groups that share this fixed row, in a fixed order
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {
    const float om = __shfl_xor(m, o, 64), ol = __shfl_xor(l, o, 64);
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    mr_merge(m, l, om, ol);
    best_merge(bv, bi, ov, oi);
    pdot = fmaxf(pdot, __shfl_xor(pdot, o, 64));               // one lane of one split holds it, the others -inf
  }
  if (g == 0 && qv) {
    float* p = part + ((size_t)blockIdx.y * rows_pad + q) * kPart;
    *(float4*)p = make_float4(m, l, pdot, bv);
    *(float4*)(p + 4) = make_float4(__int_as_float(bi), 0.f, 0.f, 0.f);
  }
}

// merge the column splits of every row (16 lanes per row, fixed xor tree), then the row's finalize in double:
// row_stats[row] = {lse (base 2) as a float, what the float left of it, 1 - P_row,pos, z_row . nn_row};
// rowterm[row] = {l_row, z_row . nn_row}; hit[row] = 1 when the positive is the lowest-index maximum of C(row).
// l_row = ln 2 (lse - t_pos) on the positive's ROUNDED logit, the number the (max, sum) was formed from: where the positive carries
// nearly all of the softmax the difference is log(1 + the rest), which the (max, rest) pair of sweep::mr_push keeps to float32's
// relative precision.  The backward reads P_pos - 1 from here (formed with expm1 in double) instead of cancelling exp2(..) - 1, and
// forms every other P from lse in two floats.
template <int D>
__global__ __launch_bounds__(256) void nnclr_finalize_rows(const float* __restrict__ part, int nsplit, int rows_pad, int two_n, int n, int N,
                                                           int rank, float scale2, const float* __restrict__ z_local,
                                                           const float* __restrict__ nn, float* __restrict__ row_stats,
                                                           double* __restrict__ rowterm, int* __restrict__ hit) {
  const int q = blockIdx.x * 16 + (threadIdx.x >> 4);
  const int j = threadIdx.x & 15;
  float m = -INFINITY, l = 0.f, pdot = -INFINITY, bv = -INFINITY;
  int bi = INT_MAX;
  double sim = 0.0;
  if (q < two_n) {
    for (int s = j; s < nsplit; s += 16) {
      const float* p = part + ((size_t)s * rows_pad + q) * kPart;
      const float4 v = *(const float4*)p;
      mr_merge(m, l, v.x, v.y);
      pdot = fmaxf(pdot, v.z);
      best_merge(bv, bi, v.w, __float_as_int(p[4]));
    }
    for (int d = j; d < D; d += 16) sim += (double)z_local[(size_t)q * D + d] * (double)nn[(size_t)q * D + d];
  }
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) {
    const float om = __shfl_xor(m, o, 64), ol = __shfl_xor(l, o, 64);
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    mr_merge(m, l, om, ol);
    best_merge(bv, bi, ov, oi);
    pdot = fmaxf(pdot, __shfl_xor(pdot, o, 64));
    sim += __shfl_xor(sim, o, 64);
  }
  if (j == 0 && q < two_n) {
    const double lse2 = (double)m + log1p((double)l) * kLog2ed;   // the sum is 1 + l: a near-one-hot row keeps its small mass
    const float tpos = logit2(pdot, scale2, 0.f);
    const double lr = (lse2 - (double)tpos) * kLn2d;
    const float lse_hi = (float)lse2;
    rowterm[2 * (size_t)q] = lr;
    rowterm[2 * (size_t)q + 1] = sim;
    hit[q] = bi == row_pos(q, n, N, rank) ? 1 : 0;
    const double one_minus_ppos = -expm1(((double)tpos - lse2) * kLn2d);
    *(float4*)(row_stats + 4 * (size_t)q) = make_float4(lse_hi, (float)(lse2 - (double)lse_hi), (float)one_minus_ppos, (float)sim);
  }
}

// out[0] = the replica's loss share = sum(l_r) / n, out[1] = the share of the 2n rows whose positive wins, out[2] = mean z_r . nn_r --
// one workgroup, fixed summation order, the count summed as integers
__global__ __launch_bounds__(256) void nnclr_reduce_out(const double* __restrict__ rowterm, const int* __restrict__ hit, int two_n,
                                                        float* __restrict__ out) {
  __shared__ double sh_l[256];
  __shared__ double sh_s[256];
  __shared__ int sh_h[256];
  double ls = 0.0, ss = 0.0;
  int hs = 0;
  for (int q = threadIdx.x; q < two_n; q += 256) {
    ls += rowterm[2 * (size_t)q];
    ss += rowterm[2 * (size_t)q + 1];
    hs += hit[q];
  }
  sh_l[threadIdx.x] = ls; sh_s[threadIdx.x] = ss; sh_h[threadIdx.x] = hs;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      sh_l[threadIdx.x] += sh_l[threadIdx.x + s];
      sh_s[threadIdx.x] += sh_s[threadIdx.x + s];
      sh_h[threadIdx.x] += sh_h[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = (float)(sh_l[0] / (0.5 * (double)two_n));
    out[1] = (float)((double)sh_h[0] / (double)two_n);
    out[2] = (float)(sh_s[0] / (double)two_n);
  }
}

// ---- backward: the key-side sweep (recompute S).  Fixed rows = 64 columns of z_all, streamed = the neighbour rows of the opposite view:
// gpart[split][c] = sum_r dS[r, c] nn_r,  dS[r, c] = exp2((t_rc - lse_hi_r) - lse_lo_r) for c in C(r) but p(r), the stored P_pos - 1 at
// c = p(r), 0 elsewhere, t the forward's rounded logit; the grad_scale a / n factor is applied by the combine.
template <int D>
__global__ __launch_bounds__(256) void nnclr_bwd_sweep(const float* __restrict__ z_all, const float* __restrict__ nn, int two_n, int two_N,
                                                       int n, int N, int rank, float scale2, const float* __restrict__ row_stats,
                                                       float* __restrict__ gpart, int rows_pad) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float4* st_s = (float4*)(lds + kTile * D);   // [64] row_stats of the streamed neighbour rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, fl = lane & 15;
  const int f = blockIdx.x * kTile + wave * 16 + fl;
  const bool fv = f < two_N;
  float4 ff[D / 16];
  load_frag<D>(ff, z_all, f, fv, g);
  const bool f_view = f >= N;                  // the column's view: its rows are the neighbour rows of the other one
  // the workgroup's neighbour rows: one view's when all its columns lie in one view, both otherwise
  const int c_first = blockIdx.x * kTile, c_last = min(c_first + kTile, two_N) - 1;
  const bool one_view = (c_first < N) == (c_last < N);
  const int wg_lo = one_view ? (c_first < N ? n : 0) : 0, wg_hi = one_view ? wg_lo + n : two_n;
  int tile_begin, tile_end;
  split_tiles(wg_lo, wg_hi, gridDim.y, blockIdx.y, tile_begin, tile_end);
  f32x4 dacc[D / 16];
#pragma unroll
  for (int i = 0; i < D / 16; ++i) dacc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int kt = tile_begin; kt < tile_end; ++kt) {
    __syncthreads();
    load_tile<D>(lds, nn, kt * kTile, two_n, tid);
    if (tid < kTile) {
      const int sr = kt * kTile + tid;
      st_s[tid] = sr < two_n ? *(const float4*)(row_stats + 4 * (size_t)sr) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      const f32x4 acc = s_frag<D>(lds, sub, fl, g, ff);
      const int s0 = kt * kTile + sub * 16 + g * 4;  // streamed row of acc[0]
      float ds[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int sr = s0 + r;
        const bool live = fv && sr < two_n && (sr >= n) != f_view;          // the column lies in C(sr): the row's own view mask
        const float4 st = st_s[sub * 16 + g * 4 + r];
        const float w = exp2f((logit2(acc[r], scale2, 0.f) - st.x) - st.y);
        ds[r] = live ? (f == row_pos(sr, n, N, rank) ? -st.z : w) : 0.f;
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

// dz_all = coeff * sum_split gpart; fixed split order
__global__ __launch_bounds__(256) void nnclr_combine(const float* __restrict__ gp, int nsplit, int rows_pad, int rows, int D, float coeff,
                                                     float* __restrict__ dz_all) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)rows * (D / 4)) return;
  const int r = (int)(i / (D / 4)), c = (int)(i % (D / 4));
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int s = 0; s < nsplit; ++s) {
    const float4 v = *(const float4*)(gp + ((size_t)s * rows_pad + r) * D + c * 4);
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  *(float4*)(dz_all + (size_t)r * D + c * 4) = make_float4(acc.x * coeff, acc.y * coeff, acc.z * coeff, acc.w * coeff);
}

// fks: column split of the forward sweep (~512 workgroups); qsplit: row split of the backward sweep (~256), the targets
// csrc/ntxent.hip measured for the same sweeps.  A workgroup inside one view has ceil(N / 64) (+1 unaligned) column tiles and
// ceil(n / 64) (+1) row tiles to cut.
struct Plan { int rows_pad_q, rows_pad_k, fks, qsplit; };
Plan make_plan(int n, int N) {
  Plan p;
  const int qtiles = ceil_div(2LL * n, kTile), ktiles = ceil_div(2LL * N, kTile);
  p.rows_pad_q = qtiles * kTile;
  p.rows_pad_k = ktiles * kTile;
  constexpr int wgs_f = 512, wgs_b = 256;
  p.fks = max(1, min((int)ceil_div((long long)N, kTile), wgs_f / max(1, qtiles)));
  p.qsplit = max(1, min((int)ceil_div((long long)n, kTile), wgs_b / max(1, ktiles)));
  return p;
}
// workspace layout (4-byte words, every offset a multiple of 64): [forward partials | gk | row terms (2 doubles a row) | hits]
size_t off_gk(const Plan& p) { return (size_t)p.fks * p.rows_pad_q * kPart; }
size_t off_rowterm(const Plan& p, int D) { return off_gk(p) + (size_t)p.qsplit * p.rows_pad_k * D; }
size_t off_hit(const Plan& p, int D) { return off_rowterm(p, D) + 4 * (size_t)p.rows_pad_q; }
size_t ws_words(int n, int N, int D) {
  const Plan p = make_plan(n, N);
  return off_hit(p, D) + (size_t)p.rows_pad_q;
}

bool shape_ok(int n, int N, int D) { return n > 0 && N >= 2 && N >= n && N % n == 0 && N <= (1 << 29) && dim_ok(D); }

}  // namespace

extern "C" {

size_t simclr_nnclr_workspace_bytes(int n, int N, int D) {
  if (!shape_ok(n, N, D)) return 0;
  return ws_words(n, N, D) * sizeof(float);
}

int simclr_nnclr_fwd(const float* nn_local, const float* z_local, const float* z_all, int n, int N, int D, int rank, float temperature,
                     float* out, float* row_stats, void* workspace, hipStream_t stream) {
  SIMCLR_CHECK_ARG(dim_ok(D), "nnclr_fwd: D must be 64/128/256 (got %d)", D);
  SIMCLR_CHECK_ARG(shape_ok(n, N, D), "nnclr_fwd: need n >= 1, N >= 2 and N = R*n (n=%d N=%d)", n, N);
  SIMCLR_CHECK_ARG(rank >= 0 && rank < N / n, "nnclr_fwd: rank %d out of range", rank);
  SIMCLR_CHECK_ARG(pos_finite(temperature), "nnclr_fwd: temperature must be > 0 and finite");
  SIMCLR_CHECK_ARG(al16(nn_local) && al16(z_local) && al16(z_all) && al4(out) && al16(row_stats) && al16(workspace),
                   "nnclr_fwd: null or misaligned argument");
  const Plan p = make_plan(n, N);
  float* part = (float*)workspace;
  const float scale2 = (float)(kLog2ed / (double)temperature);
  const dim3 grid(p.rows_pad_q / kTile, p.fks);
  const size_t lds = (size_t)kTile * D * sizeof(float);
#define LAUNCH_FWD(DD)                                                                                                               \
  hipLaunchKernelGGL((nnclr_fwd_partial<DD>), grid, dim3(256), lds, stream, nn_local, z_all, 2 * n, 2 * N, n, N, rank, scale2, part, \
                     p.rows_pad_q)
  if (D == 64) LAUNCH_FWD(64); else if (D == 128) LAUNCH_FWD(128); else LAUNCH_FWD(256);
#undef LAUNCH_FWD
  SIMCLR_CHECK_LAUNCH();
  double* rowterm = (double*)(part + off_rowterm(p, D));
  int* hit = (int*)(part + off_hit(p, D));
  const dim3 gridf(ceil_div(2LL * n, 16));
#define LAUNCH_FIN(DD)                                                                                                                \
  hipLaunchKernelGGL((nnclr_finalize_rows<DD>), gridf, dim3(256), 0, stream, part, p.fks, p.rows_pad_q, 2 * n, n, N, rank,            \
                     scale2, z_local, nn_local, row_stats, rowterm, hit)
  if (D == 64) LAUNCH_FIN(64); else if (D == 128) LAUNCH_FIN(128); else LAUNCH_FIN(256);
#undef LAUNCH_FIN
  hipLaunchKernelGGL(nnclr_reduce_out, dim3(1), dim3(256), 0, stream, rowterm, hit, 2 * n, out);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

int simclr_nnclr_bwd(const float* nn_local, const float* z_all, int n, int N, int D, int rank, float temperature, const float* row_stats,
                     float grad_scale, float* dz_all, void* workspace, hipStream_t stream) {
  SIMCLR_CHECK_ARG(dim_ok(D), "nnclr_bwd: D must be 64/128/256 (got %d)", D);
  SIMCLR_CHECK_ARG(shape_ok(n, N, D), "nnclr_bwd: need n >= 1, N >= 2 and N = R*n (n=%d N=%d)", n, N);
  SIMCLR_CHECK_ARG(rank >= 0 && rank < N / n, "nnclr_bwd: rank %d out of range", rank);
  SIMCLR_CHECK_ARG(pos_finite(temperature), "nnclr_bwd: temperature must be > 0 and finite");
  SIMCLR_CHECK_ARG(al16(nn_local) && al16(z_all) && al16(row_stats) && al16(dz_all) && al16(workspace),
                   "nnclr_bwd: null or misaligned argument");
  const Plan p = make_plan(n, N);
  float* gk = (float*)workspace + off_gk(p);
  const float scale2 = (float)(kLog2ed / (double)temperature);
  const size_t lds = (size_t)(kTile * D + 4 * kTile) * sizeof(float);
  const dim3 grid(p.rows_pad_k / kTile, p.qsplit);
#define LAUNCH_BWD(DD)                                                                                                            \
  do {                                                                                                                            \
    SIMCLR_CHECK_ARG(raise_lds(nnclr_bwd_sweep<DD>, lds), "nnclr_bwd: %d bytes of LDS refused", (int)lds);                        \
    hipLaunchKernelGGL((nnclr_bwd_sweep<DD>), grid, dim3(256), lds, stream, z_all, nn_local, 2 * n, 2 * N, n, N, rank, scale2,    \
                       row_stats, gk, p.rows_pad_k);                                                                              \
  } while (0)
  if (D == 64) LAUNCH_BWD(64); else if (D == 128) LAUNCH_BWD(128); else LAUNCH_BWD(256);
#undef LAUNCH_BWD
  SIMCLR_CHECK_LAUNCH();
  // d((1 / n) sum_r l_r) / dS = (a / n) (P - [c = p(r)])
  const float coeff = (float)((double)grad_scale / ((double)temperature * (double)n));
  const long long blocks = ceil_div(2LL * N * (D / 4), 256);
  hipLaunchKernelGGL(nnclr_combine, dim3((unsigned)blocks), dim3(256), 0, stream, gk, p.qsplit, p.rows_pad_k, 2 * N, D, coeff, dz_all);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
