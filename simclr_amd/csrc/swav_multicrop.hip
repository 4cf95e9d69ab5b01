// SwAV multi-crop (Caron et al. 2020, section 4; the official main_swav.py loss with crops_for_assign = [0, 1]) for gfx950: the
// cross-entropy of every LOCAL (low-resolution) view's K-way softmax against the Sinkhorn codes of BOTH global views of its image.
//
//   x [L b, D] = the l2-normalised local rows, view-major (row v b + i = local view v of image i);  w [K, D] = the prototypes;
//   z [2b, D] = the normalised GLOBAL rows, u [2b, D] = sum_j Pt[g, j] w_j their code expectations (csrc/swav.hip keeps both);
//   s_rj = x_r . w_j / T,  Ps = softmax_j(s_r),  i = r mod b,  V = 2 + L,  c = 1 / (2 (V - 1) b)
//   out = c sum_r (2 lse(s_r) - x_r . (u_i + u_{b+i}) / T)              (sum_j Pt[g, j] s_rj = x_r . u_g / T: no code is recomputed)
//   d out / d x_r = (c / T) (2 sum_j Ps[r, j] w_j - u_i - u_{b+i})
//   d out / d w_j = (c / T) (sum_r 2 Ps[r, j] x_r - sum_{g < 2b} Pt[g, j] m_g),   m_g = sum_v x_{v b + (g mod b)}
// The codes come from the two global views alone and are stop-gradient; the local rows take no part in the Sinkhorn.
//
// The sweeps are csrc/swav.hip's: S = X W^T tile by tile on v_mfma_f32_16x16x4_f32 (exact f32), 64 fixed rows per workgroup held as
// MFMA fragments, 64-row XOR-swizzled LDS tiles, online statistics in the base-2 domain on the ROUNDED logit, splits merged in a fixed
// order, no atomics: two calls are bitwise equal.  The code logit of the key-side sweep is the one csrc/swav.hip's statistics sweep
// rounded (the same dot product order, the same two roundings), so the lse_t of simclr_swav_fwd's row_stats normalises it.
//
// MFMA mapping, tile stager (plain and WRAPPED rows), S fragment, rounded logit and the (m, r) row statistics: csrc/sweep_tile.h.
#include "sweep_tile.h"

namespace {

using namespace sweep;

constexpr int kMaxK = 1 << 20;
constexpr int kMaxRows = 1 << 22;

// ---- statistics sweep: part[split][row] = the online (max, non-maximum mass) of s2_rj over the split's prototypes ------------------
template <int D>
__global__ __launch_bounds__(256) void swavl_stats_sweep(const float* __restrict__ x, const float* __restrict__ w, int rows, int K,
                                                         float scale2, int tiles_per_split, float* __restrict__ part, int rows_pad) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, fl = lane & 15;
  const int row = blockIdx.x * kTile + wave * 16 + fl;
  const bool rv = row < rows;
  float4 ff[D / 16];
  load_frag<D>(ff, x, row, rv, g);
  float ms = -INFINITY, rs = 0.f;
  const int ntiles = (K + kTile - 1) / kTile;
  const int tile_begin = blockIdx.y * tiles_per_split;
  const int tile_end = min(ntiles, tile_begin + tiles_per_split);
  for (int kt = tile_begin; kt < tile_end; ++kt) {
    __syncthreads();
    load_tile<D>(lds, w, kt * kTile, K, tid);
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      const f32x4 acc = s_frag<D>(lds, sub, fl, g, ff);
      const int col0 = kt * kTile + sub * 16 + g * 4;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (col0 + i < K) mr_push(ms, rs, logit2(acc[i], scale2, 0.f));   // the ragged last tile: rows past the table count nowhere
      }
    }
  }
  // the 4 lane groups that share this row, in a fixed order
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {
    const float oms = __shfl_xor(ms, o, 64), ors = __shfl_xor(rs, o, 64);
    mr_merge(ms, rs, oms, ors);
  }
  if (g == 0 && rv) *(float2*)(part + ((size_t)blockIdx.y * rows_pad + row) * 2) = make_float2(ms, rs);
}

// Merge the key splits of every row (16 lanes per row, fixed xor trees), then in double with i = r mod b:
//   row_stats[r] = lse_s in the base-2 domain (m + log2(1 + r) via log1p),   rowterm[r] = 2 lse_s ln 2 - x_r . (u_i + u_{b+i}) / T
template <int D>
__global__ __launch_bounds__(256) void swavl_finalize_rows(const float* __restrict__ part, int nsplit, int rows_pad, int rows, int b,
                                                           const float* __restrict__ x, const float* __restrict__ u, double inv_t,
                                                           float* __restrict__ row_stats, double* __restrict__ rowterm) {
  const int r = blockIdx.x * 16 + (threadIdx.x >> 4);
  const int j = threadIdx.x & 15;
  float ms = -INFINITY, rs = 0.f;
  double dot = 0.0;
  if (r < rows) {
    for (int s = j; s < nsplit; s += 16) {
      const float2 v = *(const float2*)(part + ((size_t)s * rows_pad + r) * 2);
      mr_merge(ms, rs, v.x, v.y);
    }
    const int i = r % b;
    const float4* xr = (const float4*)(x + (size_t)r * D);
    const float4* ua = (const float4*)(u + (size_t)i * D);
    const float4* ub = (const float4*)(u + (size_t)(b + i) * D);
#pragma unroll
    for (int k = 0; k < D / 64; ++k) {
      const float4 a = xr[j + 16 * k], p = ua[j + 16 * k], q = ub[j + 16 * k];
      dot += (double)a.x * ((double)p.x + (double)q.x) + (double)a.y * ((double)p.y + (double)q.y) +
             (double)a.z * ((double)p.z + (double)q.z) + (double)a.w * ((double)p.w + (double)q.w);
    }
  }
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) {
    const float oms = __shfl_xor(ms, o, 64), ors = __shfl_xor(rs, o, 64);
    mr_merge(ms, rs, oms, ors);
    dot += __shfl_xor(dot, o, 64);
  }
  if (j == 0 && r < rows) {
    const double lse = (double)ms + log1p((double)rs) * kLog2ed;
    row_stats[r] = (float)lse;
    rowterm[r] = 2.0 * lse * kLn2d - dot * inv_t;
  }
}

// out[0] = sum(rowterm) / denom -- one workgroup: thread i adds rows i, i + 256, ... in double, then a fixed binary tree
__global__ __launch_bounds__(256) void swavl_reduce_out(const double* __restrict__ rowterm, int rows, double denom,
                                                        float* __restrict__ out) {
  __shared__ double sh[256];
  double s = 0.0;
  for (int r = threadIdx.x; r < rows; r += 256) s += rowterm[r];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) sh[threadIdx.x] += sh[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (float)(sh[0] / denom);
}

// ---- probability sweep (recomputes the logits): gpart[split][row] = sum over the split's prototypes j of Ps[row, j] w_j ------------
template <int D>
__global__ __launch_bounds__(256) void swavl_prob_sweep(const float* __restrict__ x, const float* __restrict__ w, int rows, int K,
                                                        float scale2, const float* __restrict__ row_stats, int tiles_per_split,
                                                        float* __restrict__ gpart, int rows_pad) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, fl = lane & 15;
  const int row = blockIdx.x * kTile + wave * 16 + fl;
  const bool rv = row < rows;
  float4 ff[D / 16];
  load_frag<D>(ff, x, row, rv, g);
  const float lse = rv ? row_stats[row] : 0.f;
  f32x4 dacc[D / 16];
#pragma unroll
  for (int i = 0; i < D / 16; ++i) dacc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int ntiles = (K + kTile - 1) / kTile;
  const int tile_begin = blockIdx.y * tiles_per_split;
  const int tile_end = min(ntiles, tile_begin + tiles_per_split);
  for (int kt = tile_begin; kt < tile_end; ++kt) {
    __syncthreads();
    load_tile<D>(lds, w, kt * kTile, K, tid);
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      const f32x4 acc = s_frag<D>(lds, sub, fl, g, ff);
      const int col0 = kt * kTile + sub * 16 + g * 4;  // prototype of acc[0]
      float ds[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float t = logit2(acc[i], scale2, 0.f);   // the statistics sweep's rounded logit
        ds[i] = (rv && col0 + i < K) ? exp2f(t - lse) : 0.f;
      }
      // G^T[d][fixed row] += sum_proto w[proto][d] * Ps[proto][fixed row]
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int srow = sub * 16 + 4 * g + k;
          const int dcol = dt * 16 + fl;
          const float av = lds[srow * D + ((((dcol >> 2) ^ (srow & 15)) << 2) | (dcol & 3))];
          dacc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, ds[k], dacc[dt], 0, 0, 0);
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

// dx_r = coeff * (2 sum_split gpart[split][r] - u_i - u_{b+i}), i = r mod b, in a fixed split order; one 16-byte chunk per thread
__global__ __launch_bounds__(256) void swavl_combine_x(const float* __restrict__ gpart, int nsplit, int rows_pad, int rows, int b, int D,
                                                       const float* __restrict__ u, float coeff, float* __restrict__ dst) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const int C = D / 4;
  if (idx >= (long long)rows * C) return;
  const int r = (int)(idx / C), c = (int)(idx % C);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int s = 0; s < nsplit; ++s) {
    const float4 v = *(const float4*)(gpart + ((size_t)s * rows_pad + r) * D + c * 4);
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  const int i = r % b;
  const float4 ua = *(const float4*)(u + (size_t)i * D + c * 4);
  const float4 ub = *(const float4*)(u + (size_t)(b + i) * D + c * 4);
  acc.x = 2.f * acc.x - ua.x - ub.x; acc.y = 2.f * acc.y - ua.y - ub.y;
  acc.z = 2.f * acc.z - ua.z - ub.z; acc.w = 2.f * acc.w - ua.w - ub.w;
  *(float4*)(dst + (size_t)r * D + c * 4) = make_float4(coeff * acc.x, coeff * acc.y, coeff * acc.z, coeff * acc.w);
}

// m [b, D]: m_i = x_i + x_{b+i} + ... + x_{(L-1) b + i}, the views added in the order 0, 1, ...; one 16-byte chunk per thread
__global__ __launch_bounds__(256) void swavl_build_m(const float* __restrict__ x, int b, int L, int D, float* __restrict__ m) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const int C = D / 4;
  if (idx >= (long long)b * C) return;
  float4 acc = *(const float4*)(x + idx * 4);
  for (int v = 1; v < L; ++v) {
    const float4 t = *(const float4*)(x + ((size_t)v * b * C + idx) * 4);
    acc.x += t.x; acc.y += t.y; acc.z += t.z; acc.w += t.w;
  }
  *(float4*)(m + idx * 4) = acc;
}

// ---- key-side backward sweeps: a workgroup owns 64 prototypes (one fragment set) and streams 64-row tiles -------------------------
// CODE = false, the student term: wpart[split][j] = sum over the split's LOCAL rows r of Ps[r, j] x_r; rows = L b, row_stats [rows].
// CODE = true, the code term: wpart[split][j] = sum over the split's GLOBAL rows g of Pt[g, j] m_{g mod b}; src = z [2b, D] gives the
//   logits (alpha of the row's OWN view, lse_t = row_stats[2 g + 1] of simclr_swav_fwd), mult = m [b, D] is the multiplier tile.
template <int D, bool CODE>
__global__ __launch_bounds__(256) void swavl_bwd_w_sweep(const float* __restrict__ src, const float* __restrict__ mult,
                                                         const float* __restrict__ w, const float* __restrict__ alpha, int rows, int K,
                                                         float scale2, const float* __restrict__ row_stats, int tiles_per_split,
                                                         float* __restrict__ wpart, int k_pad) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* ldm = CODE ? lds + kTile * D : lds;                 // the multiplier tile (the student term multiplies by the rows themselves)
  float* lst = lds + (CODE ? 2 : 1) * kTile * D;             // the lse of the 64 streamed rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, fl = lane & 15;
  const int proto = blockIdx.x * kTile + wave * 16 + fl;
  const bool pv = proto < K;
  const int n = rows >> 1;
  float4 ff[D / 16];
  load_frag<D>(ff, w, proto, pv, g);
  // alpha of this prototype for a row of view a / view b, in the base-2 domain (the product csrc/swav.hip's statistics sweep forms)
  const float a2a = (CODE && pv) ? alpha[proto] * kLog2e : 0.f;
  const float a2b = (CODE && pv) ? alpha[(size_t)K + proto] * kLog2e : 0.f;
  f32x4 dacc[D / 16];
#pragma unroll
  for (int i = 0; i < D / 16; ++i) dacc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int ntiles = (rows + kTile - 1) / kTile;
  const int tile_begin = blockIdx.y * tiles_per_split;
  const int tile_end = min(ntiles, tile_begin + tiles_per_split);
  for (int rt = tile_begin; rt < tile_end; ++rt) {
    __syncthreads();
    load_tile<D>(lds, src, rt * kTile, rows, tid);
    if (CODE) load_tile<D, RowMap::kWrapped>(ldm, mult, rt * kTile, rows, tid);
    if (tid < kTile) {
      const int row = rt * kTile + tid;
      lst[tid] = row < rows ? row_stats[CODE ? 2 * row + 1 : row] : 0.f;
    }
    __syncthreads();
#pragma unroll 1                           // a fragment set and an accumulator set live: keep the loop rolled as csrc/swav.hip does
    for (int sub = 0; sub < 4; ++sub) {
      const f32x4 as = s_frag<D>(lds, sub, fl, g, ff);
      const int row0 = rt * kTile + sub * 16 + g * 4;  // streamed row of as[0]
      const float4 l4 = *(const float4*)(lst + sub * 16 + 4 * g);
      const float ll[4] = {l4.x, l4.y, l4.z, l4.w};
      float ds[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = row0 + i;
        const float t = logit2(as[i], scale2, CODE ? (row < n ? a2a : a2b) : 0.f);   // the statistics sweep's rounded logit
        ds[i] = (pv && row < rows) ? exp2f(t - ll[i]) : 0.f;
      }
      // dW^T[d][prototype] += sum_row mult[row][d] * P[row][prototype]
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int srow = sub * 16 + 4 * g + k;
          const int dcol = dt * 16 + fl;
          const float av = ldm[srow * D + ((((dcol >> 2) ^ (srow & 15)) << 2) | (dcol & 3))];
          dacc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, ds[k], dacc[dt], 0, 0, 0);
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

// dw_j = coeff * (2 sum_split spart[split][j] - sum_split cpart[split][j]), each sum in its fixed split order
__global__ __launch_bounds__(256) void swavl_combine_w(const float* __restrict__ spart, int ns, const float* __restrict__ cpart, int nc,
                                                       int k_pad, int K, int D, float coeff, float* __restrict__ dst) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const int C = D / 4;
  if (idx >= (long long)K * C) return;
  const int r = (int)(idx / C), c = (int)(idx % C);
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f), e = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int s = 0; s < ns; ++s) {
    const float4 v = *(const float4*)(spart + ((size_t)s * k_pad + r) * D + c * 4);
    a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
  }
  for (int s = 0; s < nc; ++s) {
    const float4 v = *(const float4*)(cpart + ((size_t)s * k_pad + r) * D + c * 4);
    e.x += v.x; e.y += v.y; e.z += v.z; e.w += v.w;
  }
  *(float4*)(dst + (size_t)r * D + c * 4) = make_float4(coeff * (2.f * a.x - e.x), coeff * (2.f * a.y - e.y),
                                                        coeff * (2.f * a.z - e.z), coeff * (2.f * a.w - e.w));
}

// fks / ftiles: key split of the statistics sweep (~512 workgroups); bks / btiles: of the probability sweep (~256); rs / rtiles: row
// split of the student key-side sweep over the L b local rows, gs / gtiles: of the code term over the 2b global rows (~256 each) --
// the targets of csrc/swav.hip
struct Plan { int rows, rows_pad, k_pad, fks, ftiles, bks, btiles, rs, rtiles, gs, gtiles, b_pad; };
Plan make_plan(int b, int L, int K) {
  Plan p;
  p.rows = b * L;
  const int qtiles = ceil_div(p.rows, kTile), ktiles = ceil_div(K, kTile), gtiles = ceil_div(2 * b, kTile);
  p.rows_pad = qtiles * kTile;
  p.k_pad = ktiles * kTile;
  p.b_pad = ceil_div(b, 4) * 4;
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
  const int gs = max(1, min(gtiles, wgs_b / max(1, ktiles)));
  p.gtiles = ceil_div(gtiles, gs);
  p.gs = ceil_div(gtiles, p.gtiles);
  return p;
}
// workspace (4-byte words): [row terms (double) | statistics partials | probability-sweep partials | m | student key-side partials |
// code key-side partials]
size_t off_part(const Plan& p) { return 2 * (size_t)p.rows_pad; }
size_t off_gpart(const Plan& p) { return off_part(p) + (size_t)p.fks * p.rows_pad * 2; }
size_t off_m(const Plan& p, int D) { return off_gpart(p) + (size_t)p.bks * p.rows_pad * D; }
size_t off_spart(const Plan& p, int D) { return off_m(p, D) + (size_t)p.b_pad * D; }
size_t off_cpart(const Plan& p, int D) { return off_spart(p, D) + (size_t)p.rs * p.k_pad * D; }
size_t total_words(const Plan& p, int D) { return off_cpart(p, D) + (size_t)p.gs * p.k_pad * D; }

bool shape_ok(int b, int L, int K) {
  return b >= 1 && L >= 1 && L <= 8 && (long long)b * L <= kMaxRows && 2LL * b <= kMaxRows && K >= 2 && K <= kMaxK;
}

}  // namespace

extern "C" {

size_t simclr_swav_local_workspace_bytes(int b, int L, int K, int D) {
  if (!shape_ok(b, L, K) || !dim_ok(D)) return 0;
  return total_words(make_plan(b, L, K), D) * sizeof(float);
}

int simclr_swav_local_key_splits(int b, int L, int K) {
  if (!shape_ok(b, L, K)) return 0;
  return make_plan(b, L, K).fks;
}

int simclr_swav_local_row_splits(int b, int L, int K) {
  if (!shape_ok(b, L, K)) return 0;
  return make_plan(b, L, K).rs;
}

int simclr_swav_local_code_row_splits(int b, int L, int K) {
  if (!shape_ok(b, L, K)) return 0;
  return make_plan(b, L, K).gs;
}

int simclr_swav_local_fwd(const float* x, const float* w, const float* u, int b, int L, int K, int D, float temperature, float* out,
                          float* row_stats, void* workspace, hipStream_t stream) {
  SIMCLR_CHECK_ARG(dim_ok(D), "swav_local_fwd: D must be 64/128/256 (got %d)", D);
  SIMCLR_CHECK_ARG(shape_ok(b, L, K), "swav_local_fwd: need b >= 1, L in [1, 8] and K in [2, 1048576] (b=%d L=%d K=%d)", b, L, K);
  SIMCLR_CHECK_ARG(pos_finite(temperature), "swav_local_fwd: the temperature must be > 0 and finite");
  SIMCLR_CHECK_ARG(al16(x) && al16(w) && al16(u) && al16(workspace) && al4(out) && al4(row_stats),
                   "swav_local_fwd: null argument, or x / w / u / workspace not 16-byte aligned");
  const Plan p = make_plan(b, L, K);
  float* wsp = (float*)workspace;
  double* rowterm = (double*)wsp;
  float* part = wsp + off_part(p);
  const float scale2 = kLog2e / temperature;
  const size_t lds1 = (size_t)kTile * D * sizeof(float);
  const dim3 grid_s(p.rows_pad / kTile, p.fks), gridr(ceil_div(p.rows, 16));
#define LAUNCH_FWD(DD)                                                                                                              \
  do {                                                                                                                              \
    hipLaunchKernelGGL((swavl_stats_sweep<DD>), grid_s, dim3(256), lds1, stream, x, w, p.rows, K, scale2, p.ftiles, part,           \
                       p.rows_pad);                                                                                                 \
    SIMCLR_CHECK_LAUNCH();                                                                                                          \
    hipLaunchKernelGGL((swavl_finalize_rows<DD>), gridr, dim3(256), 0, stream, part, p.fks, p.rows_pad, p.rows, b, x, u,            \
                       1.0 / (double)temperature, row_stats, rowterm);                                                              \
  } while (0)
  if (D == 64) LAUNCH_FWD(64); else if (D == 128) LAUNCH_FWD(128); else LAUNCH_FWD(256);
#undef LAUNCH_FWD
  SIMCLR_CHECK_LAUNCH();
  // 2 (V - 1) b with V = 2 + L
  hipLaunchKernelGGL(swavl_reduce_out, dim3(1), dim3(256), 0, stream, rowterm, p.rows, 2.0 * (double)(L + 1) * (double)b, out);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

int simclr_swav_local_bwd_x(const float* x, const float* w, const float* u, int b, int L, int K, int D, float temperature,
                            const float* row_stats, float grad_scale, float* dx, void* workspace, hipStream_t stream) {
  SIMCLR_CHECK_ARG(dim_ok(D), "swav_local_bwd_x: D must be 64/128/256 (got %d)", D);
  SIMCLR_CHECK_ARG(shape_ok(b, L, K), "swav_local_bwd_x: need b >= 1, L in [1, 8] and K in [2, 1048576] (b=%d L=%d K=%d)", b, L, K);
  SIMCLR_CHECK_ARG(pos_finite(temperature), "swav_local_bwd_x: the temperature must be > 0 and finite");
  SIMCLR_CHECK_ARG(al16(x) && al16(w) && al16(u) && al16(dx) && al16(workspace) && al4(row_stats),
                   "swav_local_bwd_x: null argument, or x / w / u / dx / workspace not 16-byte aligned");
  const Plan p = make_plan(b, L, K);
  float* gpart = (float*)workspace + off_gpart(p);
  const float scale2 = kLog2e / temperature;
  const size_t lds1 = (size_t)kTile * D * sizeof(float);
  const dim3 grid_p(p.rows_pad / kTile, p.bks);
  if (D == 64)
    hipLaunchKernelGGL((swavl_prob_sweep<64>), grid_p, dim3(256), lds1, stream, x, w, p.rows, K, scale2, row_stats, p.btiles, gpart,
                       p.rows_pad);
  else if (D == 128)
    hipLaunchKernelGGL((swavl_prob_sweep<128>), grid_p, dim3(256), lds1, stream, x, w, p.rows, K, scale2, row_stats, p.btiles, gpart,
                       p.rows_pad);
  else
    hipLaunchKernelGGL((swavl_prob_sweep<256>), grid_p, dim3(256), lds1, stream, x, w, p.rows, K, scale2, row_stats, p.btiles, gpart,
                       p.rows_pad);
  SIMCLR_CHECK_LAUNCH();
  // c / T with c = 1 / (2 (V - 1) b)
  const float coeff = grad_scale / (temperature * 2.f * (float)(L + 1) * (float)b);
  const long long chunks = (long long)p.rows * (D / 4);
  hipLaunchKernelGGL(swavl_combine_x, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, stream, gpart, p.bks, p.rows_pad, p.rows, b,
                     D, u, coeff, dx);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

int simclr_swav_local_bwd_w(const float* x, const float* z, const float* w, const float* alpha, int b, int L, int K, int D,
                            float temperature, float epsilon, const float* row_stats, const float* global_row_stats, float grad_scale,
                            float* dw, void* workspace, hipStream_t stream) {
  SIMCLR_CHECK_ARG(dim_ok(D), "swav_local_bwd_w: D must be 64/128/256 (got %d)", D);
  SIMCLR_CHECK_ARG(shape_ok(b, L, K), "swav_local_bwd_w: need b >= 1, L in [1, 8] and K in [2, 1048576] (b=%d L=%d K=%d)", b, L, K);
  SIMCLR_CHECK_ARG(pos_finite(temperature) && pos_finite(epsilon),
                   "swav_local_bwd_w: the temperature and epsilon must be > 0 and finite");
  SIMCLR_CHECK_ARG(al16(x) && al16(z) && al16(w) && al16(dw) && al16(workspace) && al4(alpha) && al4(row_stats) && al8(global_row_stats),
                   "swav_local_bwd_w: null argument, or x / z / w / dw / workspace not 16-byte aligned");
  const Plan p = make_plan(b, L, K);
  float* wsp = (float*)workspace;
  float* m = wsp + off_m(p, D);
  float* spart = wsp + off_spart(p, D);
  float* cpart = wsp + off_cpart(p, D);
  const float scale2s = kLog2e / temperature, scale2t = kLog2e / epsilon;
  const size_t lds_s = ((size_t)kTile * D + kTile) * sizeof(float), lds_c = ((size_t)2 * kTile * D + kTile) * sizeof(float);
  const dim3 grid_s(p.k_pad / kTile, p.rs), grid_c(p.k_pad / kTile, p.gs);
  const long long mchunks = (long long)b * (D / 4);
  hipLaunchKernelGGL(swavl_build_m, dim3((unsigned)((mchunks + 255) / 256)), dim3(256), 0, stream, x, b, L, D, m);
  SIMCLR_CHECK_LAUNCH();
#define LAUNCH_BWD(DD)                                                                                                              \
  do {                                                                                                                              \
    SIMCLR_CHECK_ARG(raise_lds(swavl_bwd_w_sweep<DD, false>, lds_s) && raise_lds(swavl_bwd_w_sweep<DD, true>, lds_c),               \
                     "swav_local_bwd_w: %d bytes of LDS refused", (int)lds_c);                                                      \
    hipLaunchKernelGGL((swavl_bwd_w_sweep<DD, false>), grid_s, dim3(256), lds_s, stream, x, (const float*)nullptr, w,               \
                       (const float*)nullptr, p.rows, K, scale2s, row_stats, p.rtiles, spart, p.k_pad);                             \
    SIMCLR_CHECK_LAUNCH();                                                                                                          \
    hipLaunchKernelGGL((swavl_bwd_w_sweep<DD, true>), grid_c, dim3(256), lds_c, stream, z, m, w, alpha, 2 * b, K, scale2t,          \
                       global_row_stats, p.gtiles, cpart, p.k_pad);                                                                 \
  } while (0)
  if (D == 64) LAUNCH_BWD(64); else if (D == 128) LAUNCH_BWD(128); else LAUNCH_BWD(256);
#undef LAUNCH_BWD
  SIMCLR_CHECK_LAUNCH();
  const float coeff = grad_scale / (temperature * 2.f * (float)(L + 1) * (float)b);
  const long long chunks = (long long)K * (D / 4);
  hipLaunchKernelGGL(swavl_combine_w, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, stream, spart, p.rs, cpart, p.gs, p.k_pad, K,
                     D, coeff, dw);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
