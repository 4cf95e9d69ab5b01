// MoCo v2 (He et al. 2020, Momentum Contrast; Chen et al. 2020, Improved Baselines with Momentum Contrastive Learning) for gfx950:
// InfoNCE of every query row against its ONE positive key and a queue of K keys of earlier steps.
//
//   q [2n, D] = l2-normalised online projections, [view-a rows; view-b rows];  t [2n, D] = l2-normalised momentum keys of the same rows;
//   queue [K, D] = keys of earlier steps.  Row r's positive is t_p, p = (r + n) mod 2n (the other view: BYOL's pairing, formed HERE, the
//   caller passes t unrolled).  The negatives are the K queue rows and nothing else.
//   s_r+ = q_r . t_p / T,  s_rj = q_r . queue_j / T,  l_r = logsumexp([s_r+, s_r0 .. s_r,K-1]) - s_r+,  loss = (1 / n) sum_{r < 2n} l_r
//   d loss / d q_r = (1 / (n T)) (sum_j P_rj queue_j - (1 - P_r+) t_p),  P = softmax over the K + 1 logits; t and the queue get none.
//
// The sweep is csrc/supcon.hip's query-fixed one without the predicate -- S = Q K^T tile by tile on v_mfma_f32_16x16x4_f32 (exact f32),
// 64 query rows per workgroup held as MFMA fragments, 64-row swizzled LDS queue tiles, online (max, sum) in the base-2 domain on the
// ROUNDED logit, key splits merged in a fixed order, the [2n, K] matrix never written.  The backward recomputes S and forms P . queue in
// the same one-sided sweep: there is no key-side sweep (nothing flows into the queue).  No atomics: two calls are bitwise equal.
//
// Two cancellations are avoided (near convergence l_r ~ 1e-6 and P_r+ ~ 1 - 1e-6):
//   * the row loss is never logsumexp - s+ in fp32: the negatives' running sum stays apart from the positive term until the row
//     finalize, which forms (M - s+) ln 2 + log(exp2(s+ - M) + sum_neg exp2(s_j - M)) in double -- log1p(sum_neg) when the positive
//     is the maximum;
//   * 1 - P_r+ is the negatives' share sum_neg / total, never one minus a number near one.
// The positive's dot product is formed in double by the row finalize (D fp32 products, 16 lanes per row, fixed xor tree).
//
// MFMA mapping, tile stager, S fragment and online (max, sum): csrc/sweep_tile.h.  The query rows are the fixed side.
#include "sweep_tile.h"

namespace {

using namespace sweep;

constexpr int kPart = 4;       // floats per (split, row) forward partial: {max, sum of exp2, max raw dot product, -} over the split's queue rows

// ---- forward: one partial per (key split, query row) over the split's queue rows -- the negatives only ---------------------------------
template <int D>
__global__ __launch_bounds__(256) void moco_fwd_partial(const float* __restrict__ q, const float* __restrict__ queue, int two_n, int K,
                                                        float scale2 /* log2(e) / T */, int tiles_per_split, float* __restrict__ part,
                                                        int rows_pad) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, fl = lane & 15;
  const int row = blockIdx.x * kTile + wave * 16 + fl;
  const bool rv = row < two_n;
  float4 ff[D / 16];
#pragma unroll
  for (int s = 0; s < D / 16; ++s)
    ff[s] = rv ? *(const float4*)(q + (size_t)row * D + 16 * s + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
  float m = -INFINITY, l = 0.f, nmax = -INFINITY;
  const int ntiles = (K + kTile - 1) / kTile;
  const int tile_begin = blockIdx.y * tiles_per_split;
  const int tile_end = min(ntiles, tile_begin + tiles_per_split);
  for (int kt = tile_begin; kt < tile_end; ++kt) {
    __syncthreads();
    load_tile<D>(lds, queue, kt * kTile, K, tid);
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      const f32x4 acc = s_frag<D>(lds, sub, fl, g, ff);
      const int col0 = kt * kTile + sub * 16 + g * 4;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (col0 + r < K) {                // the ragged last tile: rows past the queue count nowhere
          float t = acc[r] * scale2;
          asm volatile("" : "+v"(t));      // the ROUNDED logit everywhere: fused into t - mn the product would keep its low bits and exp2(t - t) != 1
          const float mn = fmaxf(m, t);
          l = l * exp2f(m - mn) + exp2f(t - mn);
          m = mn;
          nmax = fmaxf(nmax, acc[r]);
        }
      }
    }
  }
  // the 4 lane groups that share this query row, in a fixed order
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {
    const float om = __shfl_xor(m, o, 64), ol = __shfl_xor(l, o, 64);
    ml_merge(m, l, om, ol);
    nmax = fmaxf(nmax, __shfl_xor(nmax, o, 64));
  }
  if (g == 0 && rv) *(float4*)(part + ((size_t)blockIdx.y * rows_pad + row) * kPart) = make_float4(m, l, nmax, 0.f);
}

// Merge the key splits of every query row and add the positive (16 lanes per row, fixed xor trees).  In double, base-2 domain:
//   s+ = (q_r . t_p) log2(e) / T,  M = max(m_neg, s+),  neg = l_neg exp2(m_neg - M),  total = exp2(s+ - M) + neg
//   rowterm[r] = l_r = (M - s+) ln 2 + log(total)       (log1p(neg) when the positive is the maximum: total = 1 + neg)
//   row_stats[r] = {M + log2(total) = logsumexp over the K + 1 logits, neg / total = 1 - P_r+}
//   hit[r] = (q_r . t_p >= max_j q_r . queue_j), both as fp32
template <int D>
__global__ __launch_bounds__(256) void moco_finalize_rows(const float* __restrict__ q, const float* __restrict__ t,
                                                          const float* __restrict__ part, int nsplit, int rows_pad, int two_n,
                                                          double scale2, float* __restrict__ row_stats, double* __restrict__ rowterm,
                                                          int* __restrict__ hit) {
  const int r = blockIdx.x * 16 + (threadIdx.x >> 4);
  const int j = threadIdx.x & 15;
  float m = -INFINITY, l = 0.f, nmax = -INFINITY;
  double dot = 0.0;
  if (r < two_n) {
    for (int s = j; s < nsplit; s += 16) {
      const float4 a = *(const float4*)(part + ((size_t)s * rows_pad + r) * kPart);
      ml_merge(m, l, a.x, a.y);
      nmax = fmaxf(nmax, a.z);
    }
    const int n = two_n >> 1;
    const int p = r < n ? r + n : r - n;
    const float4* qr = (const float4*)(q + (size_t)r * D);
    const float4* tp = (const float4*)(t + (size_t)p * D);
#pragma unroll
    for (int i = 0; i < D / 64; ++i) {
      const float4 a = qr[j + 16 * i], b = tp[j + 16 * i];
      dot += (double)a.x * b.x + (double)a.y * b.y + (double)a.z * b.z + (double)a.w * b.w;
    }
  }
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) {
    const float om = __shfl_xor(m, o, 64), ol = __shfl_xor(l, o, 64);
    ml_merge(m, l, om, ol);
    nmax = fmaxf(nmax, __shfl_xor(nmax, o, 64));
    dot += __shfl_xor(dot, o, 64);
  }
  if (j == 0 && r < two_n) {
    const double sp = dot * scale2;
    const double M = fmax((double)m, sp);
    const double neg = (double)l * exp2((double)m - M);
    const double pos = exp2(sp - M);
    const double total = pos + neg;
    rowterm[r] = (M == sp) ? log1p(neg) : (M - sp) * kLn2d + log(total);
    row_stats[2 * r] = (float)(M + log2(total));
    row_stats[2 * r + 1] = (float)(neg / total);
    hit[r] = (float)dot >= nmax ? 1 : 0;
  }
}

// out[0] = loss = sum(l_r) / n, out[1] = contrast_acc = hits / 2n -- one workgroup: thread i adds rows i, i + 256, ... in double, then
// a fixed binary tree; the hits are summed as integers
__global__ __launch_bounds__(256) void moco_reduce_out(const double* __restrict__ rowterm, const int* __restrict__ hit, int two_n,
                                                       float* __restrict__ out) {
  __shared__ double sh_l[256];
  __shared__ long long sh_h[256];
  double ls = 0.0;
  long long hs = 0;
  for (int r = threadIdx.x; r < two_n; r += 256) {
    ls += rowterm[r];
    hs += hit[r];
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
    out[0] = (float)(sh_l[0] / (0.5 * (double)two_n));
    out[1] = (float)((double)sh_h[0] / (double)two_n);
  }
}

// ---- backward sweep (recomputes S): gpart[split][r] = sum over the split's queue rows j of softmax[r, j] queue_j ---------------------
template <int D>
__global__ __launch_bounds__(256) void moco_bwd_sweep(const float* __restrict__ q, const float* __restrict__ queue, int two_n, int K,
                                                      float scale2, const float* __restrict__ row_stats, int tiles_per_split,
                                                      float* __restrict__ gpart, int rows_pad) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, fl = lane & 15;
  const int row = blockIdx.x * kTile + wave * 16 + fl;
  const bool rv = row < two_n;
  float4 ff[D / 16];
#pragma unroll
  for (int s = 0; s < D / 16; ++s)
    ff[s] = rv ? *(const float4*)(q + (size_t)row * D + 16 * s + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
  const float lse = rv ? row_stats[2 * row] : 0.f;
  f32x4 dacc[D / 16];
#pragma unroll
  for (int i = 0; i < D / 16; ++i) dacc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int ntiles = (K + kTile - 1) / kTile;
  const int tile_begin = blockIdx.y * tiles_per_split;
  const int tile_end = min(ntiles, tile_begin + tiles_per_split);
  for (int kt = tile_begin; kt < tile_end; ++kt) {
    __syncthreads();
    load_tile<D>(lds, queue, kt * kTile, K, tid);
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      const f32x4 acc = s_frag<D>(lds, sub, fl, g, ff);
      const int col0 = kt * kTile + sub * 16 + g * 4;  // queue row of acc[0]
      float ds[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float t = acc[r] * scale2;
        asm volatile("" : "+v"(t));        // the forward's rounded logit, not fma(acc, scale2, -lse)
        ds[r] = (rv && col0 + r < K) ? exp2f(t - lse) : 0.f;
      }
      // dQ^T[d][query] += sum_key queue[key][d] * P[key][query]
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
  if (rv) {
    float* gp = gpart + ((size_t)blockIdx.y * rows_pad + row) * D;
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt)
      *(float4*)(gp + dt * 16 + 4 * g) = make_float4(dacc[dt][0], dacc[dt][1], dacc[dt][2], dacc[dt][3]);
  }
}

// dq_r = coeff * (sum_split gpart[split][r] - (1 - P_r+) t_p), fixed split order; one 16-byte chunk per thread
__global__ __launch_bounds__(256) void moco_combine(const float* __restrict__ gpart, int nsplit, int rows_pad, int two_n, int D,
                                                    const float* __restrict__ t, const float* __restrict__ row_stats, float coeff,
                                                    float* __restrict__ dq) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int C = D / 4;
  if (i >= (long long)two_n * C) return;
  const int r = (int)(i / C), c = (int)(i % C);
  const int n = two_n >> 1;
  const int p = r < n ? r + n : r - n;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int s = 0; s < nsplit; ++s) {
    const float4 v = *(const float4*)(gpart + ((size_t)s * rows_pad + r) * D + c * 4);
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  const float w = row_stats[2 * r + 1];
  const float4 k = *(const float4*)(t + (size_t)p * D + c * 4);
  *(float4*)(dq + (size_t)r * D + c * 4) =
      make_float4(coeff * (acc.x - w * k.x), coeff * (acc.y - w * k.y), coeff * (acc.z - w * k.z), coeff * (acc.w - w * k.w));
}

// fks / ftiles: key split of the forward sweep (~512 workgroups); bks / btiles: of the backward sweep (~256), the targets
// csrc/ntxent.hip measured for the same sweeps
struct Plan { int rows_pad, fks, ftiles, bks, btiles; };
Plan make_plan(int two_n, int K) {
  Plan p;
  const int qtiles = ceil_div(two_n, kTile), ktiles = ceil_div(K, kTile);
  p.rows_pad = qtiles * kTile;
  constexpr int wgs_f = 512, wgs_b = 256;
  const int fs = max(1, min(ktiles, wgs_f / max(1, qtiles)));
  p.ftiles = ceil_div(ktiles, fs);
  p.fks = ceil_div(ktiles, p.ftiles);
  const int bs = max(1, min(ktiles, wgs_b / max(1, qtiles)));
  p.btiles = ceil_div(ktiles, bs);
  p.bks = ceil_div(ktiles, p.btiles);
  return p;
}
// workspace layout (4-byte words): [row terms (double) | row hits | forward partials | backward partials]
size_t off_hit(const Plan& p) { return 2 * (size_t)p.rows_pad; }
size_t off_part(const Plan& p) { return off_hit(p) + (size_t)p.rows_pad; }
size_t off_gpart(const Plan& p) { return off_part(p) + (size_t)p.fks * p.rows_pad * kPart; }
size_t ws_words(const Plan& p, int D) { return off_gpart(p) + (size_t)p.bks * p.rows_pad * D; }

bool shape_ok(int two_n, int K, int D) {
  return two_n >= 2 && two_n % 2 == 0 && two_n <= (1 << 28) && K >= 1 && K <= (1 << 30) && (D == 64 || D == 128 || D == 256);
}
bool aligned16(const void* a, const void* b, const void* c, const void* d) {
  return a && b && c && d && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

}  // namespace

extern "C" {

size_t simclr_moco_workspace_bytes(int two_n, int K, int D) {
  if (!shape_ok(two_n, K, D)) return 0;
  return ws_words(make_plan(two_n, K), D) * sizeof(float);
}

int simclr_moco_key_splits(int two_n, int K) {
  if (!shape_ok(two_n, K, 64)) return 0;
  return make_plan(two_n, K).fks;
}

int simclr_moco_fwd(const float* q, const float* t, const float* queue, int two_n, int K, int D, float temperature, float* out,
                    float* row_stats, void* workspace, hipStream_t stream) {
  SIMCLR_CHECK_ARG(D == 64 || D == 128 || D == 256, "moco_fwd: D must be 64/128/256 (got %d)", D);
  SIMCLR_CHECK_ARG(shape_ok(two_n, K, D), "moco_fwd: need an even two_n >= 2 and K >= 1 (two_n=%d K=%d)", two_n, K);
  SIMCLR_CHECK_ARG(temperature > 0.f, "moco_fwd: temperature must be > 0");          // (NaN fails the comparison)
  SIMCLR_CHECK_ARG(aligned16(q, t, queue, workspace) && out && row_stats && ((uintptr_t)row_stats & 7) == 0,
                   "moco_fwd: null argument, or q / t / queue / workspace not 16-byte aligned");
  const Plan p = make_plan(two_n, K);
  float* ws = (float*)workspace;
  double* rowterm = (double*)ws;
  int* hit = (int*)(ws + off_hit(p));
  float* part = ws + off_part(p);
  const float scale2 = kLog2e / temperature;
  const dim3 grid(p.rows_pad / kTile, p.fks);
  const size_t lds = (size_t)kTile * D * sizeof(float);
  const dim3 gridr(ceil_div(two_n, 16));
  const double scale2d = kLog2ed / (double)temperature;
#define LAUNCH_FWD(DD)                                                                                                              \
  do {                                                                                                                              \
    hipLaunchKernelGGL((moco_fwd_partial<DD>), grid, dim3(256), lds, stream, q, queue, two_n, K, scale2, p.ftiles, part, p.rows_pad); \
    SIMCLR_CHECK_LAUNCH();                                                                                                          \
    hipLaunchKernelGGL((moco_finalize_rows<DD>), gridr, dim3(256), 0, stream, q, t, part, p.fks, p.rows_pad, two_n, scale2d,        \
                       row_stats, rowterm, hit);                                                                                    \
  } while (0)
  if (D == 64) LAUNCH_FWD(64); else if (D == 128) LAUNCH_FWD(128); else LAUNCH_FWD(256);
#undef LAUNCH_FWD
  SIMCLR_CHECK_LAUNCH();
  hipLaunchKernelGGL(moco_reduce_out, dim3(1), dim3(256), 0, stream, rowterm, hit, two_n, out);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

int simclr_moco_bwd(const float* q, const float* t, const float* queue, int two_n, int K, int D, float temperature,
                    const float* row_stats, float grad_scale, float* dq, void* workspace, hipStream_t stream) {
  SIMCLR_CHECK_ARG(D == 64 || D == 128 || D == 256, "moco_bwd: D must be 64/128/256 (got %d)", D);
  SIMCLR_CHECK_ARG(shape_ok(two_n, K, D), "moco_bwd: need an even two_n >= 2 and K >= 1 (two_n=%d K=%d)", two_n, K);
  SIMCLR_CHECK_ARG(temperature > 0.f, "moco_bwd: temperature must be > 0");
  SIMCLR_CHECK_ARG(aligned16(q, t, queue, workspace) && row_stats && dq && ((uintptr_t)dq & 15) == 0 && ((uintptr_t)row_stats & 7) == 0,
                   "moco_bwd: null argument, or q / t / queue / dq / workspace not 16-byte aligned");
  const Plan p = make_plan(two_n, K);
  float* gpart = (float*)workspace + off_gpart(p);
  const float scale2 = kLog2e / temperature;
  const dim3 grid(p.rows_pad / kTile, p.bks);
  const size_t lds = (size_t)kTile * D * sizeof(float);
#define LAUNCH_BWD(DD)                                                                                                                  \
  hipLaunchKernelGGL((moco_bwd_sweep<DD>), grid, dim3(256), lds, stream, q, queue, two_n, K, scale2, row_stats, p.btiles, gpart, p.rows_pad)
  if (D == 64) LAUNCH_BWD(64); else if (D == 128) LAUNCH_BWD(128); else LAUNCH_BWD(256);
#undef LAUNCH_BWD
  SIMCLR_CHECK_LAUNCH();
  // d((1 / n) sum_r l_r) / dq_r = (1 / (n T)) (sum_j P_rj queue_j - (1 - P_r+) t_p), n = two_n / 2
  const float coeff = grad_scale / (temperature * (float)(two_n / 2));
  const long long chunks = (long long)two_n * (D / 4);
  hipLaunchKernelGGL(moco_combine, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, stream, gpart, p.bks, p.rows_pad, two_n, D, t,
                     row_stats, coeff, dq);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
