// Cached-feature linear probe: l2-regularised multinomial logistic regression on frozen encoder features (simclr_amd/logreg.py).
// x [n, D] = a slab of standardised features, W [C, D], b [C], labels y_n, weights w_n (0 = padding), S = the weight total of the bank:
//   s_nc = x_n . W_c + b_c
//   f    = (1 / S) sum_n w_n (logsumexp_c s_nc - s_n,y_n)            (the l2 terms are added by the caller)
//   G_nc = (w_n / S) (softmax_c(s_n) - [c = y_n]),   dW = G^T X,   db = colsum(G)
//
// Forward, three launches (four with mode 1):
//   lr_fwd     one E x E tile of S^T = W X^T per workgroup on the exact fp32-input MFMA (csrc/gram_tile.h): classes on the MFMA's A side,
//              rows on the lane, so a lane owns W rows and walks 4 W classes of each in ascending order.  Per row it keeps the online
//              (m, r) of csrc/sweep_tile.h on the rounded base-2 logit t = logit2(dot, log2 e, fl(b_c log2 e)), the label's t where the label
//              is one of its classes, and its lowest-index maximum.  The 8 lane states of a row (2 waves x 4 lane groups) are merged through
//              LDS in one fixed order and go to slot [class tile][row].  Classes c >= C never enter a statistic.  With a store, the raw
//              logits fl(dot + b_c) go to store [n, Cpad].
//   lr_merge   one thread per row: the class tiles in ascending order, then in double lse_n = ln 2 (m + log2(1 + r)) and
//              w_n (lse_n - s_n,y_n); 256 rows are summed per workgroup in a fixed order
//   lr_finish  adds the workgroups' triples in ascending order: out = {sum w (lse - s_y), sum of w over top-1 hits, sum w}
//   lr_grad    (mode 1) store <- G in place: the label's element is (w/S) expm1(s - lse) in double, so a near-one-hot row keeps its
//              residual; every other element (w/S) exp2(fl((s - lse) log2 e))
// Backward, three launches:
//   lr_bwd     one E x E tile of G^T X per workgroup and row part, both operands in their KR orientation, written to a slab of its own
//   lr_db      column sums of G in double: 32 columns x 4096 rows per workgroup (gram_tile::col_reduce)
//   lr_reduce  dW (+)= ((p0 + p1) + p2) + ... in fp32, db (+)= fl(the chunks added in ascending order in double)
// No atomics, every order fixed: repeat calls are bitwise equal.
#include "gram_tile.h"
#include "sweep_tile.h"

#include <math.h>

namespace {

constexpr int kLrMergeRows = 256;    // rows per workgroup of lr_merge
constexpr int kLrDbRows = 4096;      // rows per workgroup of lr_db
constexpr int kLrNoIndex = 0x7fffffff;

// blockIdx.x = class tile, blockIdx.y = row tile.  Slot arrays are [class tiles][n].
template <int W, bool STORE>
__global__ __launch_bounds__(256) void lr_fwd(const float* __restrict__ x, const float* __restrict__ wt, const float* __restrict__ bias,
                                              const int* __restrict__ labels, int n, int D, int C, int cpad, float* __restrict__ store,
                                              float* __restrict__ pm, float* __restrict__ pr, float* __restrict__ pl, float* __restrict__ pv,
                                              int* __restrict__ pi) {
  constexpr int E = 32 * W;
  __shared__ __attribute__((aligned(16))) float lds[2 * gram_tile::op_floats<E>()];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, fl = lane & 15, wm = wave & 1, wn = wave >> 1;
  const int c0 = blockIdx.x * E, r0 = blockIdx.y * E;
  f32x4 acc[W][W];
  gram_tile::tile<W, false, false>(lds, wt, D, C, true, x, D, n, true, 0, D, c0, r0, acc);
  // the 4 W classes of this lane: the bias and its base-2 form (zeros past the last class: those elements are skipped below)
  float bb[W][4], b2[W][4];
#pragma unroll
  for (int i = 0; i < W; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = c0 + 16 * W * wm + 16 * i + 4 * g + k;
      bb[i][k] = c < C ? bias[c] : 0.f;
      b2[i][k] = bb[i][k] * sweep::kLog2e;
    }
  __syncthreads();      // every wave is past its last fragment read: the operand LDS becomes the 8 lane states of each row
  float* sm = lds;
  float* sr = lds + 8 * E;
  float* sl = lds + 16 * E;
  float* sv = lds + 24 * E;
  int* si = (int*)(lds + 32 * E);
#pragma unroll
  for (int w = 0; w < W; ++w) {
    const int rl = 16 * W * wn + 16 * w + fl, row = r0 + rl;
    const int lab = row < n ? labels[row] : -1;
    float m = -INFINITY, r = 0.f, tl = -INFINITY, bv = -INFINITY;
    int bi = kLrNoIndex;
#pragma unroll
    for (int i = 0; i < W; ++i) {
      const int cb = c0 + 16 * W * wm + 16 * i + 4 * g;
      float raw[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = cb + k;
        raw[k] = acc[i][w][k] + bb[i][k];
        if (c < C) {
          const float t = sweep::logit2(acc[i][w][k], sweep::kLog2e, b2[i][k]);
          sweep::mr_push(m, r, t);
          if (t > bv) { bv = t; bi = c; }      // ascending c within the lane: the first of equals stays
          if (c == lab) tl = t;
        }
      }
      if (STORE && row < n) {
        float* p = store + (size_t)row * cpad + cb;
        if (cb + 3 < C) *(float4*)p = make_float4(raw[0], raw[1], raw[2], raw[3]);
        else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (cb + k < C) p[k] = raw[k];
        }
      }
    }
    const int slot = rl * 8 + wm * 4 + g;
    sm[slot] = m; sr[slot] = r; sl[slot] = tl; sv[slot] = bv; si[slot] = bi;
  }
  __syncthreads();
  if (tid < E && r0 + tid < n) {
    float m = -INFINITY, r = 0.f, tl = -INFINITY, bv = -INFINITY;
    int bi = kLrNoIndex;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int slot = tid * 8 + s;
      sweep::mr_merge(m, r, sm[slot], sr[slot]);
      tl = fmaxf(tl, sl[slot]);                 // at most one state holds the label
      const float v = sv[slot];
      const int ix = si[slot];
      if (v > bv || (v == bv && ix < bi)) { bv = v; bi = ix; }
    }
    const size_t o = (size_t)blockIdx.x * n + r0 + tid;
    pm[o] = m; pr[o] = r; pl[o] = tl; pv[o] = bv; pi[o] = bi;
  }
}

// Sum of one double per thread over the workgroup: the butterfly of wave_sum_d, then the 4 waves in ascending order.
__device__ __forceinline__ double lr_block_sum(double v, double* sh4) {
  v = wave_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh4[0] + sh4[1]) + sh4[2]) + sh4[3];
}

__global__ __launch_bounds__(256) void lr_merge(const float* __restrict__ pm, const float* __restrict__ pr, const float* __restrict__ pl,
                                                const float* __restrict__ pv, const int* __restrict__ pi, int ntc,
                                                const int* __restrict__ labels, const float* __restrict__ weights, int n,
                                                double* __restrict__ lse, double* __restrict__ blk) {
  __shared__ double sh4[4];
  const int row = blockIdx.x * kLrMergeRows + threadIdx.x;
  double loss = 0.0, hit = 0.0, wd = 0.0;
  if (row < n) {
    float m = -INFINITY, r = 0.f, tl = -INFINITY, bv = -INFINITY;
    int bi = kLrNoIndex;
    for (int t = 0; t < ntc; ++t) {
      const size_t o = (size_t)t * n + row;
      sweep::mr_merge(m, r, pm[o], pr[o]);
      tl = fmaxf(tl, pl[o]);
      const float v = pv[o];
      if (v > bv) { bv = v; bi = pi[o]; }        // ascending tiles: the lowest index of equals stays
    }
    const double lse2 = (double)m + log2(1.0 + (double)r);
    lse[row] = lse2 * sweep::kLn2d;
    const float w = weights[row];
    if (w != 0.f) {
      wd = (double)w;
      loss = wd * ((lse2 - (double)tl) * sweep::kLn2d);
      hit = bi == labels[row] ? wd : 0.0;
    }
  }
  loss = lr_block_sum(loss, sh4);
  hit = lr_block_sum(hit, sh4);
  wd = lr_block_sum(wd, sh4);
  if (threadIdx.x == 0) {
    blk[3 * (size_t)blockIdx.x] = loss;
    blk[3 * (size_t)blockIdx.x + 1] = hit;
    blk[3 * (size_t)blockIdx.x + 2] = wd;
  }
}

__global__ __launch_bounds__(64) void lr_finish(const double* __restrict__ blk, int nblk, double* __restrict__ out) {
  if (threadIdx.x < 3) {
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += blk[3 * (size_t)b + threadIdx.x];
    out[threadIdx.x] = s;
  }
}

__global__ __launch_bounds__(256) void lr_grad(float* __restrict__ store, const double* __restrict__ lse, const int* __restrict__ labels,
                                               const float* __restrict__ weights, int n, int C, int cpad, double inv_S) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const int row = (int)(idx / cpad), c = (int)(idx - (long long)row * cpad);
  if (row >= n || c >= C) return;
  const double d = (double)store[idx] - lse[row];
  const float ws = (float)((double)weights[row] * inv_S);
  store[idx] = ws * (c == labels[row] ? (float)expm1(d) : exp2f((float)(d * sweep::kLog2ed)));
}

// blockIdx.x = class tile, blockIdx.y = feature tile, blockIdx.z = row part.  part [P][C][D].
template <int W>
__global__ __launch_bounds__(256) void lr_bwd(const float* __restrict__ gm, const float* __restrict__ x, int n, int D, int C, int cpad,
                                              int part_rows, float* __restrict__ part) {
  constexpr int E = 32 * W;
  __shared__ __attribute__((aligned(16))) float lds[2 * gram_tile::op_floats<E>()];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, fl = lane & 15, wm = wave & 1, wn = wave >> 1;
  const int c0 = blockIdx.x * E, d0 = blockIdx.y * E;
  const int kbeg = blockIdx.z * part_rows, kend = min(n, kbeg + part_rows);
  f32x4 acc[W][W];
  gram_tile::tile<W, true, true>(lds, gm, cpad, C, true, x, D, D, true, kbeg, kend, c0, d0, acc);
  float* out = part + (size_t)blockIdx.z * C * D;
#pragma unroll
  for (int i = 0; i < W; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = c0 + 16 * W * wm + 16 * i + 4 * g + k;
      if (c >= C) continue;
#pragma unroll
      for (int w = 0; w < W; ++w) {
        const int d = d0 + 16 * W * wn + 16 * w + fl;
        if (d < D) out[(size_t)c * D + d] = acc[i][w][k];
      }
    }
}

// blockIdx.x = 32-column group, blockIdx.y = row chunk.  dbpart [chunks][C].
__global__ __launch_bounds__(256) void lr_db(const float* __restrict__ gm, int n, int C, int cpad, double* __restrict__ dbpart) {
  __shared__ double sh[32 * gram_tile::kCols];
  __shared__ double res[gram_tile::kCols];
  const int tid = threadIdx.x, q = tid & 7, rg = tid >> 3;
  const int c = blockIdx.x * gram_tile::kCols + 4 * q;
  const int rbeg = blockIdx.y * kLrDbRows, rend = min(n, rbeg + kLrDbRows);
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  if (c < C) {        // the quad lies inside the pitch (a multiple of 4); its columns >= C are read and dropped below
    for (int a = rbeg + rg; a < rend; a += 32) {
      const float4 t = *(const float4*)(gm + (size_t)a * cpad + c);
      v[0] += (double)t.x; v[1] += (double)t.y; v[2] += (double)t.z; v[3] += (double)t.w;
    }
  }
  gram_tile::col_reduce(v, sh, res);
  const int col = blockIdx.x * gram_tile::kCols + tid;
  if (tid < gram_tile::kCols && col < C) dbpart[(size_t)blockIdx.y * C + col] = res[tid];
}

__global__ __launch_bounds__(256) void lr_reduce(const float* __restrict__ part, int P, const double* __restrict__ dbpart, int chunks, int C,
                                                 int D, float* __restrict__ dw, float* __restrict__ db, int accumulate) {
  const size_t cd = (size_t)C * D;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx < cd) {
    float s = part[idx];
    for (int p = 1; p < P; ++p) s += part[(size_t)p * cd + idx];
    dw[idx] = accumulate ? dw[idx] + s : s;
  } else if (idx < cd + C) {
    const int c = (int)(idx - cd);
    double s = dbpart[c];
    for (int k = 1; k < chunks; ++k) s += dbpart[(size_t)k * C + c];
    db[c] = accumulate ? db[c] + (float)s : (float)s;
  }
}

bool lr_shape_ok(int n, int D, int C) {
  return D >= 64 && D <= 8192 && D % 64 == 0 && C >= 2 && C <= 4096 && n >= 1 && n <= 65536;
}
int lr_pitch(int C) { return (C + 3) / 4 * 4; }
// Tile edges: 128 where the 128-wide grid alone gives the chip >= 256 workgroups, else 64 (the rule of csrc/vicreg.hip)
int lr_fwd_edge(int n, int C) { return (long long)ceil_div(n, 128) * ceil_div(C, 128) >= 256 ? 128 : 64; }
int lr_bwd_edge(int D, int C) { return (long long)ceil_div(C, 128) * ceil_div(D, 128) >= 256 ? 128 : 64; }
// workspace: [pm | pr | pl | pv | pi: ntc x n x 4 bytes each][blk: 3 doubles per merge workgroup][part: P C D floats][dbpart: chunks x C doubles]
struct LrPlan {
  int fe, ntc, nblk, be, P, part_rows, chunks;
  size_t slots, off_blk, off_part, off_db, bytes;
};
LrPlan lr_plan(int n, int D, int C) {
  LrPlan p;
  p.fe = lr_fwd_edge(n, C);
  p.ntc = ceil_div(C, p.fe);
  p.nblk = ceil_div(n, kLrMergeRows);
  p.be = lr_bwd_edge(D, C);
  // row parts where the C x D grid alone leaves CUs idle: at least 256 rows each, a whole number of k stages
  const long long tiles = (long long)ceil_div(C, p.be) * ceil_div(D, p.be);
  int want = tiles >= 256 ? 1 : (int)((256 + tiles - 1) / tiles);
  if (want > ceil_div(n, 256)) want = ceil_div(n, 256);
  p.part_rows = ceil_div(ceil_div(n, want), gram_tile::kKc) * gram_tile::kKc;
  p.P = ceil_div(n, p.part_rows);
  p.chunks = ceil_div(n, kLrDbRows);
  p.slots = ((size_t)p.ntc * n * sizeof(float) + 15) / 16 * 16;
  p.off_blk = 5 * p.slots;
  p.off_part = p.off_blk + ((size_t)3 * p.nblk * sizeof(double) + 15) / 16 * 16;
  p.off_db = p.off_part + (size_t)p.P * C * D * sizeof(float);        // a multiple of 16: D is one of 64
  p.bytes = p.off_db + (size_t)p.chunks * C * sizeof(double);
  return p;
}

}  // namespace

extern "C" {

size_t simclr_logreg_workspace_bytes(int n, int D, int C) { return lr_shape_ok(n, D, C) ? lr_plan(n, D, C).bytes : 0; }
int simclr_logreg_row_splits(int n, int D, int C) { return lr_shape_ok(n, D, C) ? lr_plan(n, D, C).P : 0; }
int simclr_logreg_tile_edge(int n, int D, int C) { return lr_shape_ok(n, D, C) ? lr_plan(n, D, C).fe : 0; }
int simclr_logreg_bwd_tile_edge(int n, int D, int C) { return lr_shape_ok(n, D, C) ? lr_plan(n, D, C).be : 0; }
int simclr_logreg_store_pitch(int C) { return C >= 2 && C <= 4096 ? lr_pitch(C) : 0; }

#define LR_CHECK_SHAPE(name)                                                                                                   \
  SIMCLR_CHECK_ARG(D >= 64 && D <= 8192 && D % 64 == 0, name ": the width must be a multiple of 64 in [64, 8192] (got %d)", D); \
  SIMCLR_CHECK_ARG(C >= 2 && C <= 4096, name ": need 2 <= C <= 4096 classes (got %d)", C);                                      \
  SIMCLR_CHECK_ARG(n >= 1 && n <= 65536, name ": need 1 <= n <= 65536 rows per call (got %d)", n)

int simclr_logreg_fwd(const float* x, const float* w, const float* b, const int* labels, const float* weights, int n, int D, int C,
                      double inv_S, int mode, float* store, double* lse, double* out3, void* workspace, hipStream_t stream) {
  LR_CHECK_SHAPE("logreg_fwd");
  SIMCLR_CHECK_ARG(mode >= 0 && mode <= 2, "logreg_fwd: mode must be 0 (value), 1 (value and G) or 2 (logits) (got %d)", mode);
  SIMCLR_CHECK_ARG(inv_S > 0.0 && inv_S <= 1.0e300, "logreg_fwd: inv_S must be a finite number > 0 (got %g)", inv_S);
  SIMCLR_CHECK_ARG(x && w && b && labels && weights && lse && out3 && workspace && (mode == 0 || store), "logreg_fwd: null argument");
  SIMCLR_CHECK_ARG(sweep::al16(x) && sweep::al16(w) && sweep::al16(b) && sweep::al16(labels) && sweep::al16(weights) && sweep::al16(lse) &&
                       sweep::al16(out3) && sweep::al16(workspace) && (mode == 0 || sweep::al16(store)),
                   "logreg_fwd: every pointer must be 16-byte aligned");
  const LrPlan p = lr_plan(n, D, C);
  const int cpad = lr_pitch(C);
  char* ws = (char*)workspace;
  float* pm = (float*)ws;
  float* pr = (float*)(ws + p.slots);
  float* pl = (float*)(ws + 2 * p.slots);
  float* pv = (float*)(ws + 3 * p.slots);
  int* pi = (int*)(ws + 4 * p.slots);
  double* blk = (double*)(ws + p.off_blk);
  dim3 grid(p.ntc, ceil_div(n, p.fe));
#define LR_FWD(W, ST) \
  hipLaunchKernelGGL((lr_fwd<W, ST>), grid, dim3(256), 0, stream, x, w, b, labels, n, D, C, cpad, store, pm, pr, pl, pv, pi)
  if (p.fe == 128) { if (mode) LR_FWD(4, true); else LR_FWD(4, false); }
  else { if (mode) LR_FWD(2, true); else LR_FWD(2, false); }
#undef LR_FWD
  SIMCLR_CHECK_LAUNCH();
  hipLaunchKernelGGL(lr_merge, dim3(p.nblk), dim3(256), 0, stream, (const float*)pm, (const float*)pr, (const float*)pl, (const float*)pv,
                     (const int*)pi, p.ntc, labels, weights, n, lse, blk);
  SIMCLR_CHECK_LAUNCH();
  hipLaunchKernelGGL(lr_finish, dim3(1), dim3(64), 0, stream, (const double*)blk, p.nblk, out3);
  SIMCLR_CHECK_LAUNCH();
  if (mode == 1) {
    hipLaunchKernelGGL(lr_grad, dim3(ceil_div((long long)n * cpad, 256)), dim3(256), 0, stream, store, (const double*)lse, labels, weights, n, C,
                       cpad, inv_S);
    SIMCLR_CHECK_LAUNCH();
  }
  return 0;
}

int simclr_logreg_bwd(const float* g, const float* x, int n, int D, int C, float* dw, float* db, int accumulate, void* workspace,
                      hipStream_t stream) {
  LR_CHECK_SHAPE("logreg_bwd");
  SIMCLR_CHECK_ARG(g && x && dw && db && workspace, "logreg_bwd: null argument");
  SIMCLR_CHECK_ARG(sweep::al16(g) && sweep::al16(x) && sweep::al16(dw) && sweep::al16(db) && sweep::al16(workspace),
                   "logreg_bwd: every pointer must be 16-byte aligned");
  const LrPlan p = lr_plan(n, D, C);
  const int cpad = lr_pitch(C);
  float* part = (float*)((char*)workspace + p.off_part);
  double* dbpart = (double*)((char*)workspace + p.off_db);
  dim3 grid(ceil_div(C, p.be), ceil_div(D, p.be), p.P);
  if (p.be == 128) hipLaunchKernelGGL(lr_bwd<4>, grid, dim3(256), 0, stream, g, x, n, D, C, cpad, p.part_rows, part);
  else hipLaunchKernelGGL(lr_bwd<2>, grid, dim3(256), 0, stream, g, x, n, D, C, cpad, p.part_rows, part);
  SIMCLR_CHECK_LAUNCH();
  hipLaunchKernelGGL(lr_db, dim3(ceil_div(C, gram_tile::kCols), p.chunks), dim3(256), 0, stream, g, n, C, cpad, dbpart);
  SIMCLR_CHECK_LAUNCH();
  hipLaunchKernelGGL(lr_reduce, dim3(ceil_div((long long)C * D + C, 256)), dim3(256), 0, stream, (const float*)part, p.P,
                     (const double*)dbpart, p.chunks, C, D, dw, db, accumulate ? 1 : 0);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
