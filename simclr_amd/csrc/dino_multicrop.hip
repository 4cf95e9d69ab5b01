// DINO multi-crop (Caron et al. 2021, section 3.1 and the official loss with ncrops = 2 + L) for gfx950: the key-side backward of the
// LOCAL term, the cross-entropy of every local (low-resolution) view's K-way student softmax against the teacher rows of BOTH global
// views of its image.
//
//   x [L b, D] = the l2-normalised local rows, view-major (row v b + i = local view v of image i);  ws / wt [K, D] = the row-normalised
//   prototypes of the online / the target network;  k [2b, D] = the normalised GLOBAL keys;  c [K] = the centre
//   s_rj = x_r . ws_j / Ts,  Ps = softmax_j(s_r),  t_gj = (k_g . wt_j - c_j) / Tt,  Pt[g] = softmax_j(t_g)  (global row g's OWN row)
//   u_g = sum_j Pt[g, j] ws_j (what simclr_dino_fwd returns for row g),  i = r mod b,  V = 2 + L,  cst = 1 / (2 (V - 1) b)
//   value = cst sum_r (2 lse(s_r) - x_r . (u_i + u_{b+i}) / Ts)            (sum_j Pt[g, j] s_rj = x_r . u_g / Ts: a logit is linear in ws_j)
//   d value / d ws_j = (cst / Ts) (2 sum_r Ps[r, j] x_r - sum_{g < 2b} Pt[g, j] m_g),   m_g = sum_v x_{v b + (g mod b)}
// The value and d value / d x_r read (x, ws, u, L, Ts) only: simclr_swav_local_fwd / simclr_swav_local_bwd_x compute them as they are
// (csrc/swav_multicrop.hip), and the row_stats [L b] they return -- lse_s per local row in the base-2 domain, m + log2(1 + r) of the
// logit x_r . ws_j * (log2 e / Ts) rounded ONCE after the product -- are what the student sweep here normalises with.  Only the
// key-side backward is DINO's own: the teacher rows are recomputed from the momentum keys, the target prototypes and the centre.
//
// THE lse_t OF THE ROW ITSELF.  csrc/dino.hip's key-side sweep streams online row r beside the PAIRED key p(r) and so reads
// row_stats[2 p(r) + 1].  The teacher sweep here streams global row g with its own key k_g: it reads row_stats[2 g + 1].  The
// multiplier tile is m at row g mod b.
//
// Sweeps as in csrc/dino.hip: S = X W^T tile by tile on v_mfma_f32_16x16x4_f32 (exact f32), a workgroup owns 64 prototypes held as
// MFMA fragments and streams 64-row XOR-swizzled LDS tiles, the probabilities are exp2(rounded base-2 logit - saved lse), the row
// splits are merged in a fixed order, no atomics: two calls are bitwise equal.
//
// MFMA mapping, tile stager (plain and WRAPPED rows) and S fragment: csrc/sweep_tile.h.  The prototypes are the fixed side.
#include "sweep_tile.h"

namespace {

using namespace sweep;

constexpr int kMaxK = 1 << 20;
constexpr int kMaxRows = 1 << 22;
constexpr int kMaxL = 8;

// m [b, D]: m_i = x_i + x_{b+i} + ... + x_{(L-1) b + i}, the views added in the order 0, 1, ...; one 16-byte chunk per thread
__global__ __launch_bounds__(256) void dinol_build_m(const float* __restrict__ x, int b, int L, int D, float* __restrict__ m) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long per_view = (long long)b * (D / 4);
  if (idx >= per_view) return;
  float4 acc = *(const float4*)(x + idx * 4);
  for (int v = 1; v < L; ++v) {
    const float4 t = *(const float4*)(x + ((long long)v * per_view + idx) * 4);
    acc.x += t.x; acc.y += t.y; acc.z += t.z; acc.w += t.w;
  }
  *(float4*)(m + idx * 4) = acc;
}

// ---- key-side sweeps: wpart[split][j] = sum over the split's streamed rows of P[row, j] mult[row] --------------------------------------
// TEACHER = false, the student term: src = x [rows = L b, D], the rows multiply themselves, P = exp2(x_r . ws_j scale2 - lse_s[r]) with
//   lse_s = stats[r] (simclr_swav_local_fwd's row_stats).
// TEACHER = true, the teacher term: src = k [rows = 2b, D], mult = m [b, D] wrapped (row g mod b), w = wt, P = exp2((k_g . wt_j - c_j)
//   scale2 - lse_t[g]) with lse_t = stats[2 g + 1] -- the row's OWN entry of simclr_dino_fwd's row_stats.  The subtraction and the
//   product are csrc/dino.hip's two roundings, so that lse_t normalises exactly this number.
template <int D, bool TEACHER>
__global__ __launch_bounds__(256) void dinol_bwd_w_sweep(const float* __restrict__ src, const float* __restrict__ mult,
                                                         const float* __restrict__ w, const float* __restrict__ center, int rows, int b,
                                                         int K, float scale2, const float* __restrict__ stats, int tiles_per_split,
                                                         float* __restrict__ wpart, int k_pad) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* ldm = TEACHER ? lds + kTile * D : lds;              // the multiplier tile
  float* lst = lds + (TEACHER ? 2 : 1) * kTile * D;          // the lse of the 64 streamed rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, fl = lane & 15;
  const int proto = blockIdx.x * kTile + wave * 16 + fl;
  const bool pv = proto < K;
  float4 ff[D / 16];
#pragma unroll
  for (int s = 0; s < D / 16; ++s)
    ff[s] = pv ? *(const float4*)(w + (size_t)proto * D + 16 * s + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
  const float cj = (TEACHER && pv) ? center[proto] : 0.f;
  f32x4 dacc[D / 16];
#pragma unroll
  for (int i = 0; i < D / 16; ++i) dacc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int ntiles = (rows + kTile - 1) / kTile;
  const int tile_begin = blockIdx.y * tiles_per_split;
  const int tile_end = min(ntiles, tile_begin + tiles_per_split);
  for (int rt = tile_begin; rt < tile_end; ++rt) {
    __syncthreads();
    load_tile<D>(lds, src, rt * kTile, rows, tid);
    if (TEACHER) load_tile<D, RowMap::kWrapped>(ldm, mult, rt * kTile, rows, tid);    // rows = 2b: row g reads m at g mod b
    if (tid < kTile) {
      const int row = rt * kTile + tid;
      lst[tid] = row < rows ? stats[TEACHER ? 2 * row + 1 : row] : 0.f;
    }
    __syncthreads();
#pragma unroll 1                           // a fragment set and an accumulator set live: keep the loop rolled as dino_bwd_w_sweep does
    for (int sub = 0; sub < 4; ++sub) {
      const f32x4 as = s_frag<D>(lds, sub, fl, g, ff);
      const int row0 = rt * kTile + sub * 16 + g * 4;  // streamed row of as[0]
      const float4 l4 = *(const float4*)(lst + sub * 16 + 4 * g);
      const float ll[4] = {l4.x, l4.y, l4.z, l4.w};
      float ds[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float t = TEACHER ? (as[i] - cj) * scale2 : as[i] * scale2;
        asm volatile("" : "+v"(t));        // the statistics sweeps' rounded logit
        ds[i] = (pv && row0 + i < rows) ? exp2f(t - ll[i]) : 0.f;
      }
      // dW^T[d][prototype] += sum_row mult[row][d] * P[row][prototype]
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int srow = sub * 16 + 4 * g + u;
          const int dcol = dt * 16 + fl;
          const float av = ldm[srow * D + ((((dcol >> 2) ^ (srow & 15)) << 2) | (dcol & 3))];
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

// dws_j = coeff * (2 sum_split spart[split][j] - sum_split tpart[split][j]), each sum in its fixed split order
__global__ __launch_bounds__(256) void dinol_combine_w(const float* __restrict__ spart, int ns, const float* __restrict__ tpart, int nt,
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
  for (int s = 0; s < nt; ++s) {
    const float4 v = *(const float4*)(tpart + ((size_t)s * k_pad + r) * D + c * 4);
    e.x += v.x; e.y += v.y; e.z += v.z; e.w += v.w;
  }
  *(float4*)(dst + (size_t)r * D + c * 4) = make_float4(coeff * (2.f * a.x - e.x), coeff * (2.f * a.y - e.y),
                                                        coeff * (2.f * a.z - e.z), coeff * (2.f * a.w - e.w));
}

// rs / rtiles: row split of the student sweep over the L b local rows; ts / ttiles: of the teacher sweep over the 2b global rows --
// ~256 workgroups each, the target of csrc/dino.hip's key-side sweep
struct Plan { int rows, k_pad, b_pad, rs, rtiles, ts, ttiles; };
Plan make_plan(int b, int L, int K) {
  Plan p;
  p.rows = b * L;
  const int xtiles = ceil_div(p.rows, kTile), ktiles = ceil_div(K, kTile), gtiles = ceil_div(2 * b, kTile);
  p.k_pad = ktiles * kTile;
  p.b_pad = ceil_div(b, 4) * 4;
  constexpr int wgs = 256;
  const int rs = max(1, min(xtiles, wgs / max(1, ktiles)));
  p.rtiles = ceil_div(xtiles, rs);
  p.rs = ceil_div(xtiles, p.rtiles);
  const int ts = max(1, min(gtiles, wgs / max(1, ktiles)));
  p.ttiles = ceil_div(gtiles, ts);
  p.ts = ceil_div(gtiles, p.ttiles);
  return p;
}
// workspace (4-byte words): [m | student partials | teacher partials]
size_t off_spart(const Plan& p, int D) { return (size_t)p.b_pad * D; }
size_t off_tpart(const Plan& p, int D) { return off_spart(p, D) + (size_t)p.rs * p.k_pad * D; }
size_t total_words(const Plan& p, int D) { return off_tpart(p, D) + (size_t)p.ts * p.k_pad * D; }

bool shape_ok(int b, int L, int K) {
  return b >= 1 && L >= 1 && L <= kMaxL && (long long)b * L <= kMaxRows && 2LL * b <= kMaxRows && K >= 2 && K <= kMaxK;
}

}  // namespace

extern "C" {

size_t simclr_dino_local_workspace_bytes(int b, int L, int K, int D) {
  if (!shape_ok(b, L, K) || !dim_ok(D)) return 0;
  return total_words(make_plan(b, L, K), D) * sizeof(float);
}

int simclr_dino_local_row_splits(int b, int L, int K) {
  if (!shape_ok(b, L, K)) return 0;
  return make_plan(b, L, K).rs;
}

int simclr_dino_local_teacher_row_splits(int b, int L, int K) {
  if (!shape_ok(b, L, K)) return 0;
  return make_plan(b, L, K).ts;
}

int simclr_dino_local_bwd_w(const float* x, const float* k, const float* ws, const float* wt, const float* center, int b, int L, int K,
                            int D, float student_temp, float teacher_temp, const float* local_row_stats,
                            const float* global_row_stats, float grad_scale, float* dws, void* workspace, hipStream_t stream) {
  SIMCLR_CHECK_ARG(dim_ok(D), "dino_local_bwd_w: D must be 64/128/256 (got %d)", D);
  SIMCLR_CHECK_ARG(shape_ok(b, L, K), "dino_local_bwd_w: need b >= 1, L in [1, 8] and K in [2, 1048576] (b=%d L=%d K=%d)", b, L, K);
  SIMCLR_CHECK_ARG(pos_finite(student_temp) && pos_finite(teacher_temp), "dino_local_bwd_w: the temperatures must be > 0 and finite");
  SIMCLR_CHECK_ARG(al16(x) && al16(k) && al16(ws) && al16(wt) && al16(dws) && al16(workspace) && al4(center) && al4(local_row_stats) &&
                       al8(global_row_stats),
                   "dino_local_bwd_w: null argument, or x / k / ws / wt / dws / workspace not 16-byte aligned");
  const Plan p = make_plan(b, L, K);
  float* wsp = (float*)workspace;
  float* m = wsp;
  float* spart = wsp + off_spart(p, D);
  float* tpart = wsp + off_tpart(p, D);
  const float scale2s = kLog2e / student_temp, scale2t = kLog2e / teacher_temp;
  const size_t lds_s = ((size_t)kTile * D + kTile) * sizeof(float), lds_t = ((size_t)2 * kTile * D + kTile) * sizeof(float);
  const dim3 grid_s(p.k_pad / kTile, p.rs), grid_t(p.k_pad / kTile, p.ts);
  // every refusal comes before the first launch: the LDS limits are raised (or refused) first
#define RAISE(DD)                                                                                                                   \
  SIMCLR_CHECK_ARG(raise_lds(dinol_bwd_w_sweep<DD, false>, lds_s) && raise_lds(dinol_bwd_w_sweep<DD, true>, lds_t),                 \
                   "dino_local_bwd_w: %d bytes of LDS refused", (int)lds_t)
  if (D == 64) RAISE(64); else if (D == 128) RAISE(128); else RAISE(256);
#undef RAISE
  const long long mchunks = (long long)b * (D / 4);
  hipLaunchKernelGGL(dinol_build_m, dim3((unsigned)((mchunks + 255) / 256)), dim3(256), 0, stream, x, b, L, D, m);
  SIMCLR_CHECK_LAUNCH();
#define LAUNCH_BWD(DD)                                                                                                              \
  do {                                                                                                                              \
    hipLaunchKernelGGL((dinol_bwd_w_sweep<DD, false>), grid_s, dim3(256), lds_s, stream, x, (const float*)nullptr, ws,              \
                       (const float*)nullptr, p.rows, b, K, scale2s, local_row_stats, p.rtiles, spart, p.k_pad);                    \
    SIMCLR_CHECK_LAUNCH();                                                                                                          \
    hipLaunchKernelGGL((dinol_bwd_w_sweep<DD, true>), grid_t, dim3(256), lds_t, stream, k, (const float*)m, wt, center, 2 * b, b,   \
                       K, scale2t, global_row_stats, p.ttiles, tpart, p.k_pad);                                                     \
  } while (0)
  if (D == 64) LAUNCH_BWD(64); else if (D == 128) LAUNCH_BWD(128); else LAUNCH_BWD(256);
#undef LAUNCH_BWD
  SIMCLR_CHECK_LAUNCH();
  // cst / Ts with cst = 1 / (2 (V - 1) b), V = 2 + L
  const float coeff = grad_scale / (student_temp * 2.f * (float)(L + 1) * (float)b);
  const long long chunks = (long long)K * (D / 4);
  hipLaunchKernelGGL(dinol_combine_w, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, stream, spart, p.rs, tpart, p.ts, p.k_pad,
                     K, D, coeff, dws);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
