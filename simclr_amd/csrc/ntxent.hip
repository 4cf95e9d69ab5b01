// Fused NT-Xent (SimCLR contrastive loss) forward + backward for gfx950.
//
// Replaces the un-fused TF graph of /root/reference/tf2/objective.py:53-87 (four
// [n,N] matmuls, a -1e9 diagonal mask, two 2N-wide softmax cross-entropies) and the
// consumers of logits_ab in /root/reference/tf2/metrics.py:28-35 with a flash-style
// sweep: S = Q.K^T/T is produced tile by tile on the fp32-input matrix cores
// (v_mfma_f32_16x16x4_f32, exact f32), reduced online (running max / sum-exp per
// row, per lane, merged with wave shuffles) and never written to HBM.
//
// Formulation.  Q = [z1_local; z2_local]  (2n rows, this replica's views),
//               K = [z1_all;   z2_all  ]  (2N rows, all replicas; N = R*n).
// For query row q:   q <  n (view a, i=q):   masked col = rank*n+i     (the aa diagonal,
//                                              objective.py:76-77), positive col = N+rank*n+i (ab)
//                    q >= n (view b, i=q-n): masked col = N+rank*n+i   (bb diagonal, :78-79),
//                                              positive col = rank*n+i (ba)
// loss = (1/n) sum_q [ logsumexp_{col != masked} S[q,col] - S[q,pos] ]      (:83-87)
// The masked column is skipped rather than shifted by -1e9 (exp(-1e9)=0 in fp32).
//
// MFMA mapping (16x16x4 f32): a = streamed tile row fragment, b = fixed-row fragment,
// so D[streamed=(lane>>4)*4+reg][fixed=lane&15]: every lane owns ONE fixed row and 4
// streamed rows per 16x16 tile -> the online softmax is lane-local; only the final
// merge over the 4 lane groups needs shuffles (xor 16, 32).
//
// The un-pipelined tile stager, the S fragment and the online (max, sum) are csrc/sweep_tile.h's; the wide path's staged-k Gram tile
// is csrc/gram_tile.h's.
#include "gram_tile.h"
#include "sweep_tile.h"
#include <stdlib.h>

namespace {

using namespace sweep;

constexpr float kLn2 = 0.6931471805599453f;
constexpr int kPartStride = 8; // floats per (split,row) partial record

__device__ __forceinline__ void row_cols(int q, int n, int N, int rank, int& mask_col, int& pos_col) {
  if (q < n) { mask_col = rank * n + q; pos_col = N + rank * n + q; }
  else { int i = q - n; mask_col = N + rank * n + i; pos_col = rank * n + i; }
}

// A streamed tile (kTile rows x D floats) travels global -> registers -> LDS: tile_fetch issues the loads of the NEXT tile
// before the MFMAs of the current one, tile_store puts them into the (XOR-swizzled) LDS tile after the barrier -- the
// global latency runs under the matrix work instead of between two barriers.
template <int D>
__device__ __forceinline__ void tile_fetch(float4* pf, const float* __restrict__ src, int row0, int nrows_total, int tid) {
  constexpr int C = D / 4;
#pragma unroll
  for (int j = 0; j < kTile * C / 256; ++j) {
    const int idx = tid + j * 256, r = idx / C, c = idx % C;
    pf[j] = (row0 + r < nrows_total) ? *(const float4*)(src + (size_t)(row0 + r) * D + c * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}
template <int D>
__device__ __forceinline__ void tile_store(float* lds, const float4* pf, int tid) {
  constexpr int C = D / 4;
#pragma unroll
  for (int j = 0; j < kTile * C / 256; ++j) {
    const int idx = tid + j * 256, r = idx / C, c = idx % C;
    *(float4*)(lds + r * D + ((c ^ (r & 15)) * 4)) = pf[j];
  }
}

// The backward sweeps use the un-pipelined sweep::load_tile: each 16-byte piece goes global -> LDS straight away.

// ---- split-fp16 sweeps (round 6, opt-in: D argument carries SIMCLR_FMT_TERMS(13)) ------------------------------------------------
// The sweeps are bound by the fp32-input matrix pipe (v_mfma_f32_16x16x4_f32: 1/16 of the 16-bit rate).  l2-normalised rows
// (tf2/objective.py:53-54) lie in [-1, 1] -- inside fp16's range -- so every fp32 product can run as THREE fp16-piece terms
// (x = hi + lo, 11-bit pieces: hi*hi + hi*lo + lo*hi, ~2^-22 per product; csrc/conv.hip mma_f32_chunks has the argument) on
// v_mfma_f32_16x16x32_f16: the logits carry ~2^-22 / T absolute error, three decimal orders inside the 2e-5 fixture gates at T = 0.1.
// The streamed tile sits in LDS PRE-SPLIT (common.h block format per 128-byte block, 16-byte slots XOR-swizzled by the row): the
// S = Q K^T fragments are two 16-byte reads (hi, lo) per 32-element k-step, the transposed fragments of the second product
// (dF += T^T dS) come from ds_read_b64_tr_b16 on the hi / lo runs, and dS is split in registers.  Not for un-normalised inputs.
typedef __attribute__((ext_vector_type(8))) _Float16 nt_f16x8;
typedef __attribute__((ext_vector_type(4))) short nt_s16x4;
typedef __attribute__((address_space(3))) nt_s16x4 nt_lds_s16x4;
__device__ __forceinline__ f32x4 nt_mma_f16(const u32x4& a, const u32x4& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(nt_f16x8, a), __builtin_bit_cast(nt_f16x8, b), c, 0, 0, 0);
}
// byte offset of 16-byte slot `slot` (block * 8 + t) of row r in a pre-split LDS tile of D floats per row
template <int D> __device__ __forceinline__ int ps_slot(int r, int slot) { return r * (D * 4) + ((slot ^ (r & 15)) << 4); }
// one 16-byte fp32 chunk (channels 4c..4c+3 of row r) -> its hi quad and lo quad in the pre-split tile
template <int D> __device__ __forceinline__ void ps_put(unsigned char* lds, int r, int c, const float4& v) {
  uint32_t h0, l0, h1, l1;
  split_pair<true>(v.x, v.y, h0, l0);
  split_pair<true>(v.z, v.w, h1, l1);
  const int b = c >> 3, cc = c & 7;
  unsigned char* p = lds + ps_slot<D>(r, b * 8 + (cc & 3)) + (cc >> 2) * 8;
  *(u32x2*)p = (u32x2){h0, h1};
  *(u32x2*)(lds + ps_slot<D>(r, b * 8 + 4 + (cc & 3)) + (cc >> 2) * 8) = (u32x2){l0, l1};
}
template <int D>
__device__ __forceinline__ void tile_store_ps(float* lds, const float4* pf, int tid) {
  constexpr int C = D / 4;
#pragma unroll
  for (int j = 0; j < kTile * C / 256; ++j) {
    const int idx = tid + j * 256;
    ps_put<D>((unsigned char*)lds, idx / C, idx % C, pf[j]);
  }
}
template <int D>
__device__ __forceinline__ void load_tile_ps(float* lds, const float* __restrict__ src, int row0, int nrows_total, int tid) {
  constexpr int C = D / 4;
  for (int idx = tid; idx < kTile * C; idx += 256) {
    const int r = idx / C, c = idx % C;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row0 + r < nrows_total) v = *(const float4*)(src + (size_t)(row0 + r) * D + c * 4);
    ps_put<D>((unsigned char*)lds, r, c, v);
  }
}
// this lane's fixed-row operand of 32-element k-step s (floats 32 s + 4 g .. and 32 s + 16 + 4 g ..) as fp16 pieces
__device__ __forceinline__ void split_fixed(const float4& a, const float4& b, u32x4& hi, u32x4& lo) {
  uint32_t h, l;
  split_pair<true>(a.x, a.y, h, l); hi[0] = h; lo[0] = l;
  split_pair<true>(a.z, a.w, h, l); hi[1] = h; lo[1] = l;
  split_pair<true>(b.x, b.y, h, l); hi[2] = h; lo[2] = l;
  split_pair<true>(b.z, b.w, h, l); hi[3] = h; lo[3] = l;
}
// S fragment (16 streamed rows x 16 fixed rows) of one sub-tile from the pre-split tile: acc[r] = <T[sub*16 + 4g + r], F[fl]>
template <int D>
__device__ __forceinline__ f32x4 s_frag_f16(const float* lds, int trow, int g, const u32x4* ffh, const u32x4* ffl) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const unsigned char* base = (const unsigned char*)lds;
#pragma unroll
  for (int s = 0; s < D / 32; ++s) {
    const u32x4 th = *(const u32x4*)(base + ps_slot<D>(trow, s * 8 + g));
    const u32x4 tl = *(const u32x4*)(base + ps_slot<D>(trow, s * 8 + 4 + g));
    acc = nt_mma_f16(tl, ffh[s], acc);
    acc = nt_mma_f16(th, ffl[s], acc);
    acc = nt_mma_f16(th, ffh[s], acc);
  }
  return acc;
}

__device__ __forceinline__ void arg_merge(float& v, int& i, float v2, int i2) {
  if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
}

// ------------------------------------------------------------------------------
// Forward sweep: per (query row, key split) partial statistics.
// part[split][row][8] = {m0, l0, m1, l1, pos, argval, argidx(bits), 0}
//   set0 = key cols [0,N), set1 = key cols [N,2N); values are logits*log2(e).
// ------------------------------------------------------------------------------
template <int D, bool F16 = false>
__global__ __launch_bounds__(256) void ntxent_fwd_partial(
    const float* __restrict__ zq, const float* __restrict__ zk, int n, int N, int rank,
    float scale2 /* log2(e)/T */, int tiles_per_split, float* __restrict__ part, int rows_pad) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, fl = lane & 15;
  const int q = blockIdx.x * kTile + wave * 16 + fl;
  const int two_n = 2 * n, two_N = 2 * N;
  int mask_col, pos_col;
  row_cols(q, n, N, rank, mask_col, pos_col);

  float4 ff[D / 16];
#pragma unroll
  for (int s = 0; s < D / 16; ++s) {
    ff[s] = (q < two_n) ? *(const float4*)(zq + (size_t)q * D + 16 * s + 4 * g)
                        : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float m0 = -INFINITY, l0 = 0.f, m1 = -INFINITY, l1 = 0.f, pos = -INFINITY, av = -INFINITY;
  int ai = 0x7fffffff;
  u32x4 ffh[D / 32], ffl[D / 32];
  if constexpr (F16) {
#pragma unroll
    for (int s = 0; s < D / 32; ++s) split_fixed(ff[2 * s], ff[2 * s + 1], ffh[s], ffl[s]);
  }

  const int tile_begin = blockIdx.y * tiles_per_split;
  const int ntiles = (two_N + kTile - 1) / kTile;
  const int tile_end = min(ntiles, tile_begin + tiles_per_split);
  float4 pf[kTile * (D / 4) / 256];
  if (tile_begin < tile_end) tile_fetch<D>(pf, zk, tile_begin * kTile, two_N, tid);
  for (int kt = tile_begin; kt < tile_end; ++kt) {
    __syncthreads();
    if constexpr (F16) tile_store_ps<D>(lds, pf, tid); else tile_store<D>(lds, pf, tid);
    __syncthreads();
    if (kt + 1 < tile_end) tile_fetch<D>(pf, zk, (kt + 1) * kTile, two_N, tid);
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const int trow = sub * 16 + fl;
      if constexpr (F16) {
        acc = s_frag_f16<D>(lds, trow, g, ffh, ffl);
      } else {
      // sweep::s_frag's loop, spelled out here and in ntxent_bwd_sweeps: the call form costs this kernel 32 bytes and changes that
      // one's register counts
#pragma unroll
      for (int s = 0; s < D / 16; ++s) {
        float4 tf = *(const float4*)(lds + trow * D + (((4 * s + g) ^ (trow & 15)) * 4));
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(tf.x, ff[s].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(tf.y, ff[s].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(tf.z, ff[s].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(tf.w, ff[s].w, acc, 0, 0, 0);
      }
      }
      const int col0 = kt * kTile + sub * 16 + g * 4;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int col = col0 + r;
        const float t = acc[r] * scale2;
        if (col == pos_col) pos = t;
        if (col < two_N && col != mask_col) {
          if (col < N) {
            float mn = fmaxf(m0, t);
            l0 = l0 * exp2f(m0 - mn) + exp2f(t - mn);
            m0 = mn;
          } else {
            float mn = fmaxf(m1, t);
            l1 = l1 * exp2f(m1 - mn) + exp2f(t - mn);
            m1 = mn;
            if (t > av || (t == av && col < ai)) { av = t; ai = col; }
          }
        }
      }
    }
  }
  // merge the 4 lane groups that share this fixed row
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {
    float om0 = __shfl_xor(m0, o, 64), ol0 = __shfl_xor(l0, o, 64);
    float om1 = __shfl_xor(m1, o, 64), ol1 = __shfl_xor(l1, o, 64);
    float op = __shfl_xor(pos, o, 64), oav = __shfl_xor(av, o, 64);
    int oai = __shfl_xor(ai, o, 64);
    ml_merge(m0, l0, om0, ol0);
    ml_merge(m1, l1, om1, ol1);
    pos = fmaxf(pos, op);
    arg_merge(av, ai, oav, oai);
  }
  if (g == 0 && q < two_n) {
    float* p = part + ((size_t)blockIdx.y * rows_pad + q) * kPartStride;
    p[0] = m0; p[1] = l0; p[2] = m1; p[3] = l1; p[4] = pos; p[5] = av;
    p[6] = __int_as_float(ai); p[7] = 0.f;
  }
}

// ------------------------------------------------------------------------------
// Finalize, part 1: merge the key splits of every query row -- 16 lanes per row (lane j merges splits j, j+16, ...;
// a fixed xor-shuffle tree joins them), 16 rows per 256-thread workgroup.  Writes row_stats[row] = {lse_full2, lse_ab2}
// and rowterm[row] = {loss term, arg-max hit}.  Part 2 (ntxent_reduce_out) adds the row terms in a fixed order:
// out[0] = loss, out[1] = contrast_acc.  (The former single-workgroup finalize serialised 2n * nsplit dependent loads.)
// ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ntxent_finalize_rows(const float* __restrict__ part, int nsplit,
                                                            int rows_pad, int n, int N, int rank,
                                                            float* __restrict__ row_stats,
                                                            float* __restrict__ rowterm) {
  const int q = blockIdx.x * 16 + (threadIdx.x >> 4);
  const int j = threadIdx.x & 15;
  float m0 = -INFINITY, l0 = 0.f, m1 = -INFINITY, l1 = 0.f, pos = -INFINITY, av = -INFINITY;
  int ai = 0x7fffffff;
  if (q < 2 * n) {
    for (int s = j; s < nsplit; s += 16) {
      const float4 a = *(const float4*)(part + ((size_t)s * rows_pad + q) * kPartStride);
      const float4 b = *(const float4*)(part + ((size_t)s * rows_pad + q) * kPartStride + 4);
      ml_merge(m0, l0, a.x, a.y);
      ml_merge(m1, l1, a.z, a.w);
      pos = fmaxf(pos, b.x);
      arg_merge(av, ai, b.y, __float_as_int(b.z));
    }
  }
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) {
    float om0 = __shfl_xor(m0, o, 64), ol0 = __shfl_xor(l0, o, 64);
    float om1 = __shfl_xor(m1, o, 64), ol1 = __shfl_xor(l1, o, 64);
    float op = __shfl_xor(pos, o, 64), oav = __shfl_xor(av, o, 64);
    int oai = __shfl_xor(ai, o, 64);
    ml_merge(m0, l0, om0, ol0);
    ml_merge(m1, l1, om1, ol1);
    pos = fmaxf(pos, op);
    arg_merge(av, ai, oav, oai);
  }
  if (j == 0 && q < 2 * n) {
    const float lse_ab2 = m1 + log2f(l1);
    float mf = m0, lf = l0;
    ml_merge(mf, lf, m1, l1);
    const float lse2 = mf + log2f(lf);
    row_stats[2 * q] = lse2;
    row_stats[2 * q + 1] = lse_ab2;
    int mask_col, pos_col;
    row_cols(q, n, N, rank, mask_col, pos_col);
    rowterm[2 * q] = (lse2 - pos) * kLn2;
    rowterm[2 * q + 1] = (q < n && ai == pos_col) ? 1.f : 0.f;
  }
}

__global__ __launch_bounds__(256) void ntxent_reduce_out(const float* __restrict__ rowterm, int n, float* __restrict__ out) {
  __shared__ double sh_loss[256];
  __shared__ double sh_hit[256];
  double loss = 0.0, hit = 0.0;
  for (int q = threadIdx.x; q < 2 * n; q += 256) { loss += (double)rowterm[2 * q]; hit += (double)rowterm[2 * q + 1]; }
  sh_loss[threadIdx.x] = loss;
  sh_hit[threadIdx.x] = hit;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      sh_loss[threadIdx.x] += sh_loss[threadIdx.x + s];
      sh_hit[threadIdx.x] += sh_hit[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = (float)(sh_loss[0] / n);
    out[1] = (float)(sh_hit[0] / n);
  }
}

// ------------------------------------------------------------------------------
// Backward sweep (recomputes S).  FIXED_IS_QUERY=true : fixed rows = queries,
//   streamed = keys,  gpart[split][q][D]   = sum_keys dS[q,key] * K[key,:]
// FIXED_IS_QUERY=false: fixed rows = keys, streamed = queries,
//   gpart[split][key][D] = sum_q dS[q,key] * Q[q,:]
// dS = softmax - onehot(pos) (masked col -> 0); the 1/(n*T) * upstream factor is
// applied by the combine kernel.  The query-fixed instance also accumulates the
// contrast-entropy term of tf2/metrics.py:33-35 (a rows, ab block only).
// ------------------------------------------------------------------------------
template <int D, bool FIXED_IS_QUERY, bool F16 = false>
__device__ __forceinline__ void ntxent_bwd_sweep_body(
    float* lds, const float* __restrict__ fixed_mat, int fixed_rows, const float* __restrict__ stream_mat,
    int stream_rows, int n, int N, int rank, float scale2, const float* __restrict__ row_stats,
    int tiles_per_split, float* __restrict__ gpart, int rows_pad, float* __restrict__ epart) {
  float* stats_s = lds + kTile * D;  // [64][2] row stats of the streamed queries (key-fixed mode)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, fl = lane & 15;
  const int f = blockIdx.x * kTile + wave * 16 + fl;
  const int two_N = 2 * N, two_n = 2 * n;

  float4 ff[D / 16];
#pragma unroll
  for (int s = 0; s < D / 16; ++s) {
    ff[s] = (f < fixed_rows) ? *(const float4*)(fixed_mat + (size_t)f * D + 16 * s + 4 * g)
                             : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  int f_mask = -1, f_pos = -1;
  float f_lse = 0.f, f_lse_ab = 0.f;
  if (FIXED_IS_QUERY) {
    row_cols(f, n, N, rank, f_mask, f_pos);
    if (f < two_n) { f_lse = row_stats[2 * f]; f_lse_ab = row_stats[2 * f + 1]; }
  }
  f32x4 dacc[D / 16];
#pragma unroll
  for (int i = 0; i < D / 16; ++i) dacc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float ent = 0.f;

  const int ntiles = (stream_rows + kTile - 1) / kTile;
  const int tile_begin = blockIdx.y * tiles_per_split;
  const int tile_end = min(ntiles, tile_begin + tiles_per_split);
  // (prefetching one tile ahead into registers, as the forward sweep does, was measured SLOWER here: on top of the 32 + 32
  // accumulator / fixed-row registers it costs a wave of occupancy or spills -- cfg3 shape 183 -> 193 us, profiles/r03_notes.md)
  u32x4 ffh[D / 32], ffl[D / 32];
  if constexpr (F16) {
#pragma unroll
    for (int s = 0; s < D / 32; ++s) split_fixed(ff[2 * s], ff[2 * s + 1], ffh[s], ffl[s]);
  }
  // dS of one 16 x 16 fragment from its logits (acc): softmax - onehot(pos), masked column -> 0; entropy term of the ab block
  auto ds_of = [&](const f32x4& acc, int kt, int sub, float* ds) __attribute__((always_inline)) {
    const int s0 = kt * kTile + sub * 16 + g * 4;  // streamed row of acc[0]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float t = acc[r] * scale2;
      int q, col, mask_col, pos_col;
      float lse, lse_ab;
      if (FIXED_IS_QUERY) {
        q = f; col = s0 + r; mask_col = f_mask; pos_col = f_pos; lse = f_lse; lse_ab = f_lse_ab;
      } else {
        q = s0 + r; col = f;
        row_cols(q, n, N, rank, mask_col, pos_col);
        lse = stats_s[2 * (sub * 16 + g * 4 + r)];
        lse_ab = 0.f;
      }
      float d = 0.f;
      if (q < two_n && col < two_N && col != mask_col) {
        d = exp2f(t - lse);
        if (col == pos_col) d -= 1.f;
        if (FIXED_IS_QUERY && q < n && col >= N) {
          float pab = exp2f(t - lse_ab);
          ent -= pab * __logf(pab + 1e-8f);
        }
      }
      ds[r] = d;
    }
  };
  for (int kt = tile_begin; kt < tile_end; ++kt) {
    __syncthreads();
    if constexpr (F16) load_tile_ps<D>(lds, stream_mat, kt * kTile, stream_rows, tid);
    else load_tile<D>(lds, stream_mat, kt * kTile, stream_rows, tid);
    if (!FIXED_IS_QUERY && tid < 2 * kTile) {
      int qq = kt * kTile + (tid >> 1);
      stats_s[tid] = (qq < two_n) ? row_stats[2 * qq + (tid & 1)] : 0.f;
    }
    __syncthreads();
    if constexpr (F16) {
      const unsigned char* base = (const unsigned char*)lds;
#pragma unroll
      for (int sp = 0; sp < 2; ++sp) {
        float dsa[4], dsb[4];
        ds_of(s_frag_f16<D>(lds, (2 * sp) * 16 + fl, g, ffh, ffl), kt, 2 * sp, dsa);
        ds_of(s_frag_f16<D>(lds, (2 * sp + 1) * 16 + fl, g, ffh, ffl), kt, 2 * sp + 1, dsb);
        // dS of the 32 streamed rows of this sub-tile pair as fp16 pieces: k-slots 0..3 = rows 4g.. of the first, 4..7 of the second
        u32x4 dh, dl;
        { uint32_t h, l;
          split_pair<true>(dsa[0], dsa[1], h, l); dh[0] = h; dl[0] = l;
          split_pair<true>(dsa[2], dsa[3], h, l); dh[1] = h; dl[1] = l;
          split_pair<true>(dsb[0], dsb[1], h, l); dh[2] = h; dl[2] = l;
          split_pair<true>(dsb[2], dsb[3], h, l); dh[3] = h; dl[3] = l; }
        // dF^T[position][fixed] += sum_streamed T[streamed][position] * dS[streamed][fixed]: the transposed T fragments of run R
        // (16 positions of block R >> 1, run R & 1; hi then lo plane) come from ds_read_b64_tr_b16, rows 4g + (fl >> 2) of either sub-tile
        const int ra = (2 * sp) * 16 + 4 * g + (fl >> 2), rb = ra + 16;
#pragma unroll
        for (int R = 0; R < D / 16; ++R) {
          const int slot = (R >> 1) * 8 + 2 * (R & 1) + ((fl & 3) >> 1), half = (fl & 1) * 8;
          const nt_s16x4 a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((nt_lds_s16x4*)(base + ps_slot<D>(ra, slot) + half));
          const nt_s16x4 a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((nt_lds_s16x4*)(base + ps_slot<D>(rb, slot) + half));
          const nt_s16x4 b0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((nt_lds_s16x4*)(base + ps_slot<D>(ra, slot + 4) + half));
          const nt_s16x4 b1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((nt_lds_s16x4*)(base + ps_slot<D>(rb, slot + 4) + half));
          const u32x2 x0 = __builtin_bit_cast(u32x2, a0), x1 = __builtin_bit_cast(u32x2, a1);
          const u32x2 y0 = __builtin_bit_cast(u32x2, b0), y1 = __builtin_bit_cast(u32x2, b1);
          const u32x4 th = (u32x4){x0[0], x0[1], x1[0], x1[1]}, tl = (u32x4){y0[0], y0[1], y1[0], y1[1]};
          dacc[R] = nt_mma_f16(tl, dh, dacc[R]);
          dacc[R] = nt_mma_f16(th, dl, dacc[R]);
          dacc[R] = nt_mma_f16(th, dh, dacc[R]);
        }
      }
    } else {
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const int trow = sub * 16 + fl;
#pragma unroll
      for (int s = 0; s < D / 16; ++s) {
        float4 tf = *(const float4*)(lds + trow * D + (((4 * s + g) ^ (trow & 15)) * 4));
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(tf.x, ff[s].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(tf.y, ff[s].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(tf.z, ff[s].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(tf.w, ff[s].w, acc, 0, 0, 0);
      }
      float ds[4];
      ds_of(acc, kt, sub, ds);
      // dF^T[d][fixed] += sum_streamed T[streamed][d] * dS[streamed][fixed]
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int srow = sub * 16 + 4 * g + u;
          const int dcol = dt * 16 + fl;
          float a = lds[srow * D + ((((dcol >> 2) ^ (srow & 15)) << 2) | (dcol & 3))];
          dacc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, ds[u], dacc[dt], 0, 0, 0);
        }
      }
    }
    }
  }
  if (f < fixed_rows) {
    float* gp = gpart + ((size_t)blockIdx.y * rows_pad + f) * D;
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) {
      int d0 = dt * 16 + 4 * g;
      if constexpr (F16) {       // run dt of the pre-split tile: position 4 g + reg -> channel (common.h block layout)
        const int Q = 4 * (dt & 1) + g;
        d0 = (dt >> 1) * 32 + (Q & 1) * 16 + (Q >> 1) * 4;
      }
      *(float4*)(gp + d0) = make_float4(dacc[dt][0], dacc[dt][1], dacc[dt][2], dacc[dt][3]);
    }
  }
  if (FIXED_IS_QUERY) {
    ent += __shfl_xor(ent, 16, 64);
    ent += __shfl_xor(ent, 32, 64);
    if (g == 0 && f < two_n) epart[(size_t)blockIdx.y * rows_pad + f] = ent;
  }
}

// Both sweeps in ONE launch: blockIdx.z = 0 query-fixed (gradient wrt the local rows + the entropy term),
// blockIdx.z = 1 key-fixed (gradient wrt the gathered rows).  They are independent, so they share the chip.
template <int D, bool F16 = false>
__global__ __launch_bounds__(256) void ntxent_bwd_sweeps(
    const float* __restrict__ z_local, const float* __restrict__ z_all, int n, int N, int rank, float scale2,
    const float* __restrict__ row_stats, int tiles_k, int tiles_q, float* __restrict__ gq, int rows_pad_q,
    float* __restrict__ gk, int rows_pad_k, float* __restrict__ epart, int gxq, int gyq, int gxk, int gyk) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  if (blockIdx.z == 0) {
    if ((int)blockIdx.x >= gxq || (int)blockIdx.y >= gyq) return;
    ntxent_bwd_sweep_body<D, true, F16>(lds, z_local, 2 * n, z_all, 2 * N, n, N, rank, scale2, row_stats, tiles_k, gq,
                                   rows_pad_q, epart);
  } else {
    if ((int)blockIdx.x >= gxk || (int)blockIdx.y >= gyk) return;
    ntxent_bwd_sweep_body<D, false, F16>(lds, z_all, 2 * N, z_local, 2 * n, n, N, rank, scale2, row_stats, tiles_q, gk,
                                    rows_pad_k, (float*)nullptr);
  }
}

// One launch for the three tail reductions of the backward: dz_local = scale * sum_split gq, dz_all = scale * sum_split gk
// (fixed split order), and -- last workgroup -- out[2] = contrast entropy = (1/n) sum over a-rows and splits of epart.
__global__ __launch_bounds__(256) void ntxent_combine_all(const float* __restrict__ gq, int ksplit, int rows_pad_q, int rows_q,
                                                          const float* __restrict__ gk, int qsplit, int rows_pad_k, int rows_k,
                                                          int D, float scale, float* __restrict__ dz_local,
                                                          float* __restrict__ dz_all, const float* __restrict__ epart,
                                                          int n, float* __restrict__ out, int blocks_q, int blocks_k) {
  __shared__ double sh[256];
  const int b = blockIdx.x;
  if (b < blocks_q + blocks_k) {
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
    acc.x *= scale; acc.y *= scale; acc.z *= scale; acc.w *= scale;
    *(float4*)(dst + (size_t)r * D + c * 4) = acc;
    return;
  }
  double e = 0.0;
  for (int q = threadIdx.x; q < n; q += 256)
    for (int s = 0; s < ksplit; ++s) e += (double)epart[(size_t)s * rows_pad_q + q];
  sh[threadIdx.x] = e;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[2] = (float)(sh[0] / n);
}

// ---- l2 normalise (tf.math.l2_normalize, tf2/objective.py:53-54) -------------
// one wave per row: z = x * rsqrt(max(sum x^2, 1e-12))
__global__ void l2norm_fwd_kernel(const float* __restrict__ x, float* __restrict__ z,
                                  float* __restrict__ inv, int rows, int D) {
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  float ss = 0.f;
  for (int d = lane; d < D; d += 64) { float v = x[(size_t)row * D + d]; ss += v * v; }
  ss = wave_sum(ss);
  const float r = 1.0f / sqrtf(fmaxf(ss, 1e-12f));
  for (int d = lane; d < D; d += 64) z[(size_t)row * D + d] = x[(size_t)row * D + d] * r;
  if (lane == 0) inv[row] = r;
}
// dx = (dz - z * (z . dz)) * inv        (exact for sum x^2 > 1e-12)
__global__ void l2norm_bwd_kernel(const float* __restrict__ z, const float* __restrict__ inv,
                                  const float* __restrict__ dz, float* __restrict__ dx, int rows,
                                  int D) {
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  float dot = 0.f;
  for (int d = lane; d < D; d += 64) dot += z[(size_t)row * D + d] * dz[(size_t)row * D + d];
  dot = wave_sum(dot);
  const float r = inv[row];
  for (int d = lane; d < D; d += 64)
    dx[(size_t)row * D + d] = (dz[(size_t)row * D + d] - z[(size_t)row * D + d] * dot) * r;
}

// dense logits_ab materialisation for API parity (tf2/objective.py:80,89): [n, N]
__global__ void ntxent_logits_ab_kernel(const float* __restrict__ zq, const float* __restrict__ zk,
                                        int n, int N, int D, float inv_t, float* __restrict__ out) {
  const int i = blockIdx.y;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < N; j += gridDim.x * blockDim.x) {
    const float* a = zq + (size_t)i * D;
    const float* b = zk + (size_t)(N + j) * D;
    float s = 0.f;
    for (int d = 0; d < D; ++d) s = fmaf(a[d], b[d], s);
    out[(size_t)i * N + j] = s * inv_t;
  }
}

// fks / ftiles_k: key split of the FORWARD sweep (target ~512 workgroups); ksplit / qsplit: splits of the two backward sweeps (target
// ~256 workgroups each: their partial gradients are [split][rows][D] floats that the combine kernel re-reads -- fewer, longer ranges
// measured faster: cfg3 shape 101 -> 92 us with the split-fp16 sweeps, 178 -> 177 exact; the forward prefers 512: 43 vs 56 us).
struct Plan { int rows_pad_q, rows_pad_k, qsplit, ksplit, tiles_q, tiles_k, fks, ftiles_k; };
Plan make_plan(int n, int N) {
  Plan p;
  const int qtiles = ceil_div(2 * n, kTile), ktiles = ceil_div(2 * N, kTile);
  p.rows_pad_q = qtiles * kTile;
  p.rows_pad_k = ktiles * kTile;
  constexpr int wgs_f = 512, wgs_b = 256;      // sweep in profiles/r06_notes.md section 7 (256 / 384 / 512 / 768 / 1024)
  int fs = max(1, min(ktiles, wgs_f / max(1, qtiles)));
  p.ftiles_k = ceil_div(ktiles, fs);
  p.fks = ceil_div(ktiles, p.ftiles_k);
  int ks = max(1, min(ktiles, wgs_b / max(1, qtiles)));
  p.tiles_k = ceil_div(ktiles, ks);
  p.ksplit = ceil_div(ktiles, p.tiles_k);
  int qs = max(1, min(qtiles, wgs_b / max(1, ktiles)));
  p.tiles_q = ceil_div(qtiles, qs);
  p.qsplit = ceil_div(qtiles, p.tiles_q);
  return p;
}
// workspace layout: [forward partials | gq | gk | entropy partials | row terms]
size_t off_gq(const Plan& p) { return (size_t)p.fks * p.rows_pad_q * kPartStride; }
size_t off_gk(const Plan& p, int D) { return off_gq(p) + (size_t)p.ksplit * p.rows_pad_q * D; }
size_t off_ep(const Plan& p, int D) { return off_gk(p, D) + (size_t)p.qsplit * p.rows_pad_k * D; }
size_t off_rowterm(const Plan& p, int D) { return off_ep(p, D) + (size_t)p.ksplit * p.rows_pad_q; }
size_t ws_floats(int n, int N, int D) {
  Plan p = make_plan(n, N);
  return off_rowterm(p, D) + (size_t)2 * p.rows_pad_q;
}

// ==============================================================================
// Wide NT-Xent: any D (proj_out_dim > 256, proj_head_mode=none: the encoder's 512 ... 8192-wide pooled output).
// The sweeps above keep a whole D-wide row per lane in registers and a 64 x D tile in LDS, which stops at D = 256.  Here every
// product is the LDS-tiled, k-staged gram_tile::tile of csrc/gram_tile.h, on the same fp32-input MFMA (exact f32) and the same formulation:
//   forward   S = Q K^T (keys = MFMA rows, queries = lane columns) -> per (query, 16*W-key strip) partial row statistics in the
//             forward-sweep record format -> ntxent_finalize_rows / ntxent_reduce_out (fixed-order merges, shared with the sweeps);
//   backward  S recomputed -> dS = (softmax - onehot) * grad_scale / (n T) written ONCE as a [rows_pad_q, rows_pad_k] fp32 array
//             (plus the entropy partials) -> dz_local = dS K and dz_all = dS^T Q as two GEMMs, each output element one MFMA chain
//             over the whole k range (no split-k, no atomics: bitwise run-to-run deterministic).
// A workgroup (4 waves, 2 x 2) owns an E x E output tile, E = 32 W (W = 2: 64, W = 4: 128); a wave owns W x W 16x16 blocks.
// Loads past the logical extents read zeros, so D, n and N need no padding.
// ==============================================================================

// Forward: S tile (blockIdx.x = key tile, blockIdx.y = query tile) -> part[split][q][8] as ntxent_fwd_partial writes it, one split
// per (key tile, wave row): split = 2 * blockIdx.x + wm covers the 16 W keys of that wave row.
template <int W>
__global__ __launch_bounds__(256) void ntxent_wide_fwd_partial(const float* __restrict__ zq, const float* __restrict__ zk, int n,
                                                               int N, int D, int rank, float scale2, int vec,
                                                               float* __restrict__ part, int rows_pad) {
  __shared__ __attribute__((aligned(16))) float lds[2 * gram_tile::op_floats<32 * W>()];
  constexpr int E = 32 * W;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, fl = lane & 15, wm = wave & 1, wn = wave >> 1;
  const int two_n = 2 * n, two_N = 2 * N;
  const int m0 = blockIdx.x * E, n0 = blockIdx.y * E;
  f32x4 acc[W][W];
  gram_tile::tile<W, false, false>(lds, zk, D, two_N, vec, zq, D, two_n, vec, 0, D, m0, n0, acc);
#pragma unroll
  for (int w = 0; w < W; ++w) {
    const int q = n0 + 16 * W * wn + 16 * w + fl;
    int mask_col, pos_col;
    row_cols(q, n, N, rank, mask_col, pos_col);
    float m0s = -INFINITY, l0 = 0.f, m1 = -INFINITY, l1 = 0.f, pos = -INFINITY, av = -INFINITY;
    int ai = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < W; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int col = m0 + 16 * W * wm + 16 * i + 4 * g + r;
        const float t = acc[i][w][r] * scale2;
        if (col == pos_col) pos = t;
        if (col < two_N && col != mask_col) {
          if (col < N) {
            const float mn = fmaxf(m0s, t);
            l0 = l0 * exp2f(m0s - mn) + exp2f(t - mn);
            m0s = mn;
          } else {
            const float mn = fmaxf(m1, t);
            l1 = l1 * exp2f(m1 - mn) + exp2f(t - mn);
            m1 = mn;
            if (t > av || (t == av && col < ai)) { av = t; ai = col; }
          }
        }
      }
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
      const float om0 = __shfl_xor(m0s, o, 64), ol0 = __shfl_xor(l0, o, 64);
      const float om1 = __shfl_xor(m1, o, 64), ol1 = __shfl_xor(l1, o, 64);
      const float op = __shfl_xor(pos, o, 64), oav = __shfl_xor(av, o, 64);
      const int oai = __shfl_xor(ai, o, 64);
      ml_merge(m0s, l0, om0, ol0);
      ml_merge(m1, l1, om1, ol1);
      pos = fmaxf(pos, op);
      arg_merge(av, ai, oav, oai);
    }
    if (g == 0 && q < two_n) {
      float* p = part + ((size_t)(2 * blockIdx.x + wm) * rows_pad + q) * kPartStride;
      p[0] = m0s; p[1] = l0; p[2] = m1; p[3] = l1; p[4] = pos; p[5] = av;
      p[6] = __int_as_float(ai); p[7] = 0.f;
    }
  }
}

// Backward, phase 1: S tile recomputed -> ds[q][key] = (softmax - onehot(pos)) * gscale (masked column and padding -> 0) over the
// whole [rows_pad_q, rows_pad_k] grid, and the contrast-entropy partials of tf2/metrics.py:33-35 (a rows, ab block) per split.
template <int W>
__global__ __launch_bounds__(256) void ntxent_wide_ds(const float* __restrict__ zq, const float* __restrict__ zk, int n, int N, int D,
                                                      int rank, float scale2, int vec, const float* __restrict__ row_stats,
                                                      float gscale, float* __restrict__ ds, int ldds, float* __restrict__ epart,
                                                      int rows_pad) {
  __shared__ __attribute__((aligned(16))) float lds[2 * gram_tile::op_floats<32 * W>()];
  constexpr int E = 32 * W;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, fl = lane & 15, wm = wave & 1, wn = wave >> 1;
  const int two_n = 2 * n, two_N = 2 * N;
  const int m0 = blockIdx.x * E, n0 = blockIdx.y * E;
  f32x4 acc[W][W];
  gram_tile::tile<W, false, false>(lds, zk, D, two_N, vec, zq, D, two_n, vec, 0, D, m0, n0, acc);
#pragma unroll
  for (int w = 0; w < W; ++w) {
    const int q = n0 + 16 * W * wn + 16 * w + fl;
    int mask_col, pos_col;
    row_cols(q, n, N, rank, mask_col, pos_col);
    const float lse = q < two_n ? row_stats[2 * q] : 0.f, lse_ab = q < two_n ? row_stats[2 * q + 1] : 0.f;
    float ent = 0.f;
#pragma unroll
    for (int i = 0; i < W; ++i) {
      const int c0 = m0 + 16 * W * wm + 16 * i + 4 * g;
      float d4[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int col = c0 + r;
        const float t = acc[i][w][r] * scale2;
        float d = 0.f;
        if (q < two_n && col < two_N && col != mask_col) {
          d = exp2f(t - lse);
          if (col == pos_col) d -= 1.f;
          if (q < n && col >= N) {
            const float pab = exp2f(t - lse_ab);
            ent -= pab * __logf(pab + 1e-8f);
          }
        }
        d4[r] = d * gscale;
      }
      *(float4*)(ds + (size_t)q * ldds + c0) = make_float4(d4[0], d4[1], d4[2], d4[3]);
    }
    ent += __shfl_xor(ent, 16, 64);
    ent += __shfl_xor(ent, 32, 64);
    if (g == 0 && q < two_n) epart[(size_t)(2 * blockIdx.x + wm) * rows_pad + q] = ent;
  }
}

// C[m][n] = alpha * sum_k A(m, k) B(n, k) for m < M, n < Nc (blockIdx.x = column tile, blockIdx.y = row tile): the two backward
// products and the dense logits_ab.
template <int W, bool A_KR, bool B_KR>
__global__ __launch_bounds__(256) void ntxent_wide_gemm(const float* __restrict__ A, int lda, int avec, const float* __restrict__ B,
                                                        int ldb, int bvec, int M, int Nc, int K, float alpha, float* __restrict__ C,
                                                        int ldc) {
  __shared__ __attribute__((aligned(16))) float lds[2 * gram_tile::op_floats<32 * W>()];
  constexpr int E = 32 * W;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, fl = lane & 15, wm = wave & 1, wn = wave >> 1;
  const int m0 = blockIdx.y * E, n0 = blockIdx.x * E;
  f32x4 acc[W][W];
  gram_tile::tile<W, A_KR, B_KR>(lds, A, lda, M, avec, B, ldb, Nc, bvec, 0, K, m0, n0, acc);
#pragma unroll
  for (int i = 0; i < W; ++i)
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const int c = n0 + 16 * W * wn + 16 * w + fl;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + 16 * W * wm + 16 * i + 4 * g + r;
        if (m < M && c < Nc) C[(size_t)m * ldc + c] = acc[i][w][r] * alpha;
      }
    }
}

// Tile edge of an M x Nc output: 128 where that still gives the chip >= 256 workgroups, else 64.
int wide_edge(int M, int Nc) { return (long long)ceil_div(M, 128) * ceil_div(Nc, 128) >= 256 ? 128 : 64; }
struct WidePlan { int E, rows_pad_q, rows_pad_k, nsplit; };
WidePlan make_wide_plan(int n, int N) {
  WidePlan p;
  p.E = wide_edge(2 * N, 2 * n);
  p.rows_pad_q = ceil_div(2 * n, p.E) * p.E;
  p.rows_pad_k = ceil_div(2 * N, p.E) * p.E;
  p.nsplit = 2 * (p.rows_pad_k / p.E);
  return p;
}
// workspace layout: [forward partials | row terms | entropy partials | dS]
size_t wide_off_rowterm(const WidePlan& p) { return (size_t)p.nsplit * p.rows_pad_q * kPartStride; }
size_t wide_off_ep(const WidePlan& p) { return wide_off_rowterm(p) + (size_t)2 * p.rows_pad_q; }
size_t wide_off_ds(const WidePlan& p) { return wide_off_ep(p) + (size_t)p.nsplit * p.rows_pad_q; }
size_t wide_ws_floats(int n, int N) {
  WidePlan p = make_wide_plan(n, N);
  return wide_off_ds(p) + (size_t)p.rows_pad_q * p.rows_pad_k;
}
// float4 loads allowed: 16-byte aligned base and a row pitch that keeps every row so
int vec_ok(const void* p, int ld) { return ((uintptr_t)p % 16 == 0 && ld % 4 == 0) ? 1 : 0; }

template <bool A_KR, bool B_KR>
void launch_wide_gemm(const float* A, int lda, const float* B, int ldb, int M, int Nc, int K, float alpha, float* C, int ldc,
                      hipStream_t stream) {
  const int E = wide_edge(M, Nc);
  dim3 grid(ceil_div(Nc, E), ceil_div(M, E));
  if (E == 128)
    hipLaunchKernelGGL((ntxent_wide_gemm<4, A_KR, B_KR>), grid, dim3(256), 0, stream, A, lda, vec_ok(A, lda), B, ldb, vec_ok(B, ldb),
                       M, Nc, K, alpha, C, ldc);
  else
    hipLaunchKernelGGL((ntxent_wide_gemm<2, A_KR, B_KR>), grid, dim3(256), 0, stream, A, lda, vec_ok(A, lda), B, ldb, vec_ok(B, ldb),
                       M, Nc, K, alpha, C, ldc);
}

}  // namespace

extern "C" {

size_t simclr_ntxent_workspace_bytes(int n, int N, int D) { return ws_floats(n, N, D) * sizeof(float); }

int simclr_l2norm_fwd(const float* x, float* z, float* inv, int rows, int D, hipStream_t stream) {
  SIMCLR_CHECK_ARG(rows > 0 && D > 0, "l2norm_fwd: bad shape rows=%d D=%d", rows, D);
  hipLaunchKernelGGL(l2norm_fwd_kernel, dim3(ceil_div(rows, 4)), dim3(256), 0, stream, x, z, inv, rows, D);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}
int simclr_l2norm_bwd(const float* z, const float* inv, const float* dz, float* dx, int rows, int D,
                      hipStream_t stream) {
  SIMCLR_CHECK_ARG(rows > 0 && D > 0, "l2norm_bwd: bad shape rows=%d D=%d", rows, D);
  hipLaunchKernelGGL(l2norm_bwd_kernel, dim3(ceil_div(rows, 4)), dim3(256), 0, stream, z, inv, dz, dx, rows, D);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

// Forward: out[0]=loss, out[1]=contrast_acc; row_stats[2n][2] kept for backward.
int simclr_ntxent_fwd(const float* z_local, const float* z_all, int n, int N, int D, int rank,
                      float temperature, float* out, float* row_stats, void* workspace,
                      hipStream_t stream) {
  // D may carry SIMCLR_FMT_TERMS(13) (bits 12..19): the sweeps' fp32 products as three fp16-piece terms -- for l2-NORMALISED rows only
  const int terms = ((D >> 12) & 0xff) - 1;
  D &= 0xfff;
  SIMCLR_CHECK_ARG(terms == -1 || terms == 0 || terms == 13, "ntxent_fwd: matrix arithmetic must be exact (0) or three fp16 terms (13)");
  const bool f16 = terms == 13;
  SIMCLR_CHECK_ARG(n > 0 && N >= n && N % n == 0, "ntxent_fwd: need N = R*n (n=%d N=%d)", n, N);
  SIMCLR_CHECK_ARG(rank >= 0 && rank < N / n, "ntxent_fwd: rank %d out of range", rank);
  SIMCLR_CHECK_ARG(D == 64 || D == 128 || D == 256, "ntxent_fwd: D must be 64/128/256 (got %d)", D);
  SIMCLR_CHECK_ARG(temperature > 0.f, "ntxent_fwd: temperature must be > 0");
  Plan p = make_plan(n, N);
  float* part = (float*)workspace;
  const float scale2 = kLog2e / temperature;
  dim3 grid(p.rows_pad_q / kTile, p.fks);
  const size_t lds = (size_t)kTile * D * sizeof(float);
#define LAUNCH_FWD(DD)                                                                          \
  do {                                                                                          \
    if (f16) hipLaunchKernelGGL((ntxent_fwd_partial<DD, true>), grid, dim3(256), lds, stream, z_local, z_all, n, \
                                N, rank, scale2, p.ftiles_k, part, p.rows_pad_q);               \
    else hipLaunchKernelGGL((ntxent_fwd_partial<DD>), grid, dim3(256), lds, stream, z_local, z_all, n, \
                            N, rank, scale2, p.ftiles_k, part, p.rows_pad_q);                   \
  } while (0)
  if (D == 64) LAUNCH_FWD(64); else if (D == 128) LAUNCH_FWD(128); else LAUNCH_FWD(256);
#undef LAUNCH_FWD
  SIMCLR_CHECK_LAUNCH();
  float* rowterm = part + off_rowterm(p, D);
  hipLaunchKernelGGL(ntxent_finalize_rows, dim3(ceil_div(2 * n, 16)), dim3(256), 0, stream, part, p.fks, p.rows_pad_q,
                     n, N, rank, row_stats, rowterm);
  hipLaunchKernelGGL(ntxent_reduce_out, dim3(1), dim3(256), 0, stream, rowterm, n, out);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

// Backward: dz_local[2n][D] = d loss*grad_scale / d(query-side z_local),
//           dz_all[2N][D]   = d loss*grad_scale / d(key-side z_all) (to be reduce-scattered
//           across replicas: transpose of the concat, tf2/objective.py:114-122).
// Also writes out[2] = contrast entropy (tf2/metrics.py:33-35).
int simclr_ntxent_bwd(const float* z_local, const float* z_all, int n, int N, int D, int rank,
                      float temperature, const float* row_stats, float grad_scale, float* dz_local,
                      float* dz_all, float* out, void* workspace, hipStream_t stream) {
  const int terms = ((D >> 12) & 0xff) - 1;          // see simclr_ntxent_fwd
  D &= 0xfff;
  SIMCLR_CHECK_ARG(terms == -1 || terms == 0 || terms == 13, "ntxent_bwd: matrix arithmetic must be exact (0) or three fp16 terms (13)");
  const bool f16 = terms == 13;
  SIMCLR_CHECK_ARG(n > 0 && N >= n && N % n == 0, "ntxent_bwd: need N = R*n (n=%d N=%d)", n, N);
  SIMCLR_CHECK_ARG(D == 64 || D == 128 || D == 256, "ntxent_bwd: D must be 64/128/256 (got %d)", D);
  Plan p = make_plan(n, N);
  float* part = (float*)workspace;
  float* gq = part + off_gq(p);
  float* gk = part + off_gk(p, D);
  float* ep = part + off_ep(p, D);
  const float scale2 = kLog2e / temperature;
  const size_t lds = (size_t)(kTile * D + 2 * kTile) * sizeof(float);
  dim3 gridq(p.rows_pad_q / kTile, p.ksplit), gridk(p.rows_pad_k / kTile, p.qsplit);
  dim3 gridb(max(gridq.x, gridk.x), max(gridq.y, gridk.y), 2);
#define LAUNCH_BWD(DD)                                                                                       \
  do {                                                                                                       \
    if (f16) hipLaunchKernelGGL((ntxent_bwd_sweeps<DD, true>), gridb, dim3(256), lds, stream, z_local, z_all, n, N, rank, scale2, \
                                row_stats, p.tiles_k, p.tiles_q, gq, p.rows_pad_q, gk, p.rows_pad_k, ep, (int)gridq.x, \
                                (int)gridq.y, (int)gridk.x, (int)gridk.y);                                   \
    else hipLaunchKernelGGL((ntxent_bwd_sweeps<DD>), gridb, dim3(256), lds, stream, z_local, z_all, n, N, rank, scale2, \
                            row_stats, p.tiles_k, p.tiles_q, gq, p.rows_pad_q, gk, p.rows_pad_k, ep, (int)gridq.x, \
                            (int)gridq.y, (int)gridk.x, (int)gridk.y);                                       \
  } while (0)
  if (D == 64) LAUNCH_BWD(64); else if (D == 128) LAUNCH_BWD(128); else LAUNCH_BWD(256);
#undef LAUNCH_BWD
  SIMCLR_CHECK_LAUNCH();
  const float scale = grad_scale / (temperature * (float)n);
  const int blocks_q = ceil_div(2 * n * (D / 4), 256), blocks_k = ceil_div(2 * N * (D / 4), 256);
  hipLaunchKernelGGL(ntxent_combine_all, dim3(blocks_q + blocks_k + 1), dim3(256), 0, stream, gq, p.ksplit, p.rows_pad_q,
                     2 * n, gk, p.qsplit, p.rows_pad_k, 2 * N, D, scale, dz_local, dz_all, ep, n, out, blocks_q, blocks_k);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

// Optional dense logits_ab [n,N] for API parity with objective.py:89 (not on the hot path).
int simclr_ntxent_logits_ab(const float* z_local, const float* z_all, int n, int N, int D,
                            float temperature, float* logits_ab, hipStream_t stream) {
  SIMCLR_CHECK_ARG(n > 0 && N > 0 && D > 0, "ntxent_logits_ab: bad shape");
  hipLaunchKernelGGL(ntxent_logits_ab_kernel, dim3(ceil_div(N, 256), n), dim3(256), 0, stream,
                     z_local, z_all, n, N, D, 1.0f / temperature, logits_ab);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

// ---- wide NT-Xent (any D; tf2/objective.py:53-87): same contracts as simclr_ntxent_fwd / _bwd / _logits_ab above ------------------
size_t simclr_ntxent_wide_workspace_bytes(int n, int N, int D) {
  if (n <= 0 || N < n || D <= 0) return 0;
  return wide_ws_floats(n, N) * sizeof(float);
}

int simclr_ntxent_wide_fwd(const float* z_local, const float* z_all, int n, int N, int D, int terms, int rank, float temperature,
                           float* out, float* row_stats, void* workspace, hipStream_t stream) {
  SIMCLR_CHECK_ARG(terms == 0, "ntxent_wide_fwd: matrix arithmetic must be exact (0) (got %d)", terms);
  SIMCLR_CHECK_ARG(n > 0 && N >= n && N % n == 0, "ntxent_wide_fwd: need N = R*n (n=%d N=%d)", n, N);
  SIMCLR_CHECK_ARG(rank >= 0 && rank < N / n, "ntxent_wide_fwd: rank %d out of range", rank);
  SIMCLR_CHECK_ARG(D > 0, "ntxent_wide_fwd: bad D %d", D);
  SIMCLR_CHECK_ARG(temperature > 0.f, "ntxent_wide_fwd: temperature must be > 0");
  SIMCLR_CHECK_ARG(z_local && z_all && out && row_stats && workspace, "ntxent_wide_fwd: null argument");
  const WidePlan p = make_wide_plan(n, N);
  float* part = (float*)workspace;
  float* rowterm = part + wide_off_rowterm(p);
  const float scale2 = kLog2e / temperature;
  const int vec = vec_ok(z_local, D) & vec_ok(z_all, D);
  dim3 grid(p.rows_pad_k / p.E, p.rows_pad_q / p.E);
  if (p.E == 128)
    hipLaunchKernelGGL(ntxent_wide_fwd_partial<4>, grid, dim3(256), 0, stream, z_local, z_all, n, N, D, rank, scale2, vec, part,
                       p.rows_pad_q);
  else
    hipLaunchKernelGGL(ntxent_wide_fwd_partial<2>, grid, dim3(256), 0, stream, z_local, z_all, n, N, D, rank, scale2, vec, part,
                       p.rows_pad_q);
  SIMCLR_CHECK_LAUNCH();
  hipLaunchKernelGGL(ntxent_finalize_rows, dim3(ceil_div(2 * n, 16)), dim3(256), 0, stream, part, p.nsplit, p.rows_pad_q, n, N, rank,
                     row_stats, rowterm);
  hipLaunchKernelGGL(ntxent_reduce_out, dim3(1), dim3(256), 0, stream, rowterm, n, out);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

int simclr_ntxent_wide_bwd(const float* z_local, const float* z_all, int n, int N, int D, int terms, int rank, float temperature,
                           const float* row_stats, float grad_scale, float* dz_local, float* dz_all, float* out, void* workspace,
                           hipStream_t stream) {
  SIMCLR_CHECK_ARG(terms == 0, "ntxent_wide_bwd: matrix arithmetic must be exact (0) (got %d)", terms);
  SIMCLR_CHECK_ARG(n > 0 && N >= n && N % n == 0, "ntxent_wide_bwd: need N = R*n (n=%d N=%d)", n, N);
  SIMCLR_CHECK_ARG(rank >= 0 && rank < N / n, "ntxent_wide_bwd: rank %d out of range", rank);
  SIMCLR_CHECK_ARG(D > 0, "ntxent_wide_bwd: bad D %d", D);
  SIMCLR_CHECK_ARG(temperature > 0.f, "ntxent_wide_bwd: temperature must be > 0");
  SIMCLR_CHECK_ARG(z_local && z_all && row_stats && dz_local && dz_all && out && workspace, "ntxent_wide_bwd: null argument");
  const WidePlan p = make_wide_plan(n, N);
  float* ep = (float*)workspace + wide_off_ep(p);
  float* ds = (float*)workspace + wide_off_ds(p);
  const float scale2 = kLog2e / temperature;
  const float gscale = grad_scale / (temperature * (float)n);
  const int vec = vec_ok(z_local, D) & vec_ok(z_all, D);
  dim3 grid(p.rows_pad_k / p.E, p.rows_pad_q / p.E);
  if (p.E == 128)
    hipLaunchKernelGGL(ntxent_wide_ds<4>, grid, dim3(256), 0, stream, z_local, z_all, n, N, D, rank, scale2, vec, row_stats, gscale,
                       ds, p.rows_pad_k, ep, p.rows_pad_q);
  else
    hipLaunchKernelGGL(ntxent_wide_ds<2>, grid, dim3(256), 0, stream, z_local, z_all, n, N, D, rank, scale2, vec, row_stats, gscale,
                       ds, p.rows_pad_k, ep, p.rows_pad_q);
  SIMCLR_CHECK_LAUNCH();
  // out[2] = contrast entropy: the entropy tail of ntxent_combine_all (no gradient blocks), fixed split order
  hipLaunchKernelGGL(ntxent_combine_all, dim3(1), dim3(256), 0, stream, (const float*)nullptr, p.nsplit, p.rows_pad_q, 0,
                     (const float*)nullptr, 0, 0, 0, D, 0.f, (float*)nullptr, (float*)nullptr, ep, n, out, 0, 0);
  SIMCLR_CHECK_LAUNCH();
  // dz_local[q][:] = sum_key dS[q][key] z_all[key][:];  dz_all[key][:] = sum_q dS[q][key] z_local[q][:]
  launch_wide_gemm<false, true>(ds, p.rows_pad_k, z_all, D, 2 * n, D, 2 * N, 1.f, dz_local, D, stream);
  SIMCLR_CHECK_LAUNCH();
  launch_wide_gemm<true, true>(ds, p.rows_pad_k, z_local, D, 2 * N, D, 2 * n, 1.f, dz_all, D, stream);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

int simclr_ntxent_wide_logits_ab(const float* z_local, const float* z_all, int n, int N, int D, int terms, float temperature,
                                 float* logits_ab, hipStream_t stream) {
  SIMCLR_CHECK_ARG(terms == 0, "ntxent_wide_logits_ab: matrix arithmetic must be exact (0) (got %d)", terms);
  SIMCLR_CHECK_ARG(n > 0 && N > 0 && D > 0, "ntxent_wide_logits_ab: bad shape");
  SIMCLR_CHECK_ARG(temperature > 0.f, "ntxent_wide_logits_ab: temperature must be > 0");
  SIMCLR_CHECK_ARG(z_local && z_all && logits_ab, "ntxent_wide_logits_ab: null argument");
  // logits_ab[i][j] = <z_local[i], z_all[N + j]> / T
  launch_wide_gemm<false, false>(z_local, D, z_all + (size_t)N * D, D, n, N, D, 1.0f / temperature, logits_ab, N, stream);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
