// The staged-k exact-f32 Gram tile of the wide NT-Xent (csrc/ntxent.hip), Barlow Twins (csrc/barlow.hip) and VICReg (csrc/vicreg.hip)
// kernels, and the 32-column double-precision reduction the last two share.
//
// Every product is an LDS-tiled GEMM on v_mfma_f32_16x16x4_f32 (exact f32) with a k-loop in stages of kKc.  A workgroup (4 waves,
// 2 x 2) owns an E x E output tile, E = 32 W (W = 2: 64, W = 4: 128); a wave owns W x W 16x16 blocks.  Operands are staged
// global -> registers -> LDS one stage ahead (the loads of stage c+1 run under the MFMAs of stage c), each in its global orientation:
// RK = X[r * ld + k] (row r holds k contiguous), KR = X[k * ld + r].  Loads past the logical extents read zeros, so no extent needs
// padding.  k runs in a fixed order: no atomics, two calls are bitwise equal.
#pragma once
#include "common.h"

namespace gram_tile {

constexpr int kKc = 32;   // k per LDS stage

template <int E> constexpr int op_floats() { return E * (kKc + 4); }   // LDS floats per staged operand (RK pitch kKc+4, KR pitch E+4)

// the float4s of one E x kKc operand chunk this thread moves: RK -> (row r, k..k+3) of X[r * ld + k], KR -> (k, rows r..r+3) of
// X[k * ld + r]; zeros out of range
template <int E, bool KR>
__device__ __forceinline__ void fetch(float4* pf, const float* __restrict__ X, int ld, int rlim, int klim, int r0, int k0, bool vec,
                                      int tid) {
#pragma unroll
  for (int j = 0; j < E * kKc / 1024; ++j) {
    const int idx = tid + j * 256;
    const int r = KR ? (idx % (E / 4)) * 4 : idx / (kKc / 4);
    const int k = KR ? idx / (E / 4) : (idx % (kKc / 4)) * 4;
    const int gr = r0 + r, gk = k0 + k;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (KR) {
      if (gk < klim) {
        const float* p = X + (size_t)gk * ld + gr;
        if (vec && gr + 3 < rlim) v = *(const float4*)p;
        else {
          if (gr < rlim) v.x = p[0];
          if (gr + 1 < rlim) v.y = p[1];
          if (gr + 2 < rlim) v.z = p[2];
          if (gr + 3 < rlim) v.w = p[3];
        }
      }
    } else {
      if (gr < rlim) {
        const float* p = X + (size_t)gr * ld + gk;
        if (vec && gk + 3 < klim) v = *(const float4*)p;
        else {
          if (gk < klim) v.x = p[0];
          if (gk + 1 < klim) v.y = p[1];
          if (gk + 2 < klim) v.z = p[2];
          if (gk + 3 < klim) v.w = p[3];
        }
      }
    }
    pf[j] = v;
  }
}
template <int E, bool KR>
__device__ __forceinline__ void store(float* s, const float4* pf, int tid) {
#pragma unroll
  for (int j = 0; j < E * kKc / 1024; ++j) {
    const int idx = tid + j * 256;
    if (KR) *(float4*)(s + (idx / (E / 4)) * (E + 4) + (idx % (E / 4)) * 4) = pf[j];
    else *(float4*)(s + (idx / (kKc / 4)) * (kKc + 4) + (idx % (kKc / 4)) * 4) = pf[j];
  }
}
// MFMA operand of tile row rr for the 16-k group kq: component j = X(rr, 16 kq + 4 g + j) -- k-slot g of MFMA step j (both operands
// use this k order).  The pitches (kKc+4, E+4 = 4 mod 32 dwords) keep both reads free of bank conflicts.
template <int E, bool KR>
__device__ __forceinline__ float4 frag(const float* s, int rr, int kq, int g) {
  if (KR) {
    const float* p = s + (16 * kq + 4 * g) * (E + 4) + rr;
    return make_float4(p[0], p[E + 4], p[2 * (E + 4)], p[3 * (E + 4)]);
  }
  return *(const float4*)(s + rr * (kKc + 4) + 16 * kq + 4 * g);
}

// acc[i][w][r] = sum_{kbeg <= k < kend} A(m, k) B(c, k) for m = m0 + 16 W wm + 16 i + 4 g + r, c = n0 + 16 W wn + 16 w + fl
// (wm = wave & 1, wn = wave >> 1): rows on the MFMA's A side, columns on the lane.  kbeg is a multiple of the stage; k runs in a
// fixed order.  The first LDS store sits behind a barrier, so the function may be called twice in a row on the same LDS.
template <int W, bool A_KR, bool B_KR>
__device__ __forceinline__ void tile(float* lds, const float* __restrict__ A, int lda, int mlim, bool avec, const float* __restrict__ B,
                                     int ldb, int nlim, bool bvec, int kbeg, int kend, int m0, int n0, f32x4 (&acc)[W][W]) {
  constexpr int E = 32 * W;
  float* sa = lds;
  float* sb = lds + op_floats<E>();
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, fl = lane & 15, wm = wave & 1, wn = wave >> 1;
#pragma unroll
  for (int i = 0; i < W; ++i)
#pragma unroll
    for (int w = 0; w < W; ++w) acc[i][w] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float4 pa[E * kKc / 1024], pb[E * kKc / 1024];
  const int nst = (kend - kbeg + kKc - 1) / kKc;
  if (nst > 0) {
    fetch<E, A_KR>(pa, A, lda, mlim, kend, m0, kbeg, avec, tid);
    fetch<E, B_KR>(pb, B, ldb, nlim, kend, n0, kbeg, bvec, tid);
  }
  for (int st = 0; st < nst; ++st) {
    __syncthreads();
    store<E, A_KR>(sa, pa, tid);
    store<E, B_KR>(sb, pb, tid);
    __syncthreads();
    if (st + 1 < nst) {
      fetch<E, A_KR>(pa, A, lda, mlim, kend, m0, kbeg + (st + 1) * kKc, avec, tid);
      fetch<E, B_KR>(pb, B, ldb, nlim, kend, n0, kbeg + (st + 1) * kKc, bvec, tid);
    }
#pragma unroll
    for (int kq = 0; kq < kKc / 16; ++kq) {
      float4 a[W], b[W];
#pragma unroll
      for (int i = 0; i < W; ++i) a[i] = frag<E, A_KR>(sa, 16 * W * wm + 16 * i + fl, kq, g);
#pragma unroll
      for (int w = 0; w < W; ++w) b[w] = frag<E, B_KR>(sb, 16 * W * wn + 16 * w + fl, kq, g);
#pragma unroll
      for (int i = 0; i < W; ++i)
#pragma unroll
        for (int w = 0; w < W; ++w) {
          acc[i][w] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].x, b[w].x, acc[i][w], 0, 0, 0);
          acc[i][w] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].y, b[w].y, acc[i][w], 0, 0, 0);
          acc[i][w] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].z, b[w].z, acc[i][w], 0, 0, 0);
          acc[i][w] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].w, b[w].w, acc[i][w], 0, 0, 0);
        }
    }
  }
}

// ---- column reductions: a workgroup owns 32 columns; thread (q = tid & 7, rg = tid >> 3) walks rows rg, rg + 32, ... of the column
// quad 4q .. 4q+3 with 16-byte loads and sums in double; the 32 row groups of a column are then added in the order 0 .. 31.
constexpr int kCols = 32;
// v[4] of every thread -> res[32] (column totals); sh holds 32 x 32 doubles.  Ends with a barrier: res is readable by all threads.
__device__ __forceinline__ void col_reduce(const double (&v)[4], double* sh, double* res) {
  const int tid = threadIdx.x, q = tid & 7, rg = tid >> 3;
  __syncthreads();     // sh / res may still be read from an earlier reduction
#pragma unroll
  for (int k = 0; k < 4; ++k) sh[rg * kCols + 4 * q + k] = v[k];
  __syncthreads();
  if (tid < kCols) {
    double s = 0.0;
    for (int r = 0; r < 32; ++r) s += sh[r * kCols + tid];
    res[tid] = s;
  }
  __syncthreads();
}

}  // namespace gram_tile
