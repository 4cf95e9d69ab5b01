// The 64-row sweep family of the loss kernels (csrc/ntxent.hip, gcl.hip, supcon.hip, moco.hip, dino.hip, swav.hip, swav_multicrop.hip,
// dino_multicrop.hip): S = X W^T tile by tile on v_mfma_f32_16x16x4_f32 (exact f32), 64 fixed rows per workgroup held as MFMA
// fragments, 64-row XOR-swizzled LDS tiles of the streamed side, online row statistics in the base-2 domain on the ROUNDED logit,
// splits merged in a fixed order, no atomics.
//
// MFMA mapping: a = streamed-row fragment, b = fixed-row fragment, D[streamed = (lane >> 4) * 4 + reg][fixed = lane & 15]: every lane
// owns ONE fixed row (fl = lane & 15) and 4 streamed rows per 16x16 block (g = lane >> 4), so the online statistics are lane-local and
// only the merge over the 4 lane groups needs shuffles (xor 16, 32).
#pragma once
#include "common.h"
#include <math.h>

namespace sweep {

constexpr float kLog2e = 1.4426950408889634f;
constexpr double kLog2ed = 1.4426950408889634;
constexpr double kLn2d = 0.6931471805599453;
constexpr int kTile = 64;      // rows per LDS tile / fixed rows per workgroup

// which source row tile row i (global row `row` = row0 + i of nrows_total) holds, n = nrows_total / 2:
//   kPlain    row itself;
//   kPaired   p(row) = (row + n) mod 2n, the other view's row (BYOL's pairing);
//   kWrapped  row mod n: src has n rows only (the per-image multiplier of a global row)
enum class RowMap { kPlain, kPaired, kWrapped };

// 64 x D tile, global -> LDS, 16-byte slots XOR-swizzled by the row; rows past the end read as zeros
template <int D, RowMap MAP = RowMap::kPlain>
__device__ __forceinline__ void load_tile(float* lds, const float* __restrict__ src, int row0, int nrows_total, int tid) {
  constexpr int C = D / 4;
  const int n = nrows_total >> 1;
  for (int idx = tid; idx < kTile * C; idx += 256) {
    const int r = idx / C, c = idx % C;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    const int row = row0 + r;
    if (row < nrows_total) {
      const int srow = MAP == RowMap::kPaired ? (row < n ? row + n : row - n) : MAP == RowMap::kWrapped ? (row < n ? row : row - n) : row;
      v = *(const float4*)(src + (size_t)srow * D + c * 4);
    }
    *(float4*)(lds + r * D + ((c ^ (r & 15)) * 4)) = v;
  }
}

// S fragment: acc[r] = <tile row sub * 16 + 4 g + r, this lane's fixed row>
template <int D>
__device__ __forceinline__ f32x4 s_frag(const float* lds, int sub, int fl, int g, const float4* ff) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const int trow = sub * 16 + fl;
#pragma unroll
  for (int s = 0; s < D / 16; ++s) {
    const float4 tf = *(const float4*)(lds + trow * D + (((4 * s + g) ^ (trow & 15)) * 4));
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(tf.x, ff[s].x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(tf.y, ff[s].y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(tf.z, ff[s].z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(tf.w, ff[s].w, acc, 0, 0, 0);
  }
  return acc;
}

// this lane's fragments of fixed row `row` (zeros past the end)
template <int D>
__device__ __forceinline__ void load_frag(float4* ff, const float* __restrict__ x, int row, bool valid, int g) {
#pragma unroll
  for (int s = 0; s < D / 16; ++s)
    ff[s] = valid ? *(const float4*)(x + (size_t)row * D + 16 * s + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// The rounded base-2 logit with its offset: two separate roundings, the same two in every sweep that recomputes it.  The pins keep
// the compiler from fusing the product into the add (or into a later t - m): the fused form keeps the product's low bits, so a sweep
// that recomputes the logit would not reproduce the number the saved log-sum-exp was formed from, and exp2(t - t) != 1.
__device__ __forceinline__ float logit2(float dot, float scale2, float off2) {
  float t = dot * scale2;
  asm volatile("" : "+v"(t));
  t += off2;
  asm volatile("" : "+v"(t));
  return t;
}

// ---- online row statistics in the base-2 domain ------------------------------------------------------------------------------------
// (m, l): m = the running maximum, l = sum of exp2(x - m) over all elements.  The empty state is (-inf, 0); the merge takes either
// side empty (exp2f(-inf - -inf) is never formed).
__device__ __forceinline__ void ml_push(float& m, float& l, float x) {
  const float mn = fmaxf(m, x);
  l = l * exp2f(m - mn) + exp2f(x - mn);
  m = mn;
}
__device__ __forceinline__ void ml_merge(float& m, float& l, float m2, float l2) {
  const float mn = fmaxf(m, m2);
  const float a = (m == -INFINITY) ? 0.f : l * exp2f(m - mn);
  const float b = (m2 == -INFINITY) ? 0.f : l2 * exp2f(m2 - mn);
  m = mn; l = a + b;
}

// (m, r, a): m = the maximum, r = sum over every element BUT one instance of the maximum of exp2(t - m), a = sum over all of
// exp2(t - m) (t - m) (every term <= 0).  The softmax sum is 1 + r: a near-one-hot row keeps its non-maximum mass apart from the
// maximum's own 1.  The empty state is (-inf, 0, 0).
__device__ __forceinline__ void mra_push(float& m, float& r, float& a, float t) {
  if (m == -INFINITY) { m = t; return; }     // r = a = 0 already
  if (t > m) {
    const float dm = m - t, e = exp2f(dm), l = r + 1.f;
    a = e * (a + l * dm);
    r = l * e;
    m = t;
  } else {
    const float x = t - m, p = exp2f(x);
    a += p * x;
    r += p;
  }
}
__device__ __forceinline__ void mra_merge(float& m, float& r, float& a, float m2, float r2, float a2) {
  if (m2 == -INFINITY) return;
  if (m == -INFINITY) { m = m2; r = r2; a = a2; return; }
  if (m2 > m) {
    const float tm = m, tr = r, ta = a;
    m = m2; r = r2; a = a2; m2 = tm; r2 = tr; a2 = ta;
  }
  const float dm = m2 - m, e = exp2f(dm), l2 = r2 + 1.f;   // the other side's maximum is one more non-maximum element here
  r += l2 * e;
  a += e * (a2 + l2 * dm);
}

// (m, r): the same without a (a side that needs its log-sum-exp only)
__device__ __forceinline__ void mr_push(float& m, float& r, float t) {
  if (m == -INFINITY) { m = t; return; }
  if (t > m) {
    r = (r + 1.f) * exp2f(m - t);
    m = t;
  } else {
    r += exp2f(t - m);
  }
}
__device__ __forceinline__ void mr_merge(float& m, float& r, float m2, float r2) {
  if (m2 == -INFINITY) return;
  if (m == -INFINITY) { m = m2; r = r2; return; }
  if (m2 > m) {
    const float tm = m, tr = r;
    m = m2; r = r2; m2 = tm; r2 = tr;
  }
  r += (r2 + 1.f) * exp2f(m2 - m);
}

// ---- host-side argument checks -------------------------------------------------------------------------------------------------------
static inline bool dim_ok(int D) { return D == 64 || D == 128 || D == 256; }
static inline bool pos_finite(float x) { return x > 0.f && x <= 3.0e38f; }          // (NaN fails the comparison)
static inline bool al16(const void* a) { return a && ((uintptr_t)a & 15) == 0; }
static inline bool al8(const void* a) { return a && ((uintptr_t)a & 7) == 0; }
static inline bool al4(const void* a) { return a && ((uintptr_t)a & 3) == 0; }

// more than 64 KB of dynamic LDS has to be asked for (csrc/knn.hip)
template <typename F>
bool raise_lds(F kernel, size_t lds) {
  if (lds <= 65536 || simclr_dry_run()) return true;
  return hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess;
}

}  // namespace sweep
