// Weighted k-NN evaluation of frozen features (Wu et al. 2018) for gfx950: similarity GEMM + streaming top-k, then the class vote.
//
// 1. simclr_knn_topk.  s(i, j) = <q_i, bank_j> on v_mfma_f32_16x16x4_f32 (exact f32), one MFMA chain per pair over d = 0 .. D-1 in a
//    fixed order: the value is a function of the two rows alone, whatever tile, slab or launch the pair falls in (rows past the end of
//    a tile read as zeros and feed only their own outputs).  The [Q, N] matrix is never written:
//      slab kernel   a workgroup (4 waves) owns kQT = 32 queries x one bank slab of kSlab rows.  Per 128-row bank tile it forms the
//                    128 x 32 similarities with the k-loop of the wide NT-Xent kernels (csrc/ntxent.hip: operands staged
//                    global -> registers -> LDS one chunk ahead), packs every (value, index) pair into one 64-bit key whose unsigned
//                    order IS the total order of the result, and appends the keys above the query's running k-th key to the query's
//                    LDS list (an integer LDS counter hands out the slots).  A list that could overflow on the next tile is sorted
//                    by the bitonic network (as simclr_swd_sort_match, csrc/gcl.hip) and cut back to k, which also raises the
//                    running k-th key.  The order in which lanes append is not fixed, the SET a list holds before every sort is, and
//                    the sort is a total order: the output is bitwise repeatable.  No floating-point atomics anywhere.
//      merge kernel  one workgroup per query streams the slabs' k-lists ([Q][slabs][k] keys, the only workspace) through the same
//                    filter / append / sort scheme and writes the first k of the total order.
//    Key: high word = the similarity mapped to an unsigned integer that ascends with the value (-0 counted as +0, NaN -> 0: below
//    every number), low word = ~index, so "larger key" = "similarity descending, bank index ascending".  Key 0 is "no entry".
//
// 2. simclr_knn_vote.  One workgroup per query: w_r = exp((v_r - v_0) / T), class scores in LDS, added by ONE thread in ascending
//    rank order (one defined fp32 result), then five rounds of a (score descending, class ascending) arg-max over all classes.
//
// MFMA mapping as in csrc/ntxent.hip: a = bank-row fragment, b = query fragment, D[bank = (lane >> 4) * 4 + reg][query = lane & 15].
#include "common.h"
#include <math.h>

namespace {

constexpr int kSlab = 4096;      // bank rows per workgroup of the slab kernel (simclr_knn_slab_rows, ops.KNN_SLAB)
constexpr int kBT = 128;         // bank rows per tile
constexpr int kQT = 32;          // queries per workgroup
constexpr int kKc = 32;          // k per LDS stage
constexpr int kPitch = kKc + 4;  // LDS row pitch (4 mod 32 dwords: conflict-free float4 fragment reads)
constexpr int kMaxK = 256;
constexpr int kMergeCap = 1024;  // list length of the merge kernel
constexpr int kMaxClasses = 32768;

typedef unsigned long long u64;

__device__ __forceinline__ u64 make_key(float v, int idx) {
  uint32_t hi;
  if (v != v) hi = 0u;
  else {
    if (v == 0.f) v = 0.f;                      // -0 == +0: only the index separates them
    const uint32_t b = __float_as_uint(v);
    hi = (b >> 31) ? ~b : (b | 0x80000000u);
  }
  return ((u64)hi << 32) | (u64)(~(uint32_t)idx);
}
__device__ __forceinline__ float key_value(u64 key) {
  const uint32_t hi = (uint32_t)(key >> 32);
  if (hi == 0u) return __uint_as_float(0x7fc00000u);
  return __uint_as_float((hi >> 31) ? (hi ^ 0x80000000u) : ~hi);
}
__device__ __forceinline__ int key_index(u64 key) { return (int)(~(uint32_t)key); }

// one compare-exchange stage (k, j) of the descending bitonic network over list[0 .. cap), lanes t = first, first + step, ...
__device__ __forceinline__ void bitonic_stage(u64* list, int cap, int k, int j, int first, int step) {
  for (int t = first; t < (cap >> 1); t += step) {
    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
    const int p = i | j;
    const bool desc = (i & k) == 0;
    const u64 a = list[i], b = list[p];
    if (desc ? (a < b) : (a > b)) { list[i] = b; list[p] = a; }
  }
}

// Sort the lists of the queries with cnt > k (all of them when `all`) and cut them to k.  Wave w owns queries w, w + 4, ...; the
// stage sequence is the same for every thread, so the barriers are uniform.
__device__ __forceinline__ void prune_lists(u64* lists, int* cnt, u64* thr, int cap, int k, bool all, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  for (int q = wave; q < kQT; q += 4) {
    const int c = cnt[q];
    if (all || c > k)
      for (int i = c + lane; i < cap; i += 64) lists[q * cap + i] = 0ull;
  }
  __syncthreads();
  for (int kk = 2; kk <= cap; kk <<= 1)
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int q = wave; q < kQT; q += 4)
        if (all || cnt[q] > k) bitonic_stage(lists + q * cap, cap, kk, j, lane, 64);
      __syncthreads();
    }
  if (tid < kQT) {
    const int c = cnt[tid];
    if (all || c > k) {
      const int cn = min(c, k);
      cnt[tid] = cn;
      thr[tid] = cn == k ? lists[tid * cap + k - 1] : 0ull;
    }
  }
  __syncthreads();
}

// global -> registers: this thread's float4s of the 128 x 32 bank chunk (4) and the 32 x 32 query chunk (1); zeros out of range
__device__ __forceinline__ void knn_fetch(float4* pa, float4& pb, const float* __restrict__ bank, int brow0, int brow_end,
                                          const float* __restrict__ q, int qrow0, int Q, int D, int k0, int tid) {
  const int c = (tid & 7) * 4, r = tid >> 3;
  const bool kin = k0 + c < D;                 // D is a multiple of 16: a float4 is inside or outside as a whole
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = brow0 + r + 32 * j;
    pa[j] = (kin && row < brow_end) ? *(const float4*)(bank + (size_t)row * D + k0 + c) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const int qr = qrow0 + r;
  pb = (kin && qr < Q) ? *(const float4*)(q + (size_t)qr * D + k0 + c) : make_float4(0.f, 0.f, 0.f, 0.f);
}

__global__ __launch_bounds__(256) void knn_slab_kernel(const float* __restrict__ q, const float* __restrict__ bank, int Q, int N, int D,
                                                       int k, int cap, int nslab, u64* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  u64* lists = (u64*)smem;                                    // [kQT][cap]
  u64* thr = lists + (size_t)kQT * cap;                       // [kQT] running k-th key (0: fewer than k entries yet)
  float* sa = (float*)(thr + kQT);                            // [kBT][kPitch]
  float* sb = sa + kBT * kPitch;                              // [kQT][kPitch]
  int* cnt = (int*)(sb + kQT * kPitch);                       // [kQT]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, fl = lane & 15;
  const int slab = blockIdx.x, q0 = blockIdx.y * kQT;
  const int row_begin = slab * kSlab, rows = min(kSlab, N - row_begin);     // tile rows are slab-local: no index passes 2^31
  const float* sbank = bank + (size_t)row_begin * D;
  if (tid < kQT) { cnt[tid] = 0; thr[tid] = 0ull; }
  const int nst = (D + kKc - 1) / kKc;
  for (int t0 = 0; t0 < rows; t0 += kBT) {
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int w = 0; w < 2; ++w) acc[i][w] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float4 pa[4], pb;
    knn_fetch(pa, pb, sbank, t0, rows, q, q0, Q, D, 0, tid);
    for (int st = 0; st < nst; ++st) {
      __syncthreads();
      {
        const int c = (tid & 7) * 4, r = tid >> 3;
#pragma unroll
        for (int j = 0; j < 4; ++j) *(float4*)(sa + (r + 32 * j) * kPitch + c) = pa[j];
        *(float4*)(sb + r * kPitch + c) = pb;
      }
      __syncthreads();
      if (st + 1 < nst) knn_fetch(pa, pb, sbank, t0, rows, q, q0, Q, D, (st + 1) * kKc, tid);
#pragma unroll
      for (int kq = 0; kq < kKc / 16; ++kq) {
        float4 a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) a[i] = *(const float4*)(sa + (32 * wave + 16 * i + fl) * kPitch + 16 * kq + 4 * g);
#pragma unroll
        for (int w = 0; w < 2; ++w) b[w] = *(const float4*)(sb + (16 * w + fl) * kPitch + 16 * kq + 4 * g);
        // per accumulator the chain order is x, y, z, w; the four accumulators interleave
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int w = 0; w < 2; ++w) acc[i][w] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].x, b[w].x, acc[i][w], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int w = 0; w < 2; ++w) acc[i][w] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].y, b[w].y, acc[i][w], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int w = 0; w < 2; ++w) acc[i][w] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].z, b[w].z, acc[i][w], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int w = 0; w < 2; ++w) acc[i][w] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].w, b[w].w, acc[i][w], 0, 0, 0);
      }
    }
    // append: every list has room for the kBT keys a tile can add (cnt <= cap - kBT here: checked after the previous tile, below)
#pragma unroll
    for (int w = 0; w < 2; ++w) {
      const int ql = 16 * w + fl;
      const u64 th = thr[ql];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = t0 + 32 * wave + 16 * i + 4 * g + r;
          if (row < rows) {
            const u64 key = make_key(acc[i][w][r], row_begin + row);
            if (key > th) {
              const int pos = atomicAdd(&cnt[ql], 1);
              if (pos < cap) lists[ql * cap + pos] = key;
            }
          }
        }
    }
    __syncthreads();                             // every wave's appends of this tile are counted before any count is read
    if (__syncthreads_or(tid < kQT && cnt[tid] > cap - kBT)) prune_lists(lists, cnt, thr, cap, k, false, tid);
  }
  prune_lists(lists, cnt, thr, cap, k, true, tid);
  // [Q][nslab][k]: the slab's first min(k, rows) keys in order, the rest "no entry"
  for (int e = tid; e < kQT * k; e += 256) {
    const int ql = e / k, r = e % k;
    if (q0 + ql < Q) ws[((size_t)(q0 + ql) * nslab + slab) * k + r] = r < cnt[ql] ? lists[ql * cap + r] : 0ull;
  }
}

__global__ __launch_bounds__(256) void knn_merge_kernel(const u64* __restrict__ ws, int per_query, int k, float* __restrict__ top_val,
                                                        int* __restrict__ top_idx) {
  __shared__ u64 list[kMergeCap];
  __shared__ int cnt;
  __shared__ u64 thr;
  const int tid = threadIdx.x, qi = blockIdx.x;
  const u64* src = ws + (size_t)qi * per_query;
  if (tid == 0) { cnt = 0; thr = 0ull; }
  __syncthreads();
  for (int base = 0; base < per_query; base += 256) {
    const int e = base + tid;
    if (e < per_query) {
      const u64 key = src[e];
      if (key > thr) {
        const int pos = atomicAdd(&cnt, 1);
        if (pos < kMergeCap) list[pos] = key;
      }
    }
    __syncthreads();
    const int c = cnt;
    __syncthreads();                             // every thread has read cnt before the next appends move it
    if (c > kMergeCap - 256 || base + 256 >= per_query) {
      for (int i = c + tid; i < kMergeCap; i += 256) list[i] = 0ull;
      __syncthreads();
      for (int kk = 2; kk <= kMergeCap; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
          bitonic_stage(list, kMergeCap, kk, j, tid, 256);
          __syncthreads();
        }
      if (tid == 0) {
        const int cn = min(c, k);
        cnt = cn;
        thr = cn == k ? list[k - 1] : 0ull;
      }
      __syncthreads();
    }
  }
  for (int r = tid; r < k; r += 256) {
    const bool have = r < cnt;
    top_val[(size_t)qi * k + r] = have ? key_value(list[r]) : __uint_as_float(0x7fc00000u);
    top_idx[(size_t)qi * k + r] = have ? key_index(list[r]) : -1;
  }
}

__global__ __launch_bounds__(256) void knn_vote_kernel(const float* __restrict__ top_val, const int* __restrict__ top_label, int k,
                                                       int num_classes, float temperature, int* __restrict__ pred, float* __restrict__ score) {
  extern __shared__ __attribute__((aligned(16))) float scores[];   // [num_classes]
  __shared__ float w[kMaxK];
  __shared__ int lab[kMaxK];
  __shared__ float best_s[256];
  __shared__ int best_c[256];
  const int tid = threadIdx.x, qi = blockIdx.x;
  for (int c = tid; c < num_classes; c += 256) scores[c] = 0.f;
  const float v0 = top_val[(size_t)qi * k];
  for (int r = tid; r < k; r += 256) {
    w[r] = expf((top_val[(size_t)qi * k + r] - v0) / temperature);
    lab[r] = top_label[(size_t)qi * k + r];
  }
  __syncthreads();
  if (tid == 0)
    for (int r = 0; r < k; ++r) {
      const int c = lab[r];
      if ((unsigned)c < (unsigned)num_classes) {
        scores[c] += w[r];
      }
    }
  __syncthreads();
  for (int round = 0; round < 5; ++round) {
    float bs = -1.f;
    int bc = 0x7fffffff;
    for (int c = tid; c < num_classes; c += 256) {       // ascending c per thread: a strict > keeps the lowest class id
      const float s = scores[c];
      if (s > bs) { bs = s; bc = c; }
    }
    best_s[tid] = bs; best_c[tid] = bc;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
      if (tid < st) {
        const float os = best_s[tid + st];
        const int oc = best_c[tid + st];
        if (os > best_s[tid] || (os == best_s[tid] && oc < best_c[tid])) { best_s[tid] = os; best_c[tid] = oc; }
      }
      __syncthreads();
    }
    if (tid == 0) {
      const bool have = best_s[0] >= 0.f && best_c[0] < num_classes;
      pred[(size_t)qi * 5 + round] = have ? best_c[0] : -1;
      score[(size_t)qi * 5 + round] = have ? best_s[0] : 0.f;
      if (have) scores[best_c[0]] = -2.f;                // taken
    }
    __syncthreads();
  }
}

int knn_kpad(int k) { int p = 1; while (p < k) p <<= 1; return p; }
int knn_cap(int k) { return max(2 * knn_kpad(k), 2 * kBT); }   // >= k + kBT: a pruned list (<= k) always has room for one more tile
size_t knn_slab_lds(int cap) { return (size_t)kQT * cap * 8 + kQT * 8 + (size_t)(kBT + kQT) * kPitch * 4 + kQT * 4; }
bool knn_args_ok(long long Q, long long N, long long D, long long k) {
  return k >= 1 && k <= kMaxK && N >= k && N < (1LL << 31) && D >= 16 && D % 16 == 0 && Q >= 1 && Q < (1LL << 31);
}

}  // namespace

extern "C" {

int simclr_knn_slab_rows(void) { return kSlab; }

size_t simclr_knn_workspace_bytes(int Q, int N, int D, int k) {
  if (!knn_args_ok(Q, N, D, k)) return 0;
  return (size_t)Q * ceil_div(N, kSlab) * k * sizeof(u64);
}

int simclr_knn_topk(const float* q, const float* bank, int Q, int N, int D, int k, float* top_val, int* top_idx, void* workspace,
                    hipStream_t stream) {
  SIMCLR_CHECK_ARG(k >= 1 && k <= kMaxK, "knn_topk: k must be 1..%d (got %d): a query's candidate list is sorted in LDS", kMaxK, k);
  SIMCLR_CHECK_ARG(N >= k, "knn_topk: the bank has %d rows, fewer than k = %d", N, k);
  SIMCLR_CHECK_ARG(D >= 16 && D % 16 == 0, "knn_topk: D must be a multiple of 16 (got %d)", D);
  SIMCLR_CHECK_ARG(Q >= 1, "knn_topk: bad Q=%d", Q);
  SIMCLR_CHECK_ARG(q && bank && top_val && top_idx && workspace, "knn_topk: null argument");
  const int nslab = ceil_div(N, kSlab), qtiles = ceil_div(Q, kQT);
  SIMCLR_CHECK_ARG(qtiles <= 65535, "knn_topk: at most %d queries per call (got %d)", 65535 * kQT, Q);
  SIMCLR_CHECK_ARG((long long)nslab * k < (1LL << 31), "knn_topk: N too large for k");
  const int cap = knn_cap(k);
  const size_t lds = knn_slab_lds(cap);
  if (!simclr_dry_run()) {
    hipError_t e = hipFuncSetAttribute((const void*)knn_slab_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    SIMCLR_CHECK_ARG(e == hipSuccess, "knn_topk: %d bytes of LDS refused: %s", (int)lds, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(knn_slab_kernel, dim3(nslab, qtiles), dim3(256), lds, stream, q, bank, Q, N, D, k, cap, nslab, (u64*)workspace);
  SIMCLR_CHECK_LAUNCH();
  hipLaunchKernelGGL(knn_merge_kernel, dim3(Q), dim3(256), 0, stream, (const u64*)workspace, nslab * k, k, top_val, top_idx);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

int simclr_knn_vote(const float* top_val, const int* top_label, int Q, int k, int num_classes, float temperature, int* pred, float* score,
                    hipStream_t stream) {
  SIMCLR_CHECK_ARG(k >= 1 && k <= kMaxK, "knn_vote: k must be 1..%d (got %d)", kMaxK, k);
  SIMCLR_CHECK_ARG(num_classes >= 1 && num_classes <= kMaxClasses, "knn_vote: num_classes must be 1..%d (got %d): the class scores live in LDS",
                   kMaxClasses, num_classes);
  SIMCLR_CHECK_ARG(temperature > 0.f, "knn_vote: temperature must be > 0");
  SIMCLR_CHECK_ARG(Q >= 1, "knn_vote: bad Q=%d", Q);
  SIMCLR_CHECK_ARG(top_val && top_label && pred && score, "knn_vote: null argument");
  const size_t lds = (size_t)num_classes * sizeof(float);
  if (!simclr_dry_run()) {
    hipError_t e = hipFuncSetAttribute((const void*)knn_vote_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    SIMCLR_CHECK_ARG(e == hipSuccess, "knn_vote: %d bytes of LDS refused: %s", (int)lds, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(knn_vote_kernel, dim3(Q), dim3(256), lds, stream, top_val, top_label, k, num_classes, temperature, pred, score);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
