// DropBlock (tf2/resnet.py:81-157) for gfx950: the block pattern as a bit tensor, and the streaming passes that apply it.
//
// The reference builds, per site, a float tensor of uniform noise, a float seed pattern, a k x k SAME min-pool of it, a reduce_sum
// and two full-size elementwise passes.  Here:
//   * simclr_dropblock_mask: one workgroup per (image, channel chunk) plane tile.  The seed bits -- (fp32(1 - gamma) + u >= 1) at the
//     valid block centres, 1 elsewhere -- are staged in LDS packed 8 channels per byte; the min over a window of {0, 1} is an AND, taken
//     as a row pass and a column pass on the packed words (8 or 32 channels per op); a popcount gives the number of ones.  The noise
//     never exists in memory: u of an element is a function of a 64-bit key and the element's linear NHWC index (counter-based, no
//     state).  The count is an integer sum (one integer atomic per workgroup): bitwise repeatable in any order.
//   * simclr_dropblock_apply / _tail_fwd / _tail_bwd: 16-byte streaming passes, y = x / p * m with p = float(ones) / float(total) read
//     from device memory (no host synchronisation), arithmetic in fp32, true division as the reference's graph.
#include "common.h"

namespace {

constexpr int kPlaneBytes = 32000;        // one LDS buffer of a plane tile (two are used): H = W <= 178 with 8-channel tiles
constexpr int kMaxHW = 178;

__device__ __forceinline__ uint64_t mix64(uint64_t z) {      // the splitmix64 output function
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// the 64 random bits shared by elements 2 j (low half) and 2 j + 1 (high half)
__device__ __forceinline__ uint64_t pair_bits(uint64_t key, uint64_t j) { return mix64(key + (j + 1) * 0x9E3779B97F4A7C15ull); }
__device__ __forceinline__ float unit_float(uint32_t r) { return (float)(r >> 8) * 5.9604644775390625e-08f; }   // [0, 1), 24 bits

template <bool NT> __device__ __forceinline__ u32x4 ld16(const void* p) {
  return NT ? __builtin_nontemporal_load((const u32x4*)p) : *(const u32x4*)p;
}
template <bool NT> __device__ __forceinline__ void st16(void* p, const u32x4& v) {
  if (NT) __builtin_nontemporal_store(v, (u32x4*)p); else *(u32x4*)p = v;
}

// W: the packed word one thread handles per pixel (uint32_t: 32 channels, uint8_t: 8 channels).  grid = V * (C / (8 sizeof(W))).
template <typename W>
__global__ __launch_bounds__(256) void dropblock_mask(const float* __restrict__ noise, uint64_t key, int HW, int C, int k, float keep_thresh,
                                                      unsigned char* __restrict__ bits, unsigned long long* __restrict__ count,
                                                      unsigned long long total) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int WB = (int)sizeof(W);
  const int P = HW * HW;
  const int plane = (P * WB + 15) & ~15;
  unsigned char* A = smem;
  W* Bw = (W*)(smem + plane);
  uint32_t* red = (uint32_t*)(smem + 2 * plane);        // [0]: AND of the plane (k == W), [1]: ones of this tile
  const int chunks = C / (8 * WB);
  const int v = (int)(blockIdx.x / chunks), cb0 = (int)(blockIdx.x % chunks) * WB;   // cb0: first byte (8 channels) of the tile
  const int lo = k / 2, hi = HW - (k - 1) / 2;          // valid block centres: lo <= i < hi on both axes (resnet.py:118-122)
  if (threadIdx.x == 0) { red[0] = 0xffffffffu; red[1] = 0u; }
  if (blockIdx.x == 0 && threadIdx.x == 0) count[1] = total;

  // 1. seed pattern (resnet.py:128-132), one byte = 8 channels per item
  for (int it = threadIdx.x; it < P * WB; it += 256) {
    const int p = it / WB, b = it - p * WB;
    const int h = p / HW, w = p - h * HW;
    unsigned byte = 0xffu;
    if (h >= lo && h < hi && w >= lo && w < hi) {
      const long long e0 = ((long long)v * P + p) * C + (long long)(cb0 + b) * 8;    // linear NHWC index, a multiple of 8
      float u[8];
      if (noise) {
        const f32x4 n0 = *(const f32x4*)(noise + e0), n1 = *(const f32x4*)(noise + e0 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { u[e] = n0[e]; u[4 + e] = n1[e]; }
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const uint64_t r = pair_bits(key, (uint64_t)(e0 >> 1) + q);
          u[2 * q] = unit_float((uint32_t)r);
          u[2 * q + 1] = unit_float((uint32_t)(r >> 32));
        }
      }
      byte = 0u;
#pragma unroll
      for (int e = 0; e < 8; ++e) byte |= ((keep_thresh + u[e]) >= 1.0f ? 1u : 0u) << e;      // one fp32 add, then the compare
    }
    A[it] = (unsigned char)byte;
  }
  __syncthreads();

  const W* Aw = (const W*)A;
  W* out = (W*)(bits + (long long)v * P * (C / 8) + cb0);
  const int pitch = C / (8 * WB);                       // words per pixel of the bit tensor
  int ones = 0;
  if (k == HW) {
    // reduce_min over the plane, broadcast (resnet.py:134-138); counted once per (image, channel)
    W acc = (W)~(W)0;
    for (int p = threadIdx.x; p < P; p += 256) acc &= Aw[p];
    if ((W)~acc) atomicAnd(&red[0], (uint32_t)acc | (WB == 4 ? 0u : 0xffffff00u));
    __syncthreads();
    const W r = (W)red[0];
    for (int p = threadIdx.x; p < P; p += 256) out[(long long)p * pitch] = r;
    if (threadIdx.x == 0) ones = __popc((unsigned)r);
  } else {
    // k x k stride-1 SAME min-pool (resnet.py:144-149): output i covers inputs i - (k-1)/2 .. i + k/2, clipped to the map
    const int back = (k - 1) / 2, fwd = k / 2;
    for (int p = threadIdx.x; p < P; p += 256) {
      const int h = p / HW, w = p - h * HW;
      const int w0 = max(w - back, 0), w1 = min(w + fwd, HW - 1);
      W acc = (W)~(W)0;
      for (int j = w0; j <= w1; ++j) acc &= Aw[h * HW + j];
      Bw[p] = acc;
    }
    __syncthreads();
    for (int p = threadIdx.x; p < P; p += 256) {
      const int h = p / HW, w = p - h * HW;
      const int h0 = max(h - back, 0), h1 = min(h + fwd, HW - 1);
      W acc = (W)~(W)0;
      for (int j = h0; j <= h1; ++j) acc &= Bw[j * HW + w];
      out[(long long)p * pitch] = acc;
      ones += __popc((unsigned)acc);
    }
  }
  // 2. the count: wave sum, one LDS add per wave, one integer atomic per workgroup
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ones += __shfl_xor(ones, o, 64);
  if ((threadIdx.x & 63) == 0 && ones) atomicAdd(&red[1], (uint32_t)ones);
  __syncthreads();
  if (threadIdx.x == 0 && red[1]) atomicAdd(count, (unsigned long long)red[1]);
}

// bit e of chunk i (EPC elements from linear element i * EPC): C % 8 == 0, so the packed tensor is the linear bit string of the elements
template <int EPC> __device__ __forceinline__ unsigned chunk_bits(const unsigned char* __restrict__ m, long long i) {
  return EPC == 8 ? (unsigned)m[i] : ((unsigned)m[i >> 1] >> ((int)(i & 1) * 4)) & 0xfu;
}
__device__ __forceinline__ float percent_ones(const unsigned long long* __restrict__ count) {
  return (float)count[0] / (float)count[1];             // resnet.py:151-153: both casts to fp32, then the division
}

// y = x / p * m (resnet.py:155-156); two 16-byte chunks per thread
template <typename T, bool NT>
__global__ __launch_bounds__(256) void dropblock_apply(const T* __restrict__ x, const unsigned char* __restrict__ m,
                                                       const unsigned long long* __restrict__ count, T* __restrict__ y, long long nchunks) {
  constexpr int EPC = Elem<T>::EPC;
  const float p = percent_ones(count);
  const long long base = (long long)blockIdx.x * 512 + threadIdx.x;
  u32x4 xv[2];
  unsigned mb[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const long long i = base + u * 256;
    if (i < nchunks) { xv[u] = ld16<NT>(x + i * EPC); mb[u] = chunk_bits<EPC>(m, i); }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const long long i = base + u * 256;
    if (i < nchunks) {
      float v[EPC];
      chunk_to_f32<T>(xv[u], v);
#pragma unroll
      for (int e = 0; e < EPC; ++e) v[e] = (v[e] / p) * (float)((mb[u] >> e) & 1u);
      st16<NT>(y + i * EPC, f32_to_chunk<T>(v));
    }
  }
}

// out = relu(a / pa * ma + b / pb * mb) (resnet.py:482-487 with the two DropBlock sites in front of the add); relu(o) = o < 0 ? 0 : o
template <typename T, bool NT>
__global__ __launch_bounds__(256) void dropblock_tail_fwd(const T* __restrict__ a, const unsigned char* __restrict__ ma,
                                                          const unsigned long long* __restrict__ ca, const T* __restrict__ b,
                                                          const unsigned char* __restrict__ mb, const unsigned long long* __restrict__ cb,
                                                          T* __restrict__ out, unsigned char* __restrict__ relu_bits, long long nchunks) {
  constexpr int EPC = Elem<T>::EPC;
  const float pa = percent_ones(ca), pb = percent_ones(cb);
  const long long base = (long long)blockIdx.x * 512 + threadIdx.x;
  u32x4 av[2], bv[2];
  unsigned am[2], bm[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const long long i = base + u * 256;
    if (i < nchunks) {
      av[u] = ld16<NT>(a + i * EPC); bv[u] = ld16<NT>(b + i * EPC);
      am[u] = chunk_bits<EPC>(ma, i); bm[u] = chunk_bits<EPC>(mb, i);
    }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const long long i = base + u * 256;
    if (i < nchunks) {
      float va[EPC], vb[EPC];
      chunk_to_f32<T>(av[u], va);
      chunk_to_f32<T>(bv[u], vb);
#pragma unroll
      for (int e = 0; e < EPC; ++e) {
        const float ta = (va[e] / pa) * (float)((am[u] >> e) & 1u);
        const float tb = (vb[e] / pb) * (float)((bm[u] >> e) & 1u);
        const float o = ta + tb;
        va[e] = o < 0.f ? 0.f : o;
      }
      const u32x4 packed = f32_to_chunk<T>(va);
      st16<NT>(out + i * EPC, packed);
      if (relu_bits) {                                   // the format simclr_bn_apply(relu_bits) writes: bit e = (stored out[e] > 0)
        float w[EPC];
        chunk_to_f32<T>(packed, w);
        unsigned r = 0;
#pragma unroll
        for (int e = 0; e < EPC; ++e) r |= (w[e] > 0.f ? 1u : 0u) << e;
        relu_bits[i] = (unsigned char)r;
      }
    }
  }
}

// g = relu bit ? dout : 0;  da = g / pa * ma;  db = g / pb * mb
template <typename T, bool NT>
__global__ __launch_bounds__(256) void dropblock_tail_bwd(const T* __restrict__ dout, const unsigned char* __restrict__ relu_bits,
                                                          const unsigned char* __restrict__ ma, const unsigned long long* __restrict__ ca,
                                                          const unsigned char* __restrict__ mb, const unsigned long long* __restrict__ cb,
                                                          T* __restrict__ da, T* __restrict__ db, long long nchunks) {
  constexpr int EPC = Elem<T>::EPC;
  const float pa = percent_ones(ca), pb = percent_ones(cb);
  const long long base = (long long)blockIdx.x * 512 + threadIdx.x;
  u32x4 dv[2];
  unsigned rm[2], am[2], bm[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const long long i = base + u * 256;
    if (i < nchunks) {
      dv[u] = ld16<NT>(dout + i * EPC);
      rm[u] = relu_bits[i]; am[u] = chunk_bits<EPC>(ma, i); bm[u] = chunk_bits<EPC>(mb, i);
    }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const long long i = base + u * 256;
    if (i < nchunks) {
      float g[EPC], va[EPC], vb[EPC];
      chunk_to_f32<T>(dv[u], g);
#pragma unroll
      for (int e = 0; e < EPC; ++e) {
        const float ge = ((rm[u] >> e) & 1u) ? g[e] : 0.f;
        va[e] = (ge / pa) * (float)((am[u] >> e) & 1u);
        vb[e] = (ge / pb) * (float)((bm[u] >> e) & 1u);
      }
      st16<NT>(da + i * EPC, f32_to_chunk<T>(va));
      st16<NT>(db + i * EPC, f32_to_chunk<T>(vb));
    }
  }
}

// shared argument checks of the three streaming passes; returns the grid (0: nothing to do) or -1 after setting the error
int stream_grid(const char* who, long long rows, int C, int dtype, long long* nchunks) {
  if (dtype != SIMCLR_DT_F32 && dtype != SIMCLR_DT_BF16) { simclr_set_error("%s: dtype must be fp32 or bf16 storage", who); return -1; }
  if (rows < 0 || C <= 0 || C % 8 != 0) { simclr_set_error("%s: C=%d must be a positive multiple of 8 (the masks pack 8 channels per byte)", who, C); return -1; }
  const int epc = dtype == SIMCLR_DT_BF16 ? 8 : 4;
  *nchunks = rows * (C / epc);
  const long long blocks = (*nchunks + 511) / 512;
  if (blocks >= (1ll << 31)) { simclr_set_error("%s: tensor too large for one launch", who); return -1; }
  return (int)blocks;
}

}  // namespace

extern "C" {

// tf2/resnet.py:111-153
int simclr_dropblock_mask(const float* noise, long long key, int V, int H, int W, int C, int dropblock_size, float keep_thresh,
                          unsigned char* bits, void* count, hipStream_t stream) {
  SIMCLR_CHECK_ARG(bits && count, "dropblock_mask: null argument (bits, count)");
  SIMCLR_CHECK_ARG(V > 0 && H > 0 && C > 0 && dropblock_size > 0, "dropblock_mask: bad shape");
  SIMCLR_CHECK_ARG(H == W, "dropblock_mask: Input tensor with width!=height is not supported (H=%d, W=%d)", H, W);
  SIMCLR_CHECK_ARG(C % 8 == 0, "dropblock_mask: C=%d must be a multiple of 8 (the pattern packs 8 channels per byte)", C);
  SIMCLR_CHECK_ARG(W <= kMaxHW, "dropblock_mask: a %dx%d plane does not fit the LDS tile (H = W <= %d)", H, W, kMaxHW);
  const int k = dropblock_size < W ? dropblock_size : W;                     // resnet.py:111
  const bool wide = C % 32 == 0 && W * W * 4 <= kPlaneBytes;                 // 32 channels per word where the plane fits
  const int wb = wide ? 4 : 1;
  const long long grid = (long long)V * (C / (8 * wb));
  SIMCLR_CHECK_ARG(grid < (1ll << 31), "dropblock_mask: tensor too large for one launch");
  const unsigned long long total = k == W ? (unsigned long long)V * C : (unsigned long long)V * H * W * C;   // size(block_pattern)
  const size_t lds = 2 * (size_t)((W * W * wb + 15) & ~15) + 16;
  if (simclr_dry_run()) return 0;
  if (hipMemsetAsync(count, 0, 16, stream) != hipSuccess) {
    simclr_set_error("dropblock_mask: clearing the count failed");
    return 2;
  }
  if (wide)
    hipLaunchKernelGGL((dropblock_mask<uint32_t>), dim3((unsigned)grid), dim3(256), lds, stream, noise, (uint64_t)key, W, C, k, keep_thresh,
                       bits, (unsigned long long*)count, total);
  else
    hipLaunchKernelGGL((dropblock_mask<uint8_t>), dim3((unsigned)grid), dim3(256), lds, stream, noise, (uint64_t)key, W, C, k, keep_thresh,
                       bits, (unsigned long long*)count, total);
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

// tf2/resnet.py:155-156 (and, applied to dy, its gradient)
int simclr_dropblock_apply(const void* x, const unsigned char* bits, const void* count, void* y, long long rows, int C, int dtype,
                           hipStream_t stream) {
  SIMCLR_CHECK_ARG(x && bits && count && y, "dropblock_apply: null argument");
  long long nchunks;
  const int grid = stream_grid("dropblock_apply", rows, C, dtype, &nchunks);
  if (grid < 0) return 1;
  if (grid > 0) {
    if (dtype == SIMCLR_DT_BF16)
      hipLaunchKernelGGL((dropblock_apply<uint16_t, true>), dim3(grid), dim3(256), 0, stream, (const uint16_t*)x, bits,
                         (const unsigned long long*)count, (uint16_t*)y, nchunks);
    else
      hipLaunchKernelGGL((dropblock_apply<float, true>), dim3(grid), dim3(256), 0, stream, (const float*)x, bits,
                         (const unsigned long long*)count, (float*)y, nchunks);
  }
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

// tf2/resnet.py:482-487: the shortcut's and the residual branch's DropBlock, the add and the ReLU in one pass
int simclr_dropblock_tail_fwd(const void* a, const unsigned char* bits_a, const void* count_a, const void* b, const unsigned char* bits_b,
                              const void* count_b, void* out, unsigned char* relu_bits, long long rows, int C, int dtype,
                              hipStream_t stream) {
  SIMCLR_CHECK_ARG(a && bits_a && count_a && b && bits_b && count_b && out, "dropblock_tail_fwd: null argument");
  long long nchunks;
  const int grid = stream_grid("dropblock_tail_fwd", rows, C, dtype, &nchunks);
  if (grid < 0) return 1;
  if (grid > 0) {
    if (dtype == SIMCLR_DT_BF16)
      hipLaunchKernelGGL((dropblock_tail_fwd<uint16_t, true>), dim3(grid), dim3(256), 0, stream, (const uint16_t*)a, bits_a,
                         (const unsigned long long*)count_a, (const uint16_t*)b, bits_b, (const unsigned long long*)count_b,
                         (uint16_t*)out, relu_bits, nchunks);
    else
      hipLaunchKernelGGL((dropblock_tail_fwd<float, true>), dim3(grid), dim3(256), 0, stream, (const float*)a, bits_a,
                         (const unsigned long long*)count_a, (const float*)b, bits_b, (const unsigned long long*)count_b,
                         (float*)out, relu_bits, nchunks);
  }
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

// the gradient of the above wrt a and b (pattern and percent_ones are constants, as tape.gradient sees them)
int simclr_dropblock_tail_bwd(const void* dout, const unsigned char* relu_bits, const unsigned char* bits_a, const void* count_a,
                              const unsigned char* bits_b, const void* count_b, void* da, void* db, long long rows, int C, int dtype,
                              hipStream_t stream) {
  SIMCLR_CHECK_ARG(dout && relu_bits && bits_a && count_a && bits_b && count_b && da && db, "dropblock_tail_bwd: null argument");
  long long nchunks;
  const int grid = stream_grid("dropblock_tail_bwd", rows, C, dtype, &nchunks);
  if (grid < 0) return 1;
  if (grid > 0) {
    if (dtype == SIMCLR_DT_BF16)
      hipLaunchKernelGGL((dropblock_tail_bwd<uint16_t, true>), dim3(grid), dim3(256), 0, stream, (const uint16_t*)dout, relu_bits, bits_a,
                         (const unsigned long long*)count_a, bits_b, (const unsigned long long*)count_b, (uint16_t*)da, (uint16_t*)db,
                         nchunks);
    else
      hipLaunchKernelGGL((dropblock_tail_bwd<float, true>), dim3(grid), dim3(256), 0, stream, (const float*)dout, relu_bits, bits_a,
                         (const unsigned long long*)count_a, bits_b, (const unsigned long long*)count_b, (float*)da, (float*)db, nchunks);
  }
  SIMCLR_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
