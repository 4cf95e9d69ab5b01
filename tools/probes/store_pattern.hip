// Store-pattern probe (development aid): how fast does a streaming kernel write / read-modify-write an [M][N] fp32 tensor when a wave
// instruction covers 16 rows x 64 bytes (the MFMA accumulator layout the fp32 epilogues store from: lane (fl, g) = row fl, channels
// 4g..4g+3 of a 16-column fragment) against 1 KB of consecutive bytes?   hipcc --offload-arch=gfx950 -O3 store_pattern.hip -o store_pattern
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
template <int PAT, bool RMW, int N>
__global__ __launch_bounds__(256) void k(float* __restrict__ y, long long M) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, fl = lane & 15;
  constexpr int NI = N / 16 > 4 ? 4 : N / 16;       // fragments per wave row (64 columns); N = 256: the workgroup's N-tile is blockIdx.y
  const long long tiles = (M + 127) / 128;
  const int n0 = blockIdx.y * 64;
  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
    const long long r0 = t * 128 + wave * 32;
    if (PAT == 0) {
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
          float4* p = (float4*)(y + (r0 + mi * 16 + fl) * N + n0 + ni * 16 + g * 4);
          float4 v = make_float4(1.f, 2.f, 3.f, (float)t);
          if (RMW) { float4 o = *p; v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
          *p = v;
        }
    } else {
      // 32 rows x 64 columns of this wave as 8 instructions of 4 full 256-byte row pieces each (lane = 16-byte chunk of a row piece)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float4* p = (float4*)(y + (r0 + j * 4 + g) * N + n0 + fl * 4);
        float4 v = make_float4(1.f, 2.f, 3.f, (float)t);
        if (RMW) { float4 o = *p; v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
        *p = v;
      }
    }
  }
}
template <int PAT, bool RMW, int N> float run(float* y, long long M, int grid) {
  hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
  dim3 gr(grid, N / 64);
  hipLaunchKernelGGL((k<PAT, RMW, N>), gr, dim3(256), 0, 0, y, M);
  hipEventRecord(a);
  for (int i = 0; i < 5; ++i) hipLaunchKernelGGL((k<PAT, RMW, N>), gr, dim3(256), 0, 0, y, M);
  hipEventRecord(b); hipEventSynchronize(b);
  float ms; hipEventElapsedTime(&ms, a, b); return ms / 5;
}
// Strip mode: the access shape of the short-K 1x1 layers with a wide output.  Rows of NS x W floats (W = 64 | 128: 256- | 512-byte
// strips, NS = 2 | 4 strips: 1 ... 2 KB rows).  WHOLE = 0: NS workgroups (blockIdx.y) each write ONE column strip of the same 128-row
// tiles, at whatever times the scheduler gives them (the M-inner walk of conv_igemm_persistent); WHOLE = 1: one workgroup writes the
// NS strips of its rows one after the other (the N-inner walk).  Every wave instruction covers 16 rows x 64 bytes either way (the
// accumulator layout).  READ: a same-shaped operand (residual / BatchNorm input) is read at the same offsets first.
// WHOLE = 2: whole rows with a workgroup-specific first strip (blockIdx.x % NS, wrapping): workgroups that start together do not all
// write the same strip -- the same byte range modulo the row pitch -- at the same time.
template <int W, int NS, int WHOLE, bool READ>
__global__ __launch_bounds__(256) void strip(float* __restrict__ y, const float* __restrict__ r, long long M) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, fl = lane & 15;
  constexpr int N = W * NS, NI = W / 16;
  const long long tiles = M / 128;                   // M is a multiple of 128 (main): no row masks
  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
    const long long r0 = t * 128 + wave * 32;
#pragma unroll 1
    for (int si = WHOLE ? 0 : blockIdx.y; si < (WHOLE ? NS : blockIdx.y + 1); ++si) {
      const int s = WHOLE == 2 ? (si + blockIdx.x) % NS : si;
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        float4 o[NI];
        if (READ) {
#pragma unroll
          for (int ni = 0; ni < NI; ++ni) o[ni] = *(const float4*)(r + (r0 + mi * 16 + fl) * N + s * W + ni * 16 + g * 4);
        }
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
          float4 v = make_float4(1.f, 2.f, 3.f, (float)t);
          if (READ) { v.x += o[ni].x; v.y += o[ni].y; v.z += o[ni].z; v.w += o[ni].w; }
          *(float4*)(y + (r0 + mi * 16 + fl) * N + s * W + ni * 16 + g * 4) = v;
        }
      }
    }
  }
}
template <int W, int NS, int WHOLE, bool READ> float run_strip(float* y, const float* r, long long M, int grid_total) {
  hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
  // the same number of workgroups either way: strips = grid_total / NS M-slots x NS strips, whole rows = grid_total M-slots
  dim3 gr(WHOLE ? grid_total : grid_total / NS, WHOLE ? 1 : NS);
  hipLaunchKernelGGL((strip<W, NS, WHOLE, READ>), gr, dim3(256), 0, 0, y, r, M);
  hipEventRecord(a);
  for (int i = 0; i < 5; ++i) hipLaunchKernelGGL((strip<W, NS, WHOLE, READ>), gr, dim3(256), 0, 0, y, r, M);
  hipEventRecord(b); hipEventSynchronize(b);
  float ms; hipEventElapsedTime(&ms, a, b); return ms / 5;
}
template <int W, int NS> void strip_rows(float* y, const float* r, long long bytes) {
  const long long M = bytes / (W * NS * 4) / 128 * 128;
  const double gb = (double)M * W * NS * 4 / 1e9;
  for (int grid : {512, 768}) {
    const float a = run_strip<W, NS, 0, false>(y, r, M, grid), b = run_strip<W, NS, 1, false>(y, r, M, grid), e = run_strip<W, NS, 2, false>(y, r, M, grid);
    const float c = run_strip<W, NS, 0, true>(y, r, M, grid), d = run_strip<W, NS, 1, true>(y, r, M, grid), f = run_strip<W, NS, 2, true>(y, r, M, grid);
    printf("strip %3d B x %d (row %4d B) grid %4d | store: strips %.3f ms %.0f GB/s, whole rows %.3f ms %.0f GB/s, staggered %.3f ms %.0f GB/s | read+store: "
           "strips %.3f ms %.0f GB/s, whole rows %.3f ms %.0f GB/s, staggered %.3f ms %.0f GB/s (r+w)\n", W * 4, NS, W * NS * 4, grid, a, gb / a * 1e3, b,
           gb / b * 1e3, e, gb / e * 1e3, c, 2 * gb / c * 1e3, d, 2 * gb / d * 1e3, f, 2 * gb / f * 1e3);
  }
}
int strip_main() {
  const long long bytes = 1024ll * 56 * 56 * 256 * 4;   // the 56^2 x 256-channel fp32 activation of 1024 views: 3.29 GB (y and r each)
  float *y, *r;
  if (hipMalloc(&y, bytes) != hipSuccess || hipMalloc(&r, bytes) != hipSuccess) { printf("hipMalloc failed\n"); return 1; }
  hipMemset(y, 0, bytes); hipMemset(r, 0, bytes);
  strip_rows<64, 2>(y, r, bytes);
  strip_rows<64, 4>(y, r, bytes);
  strip_rows<128, 2>(y, r, bytes);
  strip_rows<128, 4>(y, r, bytes);
  return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "strip")) return strip_main();   // store_pattern strip
  const long long M = 1024ll * 112 * 112;           // the stem's output rows; N = 64 -> 3.29 GB
  float* y; hipMalloc(&y, (size_t)M * 256 * 4 / 4); // N = 256 runs use M / 4 rows (56^2): same bytes
  hipMemset(y, 0, (size_t)M * 64 * 4);
  const double gb = (double)M * 64 * 4 / 1e9;
  for (int grid : {512, 768, 2048}) {
    float t;
    t = run<0, false, 64>(y, M, grid);  printf("grid %4d  N=64  store  16 rows x 64 B : %.3f ms  %.0f GB/s\n", grid, t, gb / t * 1e3);
    t = run<1, false, 64>(y, M, grid);  printf("grid %4d  N=64  store  4 rows x 256 B : %.3f ms  %.0f GB/s\n", grid, t, gb / t * 1e3);
    t = run<0, true, 64>(y, M, grid);   printf("grid %4d  N=64  rmw    16 rows x 64 B : %.3f ms  %.0f GB/s (r+w)\n", grid, t, 2 * gb / t * 1e3);
    t = run<1, true, 64>(y, M, grid);   printf("grid %4d  N=64  rmw    4 rows x 256 B : %.3f ms  %.0f GB/s (r+w)\n", grid, t, 2 * gb / t * 1e3);
    t = run<0, false, 256>(y, M / 4, grid / 4);  printf("grid %4d  N=256 store 16 rows x 64 B : %.3f ms  %.0f GB/s\n", grid, t, gb / t * 1e3);
    t = run<1, false, 256>(y, M / 4, grid / 4);  printf("grid %4d  N=256 store 4 rows x 256 B : %.3f ms  %.0f GB/s\n", grid, t, gb / t * 1e3);
    t = run<0, true, 256>(y, M / 4, grid / 4);   printf("grid %4d  N=256 rmw   16 rows x 64 B : %.3f ms  %.0f GB/s (r+w)\n", grid, t, 2 * gb / t * 1e3);
    t = run<1, true, 256>(y, M / 4, grid / 4);   printf("grid %4d  N=256 rmw   4 rows x 256 B : %.3f ms  %.0f GB/s (r+w)\n", grid, t, 2 * gb / t * 1e3);
  }
  return 0;
}
