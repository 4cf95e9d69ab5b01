// N-inner walk of the persistent implicit GEMM for the short-K 1x1 layers (included by conv.hip after conv_igemm_persistent).
//
// conv_igemm_persistent gives a workgroup ONE N-tile and lets it walk M-tiles: a layer with Cout / BN = 2 ... 4 N-tiles gathers every
// activation tile that many times (relying on sibling workgroups staying in lockstep on one XCD for L2 hits), splits it into fp16
// pieces in registers that many times, and writes every output row as that many strips from different workgroups at different times.
// Here a workgroup owns an M-tile and a contiguous GROUP of its N-tiles (ConvP::nw_gw columns; all of them when there are enough
// M-tiles to fill the grid, plan_nwalk):
//   - the [BM x IC] activation panel is loaded into LDS ONCE per M-tile by LDS-DMA and rewritten in place into (hi, lo) fp16 pieces
//     once, as the WPS window path of conv_igemm_persistent does (same split function on the same pairs: identical pieces);
//   - the weight tiles of the group stream through a two-stage ring, N-tile after N-tile, one 128-byte k-block per step -- the k-step
//     order and the MFMA order per output element (lo*hi, hi*lo, hi*hi per k-block) are those of conv_igemm_persistent, so every
//     output element keeps its bits;
//   - the next M-tile's panel is requested as soon as the last MFMA of this one has read the panel, i.e. together with the residual
//     loads of the last N-tile's epilogue: one memory round trip covers both.
// No flags, spins or any other traffic between workgroups.
//
// Instantiated for the class that measured faster than the M-inner walk (profiles/nwalk_microbench.json): the fp32-storage forward
// with three fp16-piece terms and the fused BatchNorm-apply epilogue of a bottleneck tail (FAS = 1: residual + ReLU + ReLU bit mask,
// 2: the same with the residual's own BatchNorm), flat 1x1 stride 1, IC = 64 | 128 (KPT = IC / 32 k-blocks), Cout a multiple of 64.
//
// Tile: BM = 64 rows x BN = 64 columns per step, 4 waves stacked along M (wave w owns rows 16 w ... 16 w + 15 of the M-tile and all 64
// columns of the N-tile: NI = 4 accumulator fragments, so a wave stores 256 consecutive bytes of each of its rows per N-tile and the
// N-tiles of a group complete the row), so the panel is 16 | 32 KB, the ring 16 KB and the BatchNorm constants 2 | 4 floats per column
// of the group: three workgroups per CU at IC = 64, two or three at IC = 128.
template <int KPT, int FAS>
__global__ __launch_bounds__(256, 3) void conv_igemm_nwalk(const ConvP p) {
  static_assert((KPT == 2 || KPT == 4) && (FAS == 1 || FAS == 2), "IC = 64 | 128; fused-tail option sets 1 | 2");
  constexpr int BM = 64, BN = 64, NI = BN / 16;
  constexpr int PJ = KPT * BM / 32;                    // LDS-DMA wave-instructions (8 rows x 128 bytes each) per wave and panel
  constexpr int NBP = FAS == 2 ? 4 : 2;                // per-column constants: scale, shift (+ the residual's scale, shift)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  u32x4* Pn = (u32x4*)smem;                            // panel: [KPT][BM] rows of 128 bytes, chunk ^= row & 7
  u32x4* Rg = Pn + KPT * BM * 8;                       // weight ring: [2][BN] rows of 128 bytes, same swizzle
  float* bnp = (float*)(Rg + 2 * BN * 8);              // [NBP][nw_gw]
  typedef __attribute__((address_space(1))) const void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, fl = lane & 15;
  const float* __restrict__ X = (const float*)p.x;
  const float* __restrict__ Wt = (const float*)p.w;
  float* __restrict__ Y = (float*)p.y;
  const int G = p.nw_gw, ngt = G / BN;
  // workgroup -> (N-group, first M-tile, M-tile stride); gridDim.x is a multiple of 8 * nw_groups, the workgroups of one M-slot
  // (different N-groups) sit on one XCD
  const int xcd = blockIdx.x & 7, l = blockIdx.x >> 3;
  const int grp = l % p.nw_groups;
  const int mslots = gridDim.x / p.nw_groups;
  const int mslot = (l / p.nw_groups) * 8 + xcd;
  const int ng0 = grp * G;
  const int count = (mslot < p.m_tiles) ? (p.m_tiles - mslot + mslots - 1) / mslots : 0;
  const int kc = (lane & 7) ^ (lane >> 3);

  for (int i = tid; i < G; i += 256) {                 // N is a multiple of nw_gw: every column of the group exists
    const int n = ng0 + i;
    bnp[i] = p.bn_scale[n];
    bnp[G + i] = p.bn_shift[n];
    if (FAS == 2) { bnp[2 * G + i] = p.bn_mean[n]; bnp[3 * G + i] = p.bn_rstd[n]; }   // the residual's scale / shift travel here
  }
  // (visibility: the first barrier of the k-loop)

  auto issue_panel = [&](int mt) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < PJ; ++j) {
      const int q = wave * PJ + j;                     // wave-uniform: k-block q / (BM / 8), 8-row group q % (BM / 8)
      const int kt = q / (BM / 8), rg = q % (BM / 8);
      const int m = mt * BM + 8 * rg + (lane >> 3);
      const void* src = m < p.M ? (const void*)(X + (long long)m * p.pixpitch + kt * 32 + kc * 4) : p.zero;
      __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(smem + q * 1024), 16, 0, 0);
    }
  };
  auto issue_w = [&](int nt, int kt, int b) __attribute__((always_inline)) {
    unsigned char* dst = (unsigned char*)(Rg + b * BN * 8) + wave * 2048;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = ng0 + nt * BN + 8 * (wave * 2 + j) + (lane >> 3);
      __builtin_amdgcn_global_load_lds((gptr_t)(Wt + (long long)n * p.K + kt * 32 + kc * 4), (lptr_t)(dst + j * 1024), 16, 0, 0);
    }
  };
  // weight cursor: one step ahead of the compute cursor; the weights do not depend on the M-tile, so it simply wraps
  int wnt = 0, wkt = 0, issued = 0, buf = 0;
  const int total = count * ngt * KPT;
  auto issue_next_w = [&]() __attribute__((always_inline)) {
    issue_w(wnt, wkt, issued & 1);
    ++issued;
    if (++wkt == KPT) { wkt = 0; if (++wnt == ngt) wnt = 0; }
  };
  if (count > 0) {
    issue_panel(mslot);
    issue_next_w();
  }
  for (int ct = 0; ct < count; ++ct) {
    const int m = (mslot + ct * mslots) * BM + wave * 16 + fl;       // this lane's row
    const long long off = m < p.M ? (long long)m * p.N : -1;         // element offset of (row, column 0), -1: a row beyond M
    for (int nt = 0; nt < ngt; ++nt) {
      f32x4 acc[NI];
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) acc[ni] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kt = 0; kt < KPT; ++kt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this step's weight stage (and, at a tile's first step, the panel) has landed
        __syncthreads();                                       // ... for every wave, and every wave is done with the other stage
        if (issued < total) issue_next_w();
        if (nt == 0 && kt == 0) {
          // the panel of an fp32 tensor, split IN PLACE once per M-tile: the two 16-byte chunks (gq, 4 + gq) of a 128-byte row -- the eight
          // values lane group gq multiplies in one MFMA -- become their (hi, lo) fp16 pieces
          for (int q = tid; q < KPT * BM * 4; q += 256) {
            const int row = q >> 2, gq = q & 3;              // row runs over all k-blocks: BM is a multiple of 8
            u32x4* w0 = Pn + row * 8 + (gq ^ (row & 7));
            u32x4* w1 = Pn + row * 8 + ((4 + gq) ^ (row & 7));
            u32x4 hi, lo;
            split_terms2_f16(*w0, *w1, hi, lo);
            *w0 = hi; *w1 = lo;
          }
          __syncthreads();
        }
        const u32x4* Bt = Rg + buf * BN * 8;
        const u32x4* Pk = Pn + kt * BM * 8;
        mma_f32_chunks<NI, 1, false, 13, true, true>(&acc[0],
            [&](int i, int ks) { const int r = i * 16 + fl; return Bt[r * 8 + ((ks * 4 + g) ^ (r & 7))]; },
            [&](int, int ks) { const int r = wave * 16 + fl; return Pk[r * 8 + ((ks * 4 + g) ^ (r & 7))]; });
        buf ^= 1;
      }
      if (nt == ngt - 1 && ct + 1 < count) {
        __syncthreads();                                       // every wave has read the panel for the last time
        issue_panel(mslot + (ct + 1) * mslots);
      }
      // ---- fused BatchNorm-apply epilogue: bn_apply<float>'s arithmetic on the fp32 accumulators, in the order of
      // conv_igemm_persistent's FAPPLY epilogue (same bits).  The row's residual operands are requested up front.
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) acc[ni] *= (1.0f / (float)(1 << F16_WSCALE_LOG2));   // the fp16 weight planes carry 2^F16_WSCALE_LOG2
      const bool ok = off >= 0;
      const int nl0 = nt * BN + g * 4;                         // this lane's first column in the group; fragment ni adds 16 * ni
      const long long a = ok ? off + ng0 + nl0 : 0;            // masked rows read (and ignore) the first elements of the residual
      float4 rr[NI];
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) rr[ni] = *(const float4*)((const float*)p.bn_x + a + ni * 16);
      u32x4 mbits;                                             // ReLU bits of the row's 64 columns: 16 bytes, held by lane group 0
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        const int nl = nl0 + ni * 16;
        const float4 sc = *(const float4*)(bnp + nl), sh = *(const float4*)(bnp + G + nl);
        float o[4] = {fmaf(acc[ni][0], sc.x, sh.x), fmaf(acc[ni][1], sc.y, sh.y), fmaf(acc[ni][2], sc.z, sh.z), fmaf(acc[ni][3], sc.w, sh.w)};
        const float4 r = rr[ni];
        if (FAS == 2) {
          const float4 rs = *(const float4*)(bnp + 2 * G + nl), rb = *(const float4*)(bnp + 3 * G + nl);
          o[0] += fmaf(r.x, rs.x, rb.x); o[1] += fmaf(r.y, rs.y, rb.y); o[2] += fmaf(r.z, rs.z, rb.z); o[3] += fmaf(r.w, rs.w, rb.w);
        } else { o[0] += r.x; o[1] += r.y; o[2] += r.z; o[3] += r.w; }
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = fmaxf(o[e], 0.f);
        if (ok) *(float4*)(Y + a + ni * 16) = make_float4(o[0], o[1], o[2], o[3]);
        // ReLU bits: one byte per 16-byte chunk = one lane's 4 channels; the 4 lane groups of a fragment row hold 4 consecutive bytes
        const unsigned bits = (o[0] > 0.f ? 1u : 0u) | (o[1] > 0.f ? 2u : 0u) | (o[2] > 0.f ? 4u : 0u) | (o[3] > 0.f ? 8u : 0u);
        const unsigned b1 = __shfl(bits, lane + 16, 64), b2 = __shfl(bits, lane + 32, 64), b3 = __shfl(bits, lane + 48, 64);
        mbits[ni] = bits | (b1 << 8) | (b2 << 16) | (b3 << 24);
      }
      if (ok && g == 0) *(u32x4*)((unsigned char*)p.bn_mask + (a >> 2)) = mbits;     // a = off + ng0 + 64 nt here: 16-byte aligned
    }
  }
}
