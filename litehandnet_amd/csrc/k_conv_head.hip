// The heatmap head (litehourglass.py:159-166: nn.Conv2d(128, 21, 1) with an NCHW result) on streaming kernels.
// The head is a memory-bound 1x1: K = 21 output features make its FLOPs negligible, its traffic is one read of the 128-channel
// map (forward) and one read plus one write of it (backward).  The generic kernels of k_conv_pw.hip keep W in LDS and run ONE
// workgroup per CU for these shapes (84 KB of LDS, __launch_bounds__(256, 1)): one wave per SIMD, so the loads, the LDS commit,
// the MFMAs and the stores of a tile add up.  Here W lives in registers (forward: 64 VGPRs, backward: 16), LDS holds only the pixel
// tile, and two workgroups share a CU: one's loads and stores run under the other's MFMA phase.
//   forward : y_nchw[n][co][p] = bias[co] + sum_ci z[m][ci] W[co][ci]              z = gate * act(table(raw x)), applied on load
//   backward: dx[m][ci] (+)= sum_co dy[m][co] W[co][ci];  dW[co][ci] += sum_m dy[m][co] z[m][ci];  dbias[co] += sum_m dy[m][co]
//             and, optionally (lhn_gatesum), the gate-gradient sums of x's buffer: the lane that holds dx[m][c] re-reads the raw
//             x[m][c] from an LDS copy of the staged tile and adds dx*act(u), dx*act'(u), dx*act'(u)*xhat per (image, channel) --
//             what k_gate_bwd_reduce (k_misc.hip) computes in a pass of its own over x and dx.
// Shapes: Cin = 128 (whole weight rows), Cout <= 32, stride 1, H*W % 4 == 0; any NCHW batch stride.  MFMA v_mfma_f32_32x32x2_f32 with
// the K permutation of k_conv_pw.hip, so the forward adds the same terms in the same order as k_pw_fwd<128,1,1>.
#include <stdlib.h>
#include "lhn_common.h"

// Which calls come here is pw_fwd_route / pw_bwd_route's decision (k_conv_pw.hip; lhn_head_shape and the LHN_HEAD_STREAM switch).
constexpr int HCIN = HEAD_CIN, HLDX = HCIN + 4;
constexpr int HLDR = HCIN + 8;      // raw copy: lane halves sit four rows apart, 4 * 136 floats = 32 banks apart (no conflict)

// ----------------------------------------------------------------------------------------------------- forward
// 128-pixel tiles, wave v owns pixel rows [32 v, 32 v + 32) and ALL (<= 32) features.  One LDS tile (67.6 KB: two workgroups per
// CU); the next tile rides in registers while this one is multiplied (k_pw_fwd_wr's scheme with one buffer).
__global__ void __launch_bounds__(256, 2) k_head_fwd(lhn_view x, const float* __restrict__ w, const float* __restrict__ bias,
                                                     float* __restrict__ y_nchw, int cout, int M, int HoWo, int ntiles, int64_t bstride) {
  constexpr int BM = 128, C4 = HCIN / 4, RP = 256 / C4, PF = BM / RP;
  extern __shared__ __attribute__((aligned(16))) float smem[];      // [BM][HLDX]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, lh = lane >> 5;
  const int co = l31;
  // B fragments: wreg[kc*4 + j] = W[co][8*kc + 4*lh + j]
  float wreg[HCIN / 2];
#pragma unroll
  for (int kc = 0; kc < HCIN / 8; ++kc) {
    f4 v = (f4){0.f, 0.f, 0.f, 0.f};
    if (co < cout) v = *reinterpret_cast<const f4*>(w + (int64_t)co * HCIN + kc * 8 + 4 * lh);
    wreg[kc * 4 + 0] = v.x; wreg[kc * 4 + 1] = v.y; wreg[kc * 4 + 2] = v.z; wreg[kc * 4 + 3] = v.w;
  }
  const float bv = (bias && co < cout) ? bias[co] : 0.f;
  const int c4 = tid % C4, row0 = tid / C4, cabs = x.coff + 4 * c4;
  const bool uni = HoWo % BM == 0;      // a tile inside one image: its gate is one float4 per thread, fetched with the tile
  const f4 one4 = (f4){1.f, 1.f, 1.f, 1.f};
  f4 pre[PF], gpre = one4;
  auto issue = [&](int tile) __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < PF; ++p) {
      const int m = min(tile * BM + row0 + p * RP, M - 1);      // clamped: rows >= M are zeroed at commit
      pre[p] = *reinterpret_cast<const f4*>(x.data + (int64_t)m * x.cstride + cabs);
    }
    if (uni) gpre = x.gate ? *reinterpret_cast<const f4*>(x.gate + (int64_t)(min(tile * BM, M - 1) / HoWo) * x.cstride + cabs) : one4;
  };
  int tile = blockIdx.x;
  if (tile < ntiles) issue(tile);
  const Xf4 xf = lhn_load_xf(x, cabs);
  for (; tile < ntiles; tile += gridDim.x) {
#pragma unroll
    for (int p = 0; p < PF; ++p) {
      const int row = row0 + p * RP, m = tile * BM + row;
      f4 g = gpre;
      if (!uni) g = x.gate ? *reinterpret_cast<const f4*>(x.gate + (int64_t)(min(m, M - 1) / HoWo) * x.cstride + cabs) : one4;
      const f4 v = lhn_apply_xf(pre[p], xf) * g;
      *reinterpret_cast<f4*>(smem + row * HLDX + 4 * c4) = m < M ? v : (f4){0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();
    if (tile + (int)gridDim.x < ntiles) issue(tile + gridDim.x);
    f16v acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float* arow = smem + (wave * 32 + l31) * HLDX + 4 * lh;
#pragma unroll
    for (int kc = 0; kc < HCIN / 8; ++kc) {
      const f4 a = *reinterpret_cast<const f4*>(arow + kc * 8);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, wreg[kc * 4 + 0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, wreg[kc * 4 + 1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, wreg[kc * 4 + 2], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, wreg[kc * 4 + 3], acc, 0, 0, 0);
    }
    __syncthreads();      // the tile is consumed: the next commit may overwrite it while the stores below drain
    // C/D layout: col = lane&31 (feature), row = (r&3) + 8*(r>>2) + 4*(lane>>5) (pixel): registers 4g..4g+3 are four consecutive
    // pixels of one plane (H*W % 4 == 0, host-checked: they share an image)
    if (co < cout) {
      const int mbase = tile * BM + wave * 32 + 4 * lh;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int m0 = mbase + 8 * g;
        if (m0 < M) {
          const int n = m0 / HoWo, p = m0 - n * HoWo;
          *reinterpret_cast<f4*>(y_nchw + (int64_t)n * bstride + (int64_t)co * HoWo + p) =
              (f4){acc[4 * g] + bv, acc[4 * g + 1] + bv, acc[4 * g + 2] + bv, acc[4 * g + 3] + bv};
        }
      }
    }
  }
}

int lhn_head_fwd(const lhn_view* x, const float* w, const float* bias, float* y_nchw, int cout, int HoWo, int64_t bstride, hipStream_t s) {
  const int M = x->N * HoWo, ntiles = (M + 127) / 128;
  const size_t lds = (size_t)128 * HLDX * sizeof(float);
  static LhnKernelCfg cfg;
  int per_cu = 1;
  if (!lhn_kernel_cfg(cfg, &k_head_fwd, lds, 2, &per_cu)) {
    lhn_set_error("lhn_conv_pw_fwd: cannot reserve %zu B of LDS", lds);
    return 2;
  }
  int grid = lhn_num_cus() * per_cu;
  if (grid > ntiles) grid = ntiles;
  hipLaunchKernelGGL(k_head_fwd, dim3(grid), dim3(256), lds, s, *x, w, bias, y_nchw, cout, M, HoWo, ntiles, bstride);
  return 0;
}

// ----------------------------------------------------------------------------------------------------- backward
// Gate-gradient sums of x's buffer (lhn_gatesum resolved by the host): dgate[N][cs], tsum[N][2][cs] at the buffer's channel stride,
// mean | invstd of the (up to two) BatchNorm slices; channels outside every slice use mean 0, invstd 1 (lhn_slice_mi4, k_misc.hip)
struct HeadGate {
  float* dgate;
  float* tsum;
  const float* save[2];
  int lo[2], C[2], n;
};

// 64-pixel tiles.  Wave v owns input channels [32 v, 32 v + 32): its column of dX (two 32-pixel sub-tiles, B operand = its slice of
// W in 16 registers) and its 32 x 32 tile of dW (accumulators for the whole launch, one atomic flush per workgroup into its
// replica).  dy comes straight from the NCHW planes as float4 over four pixels of a plane; its column sums are dbias.  A workgroup
// takes a CONTIGUOUS run of tiles, so consecutive tiles belong to one image and the gate sums (GS) stay in registers until the image
// changes: few atomics per address.  GS needs tiles that do not straddle images (H*W % 64 == 0, host-checked).
template <bool GS>
__global__ void __launch_bounds__(256, 2) k_head_bwd(lhn_view x, const float* __restrict__ w, const float* __restrict__ dy,
                                                     float* __restrict__ dx, int dx_acc, float* __restrict__ dw, float* __restrict__ dbias,
                                                     int cout, int M, int HoWo, int ntiles, int chunk, int64_t bstride, int nrep,
                                                     int64_t rep_stride, HeadGate hg) {
  constexpr int PX = 64, LDY = 36, XC4 = HCIN / 4, XRP = 256 / XC4, XPF = PX / XRP;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* dYs = smem;                  // [PX][LDY]   dy, zero beyond cout and beyond M
  float* Xs = dYs + PX * LDY;         // [PX][HLDX]  consumed x
  float* Xr = Xs + PX * HLDX;         // [PX][HLDR]  raw x (GS only)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, lh = lane >> 5;
  const int xc4 = tid % XC4, xr0 = tid / XC4, xabs = x.coff + 4 * xc4;
  const int yr4 = tid & 15, yco = tid >> 4;      // dy loader: pixels [4 yr4, 4 yr4 + 4) of planes yco and yco + 16
  const bool uni = HoWo % PX == 0;
  const f4 one4 = (f4){1.f, 1.f, 1.f, 1.f}, zero4 = (f4){0.f, 0.f, 0.f, 0.f};
  f4 xraw[XPF], yraw[2], gpre = one4;
  auto issue = [&](int tile) __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < XPF; ++p) {
      const int m = min(tile * PX + xr0 + p * XRP, M - 1);      // clamped; commit zeroes rows >= M
      xraw[p] = *reinterpret_cast<const f4*>(x.data + (int64_t)m * x.cstride + xabs);
    }
    const int m4 = min(tile * PX + 4 * yr4, M - 4);             // M % 4 == 0: a group of four is whole or absent
    const int n = m4 / HoWo, p = m4 - n * HoWo;
#pragma unroll
    for (int k = 0; k < 2; ++k)
      yraw[k] = yco + 16 * k < cout ? *reinterpret_cast<const f4*>(dy + (int64_t)n * bstride + (int64_t)(yco + 16 * k) * HoWo + p) : zero4;
    if (uni) gpre = x.gate ? *reinterpret_cast<const f4*>(x.gate + (int64_t)(min(tile * PX, M - 1) / HoWo) * x.cstride + xabs) : one4;
  };
  const int t0 = blockIdx.x * chunk, t1 = min(ntiles, t0 + chunk);
  if (t0 < t1) issue(t0);
  const Xf4 xf = lhn_load_xf(x, xabs);
  // B fragments of the data gradient: wreg[kc*4 + j] = W[8*kc + 4*lh + j][32*wave + l31], zero rows beyond cout
  float wreg[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int co = (k >> 2) * 8 + 4 * lh + (k & 3);
    wreg[k] = (dx && co < cout) ? w[(int64_t)co * HCIN + 32 * wave + l31] : 0.f;
  }
  f16v accw;
#pragma unroll
  for (int r = 0; r < 16; ++r) accw[r] = 0.f;
  double bsum[2] = {0.0, 0.0};      // in double, as k_bias_grad_nchw sums: one float rounding per workgroup, at the flush
  // gate sums: the constants of this lane's channel and its three partial sums of the current image
  const int cg = x.coff + 32 * wave + l31;
  float g_sc = 1.f, g_sh = 0.f, g_sl = 1.f, g_mean = 0.f, g_inv = 1.f, g_d = 0.f, g_0 = 0.f, g_1 = 0.f;
  int n_cur = -1;
  if (GS) {
    if (x.table) {
      g_sc = x.table[cg];
      g_sh = x.table[x.cstride + cg];
      g_sl = x.table[2 * x.cstride + cg];
    }
#pragma unroll
    for (int k = 0; k < 2; ++k)
      if (k < hg.n && cg >= hg.lo[k] && cg < hg.lo[k] + hg.C[k]) {
        g_mean = hg.save[k][cg - hg.lo[k]];
        g_inv = hg.save[k][hg.C[k] + cg - hg.lo[k]];
      }
  }
  auto gflush = [&]() __attribute__((always_inline)) {      // the two lane halves (pixel groups) meet by shuffle, one add per sum
    const float sd = g_d + __shfl_xor(g_d, 32, 64), s0 = g_0 + __shfl_xor(g_0, 32, 64), s1 = g_1 + __shfl_xor(g_1, 32, 64);
    if (lh == 0 && n_cur >= 0) {
      atomicAdd(hg.dgate + (int64_t)n_cur * x.cstride + cg, sd);
      atomicAdd(hg.tsum + ((int64_t)n_cur * 2 + 0) * x.cstride + cg, s0);
      atomicAdd(hg.tsum + ((int64_t)n_cur * 2 + 1) * x.cstride + cg, s1);
    }
    g_d = g_0 = g_1 = 0.f;
  };

  for (int tile = t0; tile < t1; ++tile) {
    // ---- commit: registers -> LDS
#pragma unroll
    for (int p = 0; p < XPF; ++p) {
      const int row = xr0 + p * XRP, m = tile * PX + row;
      f4 g = gpre;
      if (!uni) g = x.gate ? *reinterpret_cast<const f4*>(x.gate + (int64_t)(min(m, M - 1) / HoWo) * x.cstride + xabs) : one4;
      const f4 v = lhn_apply_xf(xraw[p], xf) * g;
      *reinterpret_cast<f4*>(Xs + row * HLDX + 4 * xc4) = m < M ? v : zero4;
      if (GS) *reinterpret_cast<f4*>(Xr + row * HLDR + 4 * xc4) = m < M ? xraw[p] : zero4;
    }
    const bool yin = tile * PX + 4 * yr4 < M;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const f4 v = yin ? yraw[k] : zero4;
      float* d = dYs + (4 * yr4) * LDY + yco + 16 * k;
      d[0] = v.x; d[LDY] = v.y; d[2 * LDY] = v.z; d[3 * LDY] = v.w;
      bsum[k] += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
    }
    __syncthreads();
    if (tile + 1 < t1) issue(tile + 1);
    // ---- dW += dY^T X   (K = 64 pixels)
    {
      const float* ap = dYs + lh * LDY + l31;
      const float* bp = Xs + lh * HLDX + 32 * wave + l31;
#pragma unroll 8
      for (int ks = 0; ks < PX / 2; ++ks) accw = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * ks * LDY], bp[2 * ks * HLDX], accw, 0, 0, 0);
    }
    // ---- dX = dY W   (K = 32 features, rows beyond cout are zero on both sides)
    if (dx) {
      if (GS) {
        const int n = (tile * PX) / HoWo;
        if (n != n_cur) {
          gflush();
          n_cur = n;
        }
      }
#pragma unroll 1      // (the two sub-tiles one after the other: unrolled, the gate-sum instance kept both live and spilled)
      for (int hh = 0; hh < 2; ++hh) {
        f16v accx;
#pragma unroll
        for (int r = 0; r < 16; ++r) accx[r] = 0.f;
        const float* arow = dYs + (hh * 32 + l31) * LDY + 4 * lh;
#pragma unroll
        for (int kc = 0; kc < 4; ++kc) {
          const f4 a = *reinterpret_cast<const f4*>(arow + kc * 8);
          accx = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, wreg[kc * 4 + 0], accx, 0, 0, 0);
          accx = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, wreg[kc * 4 + 1], accx, 0, 0, 0);
          accx = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, wreg[kc * 4 + 2], accx, 0, 0, 0);
          accx = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, wreg[kc * 4 + 3], accx, 0, 0, 0);
        }
        // C/D layout: col = lane&31 (input channel), row = (r&3) + 8*(r>>2) + 4*(lane>>5) (pixel)
        if (GS) {      // rows beyond M are zero rows of dYs: their dX is exactly 0 and adds nothing
          const float* xr = Xr + (hh * 32 + 4 * lh) * HLDR + 32 * wave + l31;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float raw = xr[((r & 3) + 8 * (r >> 2)) * HLDR];
            const float u = raw * g_sc + g_sh;
            const float da = accx[r] * (u > 0.f ? 1.f : g_sl);
            g_d += accx[r] * lhn_lrelu(u, g_sl);
            g_0 += da;
            g_1 += da * ((raw - g_mean) * g_inv);
          }
        }
        const int cs = x.cstride, mbase = tile * PX + hh * 32 + 4 * lh;
        float* o = dx + (int64_t)mbase * cs + cg;
        if (tile * PX + PX <= M) {
          if (dx_acc) {
#pragma unroll
            for (int r = 0; r < 16; ++r) o[((r & 3) + 8 * (r >> 2)) * cs] += accx[r];
          } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) o[((r & 3) + 8 * (r >> 2)) * cs] = accx[r];
          }
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int ro = (r & 3) + 8 * (r >> 2);
            if (mbase + ro < M) o[(int64_t)ro * cs] = dx_acc ? o[(int64_t)ro * cs] + accx[r] : accx[r];
          }
        }
      }
    }
    __syncthreads();
  }
  if (GS) gflush();
  if (t0 >= t1) return;      // (more workgroups than runs of tiles: nothing to add)
  // ---- flush dW (C/D layout: row = feature, col = lane&31 = input channel of this wave's tile) and dbias into the replica
  float* rep = dw + (size_t)(blockIdx.x % nrep) * rep_stride;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int co = (r & 3) + 8 * (r >> 2) + 4 * lh;
    if (co < cout) atomicAdd(rep + (int64_t)co * HCIN + 32 * wave + l31, accw[r]);
  }
  if (dbias) {      // the 16 lanes that share a plane meet by shuffle in a fixed order: one add per feature and workgroup
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      double v = bsum[k];
      v += __shfl_xor(v, 1, 64);
      v += __shfl_xor(v, 2, 64);
      v += __shfl_xor(v, 4, 64);
      v += __shfl_xor(v, 8, 64);
      if (yr4 == 0 && yco + 16 * k < cout) atomicAdd(dbias + (size_t)(blockIdx.x % nrep) * rep_stride + yco + 16 * k, (float)v);
    }
  }
}

template <bool GS>
static int launch_head_bwd(const lhn_view* x, const float* w, const float* dy, float* dx, int dx_acc, float* dw, float* dbias, int cout,
                           int HoWo, int64_t bstride, int nrep, int64_t rep_stride, const HeadGate& hg, hipStream_t s) {
  const int M = x->N * HoWo, ntiles = (M + 63) / 64;
  const size_t lds = (size_t)(64 * 36 + 64 * HLDX + (GS ? 64 * HLDR : 0)) * sizeof(float);
  static LhnKernelCfg cfg;
  int per_cu = 1;
  if (!lhn_kernel_cfg(cfg, &k_head_bwd<GS>, lds, 2, &per_cu)) {
    lhn_set_error("lhn_conv_pw_bwd: cannot reserve %zu B of LDS", lds);
    return 2;
  }
  int grid = lhn_num_cus() * per_cu;
  if (grid > ntiles) grid = ntiles;
  const int chunk = (ntiles + grid - 1) / grid;
  grid = (ntiles + chunk - 1) / chunk;      // every workgroup has at least one tile
  hipLaunchKernelGGL(k_head_bwd<GS>, dim3(grid), dim3(256), lds, s, *x, w, dy, dx, dx_acc, dw, dbias, cout, M, HoWo, ntiles, chunk, bstride,
                     nrep, rep_stride, hg);
  return 0;
}

// gs: the gate sums of x's buffer or NULL.  The caller has checked the shape (lhn_conv_pw_bwd5).
int lhn_head_bwd(const lhn_view* x, const float* w, const float* dy, float* dx, int dx_acc, float* dw, float* dbias, int cout, int HoWo,
                 int64_t bstride, int nrep, int64_t rep_stride, const lhn_gatesum* gs, hipStream_t s) {
  HeadGate hg;
  memset(&hg, 0, sizeof(hg));
  if (!gs) return launch_head_bwd<false>(x, w, dy, dx, dx_acc, dw, dbias, cout, HoWo, bstride, nrep, rep_stride, hg, s);
  hg.dgate = gs->dgate;
  hg.tsum = gs->dgate + (size_t)x->N * x->cstride;
  if (gs->slices)
    for (int k = 0; k < gs->slices->n; ++k) {
      hg.save[hg.n] = gs->slices->save[k];
      hg.lo[hg.n] = gs->slices->lo[k];
      hg.C[hg.n] = gs->slices->C[k];
      ++hg.n;
    }
  return launch_head_bwd<true>(x, w, dy, dx, dx_acc, dw, dbias, cout, HoWo, bstride, nrep, rep_stride, hg, s);
}
