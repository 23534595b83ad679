// Inference only: BottleNeck (liteHandNet.py:23-37 over repblocks.py:8-44) -- 1x1 (C -> Cm), dense 3x3 (Cm -> Cm), 1x1 (Cm -> C),
// residual sum and output activation -- in ONE launch (lhn_bottleneck_fwd).  Outside training the three pending transforms are
// known before the launch, so the three intermediate tensors live in LDS only: x is read once (plus the 10 x 10 halo) and the
// sum is written once.  All three convolutions run on v_mfma_f32_32x32x2_f32 with the operand maps of k_conv_pw.hip / k_conv_dwpw.hip:
// A = 32 features x 2 k (lane & 31 = feature, lane >> 5 = k), B = 2 k x 32 pixels, D column = lane & 31 (pixel), D row =
// (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) (feature).
#include "lhn_common.h"

// A workgroup (4 waves) computes ONE 8 x 8 output tile of one image (a persistent tile loop made the compiler hoist every weight and
// table load out of it: 82 spilled VGPRs; straight-line it needs 112):
//   load     the 10 x 10 halo of value(x) (table and gate applied, addresses clamped into the map) -> xs[100][C + 4]
//   stage 1  t1 = act1(w1 . xs (+ b1)) for the 100 halo pixels (4 pixel tiles of 32, rows >= 100 read row 99 and are dropped),
//            w1 in registers; a halo pixel OUTSIDE the map stores 0 -- the 3x3 pads t1, not x -> ts1[100][CM + 4]
//   stage 2  t2 = act2(conv3x3(ts1)): nine shifted GEMMs over the 64 output pixels, the A operand (w2 of one tap) streamed from
//            L2 one tap ahead.  CM = 64: wave = (feature tile, pixel tile).  CM = 32 has two wave tiles only, so the wave pairs
//            split the taps (0..4 | 5..8) and meet through LDS.  -> ts2[64][CM + 4], which re-uses xs (dead after stage 1)
//   stage 3  y = lrelu_out(value(x) + act3(w3 . ts2 (+ b3))): wave = feature tile of 32, both pixel tiles; the residual is
//            re-read from memory (an L2 hit: this workgroup loaded it a few microseconds ago) while the MFMAs run.
// A pixel is one column of every MFMA, so tile pixels outside the map compute on clamped loads and are never stored.
// TM: w2 is the tap-major copy [9][CM][CM] (16-byte loads); else the OIHW tensor itself (4-byte loads, 36-byte stride).
// No statistics, no atomics, fixed summation order: repeated runs give identical bits.
template <int CM, bool TM>
__global__ void __launch_bounds__(256, 2)
k_bottleneck_fwd(lhn_view x, const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ t1,
                 const float* __restrict__ w2, const float* __restrict__ t2, const float* __restrict__ w3,
                 const float* __restrict__ b3, const float* __restrict__ t3, float out_slope, lhn_view y, int tiles_x, int tiles_y) {
  constexpr int C = 128, LDX = C + 4, LDT = CM + 4, HP = 100, NF = CM / 32, NP1 = NF, NLD = 13;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* xs = smem;                    // [100][LDX]  value(x) of the halo tile
  float* ts1 = smem + HP * LDX;        // [100][LDT]  t1, zero outside the map
  float* ts2 = smem;                   // [64][LDT]   t2 (over xs)
  float* red = smem + 64 * LDT;        // CM == 32: [2][16][64] partial accumulators of the second tap group (over xs)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, lh = lane >> 5;
  const int H = x.H, W = x.W;
  const f4 zero = (f4){0.f, 0.f, 0.f, 0.f};

  // ---- loader: thread = (channel group c4, pixel lane pl of 8)
  const int c4 = tid & 31, pl = tid >> 5;
  const int cabs = x.coff + 4 * c4;
  const Xf4 xf = lhn_load_xf(x, cabs);
  // ---- stage 1 operands: w1reg[kc * 4 + j] = w1[ft1 * 32 + l31][8 * kc + 4 * lh + j]
  const int ft1 = NF == 2 ? (wave & 1) : 0;
  // ---- stage 2 geometry
  const int ft2 = NF == 2 ? (wave & 1) : 0, pt2 = NF == 2 ? (wave >> 1) : (wave & 1), tg = NF == 2 ? 0 : (wave >> 1);
  const int tap_b = NF == 2 ? 0 : (tg ? 5 : 0), tap_e = NF == 2 ? 9 : (tg ? 9 : 5);
  const int p2 = pt2 * 32 + l31, hrow2 = (p2 >> 3) * 10 + (p2 & 7);
  auto load_w2 = [&](int tap, float (&dst)[CM / 2]) __attribute__((always_inline)) {
#pragma unroll
    for (int kc = 0; kc < CM / 8; ++kc) {
      if (TM) {
        const f4 v = *reinterpret_cast<const f4*>(w2 + ((size_t)tap * CM + ft2 * 32 + l31) * CM + kc * 8 + 4 * lh);
        dst[kc * 4 + 0] = v.x; dst[kc * 4 + 1] = v.y; dst[kc * 4 + 2] = v.z; dst[kc * 4 + 3] = v.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) dst[kc * 4 + j] = w2[((size_t)(ft2 * 32 + l31) * CM + kc * 8 + 4 * lh + j) * 9 + tap];
      }
    }
  };
  {
    const int tile = blockIdx.x;
    const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, n = tile / (tiles_x * tiles_y);
    const int ty0 = ty * 8, tx0 = tx * 8;
    const float* xn = x.data + (int64_t)n * H * W * x.cstride;
    // ---- load the halo tile
    {
      f4 pre[NLD];
#pragma unroll
      for (int p = 0; p < NLD; ++p) {
        const int hp = min(pl + 8 * p, HP - 1), hy = hp / 10, hx = hp - hy * 10;
        const int iy = min(max(ty0 - 1 + hy, 0), H - 1), ix = min(max(tx0 - 1 + hx, 0), W - 1);
        pre[p] = *reinterpret_cast<const f4*>(xn + ((int64_t)iy * W + ix) * x.cstride + cabs);
      }
      const f4 gate = x.gate ? *reinterpret_cast<const f4*>(x.gate + (int64_t)n * x.cstride + cabs) : (f4){1.f, 1.f, 1.f, 1.f};
#pragma unroll
      for (int p = 0; p < NLD; ++p) {
        const int hp = pl + 8 * p;
        if (hp < HP) *reinterpret_cast<f4*>(xs + hp * LDX + 4 * c4) = lhn_apply_xf(pre[p], xf) * gate;
      }
    }
    __syncthreads();      // xs is in

    // ---- stage 1: t1 of the halo pixels
    {
      float w1reg[C / 2];
#pragma unroll
      for (int kc = 0; kc < C / 8; ++kc) {
        const f4 v = *reinterpret_cast<const f4*>(w1 + (ft1 * 32 + l31) * C + kc * 8 + 4 * lh);
        w1reg[kc * 4 + 0] = v.x; w1reg[kc * 4 + 1] = v.y; w1reg[kc * 4 + 2] = v.z; w1reg[kc * 4 + 3] = v.w;
      }
      f16v acc[NP1];
#pragma unroll
      for (int j = 0; j < NP1; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
      const float* brow[NP1];
#pragma unroll
      for (int j = 0; j < NP1; ++j) {
        const int pt = NF == 2 ? (wave >> 1) + 2 * j : wave;
        brow[j] = xs + min(pt * 32 + l31, HP - 1) * LDX + 4 * lh;
      }
#pragma unroll
      for (int kc = 0; kc < C / 8; ++kc) {
#pragma unroll
        for (int j = 0; j < NP1; ++j) {
          const f4 b = *reinterpret_cast<const f4*>(brow[j] + kc * 8);
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1reg[kc * 4 + 0], b.x, acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1reg[kc * 4 + 1], b.y, acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1reg[kc * 4 + 2], b.z, acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1reg[kc * 4 + 3], b.w, acc[j], 0, 0, 0);
        }
      }
#pragma unroll
      for (int j = 0; j < NP1; ++j) {
        const int pt = NF == 2 ? (wave >> 1) + 2 * j : wave;
        const int hp = pt * 32 + l31, hy = hp / 10, hx = hp - hy * 10;
        const int iy = ty0 - 1 + hy, ix = tx0 - 1 + hx;
        const bool inside = iy >= 0 && iy < H && ix >= 0 && ix < W;
        if (hp < HP) {
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int f = ft1 * 32 + 8 * g + 4 * lh;
            f4 v = (f4){acc[j][4 * g + 0], acc[j][4 * g + 1], acc[j][4 * g + 2], acc[j][4 * g + 3]};
            if (b1) v += *reinterpret_cast<const f4*>(b1 + f);
            v = lhn_apply_xf(v, lhn_load_xf_t(t1, CM, f));
            *reinterpret_cast<f4*>(ts1 + hp * LDT + f) = inside ? v : zero;
          }
        }
      }
    }
    __syncthreads();      // ts1 is in; nobody reads xs any more

    // ---- stage 2: nine shifted GEMMs, weights one tap ahead
    {
      f16v acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      float wa[CM / 2];
      load_w2(tap_b, wa);
#pragma unroll 1
      for (int tap = tap_b; tap < tap_e; ++tap) {
        float wn[CM / 2];
        load_w2(min(tap + 1, tap_e - 1), wn);
        const int dy = tap / 3, dx = tap - dy * 3;
        const float* brow = ts1 + (hrow2 + dy * 10 + dx) * LDT + 4 * lh;
#pragma unroll
        for (int kc = 0; kc < CM / 8; ++kc) {
          const f4 b = *reinterpret_cast<const f4*>(brow + kc * 8);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[kc * 4 + 0], b.x, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[kc * 4 + 1], b.y, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[kc * 4 + 2], b.z, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[kc * 4 + 3], b.w, acc, 0, 0, 0);
        }
#pragma unroll
        for (int k = 0; k < CM / 2; ++k) wa[k] = wn[k];
      }
      if (NF == 1) {      // taps 5..8 join taps 0..4 (always in this order)
        if (tg == 1) {
#pragma unroll
          for (int r = 0; r < 16; ++r) red[(pt2 * 16 + r) * 64 + lane] = acc[r];
        }
        __syncthreads();
        if (tg == 0) {
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[r] += red[(pt2 * 16 + r) * 64 + lane];
        }
      }
      if (tg == 0) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int f = ft2 * 32 + 8 * g + 4 * lh;
          const f4 v = (f4){acc[4 * g + 0], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
          *reinterpret_cast<f4*>(ts2 + p2 * LDT + f) = lhn_apply_xf(v, lhn_load_xf_t(t2, CM, f));
        }
      }
    }
    __syncthreads();      // ts2 is in

    // ---- stage 3: the second 1x1, residual sum, output activation; w3reg[kc * 4 + j] = w3[wave * 32 + l31][8 * kc + 4 * lh + j]
    {
      float w3reg[CM / 2];
#pragma unroll
      for (int kc = 0; kc < CM / 8; ++kc) {
        const f4 v = *reinterpret_cast<const f4*>(w3 + (wave * 32 + l31) * CM + kc * 8 + 4 * lh);
        w3reg[kc * 4 + 0] = v.x; w3reg[kc * 4 + 1] = v.y; w3reg[kc * 4 + 2] = v.z; w3reg[kc * 4 + 3] = v.w;
      }
      f4 xr[2][4];
      bool valid[2];
      int64_t pix[2];
#pragma unroll
      for (int pt = 0; pt < 2; ++pt) {
        const int p = pt * 32 + l31, iy = ty0 + (p >> 3), ix = tx0 + (p & 7);
        valid[pt] = iy < H && ix < W;
        pix[pt] = ((int64_t)n * H + min(iy, H - 1)) * W + min(ix, W - 1);
#pragma unroll
        for (int g = 0; g < 4; ++g)
          xr[pt][g] = *reinterpret_cast<const f4*>(x.data + pix[pt] * x.cstride + x.coff + wave * 32 + 8 * g + 4 * lh);
      }
      f16v acc[2];
#pragma unroll
      for (int pt = 0; pt < 2; ++pt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[pt][r] = 0.f;
#pragma unroll
      for (int kc = 0; kc < CM / 8; ++kc) {
#pragma unroll
        for (int pt = 0; pt < 2; ++pt) {
          const f4 b = *reinterpret_cast<const f4*>(ts2 + (pt * 32 + l31) * LDT + 4 * lh + kc * 8);
          acc[pt] = __builtin_amdgcn_mfma_f32_32x32x2f32(w3reg[kc * 4 + 0], b.x, acc[pt], 0, 0, 0);
          acc[pt] = __builtin_amdgcn_mfma_f32_32x32x2f32(w3reg[kc * 4 + 1], b.y, acc[pt], 0, 0, 0);
          acc[pt] = __builtin_amdgcn_mfma_f32_32x32x2f32(w3reg[kc * 4 + 2], b.z, acc[pt], 0, 0, 0);
          acc[pt] = __builtin_amdgcn_mfma_f32_32x32x2f32(w3reg[kc * 4 + 3], b.w, acc[pt], 0, 0, 0);
        }
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int f = wave * 32 + 8 * g + 4 * lh;
        const Xf4 tf = lhn_load_xf_t(t3, C, f), xg = lhn_load_xf(x, x.coff + f);
        const f4 gate = x.gate ? *reinterpret_cast<const f4*>(x.gate + (int64_t)n * x.cstride + x.coff + f) : (f4){1.f, 1.f, 1.f, 1.f};
        const f4 bv = b3 ? *reinterpret_cast<const f4*>(b3 + f) : zero;
#pragma unroll
        for (int pt = 0; pt < 2; ++pt) {
          const f4 v = (f4){acc[pt][4 * g + 0], acc[pt][4 * g + 1], acc[pt][4 * g + 2], acc[pt][4 * g + 3]} + bv;
          const f4 s = lhn_apply_xf(xr[pt][g], xg) * gate + lhn_apply_xf(v, tf);
          if (valid[pt])
            *reinterpret_cast<f4*>(y.data + pix[pt] * y.cstride + y.coff + f) =
                (f4){lhn_lrelu(s.x, out_slope), lhn_lrelu(s.y, out_slope), lhn_lrelu(s.z, out_slope), lhn_lrelu(s.w, out_slope)};
        }
      }
    }
  }
}

// w2 [CM][CM][3][3] -> wt [9][CM][CM] (tap, output feature, input feature)
__global__ void __launch_bounds__(256) k_bottleneck_w2_tapmajor(const float* __restrict__ w, float* __restrict__ wt, int cm) {
  const int total = 9 * cm * cm;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int k = i % cm, r = (i / cm) % cm, tap = i / (cm * cm);
    wt[i] = w[((size_t)r * cm + k) * 9 + tap];
  }
}

template <int CM, bool TM>
static int launch_bottleneck(const lhn_view* x, const float* w1, const float* b1, const float* t1, const float* w2, const float* t2,
                             const float* w3, const float* b3, const float* t3, float out_slope, const lhn_view* y, hipStream_t s) {
  const size_t lds = (size_t)(100 * (128 + 4) + 100 * (CM + 4)) * sizeof(float);
  static LhnKernelCfg cfg;
  if (!lhn_kernel_cfg(cfg, &k_bottleneck_fwd<CM, TM>, lds, 2, nullptr)) {
    lhn_set_error("lhn_bottleneck_fwd: cannot reserve %zu B of LDS", lds);
    return 2;
  }
  // work item = workgroup = one 8 x 8 output tile of one image; two of them are resident on a CU at a time (67,200 / 80,000 B of LDS),
  // so a grid beyond 2 * lhn_num_cus() runs in several rounds
  const int tiles_x = (x->W + 7) / 8, tiles_y = (x->H + 7) / 8;
  const int64_t ntiles = (int64_t)x->N * tiles_x * tiles_y;
  if (ntiles > 0x7fffffff) {
    lhn_set_error("lhn_bottleneck_fwd: too many tiles");
    return 1;
  }
  hipLaunchKernelGGL((k_bottleneck_fwd<CM, TM>), dim3((unsigned)ntiles), dim3(256), lds, s, *x, w1, b1, t1, w2, t2, w3, b3, t3, out_slope, *y,
                     tiles_x, tiles_y);
  return 0;
}

// (litehandnet_amd/plan.py: FUSE_BNECK_CHANNELS mirrors this rule)
static bool bottleneck_supported(int c, int cm) { return c == 128 && (cm == 32 || cm == 64); }

// relayout: 0 = wt_scratch already holds the tap-major copy of w2 (the plan executor, when nothing has changed since the run that
// wrote it: LHN_RUN_TABLES_CURRENT), 1 = write it first.  The exported entry point always writes it.
int lhn_bottleneck_fwd_impl(const lhn_view* x, int Cm, const float* w1, const float* b1, const float* t1, const float* w2, const float* t2,
                            const float* w3, const float* b3, const float* t3, float out_slope, const lhn_view* y, float* wt_scratch,
                            int relayout, void* stream) {
  LHN_CHECK_ARG(lhn_view_ok(x) && lhn_view_ok(y) && lhn_no_pend(x) && lhn_no_pend(y) && w1 && w2 && w3, "lhn_bottleneck_fwd: bad view / null pointer");
  LHN_CHECK_ARG(y->N == x->N && y->H == x->H && y->W == x->W, "lhn_bottleneck_fwd: same-size output");
  LHN_CHECK_ARG(y->C == x->C && bottleneck_supported(x->C, Cm),
                "lhn_bottleneck_fwd: unsupported shape: built for 128 -> 32 / 64 -> 128 channels (got %d -> %d -> %d, map %d x %d)", x->C, Cm,
                y->C, x->H, x->W);
  LHN_CHECK_ARG(out_slope >= 0.f && out_slope <= 1.f, "lhn_bottleneck_fwd: unsupported shape: the output activation is a leaky slope in [0, 1] (got %g)",
                (double)out_slope);
  LHN_CHECK_ARG(!(x->data == y->data && x->coff < y->coff + y->C && y->coff < x->coff + x->C),
                "lhn_bottleneck_fwd: unsupported shape: y overlaps x (a pixel's neighbours are read after it is written)");
  hipStream_t s = (hipStream_t)stream;
  if (wt_scratch && relayout) {
    const int total = 9 * Cm * Cm;
    hipLaunchKernelGGL(k_bottleneck_w2_tapmajor, dim3((total + 255) / 256), dim3(256), 0, s, w2, wt_scratch, Cm);
  }
  int rc;
  if (Cm == 64) rc = wt_scratch ? launch_bottleneck<64, true>(x, w1, b1, t1, wt_scratch, t2, w3, b3, t3, out_slope, y, s)
                                : launch_bottleneck<64, false>(x, w1, b1, t1, w2, t2, w3, b3, t3, out_slope, y, s);
  else rc = wt_scratch ? launch_bottleneck<32, true>(x, w1, b1, t1, wt_scratch, t2, w3, b3, t3, out_slope, y, s)
                       : launch_bottleneck<32, false>(x, w1, b1, t1, w2, t2, w3, b3, t3, out_slope, y, s);
  if (rc) return rc;
  LHN_CHECK_LAUNCH("lhn_bottleneck_fwd");
  return 0;
}

extern "C" int lhn_bottleneck_fwd(const lhn_view* x, int Cm, const float* w1, const float* b1, const float* t1, const float* w2,
                                  const float* t2, const float* w3, const float* b3, const float* t3, float out_slope, const lhn_view* y,
                                  float* wt_scratch, void* stream) {
  return lhn_bottleneck_fwd_impl(x, Cm, w1, b1, t1, w2, t2, w3, b3, t3, out_slope, y, wt_scratch, 1, stream);
}
