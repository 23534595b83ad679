// Inference only: BottleNeck (liteHandNet.py:23-37 over repblocks.py:8-44) -- 1x1 (C -> Cm), dense 3x3 (Cm -> Cm), 1x1 (Cm -> C),
// residual sum and output activation -- in ONE launch (lhn_bottleneck_fwd).  Outside training the three pending transforms are
// known before the launch, so the three intermediate tensors live in LDS only: x is read once (plus the 10 x 10 halo) and the
// sum is written once.  All three convolutions run on v_mfma_f32_32x32x2_f32 with the operand maps of k_conv_pw.hip / k_conv_dwpw.hip:
// A = 32 features x 2 k (lane & 31 = feature, lane >> 5 = k), B = 2 k x 32 pixels, D column = lane & 31 (pixel), D row =
// (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) (feature).
#include "lhn_common.h"

// A workgroup (4 waves) computes ONE 8 x 8 output tile of one image (a persistent tile loop made the compiler hoist every weight and
// table load out of it: 82 spilled VGPRs; straight-line it needs 112):
//   load     the 10 x 10 halo of value(x) (table and gate applied, addresses clamped into the map) -> xs[100][KC + 4], KC channels
//            at a time: C = 128 in one piece; C = 256 in K chunks that re-use xs (below)
//   stage 1  t1 = act1(w1 . xs (+ b1)) for the 100 halo pixels (4 pixel tiles of 32, rows >= 100 read row 99 and are dropped),
//            w1 of the chunk in registers, the accumulators live across the chunks (channels ascending: one fixed order); a halo
//            pixel OUTSIDE the map stores 0 -- the 3x3 pads t1, not x -> ts1[100][CM + 4]
//   stage 2  t2 = act2(conv3x3(ts1)): nine shifted GEMMs over the 64 output pixels, the A operand (w2 of one tap, at most 64 input
//            features of it) streamed from L2 one step ahead.  CM = 64: wave = (feature tile, pixel tile).  CM = 32 has two wave
//            tiles only, so the wave pairs split the taps (0..4 | 5..8) and meet through LDS.  CM = 128: wave = feature tile, both
//            pixel tiles on one copy of the weights.  -> ts2[64][CM + 4], which re-uses xs (dead after stage 1)
//   stage 3  y = lrelu_out(value(x) + act3(w3 . ts2 (+ b3))): wave = feature tile of 32, both pixel tiles (C = 256: eight feature
//            tiles, so wave and wave + 4, one after the other); the residual is re-read from memory (an L2 hit: this workgroup
//            loaded it a few microseconds ago) while the MFMAs run.
// A pixel is one column of every MFMA, so tile pixels outside the map compute on clamped loads and are never stored.
// TM: w2 is the tap-major copy [9][CM][CM] (16-byte loads); else the OIHW tensor itself (4-byte loads, 36-byte stride).
// No statistics, no atomics, fixed summation order: repeated runs give identical bits.
//
// C = 256.  The whole halo (xs[100][260], 104,000 B) and all of w1 for a feature tile (128 VGPRs) do not fit beside ts1, so stage 1
// runs over K chunks of x through the same xs; the next chunk's global loads are issued before the MFMAs of the present one and
// land in xs after them.  What is resident per CU is always TWO workgroups (8 waves, 2 per SIMD, 256 registers each), as at C = 128:
//   Cm = 64   two chunks of 128 channels: xs 52,800 B + ts1 27,200 B = 80,000 B per workgroup, 64 weight registers per chunk
//   Cm = 128  ts1 alone is 52,800 B, so xs takes four chunks of 64 channels (27,200 B): 80,000 B again.  One workgroup per CU with
//             128-channel chunks (105,600 B) would leave a CU with one wave per SIMD and nothing to run during the barriers and the
//             chunk loads; four short chunks cost two more barrier pairs per tile.  Stage 1: wave = feature tile, all four pixel
//             tiles (64 accumulators, 32 weight registers).  ts2 (33,792 B) is larger than xs and reaches into ts1: one more
//             barrier between the last read of ts1 and the store of ts2.
template <int C, int CM, bool TM>
__global__ void __launch_bounds__(256, 2)
k_bottleneck_fwd(lhn_view x, const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ t1,
                 const float* __restrict__ w2, const float* __restrict__ t2, const float* __restrict__ w3,
                 const float* __restrict__ b3, const float* __restrict__ t3, float out_slope, lhn_view y, int tiles_x, int tiles_y) {
  constexpr int KC = (C == 256 && CM == 128) ? 64 : 128, NKC = C / KC;      // stage 1: channels of x in LDS at a time
  constexpr int LDX = KC + 4, LDT = CM + 4, HP = 100, NF = CM / 32, NP1 = NF;
  constexpr int CG = KC / 4, PLN = 256 / CG, NLD = (HP + PLN - 1) / PLN;    // loader: channel groups, pixel lanes, pixels per thread
  constexpr int KS = CM > 64 ? 64 : CM, NKS = CM / KS, NP2 = NF == 4 ? 2 : 1;   // stage 2: input features per step, pixel tiles per wave
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* xs = smem;                    // [100][LDX]  value(x) of the halo tile, KC channels of it
  float* ts1 = smem + HP * LDX;        // [100][LDT]  t1, zero outside the map
  float* ts2 = smem;                   // [64][LDT]   t2 (over xs; CM == 128: and over the head of ts1)
  float* red = smem + 64 * LDT;        // CM == 32: [2][16][64] partial accumulators of the second tap group (over xs)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, lh = lane >> 5;
  const int H = x.H, W = x.W;
  const f4 zero = (f4){0.f, 0.f, 0.f, 0.f};

  // ---- loader: thread = (channel group c4, pixel lane pl of PLN)
  const int c4 = tid % CG, pl = tid / CG;
  const int cabs = x.coff + 4 * c4;
  // ---- stage 1 operands: w1reg[kc * 4 + j] = w1[ft1 * 32 + l31][k0 + 8 * kc + 4 * lh + j]
  const int ft1 = NF == 4 ? wave : NF == 2 ? (wave & 1) : 0;
  // ---- stage 2 geometry
  const int ft2 = NF == 4 ? wave : NF == 2 ? (wave & 1) : 0, pt2 = NF == 2 ? (wave >> 1) : (wave & 1), tg = NF == 1 ? (wave >> 1) : 0;
  const int tap_b = NF == 1 ? (tg ? 5 : 0) : 0, tap_e = NF == 1 ? (tg ? 9 : 5) : 9;
  int p2[NP2], hrow2[NP2];
#pragma unroll
  for (int j = 0; j < NP2; ++j) {
    p2[j] = (NP2 == 2 ? j : pt2) * 32 + l31;
    hrow2[j] = (p2[j] >> 3) * 10 + (p2[j] & 7);
  }
  // step = (tap, block of KS input features)
  auto load_w2 = [&](int step, float (&dst)[KS / 2]) __attribute__((always_inline)) {
    const int tap = step / NKS, k0 = (step - tap * NKS) * KS;
#pragma unroll
    for (int kc = 0; kc < KS / 8; ++kc) {
      if (TM) {
        const f4 v = *reinterpret_cast<const f4*>(w2 + ((size_t)tap * CM + ft2 * 32 + l31) * CM + k0 + kc * 8 + 4 * lh);
        dst[kc * 4 + 0] = v.x; dst[kc * 4 + 1] = v.y; dst[kc * 4 + 2] = v.z; dst[kc * 4 + 3] = v.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) dst[kc * 4 + j] = w2[((size_t)(ft2 * 32 + l31) * CM + k0 + kc * 8 + 4 * lh + j) * 9 + tap];
      }
    }
  };
  {
    const int tile = blockIdx.x;
    const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, n = tile / (tiles_x * tiles_y);
    const int ty0 = ty * 8, tx0 = tx * 8;
    const float* xn = x.data + (int64_t)n * H * W * x.cstride;
    // ---- the halo tile, one K chunk: global loads into registers, then table and gate into xs
    auto issue_x = [&](int k0, f4 (&pre)[NLD]) __attribute__((always_inline)) {
#pragma unroll
      for (int p = 0; p < NLD; ++p) {
        const int hp = min(pl + PLN * p, HP - 1), hy = hp / 10, hx = hp - hy * 10;
        const int iy = min(max(ty0 - 1 + hy, 0), H - 1), ix = min(max(tx0 - 1 + hx, 0), W - 1);
        pre[p] = *reinterpret_cast<const f4*>(xn + ((int64_t)iy * W + ix) * x.cstride + cabs + k0);
      }
    };
    auto commit_x = [&](int k0, const f4 (&pre)[NLD]) __attribute__((always_inline)) {
      const Xf4 xf = lhn_load_xf(x, cabs + k0);
      const f4 gate = x.gate ? *reinterpret_cast<const f4*>(x.gate + (int64_t)n * x.cstride + cabs + k0) : (f4){1.f, 1.f, 1.f, 1.f};
#pragma unroll
      for (int p = 0; p < NLD; ++p) {
        const int hp = pl + PLN * p;
        if (hp < HP) *reinterpret_cast<f4*>(xs + hp * LDX + 4 * c4) = lhn_apply_xf(pre[p], xf) * gate;
      }
    };

    // ---- stage 1: t1 of the halo pixels, over the K chunks of x
    {
      f4 pre[NLD];
      issue_x(0, pre);
      f16v acc[NP1];
#pragma unroll
      for (int j = 0; j < NP1; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
      const float* brow[NP1];
#pragma unroll
      for (int j = 0; j < NP1; ++j) {
        const int pt = NF == 4 ? j : NF == 2 ? (wave >> 1) + 2 * j : wave;
        brow[j] = xs + min(pt * 32 + l31, HP - 1) * LDX + 4 * lh;
      }
#pragma unroll
      for (int ch = 0; ch < NKC; ++ch) {
        if (ch) __syncthreads();      // nobody reads the previous chunk any more
        commit_x(ch * KC, pre);
        float w1reg[KC / 2];
#pragma unroll
        for (int kc = 0; kc < KC / 8; ++kc) {
          const f4 v = *reinterpret_cast<const f4*>(w1 + (ft1 * 32 + l31) * C + ch * KC + kc * 8 + 4 * lh);
          w1reg[kc * 4 + 0] = v.x; w1reg[kc * 4 + 1] = v.y; w1reg[kc * 4 + 2] = v.z; w1reg[kc * 4 + 3] = v.w;
        }
        __syncthreads();      // xs is in
        if (ch + 1 < NKC) issue_x((ch + 1) * KC, pre);
#pragma unroll
        for (int kc = 0; kc < KC / 8; ++kc) {
#pragma unroll
          for (int j = 0; j < NP1; ++j) {
            const f4 b = *reinterpret_cast<const f4*>(brow[j] + kc * 8);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1reg[kc * 4 + 0], b.x, acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1reg[kc * 4 + 1], b.y, acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1reg[kc * 4 + 2], b.z, acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1reg[kc * 4 + 3], b.w, acc[j], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < NP1; ++j) {
        const int pt = NF == 4 ? j : NF == 2 ? (wave >> 1) + 2 * j : wave;
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

    // ---- stage 2: nine shifted GEMMs, weights one step ahead
    {
      f16v acc[NP2];
#pragma unroll
      for (int j = 0; j < NP2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
      const int step_b = tap_b * NKS, step_e = tap_e * NKS;
      float wa[KS / 2];
      load_w2(step_b, wa);
#pragma unroll 1
      for (int step = step_b; step < step_e; ++step) {
        float wn[KS / 2];
        load_w2(min(step + 1, step_e - 1), wn);
        const int tap = step / NKS, k0 = (step - tap * NKS) * KS;
        const int dy = tap / 3, dx = tap - dy * 3;
        const float* brow[NP2];
#pragma unroll
        for (int j = 0; j < NP2; ++j) brow[j] = ts1 + (hrow2[j] + dy * 10 + dx) * LDT + k0 + 4 * lh;
#pragma unroll
        for (int kc = 0; kc < KS / 8; ++kc) {
#pragma unroll
          for (int j = 0; j < NP2; ++j) {
            const f4 b = *reinterpret_cast<const f4*>(brow[j] + kc * 8);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[kc * 4 + 0], b.x, acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[kc * 4 + 1], b.y, acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[kc * 4 + 2], b.z, acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[kc * 4 + 3], b.w, acc[j], 0, 0, 0);
          }
        }
#pragma unroll
        for (int k = 0; k < KS / 2; ++k) wa[k] = wn[k];
      }
      if (NF == 1) {      // taps 5..8 join taps 0..4 (always in this order)
        if (tg == 1) {
#pragma unroll
          for (int r = 0; r < 16; ++r) red[(pt2 * 16 + r) * 64 + lane] = acc[0][r];
        }
        __syncthreads();
        if (tg == 0) {
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[0][r] += red[(pt2 * 16 + r) * 64 + lane];
        }
      }
      if (64 * LDT > HP * LDX) __syncthreads();      // ts2 reaches into ts1: every wave has read its last tap
      if (tg == 0) {
#pragma unroll
        for (int j = 0; j < NP2; ++j)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int f = ft2 * 32 + 8 * g + 4 * lh;
            const f4 v = (f4){acc[j][4 * g + 0], acc[j][4 * g + 1], acc[j][4 * g + 2], acc[j][4 * g + 3]};
            *reinterpret_cast<f4*>(ts2 + p2[j] * LDT + f) = lhn_apply_xf(v, lhn_load_xf_t(t2, CM, f));
          }
      }
    }
    __syncthreads();      // ts2 is in

    // ---- stage 3: the second 1x1, residual sum, output activation; w3reg[kc * 4 + j] = w3[ft3 * 32 + l31][8 * kc + 4 * lh + j]
#pragma unroll 1
    for (int ft3 = wave; ft3 < C / 32; ft3 += 4) {
      float w3reg[CM / 2];
#pragma unroll
      for (int kc = 0; kc < CM / 8; ++kc) {
        const f4 v = *reinterpret_cast<const f4*>(w3 + (ft3 * 32 + l31) * CM + kc * 8 + 4 * lh);
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
          xr[pt][g] = *reinterpret_cast<const f4*>(x.data + pix[pt] * x.cstride + x.coff + ft3 * 32 + 8 * g + 4 * lh);
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
        const int f = ft3 * 32 + 8 * g + 4 * lh;
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

template <int C, int CM, bool TM>
static int launch_bottleneck(const lhn_view* x, const float* w1, const float* b1, const float* t1, const float* w2, const float* t2,
                             const float* w3, const float* b3, const float* t3, float out_slope, const lhn_view* y, hipStream_t s) {
  constexpr int KC = (C == 256 && CM == 128) ? 64 : 128;      // the kernel's K chunk of x
  const size_t lds = (size_t)(100 * (KC + 4) + 100 * (CM + 4)) * sizeof(float);
  static LhnKernelCfg cfg;
  if (!lhn_kernel_cfg(cfg, &k_bottleneck_fwd<C, CM, TM>, lds, 2, nullptr)) {
    lhn_set_error("lhn_bottleneck_fwd: cannot reserve %zu B of LDS", lds);
    return 2;
  }
  // work item = workgroup = one 8 x 8 output tile of one image; two of them are resident on a CU at a time (67,200 B of LDS at
  // 128 -> 32, 80,000 B in every other instantiation), so a grid beyond 2 * lhn_num_cus() runs in several rounds
  const int tiles_x = (x->W + 7) / 8, tiles_y = (x->H + 7) / 8;
  const int64_t ntiles = (int64_t)x->N * tiles_x * tiles_y;
  if (ntiles > 0x7fffffff) {
    lhn_set_error("lhn_bottleneck_fwd: too many tiles");
    return 1;
  }
  hipLaunchKernelGGL((k_bottleneck_fwd<C, CM, TM>), dim3((unsigned)ntiles), dim3(256), lds, s, *x, w1, b1, t1, w2, t2, w3, b3, t3, out_slope, *y,
                     tiles_x, tiles_y);
  return 0;
}

template <int C, int CM>
static int launch_bottleneck_w2(const lhn_view* x, const float* w1, const float* b1, const float* t1, const float* w2, const float* t2,
                                const float* w3, const float* b3, const float* t3, float out_slope, const lhn_view* y, const float* wt,
                                hipStream_t s) {
  return wt ? launch_bottleneck<C, CM, true>(x, w1, b1, t1, wt, t2, w3, b3, t3, out_slope, y, s)
            : launch_bottleneck<C, CM, false>(x, w1, b1, t1, w2, t2, w3, b3, t3, out_slope, y, s);
}

// (litehandnet_amd/plan.py: FUSE_BNECK_CHANNELS holds the pairs of this rule that inference plans are rewritten for)
static bool bottleneck_supported(int c, int cm) { return (c == 128 && (cm == 32 || cm == 64)) || (c == 256 && (cm == 64 || cm == 128)); }

// relayout: 0 = wt_scratch already holds the tap-major copy of w2 (the plan executor, when nothing has changed since the run that
// wrote it: LHN_RUN_TABLES_CURRENT), 1 = write it first.  The exported entry point always writes it.
int lhn_bottleneck_fwd_impl(const lhn_view* x, int Cm, const float* w1, const float* b1, const float* t1, const float* w2, const float* t2,
                            const float* w3, const float* b3, const float* t3, float out_slope, const lhn_view* y, float* wt_scratch,
                            int relayout, void* stream) {
  LHN_CHECK_ARG(lhn_view_ok(x) && lhn_view_ok(y) && lhn_no_pend(x) && lhn_no_pend(y) && w1 && w2 && w3, "lhn_bottleneck_fwd: bad view / null pointer");
  LHN_CHECK_ARG(y->N == x->N && y->H == x->H && y->W == x->W, "lhn_bottleneck_fwd: same-size output");
  LHN_CHECK_ARG(y->C == x->C && bottleneck_supported(x->C, Cm),
                "lhn_bottleneck_fwd: unsupported shape: built for 128 -> 32 / 64 -> 128 and 256 -> 64 / 128 -> 256 channels (got %d -> %d -> %d, "
                "map %d x %d)", x->C, Cm, y->C, x->H, x->W);
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
  if (x->C == 128) rc = Cm == 64 ? launch_bottleneck_w2<128, 64>(x, w1, b1, t1, w2, t2, w3, b3, t3, out_slope, y, wt_scratch, s)
                                 : launch_bottleneck_w2<128, 32>(x, w1, b1, t1, w2, t2, w3, b3, t3, out_slope, y, wt_scratch, s);
  else rc = Cm == 64 ? launch_bottleneck_w2<256, 64>(x, w1, b1, t1, w2, t2, w3, b3, t3, out_slope, y, wt_scratch, s)
                     : launch_bottleneck_w2<256, 128>(x, w1, b1, t1, w2, t2, w3, b3, t3, out_slope, y, wt_scratch, s);
  if (rc) return rc;
  LHN_CHECK_LAUNCH("lhn_bottleneck_fwd");
  return 0;
}

extern "C" int lhn_bottleneck_fwd(const lhn_view* x, int Cm, const float* w1, const float* b1, const float* t1, const float* w2,
                                  const float* t2, const float* w3, const float* b3, const float* t3, float out_slope, const lhn_view* y,
                                  float* wt_scratch, void* stream) {
  return lhn_bottleneck_fwd_impl(x, Cm, w1, b1, t1, w2, t2, w3, b3, t3, out_slope, y, wt_scratch, 1, stream);
}
