// Inference only: the stem after its first convolution (liteHandNet.py:169-193, models/pose_hg_ms_att.py:196-228) -- depthwise K x K,
// 1x1 (m -> m), dense 3x3 stride 2 (m -> m), max pool 2 x 2 (ceil), concatenation, 1x1 (2m -> C) -- in ONE launch (lhn_stem_tail_fwd).
// Outside training every pending transform is known before the launch, so t, u, v and the concatenation live in LDS only: x is read
// once (plus the halo) and y is written once.  The three dense stages run on v_mfma_f32_32x32x2_f32 with the operand maps of
// k_bottleneck.hip: A = 32 features x 2 k (lane & 31 = feature, lane >> 5 = k), B = 2 k x 32 pixels, D column = lane & 31 (pixel),
// D row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) (feature).
#include "lhn_common.h"

// A workgroup (4 waves) computes ONE tile of y of one image, 4 rows x 8 columns.  v at (oy, ox) reads u at rows 2 oy - 1 .. 2 oy + 1,
// so the tile needs t and u over 9 x 17 pixels (origin 2 * tile origin - 1) and value(x) over (8 + K) x (16 + K):
//   load     value(x) of the halo (table and gate applied, 0 outside the map) -> xs[(8 + K)(16 + K)][36]; K == 0: straight into ts.
//            The depthwise weights go to wdw[K * K][32], tap-major
//   stage T  t = actT(dwKxK(xs) + bT): thread = (4 channels, row, strip of 6 columns), a (6 + K - 1)-wide register window per
//            kernel row, 9.5 LDS reads per output instead of 49 -> ts[153][36]
//   stage U  u = actU(w1 . ts + b1) for the 153 pixels (5 pixel tiles of 32 over the 4 waves, rows >= 153 read row 152 and are
//            dropped), w1 in registers; a pixel OUTSIDE the map stores 0 -- the 3x3 pads u, not t -> us[153][36] (over xs)
//   pool     p = max of the 2 x 2 window of ts, rows and columns clamped into the map (ceil_mode clips the window; ts already
//            holds actT(..), so the table is applied before the max) -> cat[32][68], channels 32..63
//   stage V  v = actV(conv3x3 stride 2 (us) + b2): one pixel tile, the four waves take the tap groups 0..2 | 3,4 | 5,6 | 7,8, the
//            A operand (w2 of one tap) streamed from L2 one tap ahead; the groups meet through LDS (over ts) and are added in the
//            order 0, 1, 2, 3 -> cat channels 0..31
//   stage Y  y = w3 . cat + b3: wave = feature tile of 32, stored raw.
// A pixel is one column of every MFMA, so tile pixels outside the map compute on finite values and are never stored.
// TM: w2 is the tap-major copy [9][32][32] (16-byte loads); else the OIHW tensor itself (4-byte loads, 36-byte stride): the same
// products in the same order.  No statistics, no atomics, fixed summation order: repeated runs give identical bits.
// The phases are serial and every global load is exposed inside its workgroup, so the latency is hidden by OTHER workgroups of the
// CU: an 8 x 8 tile (8 waves, 125 KB of LDS, one workgroup per CU) ran the K = 0 launch in 217 us at batch 64, 128 x 128; STEM_TH
// = 4 keeps 52,768 B (K = 0), 53,280 B (K = 3) or 77,984 B (K = 7), i.e. three / three / two workgroups per CU.
#define STEM_M 32
#define STEM_C 128
#define STEM_TH 4                                   /* rows of y per workgroup (8 columns) */
#define STEM_TW 17
#define STEM_LDT (STEM_M + 4)
#define STEM_LDC (2 * STEM_M + 4)
// LDS floats of an instance: ts | max(xs + wdw, us + cat); the tap groups' partial accumulators (red) lie over ts, dead by then
template <int K, int TH>
struct StemLds {
  static constexpr int TR = 2 * TH + 1, NT = TR * STEM_TW, P = TH * 8, NW = P / 8;
  static constexpr int XH = K ? TR + K - 1 : TR, XW = K ? 16 + K : STEM_TW;
  static constexpr int XS = K ? XH * XW * STEM_LDT : 0, WDW = K * K * STEM_M;
  static constexpr int US = NT * STEM_LDT, CAT = P * STEM_LDC, RED = (P / 32) * 3 * 16 * 64;
  static constexpr int B = XS + WDW > US + CAT ? XS + WDW : US + CAT;
  static constexpr int FLOATS = US + B;
  static_assert(RED <= US, "red fits over ts");
};

template <int K, bool TM, int TH>
__global__ void __launch_bounds__(TH * 64, 2)
k_stem_tail_fwd(lhn_view x, const float* __restrict__ w_dw, const float* __restrict__ bT, const float* __restrict__ tT,
                const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ tU, const float* __restrict__ w2,
                const float* __restrict__ b2, const float* __restrict__ tV, int tv_stride, const float* __restrict__ w3,
                const float* __restrict__ b3, lhn_view y, int tiles_x, int tiles_y) {
  using L = StemLds<K, TH>;
  constexpr int M = STEM_M, TW = STEM_TW, LDT = STEM_LDT, LDC = STEM_LDC;
  constexpr int TR = L::TR, NT = L::NT, NW = L::NW, NTHR = 64 * NW, NPT = L::P / 32;      // t rows, t pixels, waves, threads, pixel tiles of y
  constexpr int XH = L::XH, XW = L::XW;    // the value(x) halo
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* ts = smem;                        // [NT][LDT]      t
  float* xs = smem + NT * LDT;             // [XH * XW][LDT] value(x) of the halo (K > 0)
  float* wdw = xs + L::XS;                 // [K * K][32]    depthwise weights, tap-major
  float* us = xs;                          // [NT][LDT]      u, zero outside the map (over xs)
  float* cat = xs + L::US;                 // [P][LDC]       v | p
  float* red = smem;                       // [NPT][3][16][64] partial accumulators of tap groups 1..3 (over ts, dead after the pool)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, lh = lane >> 5;
  const int H = x.H, W = x.W, OH = y.H, OW = y.W;
  const f4 zero = (f4){0.f, 0.f, 0.f, 0.f};
  const int tile = blockIdx.x;
  const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, n = tile / (tiles_x * tiles_y);
  const int oy0 = ty * TH, ox0 = tx * 8;
  const int ty_org = 2 * oy0 - 1, tx_org = 2 * ox0 - 1;      // map coordinates of ts[0]
  const int c4 = tid & 7;                                    // loader / stage T / pool: 4 channels per thread

  // ---- load the halo of value(x): thread = (channel group c4, pixel lane of 64)
  {
    constexpr int PLN = NTHR / 8, NPX = XH * XW, NLD = (NPX + PLN - 1) / PLN;
    float* dst = K ? xs : ts;
    const float* xn = x.data + (int64_t)n * H * W * x.cstride;
    const int cabs = x.coff + 4 * c4, pl = tid >> 3;
    const int org_y = ty_org - K / 2, org_x = tx_org - K / 2;
    const Xf4 xf = lhn_load_xf(x, cabs);
    f4 pre[NLD];
#pragma unroll
    for (int p = 0; p < NLD; ++p) {
      const int px = min(pl + PLN * p, NPX - 1), hy = px / XW, hx = px - hy * XW;
      const int iy = min(max(org_y + hy, 0), H - 1), ix = min(max(org_x + hx, 0), W - 1);
      pre[p] = *reinterpret_cast<const f4*>(xn + ((int64_t)iy * W + ix) * x.cstride + cabs);
    }
    const f4 gate = x.gate ? *reinterpret_cast<const f4*>(x.gate + (int64_t)n * x.cstride + cabs) : (f4){1.f, 1.f, 1.f, 1.f};
    if (K) {
      for (int i = tid; i < K * K * M; i += NTHR) wdw[i] = w_dw[(i & (M - 1)) * (K * K) + (i >> 5)];
    }
#pragma unroll
    for (int p = 0; p < NLD; ++p) {
      const int px = pl + PLN * p, hy = px / XW, hx = px - hy * XW;
      const int iy = org_y + hy, ix = org_x + hx;
      const bool inside = iy >= 0 && iy < H && ix >= 0 && ix < W;
      if (px < NPX) *reinterpret_cast<f4*>(dst + px * LDT + 4 * c4) = inside ? lhn_apply_xf(pre[p], xf) * gate : zero;
    }
  }
  __syncthreads();      // xs (K == 0: ts) and wdw are in

  // ---- stage T: the depthwise convolution, 6 output columns per thread
  if (K) {
    constexpr int S = 6, KK = K ? K : 1;
    if (tid < 8 * TR * 3) {
      const int rest = tid >> 3, row = rest / 3, x0 = (rest - row * 3) * S;
      f4 acc[S];
#pragma unroll
      for (int s = 0; s < S; ++s) acc[s] = zero;
#pragma unroll 1      // (unrolled, the compiler hoists all K * K weight loads and K rows of x: 318 spilled VGPRs at K = 7)
      for (int ky = 0; ky < KK; ++ky) {
        f4 xin[S + KK - 1];
#pragma unroll
        for (int j = 0; j < S + KK - 1; ++j)
          xin[j] = *reinterpret_cast<const f4*>(xs + ((row + ky) * XW + min(x0 + j, XW - 1)) * LDT + 4 * c4);
#pragma unroll
        for (int kx = 0; kx < KK; ++kx) {
          const f4 wv = *reinterpret_cast<const f4*>(wdw + (ky * KK + kx) * M + 4 * c4);
#pragma unroll
          for (int s = 0; s < S; ++s) acc[s] += wv * xin[s + kx];
        }
      }
      const f4 bv = bT ? *reinterpret_cast<const f4*>(bT + 4 * c4) : zero;
      const Xf4 tf = lhn_load_xf_t(tT, M, 4 * c4);
#pragma unroll
      for (int s = 0; s < S; ++s)
        if (x0 + s < TW) *reinterpret_cast<f4*>(ts + (row * TW + x0 + s) * LDT + 4 * c4) = lhn_apply_xf(acc[s] + bv, tf);
    }
    __syncthreads();    // ts is in; nobody reads xs any more
  }

  // ---- stage U: the first 1x1 over the 289 pixels; w1reg[kc * 4 + j] = w1[l31][8 * kc + 4 * lh + j]
  {
    float w1reg[M / 2];
#pragma unroll
    for (int kc = 0; kc < M / 8; ++kc) {
      const f4 v = *reinterpret_cast<const f4*>(w1 + l31 * M + kc * 8 + 4 * lh);
      w1reg[kc * 4 + 0] = v.x; w1reg[kc * 4 + 1] = v.y; w1reg[kc * 4 + 2] = v.z; w1reg[kc * 4 + 3] = v.w;
    }
#pragma unroll 1
    for (int pt = wave; pt < (NT + 31) / 32; pt += NW) {
      const int hp = pt * 32 + l31;
      const float* brow = ts + min(hp, NT - 1) * LDT + 4 * lh;
      f16v acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
      for (int kc = 0; kc < M / 8; ++kc) {
        const f4 b = *reinterpret_cast<const f4*>(brow + kc * 8);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w1reg[kc * 4 + 0], b.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w1reg[kc * 4 + 1], b.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w1reg[kc * 4 + 2], b.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w1reg[kc * 4 + 3], b.w, acc, 0, 0, 0);
      }
      const int hy = hp / TW, hx = hp - hy * TW;
      const int iy = ty_org + hy, ix = tx_org + hx;
      const bool inside = iy >= 0 && iy < H && ix >= 0 && ix < W;
      if (hp < NT) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int f = 8 * g + 4 * lh;
          f4 v = (f4){acc[4 * g + 0], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
          if (b1) v += *reinterpret_cast<const f4*>(b1 + f);
          v = lhn_apply_xf(v, lhn_load_xf_t(tU, M, f));
          *reinterpret_cast<f4*>(us + hp * LDT + f) = inside ? v : zero;
        }
      }
    }
  }

  // ---- pool: thread = (output pixel, channel group); the window is clamped into the map
  {
    const int p = tid >> 3, r0 = 1 + 2 * (p >> 3), q0 = 1 + 2 * (p & 7);
    const int ra = min(r0, H - 1 - ty_org), rb = min(r0 + 1, H - 1 - ty_org);
    const int qa = min(q0, W - 1 - tx_org), qb = min(q0 + 1, W - 1 - tx_org);
    const f4 a = *reinterpret_cast<const f4*>(ts + (ra * TW + qa) * LDT + 4 * c4);
    const f4 b = *reinterpret_cast<const f4*>(ts + (ra * TW + qb) * LDT + 4 * c4);
    const f4 c = *reinterpret_cast<const f4*>(ts + (rb * TW + qa) * LDT + 4 * c4);
    const f4 d = *reinterpret_cast<const f4*>(ts + (rb * TW + qb) * LDT + 4 * c4);
    *reinterpret_cast<f4*>(cat + p * LDC + M + 4 * c4) =
        (f4){fmaxf(fmaxf(a.x, b.x), fmaxf(c.x, d.x)), fmaxf(fmaxf(a.y, b.y), fmaxf(c.y, d.y)), fmaxf(fmaxf(a.z, b.z), fmaxf(c.z, d.z)),
             fmaxf(fmaxf(a.w, b.w), fmaxf(c.w, d.w))};
  }
  __syncthreads();      // us is in

  // ---- stage V: nine shifted stride-2 GEMMs, weights one tap ahead
  {
    const int pt = wave % NPT, tg = wave / NPT;
    const int tap_b = tg ? 1 + 2 * tg : 0, tap_e = tg ? 3 + 2 * tg : 3;
    const int p = pt * 32 + l31, base = 2 * (p >> 3) * TW + 2 * (p & 7);
    auto load_w2 = [&](int tap, float (&dst)[M / 2]) __attribute__((always_inline)) {
#pragma unroll
      for (int kc = 0; kc < M / 8; ++kc) {
        if (TM) {
          const f4 v = *reinterpret_cast<const f4*>(w2 + ((size_t)tap * M + l31) * M + kc * 8 + 4 * lh);
          dst[kc * 4 + 0] = v.x; dst[kc * 4 + 1] = v.y; dst[kc * 4 + 2] = v.z; dst[kc * 4 + 3] = v.w;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) dst[kc * 4 + j] = w2[((size_t)l31 * M + kc * 8 + 4 * lh + j) * 9 + tap];
        }
      }
    };
    f16v acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float wa[M / 2];
    load_w2(tap_b, wa);
#pragma unroll 1
    for (int tap = tap_b; tap < tap_e; ++tap) {
      float wn[M / 2];
      load_w2(min(tap + 1, tap_e - 1), wn);
      const int dy = tap / 3, dx = tap - dy * 3;
      const float* brow = us + (base + dy * TW + dx) * LDT + 4 * lh;
#pragma unroll
      for (int kc = 0; kc < M / 8; ++kc) {
        const f4 b = *reinterpret_cast<const f4*>(brow + kc * 8);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[kc * 4 + 0], b.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[kc * 4 + 1], b.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[kc * 4 + 2], b.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[kc * 4 + 3], b.w, acc, 0, 0, 0);
      }
#pragma unroll
      for (int k = 0; k < M / 2; ++k) wa[k] = wn[k];
    }
    if (tg) {
#pragma unroll
      for (int r = 0; r < 16; ++r) red[((pt * 3 + tg - 1) * 16 + r) * 64 + lane] = acc[r];
    }
    __syncthreads();
    if (tg == 0) {      // taps 3,4 then 5,6 then 7,8 join taps 0..2 (always in this order)
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] += red[((pt * 3 + k) * 16 + r) * 64 + lane];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int f = 8 * g + 4 * lh;
        f4 v = (f4){acc[4 * g + 0], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
        if (b2) v += *reinterpret_cast<const f4*>(b2 + f);
        *reinterpret_cast<f4*>(cat + p * LDC + f) = lhn_apply_xf(v, lhn_load_xf_t(tV, tv_stride, f));
      }
    }
  }
  __syncthreads();      // cat is in

  // ---- stage Y: the last 1x1; w3reg[kc * 4 + j] = w3[ft * 32 + l31][8 * kc + 4 * lh + j]
  {
    const int ft = wave & 3, pt = wave >> 2;      // NW = 4 * NPT waves
    float w3reg[M];
#pragma unroll
    for (int kc = 0; kc < 2 * M / 8; ++kc) {
      const f4 v = *reinterpret_cast<const f4*>(w3 + (ft * 32 + l31) * 2 * M + kc * 8 + 4 * lh);
      w3reg[kc * 4 + 0] = v.x; w3reg[kc * 4 + 1] = v.y; w3reg[kc * 4 + 2] = v.z; w3reg[kc * 4 + 3] = v.w;
    }
    const int p = pt * 32 + l31;
    const float* brow = cat + p * LDC + 4 * lh;
    f16v acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int kc = 0; kc < 2 * M / 8; ++kc) {
      const f4 b = *reinterpret_cast<const f4*>(brow + kc * 8);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w3reg[kc * 4 + 0], b.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w3reg[kc * 4 + 1], b.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w3reg[kc * 4 + 2], b.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w3reg[kc * 4 + 3], b.w, acc, 0, 0, 0);
    }
    const int oy = oy0 + (p >> 3), ox = ox0 + (p & 7);
    if (oy < OH && ox < OW) {
      float* yp = y.data + (((int64_t)n * OH + oy) * OW + ox) * y.cstride + y.coff;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int f = ft * 32 + 8 * g + 4 * lh;
        f4 v = (f4){acc[4 * g + 0], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
        if (b3) v += *reinterpret_cast<const f4*>(b3 + f);
        *reinterpret_cast<f4*>(yp + f) = v;
      }
    }
  }
}

// w2 [32][32][3][3] -> wt [9][32][32] (tap, output feature, input feature)
__global__ void __launch_bounds__(256) k_stem_w2_tapmajor(const float* __restrict__ w, float* __restrict__ wt) {
  constexpr int M = STEM_M;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < 9 * M * M) {
    const int k = i % M, r = (i / M) % M, tap = i / (M * M);
    wt[i] = w[((size_t)r * M + k) * 9 + tap];
  }
}

template <int K, bool TM>
static int launch_stem_tail(const lhn_view* x, const float* w_dw, const float* bT, const float* tT, const float* w1, const float* b1,
                            const float* tU, const float* w2, const float* b2, const float* tV, int tv_stride, const float* w3,
                            const float* b3, const lhn_view* y, hipStream_t s) {
  constexpr int TH = STEM_TH;
  const size_t lds = (size_t)StemLds<K, TH>::FLOATS * sizeof(float);
  static LhnKernelCfg cfg;
  if (!lhn_kernel_cfg(cfg, &k_stem_tail_fwd<K, TM, TH>, lds, 4, nullptr)) {
    lhn_set_error("lhn_stem_tail_fwd: cannot reserve %zu B of LDS", lds);
    return 2;
  }
  // work item = workgroup (4 waves) = one 4 x 8 tile of y of one image; 52,768 B (K = 0), 53,280 B (K = 3) or 77,984 B (K = 7) of LDS
  // each, so three (K = 7: two) are resident on a CU at a time and a larger grid runs in several rounds
  const int tiles_x = (y->W + 7) / 8, tiles_y = (y->H + TH - 1) / TH;
  const int64_t ntiles = (int64_t)x->N * tiles_x * tiles_y;
  if (ntiles > 0x7fffffff) {
    lhn_set_error("lhn_stem_tail_fwd: too many tiles");
    return 1;
  }
  hipLaunchKernelGGL((k_stem_tail_fwd<K, TM, TH>), dim3((unsigned)ntiles), dim3(TH * 64), lds, s, *x, w_dw, bT, tT, w1, b1, tU, w2, b2, tV,
                     tv_stride, w3, b3, *y, tiles_x, tiles_y);
  return 0;
}

// (litehandnet_amd/plan.py: FUSE_STEM_CHANNELS / FUSE_STEM_K mirror this rule)
static bool stem_tail_supported(int m, int c, int K) { return m == STEM_M && c == STEM_C && (K == 0 || K == 3 || K == 7); }

// the slope row of `count` channels of a [3][stride] table starting at channel `first`: all inside [0, 1]?
static bool stem_slopes_ok(const float* tab, int stride, int first, int count) {
  if (!tab) return true;
  float h[STEM_M];
  if (hipMemcpy(h, tab + 2 * (size_t)stride + first, sizeof(float) * count, hipMemcpyDeviceToHost) != hipSuccess) return false;
  for (int k = 0; k < count; ++k)
    if (!(h[k] >= 0.f && h[k] <= 1.f)) return false;
  return true;
}

int lhn_stem_tail_fwd_impl(const lhn_view* x, int K, const float* w_dw, const float* bT, const float* tT, const float* w1, const float* b1,
                           const float* tU, const float* w2, const float* b2, const float* tV, int tv_stride, const float* w3, const float* b3,
                           const lhn_view* y, float* wt_scratch, int relayout, int check_slopes, void* stream) {
  LHN_CHECK_ARG(lhn_view_ok(x) && lhn_view_ok(y) && lhn_no_pend(x) && lhn_no_pend(y) && w1 && w2 && w3, "lhn_stem_tail_fwd: bad view / null pointer");
  LHN_CHECK_ARG(stem_tail_supported(x->C, y->C, K),
                "lhn_stem_tail_fwd: unsupported shape: built for 32 -> 128 channels and K in {0, 3, 7} (got %d -> %d, K = %d, map %d x %d)", x->C,
                y->C, K, x->H, x->W);
  LHN_CHECK_ARG(K == 0 || w_dw, "lhn_stem_tail_fwd: bad view / null pointer (depthwise weights)");
  LHN_CHECK_ARG(y->N == x->N && y->H == (x->H + 1) / 2 && y->W == (x->W + 1) / 2 && tv_stride >= STEM_M,
                "lhn_stem_tail_fwd: the output is N x ceil(H/2) x ceil(W/2)");
  LHN_CHECK_ARG(!(x->data == y->data && x->coff < y->coff + y->C && y->coff < x->coff + x->C),
                "lhn_stem_tail_fwd: unsupported shape: y overlaps x (a pixel's neighbours are read after it is written)");
  hipStream_t s = (hipStream_t)stream;
  if (check_slopes && (x->table || (K && tT) || tU || tV)) {
    LHN_CHECK_ARG(hipStreamSynchronize(s) == hipSuccess, "lhn_stem_tail_fwd: cannot wait for the stream to read the tables' slopes");
    LHN_CHECK_ARG(stem_slopes_ok(x->table, x->cstride, x->coff, STEM_M) && stem_slopes_ok(K ? tT : nullptr, STEM_M, 0, STEM_M) &&
                      stem_slopes_ok(tU, STEM_M, 0, STEM_M) && stem_slopes_ok(tV, tv_stride, 0, STEM_M),
                  "lhn_stem_tail_fwd: unsupported shape: every table slope is a leaky slope in [0, 1] (SiLU / relu-sigmoid are not built)");
  }
  if (wt_scratch && relayout) hipLaunchKernelGGL(k_stem_w2_tapmajor, dim3((9 * STEM_M * STEM_M + 255) / 256), dim3(256), 0, s, w2, wt_scratch);
  const float* w2k = wt_scratch ? wt_scratch : w2;
  int rc;
#define STEM_GO(KK)                                                                                                          \
  (wt_scratch ? launch_stem_tail<KK, true>(x, w_dw, bT, tT, w1, b1, tU, w2k, b2, tV, tv_stride, w3, b3, y, s)                \
              : launch_stem_tail<KK, false>(x, w_dw, bT, tT, w1, b1, tU, w2k, b2, tV, tv_stride, w3, b3, y, s))
  if (K == 7) rc = STEM_GO(7);
  else if (K == 3) rc = STEM_GO(3);
  else rc = STEM_GO(0);
#undef STEM_GO
  if (rc) return rc;
  LHN_CHECK_LAUNCH("lhn_stem_tail_fwd");
  return 0;
}

extern "C" int lhn_stem_tail_fwd(const lhn_view* x, int K, const float* w_dw, const float* bT, const float* tT, const float* w1, const float* b1,
                                 const float* tU, const float* w2, const float* b2, const float* tV, const float* w3, const float* b3,
                                 const lhn_view* y, float* wt_scratch, void* stream) {
  return lhn_stem_tail_fwd_impl(x, K, w_dw, bT, tT, w1, b1, tU, w2, b2, tV, STEM_M, w3, b3, y, wt_scratch, 1, 1, stream);
}
