// Inference only: dense 3x3 convolution (pad 1, stride 1) on the bf16 MFMA with a three-term split ("bf16x3"), NHWC
// (liteHandNet.py:31,45 BottleNeck / BasicBlock 3x3, hourglassnet.py:33 Residual.conv2 -- the launches k_kxk<.., 0, 9> serves at fp32 rate).
//     v = hi(v) + lo(v) + O(2^-16 |v|),   hi(v) = bf16(v),  lo(v) = bf16(v - float(hi(v)))    (both round-to-nearest-even)
//     Y[p][co] = sum_tap sum_ci  lo(w) hi(v) + hi(w) lo(v) + hi(w) hi(v)                       (lo * lo, ~2^-16 relative, is dropped)
// on v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  Operand roles as in k_bottleneck.hip: A = weights (row = feature), B = pixels
// (column = pixel); lane l (r = l & 31, h = l >> 5) holds A[feature r][k = 8h .. 8h+7] and B[k = 8h .. 8h+7][pixel r], one 16-byte
// fragment each; D column = lane & 31 (pixel), D row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5) (feature): a lane ends up with
// groups of four consecutive features of one pixel -> float4 stores.
#include "lhn_common.h"

typedef __bf16 bf8v __attribute__((ext_vector_type(8)));
typedef unsigned short us4 __attribute__((ext_vector_type(4)));

// fp32 -> bf16 bits, round-to-nearest-even on the integer image (what torch's .to(torch.bfloat16) does); NaN -> quiet NaN
__host__ __device__ __forceinline__ unsigned lhn_bf16_rne(float v) {
  unsigned u;
  memcpy(&u, &v, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
__host__ __device__ __forceinline__ float lhn_bf16_f32(unsigned b) {
  const unsigned u = b << 16;
  float v;
  memcpy(&v, &u, 4);
  return v;
}
// v -> (hi, lo) bf16 bits; v - float(hi) is exact in fp32
__host__ __device__ __forceinline__ void lhn_bf16_split(float v, unsigned& hi, unsigned& lo) {
  hi = lhn_bf16_rne(v);
  lo = lhn_bf16_rne(v - lhn_bf16_f32(hi));
}

// OIHW fp32 weights -> ws[2][9][Cout][Cin] bf16: the hi image, then the lo image, tap-major (a lane's A fragment -- 8 consecutive
// input channels of one feature and tap -- is one 16-byte load).  9 * Cout * Cin * 4 bytes: the size of a KXK record's fp32 scratch.
__global__ void __launch_bounds__(256) k_w_split_tapmajor(const float* __restrict__ w, unsigned short* __restrict__ ws, int Cout, int Cin) {
  const int total = 9 * Cout * Cin;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int k = i % Cin, r = (i / Cin) % Cout, tap = i / (Cin * Cout);
    unsigned hi, lo;
    lhn_bf16_split(w[((size_t)r * Cin + k) * 9 + tap], hi, lo);
    ws[i] = (unsigned short)hi;
    ws[total + i] = (unsigned short)lo;
  }
}

// A workgroup (4 waves) computes ONE 8 x 16 output tile of one image:
//   load   the 10 x 18 halo of value(x) (table, slope and gate applied in fp32 with the helpers k_kxk uses; addresses clamped into the
//          map, pixels OUTSIDE the map are zero: the convolution pads the value) and split it -> his / los [180][CIN + 8] bf16.  The
//          row pitch 2 * CIN + 16 bytes is an odd number of 16-byte slots, so 16 consecutive halo pixels at one channel offset fill
//          the 16 slots of a 256-byte bank row.
//   taps   nine shifted GEMMs out of LDS (no re-read of x).  An MFMA pixel tile is 2 rows x 16 columns of the output tile; lane r
//          takes column r & 15 of row (0x96 >> (r >> 2)) & 1, which puts the 16 columns of ONE row on each 16-lane group of a
//          16-byte LDS read ({0-3, 12-15, 20-27} / {4-11, 16-19, 28-31}): conflict-free for every tap.
//          wave = (feature tile ft = wave % NF, pixel-tile group wave / NF) with NF = COUT / 32 accumulators each, so every feature
//          tile's weights are read from L2 by 4 / NF waves only; the A fragments of a tap (hi and lo, CIN / 16 K-steps) are loaded one
//          tap ahead into registers.
//   K-step three MFMAs into ONE accumulator, always in the order  lo(w) hi(v),  hi(w) lo(v),  hi(w) hi(v)  -- the small terms first,
//          so that they are added to each other before they meet the large one.
// Taps in the order 0 .. 8, K-steps ascending: the summation order of an output element is fixed.  No statistics, no atomics:
// repeated runs give identical bits in every mode.  A pixel is one column of every MFMA, so tile pixels outside the map compute on
// zeros / neighbours and are never stored.
template <int CIN, int COUT>
__global__ void __launch_bounds__(256) k_kxk_fwd_bf16x3(lhn_view x, const unsigned short* __restrict__ ws, lhn_view y, int tiles_x, int tiles_y) {
  constexpr int TH = 8, TW = 16, HW_ = TW + 2, HP = (TH + 2) * HW_;      // 180 halo pixels
  constexpr int LDP = CIN + 8;                                             // row pitch in bf16 elements
  constexpr int NF = COUT / 32, KS = CIN / 16;
  constexpr int C4 = CIN / 4, PL = 256 / C4, NLD = (HP + PL - 1) / PL, CH = 8;
  extern __shared__ __attribute__((aligned(16))) unsigned short smem_h[];
  unsigned short* his = smem_h;                 // [180][LDP]
  unsigned short* los = smem_h + HP * LDP;      // [180][LDP]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, lh = lane >> 5;
  const int H = x.H, W = x.W;
  const int tile = blockIdx.x;
  const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, n = tile / (tiles_x * tiles_y);
  const int ty0 = ty * TH, tx0 = tx * TW;

  // ---- weights of tap 0 first: their latency hides behind the halo load
  const int ft = wave % NF, pg = wave / NF;
  const size_t wimg = (size_t)9 * COUT * CIN;
  const unsigned short* wrow = ws + (size_t)(ft * 32 + l31) * CIN + 8 * lh;
  auto load_w = [&](int tap, bf8v (&dh)[KS], bf8v (&dl)[KS]) __attribute__((always_inline)) {
    const unsigned short* p = wrow + (size_t)tap * COUT * CIN;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      dh[ks] = *reinterpret_cast<const bf8v*>(p + ks * 16);
      dl[ks] = *reinterpret_cast<const bf8v*>(p + wimg + ks * 16);
    }
  };
  bf8v wah[KS], wal[KS];
  load_w(0, wah, wal);

  // ---- load and split the halo tile: thread = (channel group c4, pixel lane pl)
  {
    const int c4 = tid % C4, pl = tid / C4;
    const int cabs = x.coff + 4 * c4;
    const Xf4 xf = lhn_load_xf(x, cabs);
    const float* xn = x.data + (int64_t)n * H * W * x.cstride;
    const f4 gate = x.gate ? *reinterpret_cast<const f4*>(x.gate + (int64_t)n * x.cstride + cabs) : (f4){1.f, 1.f, 1.f, 1.f};
#pragma unroll 1
    for (int p0 = 0; p0 < NLD; p0 += CH) {
      f4 pre[CH];
#pragma unroll
      for (int p = 0; p < CH; ++p) {
        const int hp = min(pl + PL * (p0 + p), HP - 1), hy = hp / HW_, hx = hp - hy * HW_;
        const int iy = min(max(ty0 - 1 + hy, 0), H - 1), ix = min(max(tx0 - 1 + hx, 0), W - 1);
        pre[p] = *reinterpret_cast<const f4*>(xn + ((int64_t)iy * W + ix) * x.cstride + cabs);
      }
#pragma unroll
      for (int p = 0; p < CH; ++p) {
        const int hp = pl + PL * (p0 + p), hy = hp / HW_, hx = hp - hy * HW_;
        const int iy = ty0 - 1 + hy, ix = tx0 - 1 + hx;
        const bool inside = iy >= 0 && iy < H && ix >= 0 && ix < W;
        const f4 v = lhn_apply_xf(pre[p], xf) * gate;
        const float vv[4] = {v.x, v.y, v.z, v.w};
        us4 h4, l4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          unsigned hi, lo;
          lhn_bf16_split(vv[j], hi, lo);
          h4[j] = inside ? (unsigned short)hi : (unsigned short)0;
          l4[j] = inside ? (unsigned short)lo : (unsigned short)0;
        }
        if (hp < HP) {
          *reinterpret_cast<us4*>(his + hp * LDP + 4 * c4) = h4;
          *reinterpret_cast<us4*>(los + hp * LDP + 4 * c4) = l4;
        }
      }
    }
  }
  __syncthreads();

  // ---- nine shifted GEMMs
  const int prow = (0x96 >> (l31 >> 2)) & 1, pcol = l31 & 15;
  int hbase[NF];      // halo pixel of this lane's output pixel in pixel tile j of the wave, tap (0, 0)
#pragma unroll
  for (int j = 0; j < NF; ++j) hbase[j] = (2 * (pg * NF + j) + prow) * HW_ + pcol;
  f16v acc[NF];
#pragma unroll
  for (int j = 0; j < NF; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
#pragma unroll 1
  for (int tap = 0; tap < 9; ++tap) {
    bf8v wnh[KS], wnl[KS];
    load_w(min(tap + 1, 8), wnh, wnl);
    const int dy = tap / 3, dx = tap - dy * 3, shift = (dy * HW_ + dx) * LDP + 8 * lh;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        const int o = hbase[j] * LDP + shift + ks * 16;
        const bf8v bh = *reinterpret_cast<const bf8v*>(his + o);
        const bf8v bl = *reinterpret_cast<const bf8v*>(los + o);
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wal[ks], bh, acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wah[ks], bl, acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wah[ks], bh, acc[j], 0, 0, 0);
      }
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      wah[ks] = wnh[ks];
      wal[ks] = wnl[ks];
    }
  }

  // ---- raw store: 16 features of one pixel per lane and accumulator, as four float4
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    const int oy = ty0 + 2 * (pg * NF + j) + prow, ox = tx0 + pcol;
    if (oy < H && ox < W) {
      float* yp = y.data + (((int64_t)n * H + oy) * W + ox) * y.cstride + y.coff + ft * 32 + 4 * lh;
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<f4*>(yp + 8 * g) = (f4){acc[j][4 * g + 0], acc[j][4 * g + 1], acc[j][4 * g + 2], acc[j][4 * g + 3]};
    }
  }
}

template <int CIN, int COUT>
static int launch_kxk_bf16x3(const lhn_view* x, const unsigned short* ws, const lhn_view* y, hipStream_t s) {
  const size_t lds = (size_t)2 * 180 * (CIN + 8) * sizeof(unsigned short);
  static LhnKernelCfg cfg;
  if (!lhn_kernel_cfg(cfg, &k_kxk_fwd_bf16x3<CIN, COUT>, lds, 8, nullptr)) {
    lhn_set_error("lhn_conv_kxk_fwd_bf16x3: cannot reserve %zu B of LDS", lds);
    return 2;
  }
  // work item = workgroup = one 8 x 16 output tile of one image (97,920 / 51,840 / 28,800 B of LDS for 128 / 64 / 32 input channels:
  // 1 / 3 / 5 workgroups resident on a CU); a larger grid runs in rounds
  const int tiles_x = (x->W + 15) / 16, tiles_y = (x->H + 7) / 8;
  hipLaunchKernelGGL((k_kxk_fwd_bf16x3<CIN, COUT>), dim3((unsigned)((int64_t)x->N * tiles_x * tiles_y)), dim3(256), lds, s, *x, ws, *y, tiles_x,
                     tiles_y);
  return 0;
}

// (litehandnet_amd/plan.py: BF16X3_CHANNELS mirrors this rule; bf16x3_eligible, what the plan pass marks, is a subset of what this entry takes)
static bool kxk_bf16x3_channels(int c) { return c == 32 || c == 64 || c == 128; }

extern "C" int lhn_conv_kxk_fwd_bf16x3(const lhn_view* x, const float* w, const lhn_view* y, void* wsplit, int relay, void* stream) {
  LHN_CHECK_ARG(lhn_view_ok(x) && lhn_view_ok(y) && w && lhn_no_pend(x) && lhn_no_pend(y), "lhn_conv_kxk_fwd_bf16x3: bad view / null pointer");
  LHN_CHECK_ARG(y->N == x->N && y->H == x->H && y->W == x->W,
                "lhn_conv_kxk_fwd_bf16x3: unsupported shape: stride 1 only (a %d x %d map gives %d x %d)", x->H, x->W, y->H, y->W);
  LHN_CHECK_ARG(kxk_bf16x3_channels(x->C) && kxk_bf16x3_channels(y->C),
                "lhn_conv_kxk_fwd_bf16x3: unsupported shape: built for 32 / 64 / 128 channels in and out (got %d -> %d)", x->C, y->C);
  LHN_CHECK_ARG(wsplit, "lhn_conv_kxk_fwd_bf16x3: the split-weight scratch (9 * Cout * Cin * 4 bytes) is required");
  LHN_CHECK_ARG(!(x->data == y->data && x->coff < y->coff + y->C && y->coff < x->coff + x->C),
                "lhn_conv_kxk_fwd_bf16x3: unsupported shape: y overlaps x (a pixel's neighbours are read after it is written)");
  LHN_CHECK_ARG((int64_t)x->N * ((x->W + 15) / 16) * ((x->H + 7) / 8) <= 0x7fffffff, "lhn_conv_kxk_fwd_bf16x3: too many tiles");
  // every instance exists (3 x 3 channel pairs): nothing below can refuse after the first launch
  hipStream_t s = (hipStream_t)stream;
  unsigned short* ws = static_cast<unsigned short*>(wsplit);
  if (relay) {
    const int total = 9 * y->C * x->C;
    hipLaunchKernelGGL(k_w_split_tapmajor, dim3((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024), dim3(256), 0, s, w, ws, y->C, x->C);
  }
  int rc = -1;
#define KB(CI, CO) if (x->C == CI && y->C == CO) rc = launch_kxk_bf16x3<CI, CO>(x, ws, y, s);
  KB(32, 32) KB(32, 64) KB(32, 128) KB(64, 32) KB(64, 64) KB(64, 128) KB(128, 32) KB(128, 64) KB(128, 128)
#undef KB
  if (rc) return rc < 0 ? 1 : rc;
  LHN_CHECK_LAUNCH("lhn_conv_kxk_fwd_bf16x3");
  return 0;
}
