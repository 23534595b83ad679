// Inference only: 1x1 convolution -> pending (scale, shift, slope) -> depthwise 3x3 in ONE launch (lhn_conv_pw_dw3_fwd).
// The right branch of RepBasicUnit (litehourglass.py:52-78) is RepConv 1x1 followed by RepConv depthwise 3x3; outside training
// the transform between them is known before the launch, so the intermediate tensor t lives in LDS only.
#include "lhn_common.h"

// A workgroup owns one image, one column strip and one band of output rows, and walks the band downwards.  A step takes 64
// pixels = RPS rows of TW columns (TW = 64, 32, 16, 8 for maps up to that wide; RPS = 64 / TW):
//   commit   the step's x values (table and gate applied) go from registers to LDS; the next step's global loads are issued
//   1x1      the four waves each run one 32-feature x 32-pixel MFMA tile (v_mfma_f32_32x32x2_f32; W1 stays in registers for
//            the whole launch, as in k_pw_fwd_wr), apply t_table and write t into a ring of RPS + 2 rows
//   taps     the nine taps of the RPS output rows that now have their lower neighbour, raw store into y
// t is ZERO outside the map (the depthwise convolution pads t, not x): pixels outside are selected to zero after the
// transform, whatever shift1 is.  Column slots 0 and TW + 1 of a ring row are the padding of a single-strip map and are
// never written.  Maps wider than 64 run strips of 64 computed / 62 stored columns; a band computes the t rows
// just above and below its output rows itself (two rows per band), nothing else is computed twice.  No statistics, no atomics: repeated runs give identical bits.
template <int TW>
__global__ void __launch_bounds__(256, 2)
k_pw_dw3_fwd(lhn_view x, const float* __restrict__ w1, const float* __restrict__ ttab, const float* __restrict__ w2, lhn_view y,
             int nstrips, int nbands, int band_rows) {
  constexpr int C = 64, LDA = C + 4, LDT = C + 4, RPS = 64 / TW, RING = RPS + 2, SLOTS = TW + 2, CG = TW / 4;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* xs = smem;                        // [64][LDA]   the step's input pixels
  float* ring = xs + 64 * LDA;             // [RING][SLOTS][LDT]
  float* tt = ring + RING * SLOTS * LDT;   // [3][C]      t_table
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, lh = lane >> 5;
  const int H = x.H, W = x.W;
  int bid = blockIdx.x;
  const int strip = bid % nstrips;
  bid /= nstrips;
  const int band = bid % nbands, n = bid / nbands;
  const int rb = band * band_rows, re = min(H, rb + band_rows);      // output rows of this band
  const int ts = rb - 1;                                             // first t row (row -1 is padding)
  const int c0 = nstrips == 1 ? 0 : strip * 62 - 1;                  // first computed column
  const int olo = nstrips == 1 ? 0 : 1, ohi = nstrips == 1 ? W : min(63, W - c0);      // stored columns, tile coordinates
  const int nsteps = (re - rb + 1) / RPS + 1;

  // ---- 1x1 operands: wave = (feature tile ft, pixel tile pt); wreg[kc*4 + j] = W1[ft*32 + l31][8*kc + 4*lh + j]
  const int ft = wave & 1, pt = wave >> 1;
  float wreg[C / 2];
#pragma unroll
  for (int kc = 0; kc < C / 8; ++kc) {
    const f4 v = *reinterpret_cast<const f4*>(w1 + (ft * 32 + l31) * C + kc * 8 + 4 * lh);
    wreg[kc * 4 + 0] = v.x; wreg[kc * 4 + 1] = v.y; wreg[kc * 4 + 2] = v.z; wreg[kc * 4 + 3] = v.w;
  }
  // ---- loader / tap geometry: thread = (channel group c4, pixel lane pl)
  const int c4 = tid & 15, pl = tid >> 4;
  const int cabs = x.coff + 4 * c4;
  const float* xn = x.data + (int64_t)n * H * W * x.cstride + cabs;
  float* yn = y.data + (int64_t)n * H * W * y.cstride + y.coff + 4 * c4;
  f4 pre[4];
  auto issue = [&](int step) __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int m = pl + 16 * p;
      const int row = min(max(ts + step * RPS + m / TW, 0), H - 1), col = min(max(c0 + m % TW, 0), W - 1);      // clamped: pixels
      pre[p] = *reinterpret_cast<const f4*>(xn + ((int64_t)row * W + col) * x.cstride);                      // outside become t = 0
    }
  };
  issue(0);
  const Xf4 xf = lhn_load_xf(x, cabs);
  const f4 gate = x.gate ? *reinterpret_cast<const f4*>(x.gate + (int64_t)n * x.cstride + cabs) : (f4){1.f, 1.f, 1.f, 1.f};
  f4 wk[9];      // depthwise taps of this thread's 4 channels
#pragma unroll
  for (int k = 0; k < 9; ++k) wk[k] = (f4){w2[(4 * c4 + 0) * 9 + k], w2[(4 * c4 + 1) * 9 + k], w2[(4 * c4 + 2) * 9 + k], w2[(4 * c4 + 3) * 9 + k]};
  if (tid < 3 * C) tt[tid] = ttab ? ttab[tid] : (tid < C || tid >= 2 * C ? 1.f : 0.f);
  for (int i = tid; i < RING * 2 * (LDT / 4); i += 256) {      // the two padding slots of every ring row
    const int r = i / (2 * (LDT / 4)), j = i % (2 * (LDT / 4));
    *reinterpret_cast<f4*>(ring + (r * SLOTS + (j >= LDT / 4 ? TW + 1 : 0)) * LDT + 4 * (j % (LDT / 4))) = (f4){0.f, 0.f, 0.f, 0.f};
  }
  const int orow = pl / CG, ocol0 = (pl % CG) * 4;      // taps: output row within the step, first of 4 output columns

  for (int step = 0; step < nsteps; ++step) {
#pragma unroll
    for (int p = 0; p < 4; ++p)
      *reinterpret_cast<f4*>(xs + (pl + 16 * p) * LDA + 4 * c4) = lhn_apply_xf(pre[p], xf) * gate;
    __syncthreads();      // xs complete; the taps of the previous step are done with the ring rows this step overwrites
    if (step + 1 < nsteps) issue(step + 1);
    {
      f16v acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      const float* brow = xs + (pt * 32 + l31) * LDA + 4 * lh;
#pragma unroll
      for (int kc = 0; kc < C / 8; ++kc) {
        const f4 b = *reinterpret_cast<const f4*>(brow + kc * 8);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wreg[kc * 4 + 0], b.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wreg[kc * 4 + 1], b.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wreg[kc * 4 + 2], b.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wreg[kc * 4 + 3], b.w, acc, 0, 0, 0);
      }
      // C/D layout: column = lane & 31 (pixel), row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) (feature)
      const int m = pt * 32 + l31, rr = m / TW, cc = m % TW;
      const int row = ts + step * RPS + rr, col = c0 + cc;
      const bool inside = row >= 0 && row < H && col >= 0 && col < W;
      float* trow = ring + (((step * RPS + rr) % RING) * SLOTS + cc + 1) * LDT + ft * 32 + 4 * lh;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int f = ft * 32 + 8 * g + 4 * lh;
        const f4 sc = *reinterpret_cast<const f4*>(tt + f), sh = *reinterpret_cast<const f4*>(tt + C + f),
                 sl = *reinterpret_cast<const f4*>(tt + 2 * C + f);
        f4 t;
        t.x = lhn_lrelu(acc[4 * g + 0] * sc.x + sh.x, sl.x);
        t.y = lhn_lrelu(acc[4 * g + 1] * sc.y + sh.y, sl.y);
        t.z = lhn_lrelu(acc[4 * g + 2] * sc.z + sh.z, sl.z);
        t.w = lhn_lrelu(acc[4 * g + 3] * sc.w + sh.w, sl.w);
        *reinterpret_cast<f4*>(trow + 8 * g) = inside ? t : (f4){0.f, 0.f, 0.f, 0.f};
      }
    }
    __syncthreads();      // t rows of this step are in the ring
    // output row o (relative to ts: orel) reads t rows orel - 1 .. orel + 1; rows before the band's first output are skipped
    const int orel = step * RPS - 1 + orow, o = ts + orel;
    if (o >= rb && o < re && ocol0 < ohi) {
      f4 out[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) out[j] = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const float* tr = ring + ((orel - 1 + d) % RING) * SLOTS * LDT + 4 * c4;
        f4 v[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) v[q] = *reinterpret_cast<const f4*>(tr + (ocol0 + q) * LDT);
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] += v[j] * wk[3 * d] + v[j + 1] * wk[3 * d + 1] + v[j + 2] * wk[3 * d + 2];
      }
      float* yo = yn + ((int64_t)o * W + c0) * y.cstride;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int cc = ocol0 + j;
        if (cc >= olo && cc < ohi) *reinterpret_cast<f4*>(yo + (int64_t)cc * y.cstride) = out[j];
      }
    }
  }
}

template <int TW>
static int launch_pw_dw3(const lhn_view* x, const float* w1, const float* ttab, const float* w2, const lhn_view* y, hipStream_t s) {
  constexpr int RPS = 64 / TW;
  const size_t lds = (size_t)(64 * 68 + (RPS + 2) * (TW + 2) * 68 + 3 * 64) * sizeof(float);
  static LhnKernelCfg cfg;
  int per_cu = 1;
  if (!lhn_kernel_cfg(cfg, &k_pw_dw3_fwd<TW>, lds, 2, &per_cu)) {
    lhn_set_error("lhn_conv_pw_dw3_fwd: cannot reserve %zu B of LDS", lds);
    return 2;
  }
  const int nstrips = x->W <= 64 ? 1 : (x->W + 61) / 62;
  // bands: enough workgroups for one resident round of the device, but at least 8 output rows (and one step) each -- every
  // band recomputes the t row above it
  const int64_t want = (int64_t)lhn_num_cus() * per_cu, cols = (int64_t)x->N * nstrips;
  const int min_rows = RPS > 8 ? RPS : 8;
  int nbands = (int)((want + cols - 1) / cols);
  if (nbands > (x->H + min_rows - 1) / min_rows) nbands = (x->H + min_rows - 1) / min_rows;
  if (nbands < 1) nbands = 1;
  int band_rows = (x->H + nbands - 1) / nbands;
  band_rows = (band_rows + RPS - 1) / RPS * RPS;
  nbands = (x->H + band_rows - 1) / band_rows;
  const int64_t grid = cols * nbands;
  if (grid > 0x7fffffff) {
    lhn_set_error("lhn_conv_pw_dw3_fwd: grid too large");
    return 1;
  }
  hipLaunchKernelGGL((k_pw_dw3_fwd<TW>), dim3((unsigned)grid), dim3(256), lds, s, *x, w1, ttab, w2, *y, nstrips, nbands, band_rows);
  return 0;
}

// (litehandnet_amd/plan.py: _fusable_pw_dw mirrors this rule)
static bool pw_dw3_supported(int cin, int cm) { return cin == 64 && cm == 64; }

extern "C" int lhn_conv_pw_dw3_fwd(const lhn_view* x, const float* w1, const float* t_table, const float* w2, const lhn_view* y,
                                   void* stream) {
  LHN_CHECK_ARG(lhn_view_ok(x) && lhn_view_ok(y) && lhn_no_pend(x) && lhn_no_pend(y) && w1 && w2, "lhn_conv_pw_dw3_fwd: bad view / null pointer");
  LHN_CHECK_ARG(y->N == x->N && y->H == x->H && y->W == x->W, "lhn_conv_pw_dw3_fwd: same-size output");
  LHN_CHECK_ARG(pw_dw3_supported(x->C, y->C),
                "lhn_conv_pw_dw3_fwd: unsupported shape: built for 64 -> 64 channels (got %d -> %d, map %d x %d)", x->C, y->C, x->H, x->W);
  LHN_CHECK_ARG(!(x->data == y->data && x->coff < y->coff + y->C && y->coff < x->coff + x->C),
                "lhn_conv_pw_dw3_fwd: y overlaps x (a pixel's neighbours are read after it is written)");
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if (x->W <= 8) rc = launch_pw_dw3<8>(x, w1, t_table, w2, y, s);
  else if (x->W <= 16) rc = launch_pw_dw3<16>(x, w1, t_table, w2, y, s);
  else if (x->W <= 32) rc = launch_pw_dw3<32>(x, w1, t_table, w2, y, s);
  else rc = launch_pw_dw3<64>(x, w1, t_table, w2, y, s);
  if (rc) return rc;
  LHN_CHECK_LAUNCH("lhn_conv_pw_dw3_fwd");
  return 0;
}
