// Inference only: depthwise 3x3 convolution -> pending (scale, shift, slope) -> 1x1 convolution in ONE launch (lhn_conv_dw3_pw_fwd).
// DWConv (liteHandNet.py:8-21) is RepConv depthwise 3x3 (dilation 1 or 2) followed by RepConv 1x1; outside training the transform
// between them is known before the launch, so the intermediate tensor t lives in LDS only.  k_pw_dw3_fwd (k_conv_pwdw.hip) with
// the stages swapped: the GEMM has no halo, so nothing is computed twice -- a band only re-reads 2 * DIL input rows.
#include "lhn_common.h"

// A workgroup owns one image, one column strip and one band of output rows, and walks the band downwards.  A step takes 64
// pixels = RPS rows of TW columns (TW = 64, 32, 16, 8 for maps up to that wide; RPS = 64 / TW):
//   commit   the step's RPS new x rows (table and gate applied, ZERO outside the map: the depthwise convolution pads the value of
//            x, not the raw tensor) go from registers into a ring of RPS + 2 * DIL rows; the next step's global loads are issued
//   taps     the nine taps of the RPS output rows whose lowest input row has just arrived, t_table applied, t into a [64][CIN] tile
//   1x1      32-feature x 32-pixel MFMA tiles (v_mfma_f32_32x32x2_f32; the 1x1's weights stay in registers for the whole launch,
//            as in k_pw_fwd_wr), bias added, raw store into y.  COUT = 64: one tile per wave; COUT = 32: waves 0 and 1 only.
// Ring slot j of a row is column c0 + j - DIL; slots [0, DIL) and [TW + DIL, TW + 2 * DIL) are the padding of a single-strip map and
// are never written after their zero fill.  Maps wider than 64 run strips of 64 loaded / 64 - 2 * DIL stored columns.  Output pixels
// outside the band or the strip are computed from whatever the ring holds and never stored: a pixel is one column of the MFMA, so
// nothing leaks between pixels.  No statistics, no atomics: repeated runs give identical bits.
template <int CIN, int COUT, int TW, int DIL>
__global__ void __launch_bounds__(256, 2)
k_dw3_pw_fwd(lhn_view x, const float* __restrict__ wd, const float* __restrict__ ttab, const float* __restrict__ wp,
             const float* __restrict__ bias, lhn_view y, int nstrips, int nbands, int band_rows) {
  constexpr int C4 = CIN / 4, PL = 256 / C4, PPT = 64 / PL, RPS = 64 / TW, RING = RPS + 2 * DIL, SLOTS = TW + 2 * DIL, LDT = CIN + 4,
                CG = TW / PPT, NV = PPT + 2 * DIL, NFT = COUT / 32;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* ring = smem;                         // [RING][SLOTS][CIN]   value(x), zero outside the map
  float* ts = ring + RING * SLOTS * CIN;      // [64][LDT]            the step's t pixels
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, lh = lane >> 5;
  const int H = x.H, W = x.W;
  int bid = blockIdx.x;
  const int strip = bid % nstrips;
  bid /= nstrips;
  const int band = bid % nbands, n = bid / nbands;
  const int rb = band * band_rows, re = min(H, rb + band_rows);      // output rows of this band
  const int xs0 = rb - DIL;                                          // first x row of the stream (may be padding)
  const int c0 = nstrips == 1 ? 0 : strip * (TW - 2 * DIL) - DIL;    // first loaded column
  const int olo = nstrips == 1 ? 0 : DIL, ohi = nstrips == 1 ? W : min(TW - DIL, W - c0);      // stored columns, tile coordinates
  const int nsteps = (re - rb + 2 * DIL + RPS - 1) / RPS;

  // ---- 1x1 operands: wave = (feature tile ft, pixel tile pt); wreg[kc*4 + j] = Wp[ft*32 + l31][8*kc + 4*lh + j]
  const int ft = NFT == 2 ? (wave & 1) : 0, pt = NFT == 2 ? (wave >> 1) : wave;
  const bool gemm_wave = pt < 2;
  float wreg[CIN / 2];
  f4 bv[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) bv[g] = (f4){0.f, 0.f, 0.f, 0.f};
  if (gemm_wave) {
#pragma unroll
    for (int kc = 0; kc < CIN / 8; ++kc) {
      const f4 v = *reinterpret_cast<const f4*>(wp + (ft * 32 + l31) * CIN + kc * 8 + 4 * lh);
      wreg[kc * 4 + 0] = v.x; wreg[kc * 4 + 1] = v.y; wreg[kc * 4 + 2] = v.z; wreg[kc * 4 + 3] = v.w;
    }
    if (bias) {
#pragma unroll
      for (int g = 0; g < 4; ++g) bv[g] = *reinterpret_cast<const f4*>(bias + ft * 32 + 8 * g + 4 * lh);
    }
  }
  // ---- loader / tap geometry: thread = (channel group c4, pixel lane pl)
  const int c4 = tid % C4, pl = tid / C4;
  const int cabs = x.coff + 4 * c4;
  const float* xn = x.data + (int64_t)n * H * W * x.cstride + cabs;
  f4 pre[PPT];
  auto issue = [&](int step) __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < PPT; ++p) {
      const int m = pl + PL * p;
      const int row = min(max(xs0 + step * RPS + m / TW, 0), H - 1), col = min(max(c0 + m % TW, 0), W - 1);      // clamped: pixels
      pre[p] = *reinterpret_cast<const f4*>(xn + ((int64_t)row * W + col) * x.cstride);                        // outside become 0
    }
  };
  issue(0);
  const Xf4 xf = lhn_load_xf(x, cabs);
  const f4 gate = x.gate ? *reinterpret_cast<const f4*>(x.gate + (int64_t)n * x.cstride + cabs) : (f4){1.f, 1.f, 1.f, 1.f};
  const Xf4 tf = lhn_load_xf_t(ttab, CIN, 4 * c4);
  f4 wk[9];      // depthwise taps of this thread's 4 channels
#pragma unroll
  for (int k = 0; k < 9; ++k) wk[k] = (f4){wd[(4 * c4 + 0) * 9 + k], wd[(4 * c4 + 1) * 9 + k], wd[(4 * c4 + 2) * 9 + k], wd[(4 * c4 + 3) * 9 + k]};
  for (int i = tid; i < RING * 2 * DIL * C4; i += 256) {      // the padding slots of every ring row
    const int r = i / (2 * DIL * C4), j = (i / C4) % (2 * DIL), c = i % C4;
    *reinterpret_cast<f4*>(ring + (r * SLOTS + (j < DIL ? j : TW + j)) * CIN + 4 * c) = (f4){0.f, 0.f, 0.f, 0.f};
  }
  const int orow = pl / CG, ocol0 = (pl % CG) * PPT;      // taps: output row within the step, first of PPT output columns

  for (int step = 0; step < nsteps; ++step) {
#pragma unroll
    for (int p = 0; p < PPT; ++p) {
      const int m = pl + PL * p, rr = m / TW, cc = m % TW;
      const int row = xs0 + step * RPS + rr, col = c0 + cc;
      const bool inside = row >= 0 && row < H && col >= 0 && col < W;
      *reinterpret_cast<f4*>(ring + (((step * RPS + rr) % RING) * SLOTS + cc + DIL) * CIN + 4 * c4) =
          inside ? lhn_apply_xf(pre[p], xf) * gate : (f4){0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();      // ring rows of this step are in; the MFMAs of the previous step are done with ts
    if (step + 1 < nsteps) issue(step + 1);
    // output row o reads x rows o - DIL, o, o + DIL = stream rows q0, q0 + DIL, q0 + 2 * DIL; the last one arrived in this step
    const int q0 = step * RPS - 2 * DIL + orow, o = rb + q0;
    if (o >= rb && o < re && ocol0 < ohi) {
      f4 out[PPT];
#pragma unroll
      for (int j = 0; j < PPT; ++j) out[j] = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const float* xr = ring + (((q0 + d * DIL) % RING) * SLOTS + ocol0) * CIN + 4 * c4;
        f4 v[NV];
#pragma unroll
        for (int q = 0; q < NV; ++q) v[q] = *reinterpret_cast<const f4*>(xr + q * CIN);
#pragma unroll
        for (int j = 0; j < PPT; ++j) out[j] += v[j] * wk[3 * d] + v[j + DIL] * wk[3 * d + 1] + v[j + 2 * DIL] * wk[3 * d + 2];
      }
#pragma unroll
      for (int j = 0; j < PPT; ++j)
        *reinterpret_cast<f4*>(ts + (orow * TW + ocol0 + j) * LDT + 4 * c4) = lhn_apply_xf(out[j], tf);
    }
    __syncthreads();      // t pixels of this step are in ts; the taps are done with the ring rows the next step overwrites
    if (gemm_wave) {
      f16v acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      const float* brow = ts + (pt * 32 + l31) * LDT + 4 * lh;
#pragma unroll
      for (int kc = 0; kc < CIN / 8; ++kc) {
        const f4 b = *reinterpret_cast<const f4*>(brow + kc * 8);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wreg[kc * 4 + 0], b.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wreg[kc * 4 + 1], b.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wreg[kc * 4 + 2], b.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wreg[kc * 4 + 3], b.w, acc, 0, 0, 0);
      }
      // C/D layout: column = lane & 31 (pixel), row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) (feature)
      const int m = pt * 32 + l31, rr = m / TW, cc = m % TW;
      const int oy = rb + step * RPS - 2 * DIL + rr;
      if (oy >= rb && oy < re && cc >= olo && cc < ohi) {
        float* yp = y.data + (((int64_t)n * H + oy) * W + c0 + cc) * y.cstride + y.coff + ft * 32 + 4 * lh;
#pragma unroll
        for (int g = 0; g < 4; ++g)
          *reinterpret_cast<f4*>(yp + 8 * g) = (f4){acc[4 * g + 0], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]} + bv[g];
      }
    }
  }
}

template <int CIN, int COUT, int TW, int DIL>
static int launch_dw3_pw(const lhn_view* x, const float* wd, const float* ttab, const float* wp, const float* bias, const lhn_view* y,
                         hipStream_t s) {
  constexpr int RPS = 64 / TW;
  const size_t lds = (size_t)((RPS + 2 * DIL) * (TW + 2 * DIL) * CIN + 64 * (CIN + 4)) * sizeof(float);
  static LhnKernelCfg cfg;
  int per_cu = 1;
  if (!lhn_kernel_cfg(cfg, &k_dw3_pw_fwd<CIN, COUT, TW, DIL>, lds, 2, &per_cu)) {
    lhn_set_error("lhn_conv_dw3_pw_fwd: cannot reserve %zu B of LDS", lds);
    return 2;
  }
  const int nstrips = x->W <= 64 ? 1 : (x->W + (64 - 2 * DIL) - 1) / (64 - 2 * DIL);
  // bands: enough workgroups for one resident round of the device, but at least 8 output rows (and one step) each -- every
  // band re-reads the 2 * DIL input rows around it
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
    lhn_set_error("lhn_conv_dw3_pw_fwd: grid too large");
    return 1;
  }
  hipLaunchKernelGGL((k_dw3_pw_fwd<CIN, COUT, TW, DIL>), dim3((unsigned)grid), dim3(256), lds, s, *x, wd, ttab, wp, bias, *y, nstrips,
                     nbands, band_rows);
  return 0;
}

template <int CIN, int COUT, int DIL>
static int launch_dw3_pw_w(const lhn_view* x, const float* wd, const float* ttab, const float* wp, const float* bias, const lhn_view* y,
                           hipStream_t s) {
  if (x->W <= 8) return launch_dw3_pw<CIN, COUT, 8, DIL>(x, wd, ttab, wp, bias, y, s);
  if (x->W <= 16) return launch_dw3_pw<CIN, COUT, 16, DIL>(x, wd, ttab, wp, bias, y, s);
  if (x->W <= 32) return launch_dw3_pw<CIN, COUT, 32, DIL>(x, wd, ttab, wp, bias, y, s);
  return launch_dw3_pw<CIN, COUT, 64, DIL>(x, wd, ttab, wp, bias, y, s);
}

template <int CIN, int COUT>
static int launch_dw3_pw_d(const lhn_view* x, const float* wd, int dil, const float* ttab, const float* wp, const float* bias,
                           const lhn_view* y, hipStream_t s) {
  return dil == 1 ? launch_dw3_pw_w<CIN, COUT, 1>(x, wd, ttab, wp, bias, y, s) : launch_dw3_pw_w<CIN, COUT, 2>(x, wd, ttab, wp, bias, y, s);
}

// (litehandnet_amd/plan.py: _fusable_dw_pw mirrors this rule)
static bool dw3_pw_supported(int cin, int cout, int dil) {
  return (cin == 32 || cin == 64) && (cout == 32 || cout == 64) && (dil == 1 || dil == 2);
}

extern "C" int lhn_conv_dw3_pw_fwd(const lhn_view* x, const float* w_dw, int dil, const float* t_table, const float* w_pw,
                                   const float* bias, const lhn_view* y, void* stream) {
  LHN_CHECK_ARG(lhn_view_ok(x) && lhn_view_ok(y) && lhn_no_pend(x) && lhn_no_pend(y) && w_dw && w_pw, "lhn_conv_dw3_pw_fwd: bad view / null pointer");
  LHN_CHECK_ARG(y->N == x->N && y->H == x->H && y->W == x->W, "lhn_conv_dw3_pw_fwd: same-size output");
  LHN_CHECK_ARG(dw3_pw_supported(x->C, y->C, dil),
                "lhn_conv_dw3_pw_fwd: unsupported shape: built for 32 / 64 -> 32 / 64 channels at dilation 1 or 2 (got %d -> %d, dilation %d, map %d x %d)",
                x->C, y->C, dil, x->H, x->W);
  LHN_CHECK_ARG(!(x->data == y->data && x->coff < y->coff + y->C && y->coff < x->coff + x->C),
                "lhn_conv_dw3_pw_fwd: unsupported shape: y overlaps x (a pixel's neighbours are read after it is written)");
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if (x->C == 64 && y->C == 64) rc = launch_dw3_pw_d<64, 64>(x, w_dw, dil, t_table, w_pw, bias, y, s);
  else if (x->C == 64) rc = launch_dw3_pw_d<64, 32>(x, w_dw, dil, t_table, w_pw, bias, y, s);
  else if (y->C == 64) rc = launch_dw3_pw_d<32, 64>(x, w_dw, dil, t_table, w_pw, bias, y, s);
  else rc = launch_dw3_pw_d<32, 32>(x, w_dw, dil, t_table, w_pw, bias, y, s);
  if (rc) return rc;
  LHN_CHECK_LAUNCH("lhn_conv_dw3_pw_fwd");
  return 0;
}
