// One MSRB round (litehourglass.py:13-50) of an inference plan as ONE pass over the feature map: the dilation-1 depthwise 3x3 over
// the left half of the channels, the dilation-2 depthwise 3x3 over the right half and -- when the round's output is gated by
// ChannelAttension / SEBlock (common.py:23-66) -- the adaptive-average-pool sums their attention MLP reads.
//
// Work item = (image, 8 x 32 output tile, 32-channel group); the channel group chooses the branch (block-uniform: a block keeps
// its group for the whole launch, as in k_dwk_fwd_lds), so the tile walker is one device function templated on the dilation.
// The halo tile is staged exactly as k_dwk_fwd_lds stages it (loads of the NEXT item issued into registers before the taps,
// table and gate applied once, zeros outside the map, second source summed at commit time); dilation 2 reads its taps
// directly from a (8 + 4) x (32 + 4) halo, so maps narrower than 8 or smaller than the dilation need no second kernel.
// Pooling: no float atomics.  Every work item writes its per-(bin, channel) sum of the CONSUMED output value (y's table applied
// to the raw result) into its own slot of `scratch`, zeros for the bins it does not touch; k_msrb_fold, launched behind it by
// the same entry point, adds the slots of one image in tile order and divides by the bin's pixel count.  Same bits every call.
#include "lhn_common.h"

struct MsrbArgs {
  lhn_view x[2], ex[2], y;
  const float* w[2];
  float coef[2];
  float* part;        // [N][tiles_h * tiles_w][nb * nb][C] per-item pooling sums, or NULL
  int nb;             // bins per axis: 3 (ChannelAttension), 1 (SEBlock)
  int tiles_h, tiles_w, cgroups;
};

// adaptive_avg_pool2d bin i of nb over an extent S: [floor(i * S / nb), ceil((i + 1) * S / nb))  (k_avgpool_fwd's rule)
__host__ __device__ static inline int msrb_bin_lo(int i, int S, int nb) { return (i * S) / nb; }
__host__ __device__ static inline int msrb_bin_hi(int i, int S, int nb) { return ((i + 1) * S + nb - 1) / nb; }

template <int DIL, int NS>
__device__ __forceinline__ void msrb_walk(const MsrbArgs& a, const lhn_view& x, const lhn_view& ex, const float* __restrict__ w,
                                          const int lcg /*group inside the half*/, const int cg /*group inside y*/, float* smem) {
  constexpr int TH = 8, TW = 32, P = DIL, WW = TW + 2 * P, PIX = (TH + 2 * P) * WW, NIT = (PIX + 31) / 32;
  const lhn_view& y = a.y;
  f4* tile = reinterpret_cast<f4*>(smem);      // [PIX][8]; after the taps its head holds the per-column pooling sums [32][3][8]
  const int tid = threadIdx.x, c4 = tid & 7, pl = tid >> 3;      // pl = output column 0..31
  const int H = y.H, W = y.W, cgroups = a.cgroups, tiles_w = a.tiles_w, tiles_h = a.tiles_h;
  const int ntile = y.N * tiles_h * tiles_w * cgroups;
  const int cin = x.coff + lcg * 32 + 4 * c4, cin2 = NS > 1 ? ex.coff + lcg * 32 + 4 * c4 : 0, cout = y.coff + cg * 32 + 4 * c4;
  f4 wt[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const float* wp = w + (size_t)(lcg * 32 + 4 * c4) * 9 + k;
    wt[k] = (f4){wp[0], wp[9], wp[18], wp[27]};
  }
  const int nb = a.nb;
  int rlo[3], rhi[3];                        // row bins of the pooling (empty: no pooling / SEBlock's single bin is rb 0)
#pragma unroll
  for (int rb = 0; rb < 3; ++rb) {
    rlo[rb] = rb < nb ? msrb_bin_lo(rb, H, nb) : 0;
    rhi[rb] = rb < nb ? msrb_bin_hi(rb, H, nb) : 0;
  }
  f4 raw[NIT];
  auto issue = [&](int t) __attribute__((always_inline)) {
    int r = t / cgroups;
    const int tw = r % tiles_w;
    r /= tiles_w;
    const int th = r % tiles_h, n = r / tiles_h;
    const int h0 = th * TH - P, w0 = tw * TW - P;
    const float* xin = x.data + (size_t)n * H * W * x.cstride + cin;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = min(pl + 32 * it, PIX - 1);
      const int ph = i / WW, pw = i - ph * WW;
      const int ih = min(max(h0 + ph, 0), H - 1), iw = min(max(w0 + pw, 0), W - 1);       // clamped: always inside the map
      raw[it] = *reinterpret_cast<const f4*>(xin + ((size_t)ih * W + iw) * x.cstride);
    }
  };
  int t = blockIdx.x;
  if (t < ntile) issue(t);
  const Xf4 xf = lhn_load_xf(x, cin);
  Xf4 xf2 = xf, yf = xf;
  if (NS > 1) xf2 = lhn_load_xf(ex, cin2);
  if (a.part) yf = lhn_load_xf(y, cout);
  for (; t < ntile; t += gridDim.x) {
    int r = t / cgroups;
    const int tw = r % tiles_w;
    r /= tiles_w;
    const int th = r % tiles_h, n = r / tiles_h;
    const int h0 = th * TH - P, w0 = tw * TW - P;
    f4 gate = x.gate ? *reinterpret_cast<const f4*>(x.gate + (size_t)n * x.cstride + cin) : (f4){1.f, 1.f, 1.f, 1.f};
    f4 gate2 = (f4){0.f, 0.f, 0.f, 0.f};
    if (NS > 1) {
      gate *= a.coef[0];
      gate2 = (ex.gate ? *reinterpret_cast<const f4*>(ex.gate + (size_t)n * ex.cstride + cin2) : (f4){1.f, 1.f, 1.f, 1.f}) * a.coef[1];
    }
    __syncthreads();      // the previous item's taps and pooling reads are done
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = pl + 32 * it;
      if (i < PIX) {
        const int ph = i / WW, pw = i - ph * WW;
        const int ih = h0 + ph, iw = w0 + pw;
        const bool inb = ih >= 0 && ih < H && iw >= 0 && iw < W;
        f4 v = lhn_apply_xf(raw[it], xf) * gate;
        if (NS > 1) {
          const float* xin2 = ex.data + (size_t)n * H * W * ex.cstride + cin2;
          const f4 r2 = *reinterpret_cast<const f4*>(xin2 + ((size_t)min(max(ih, 0), H - 1) * W + min(max(iw, 0), W - 1)) * ex.cstride);
          v += lhn_apply_xf(r2, xf2) * gate2;
        }
        tile[i * 8 + c4] = inb ? v : (f4){0.f, 0.f, 0.f, 0.f};      // the convolution pads the VALUE with zeros
      }
    }
    __syncthreads();
    if (t + (int)gridDim.x < ntile) issue(t + gridDim.x);
    const int wo = tw * TW + pl;
    f4 rs[3];
    rs[0] = rs[1] = rs[2] = (f4){0.f, 0.f, 0.f, 0.f};
    if (wo < W) {
      const f4* col = tile + (pl + P) * 8 + c4;      // centre column of this thread, halo row 0
      float* yout = y.data + ((size_t)(n * H + th * TH) * W + wo) * y.cstride + cout;
      f4 win[3][3];                                  // dilation 1: sliding window over the halo rows rr .. rr + 2 (3 LDS reads per output)
      if (DIL == 1) {
#pragma unroll
        for (int q = 1; q < 3; ++q)
#pragma unroll
          for (int b = 0; b < 3; ++b) win[q][b] = col[((q - 1) * WW + (b - 1)) * 8];
      }
#pragma unroll
      for (int rr = 0; rr < TH; ++rr) {
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          if (DIL == 1) {
            win[0][b] = win[1][b];
            win[1][b] = win[2][b];
            win[2][b] = col[((rr + 2) * WW + (b - 1)) * 8];
          }
        }
        const int h = th * TH + rr;
        if (h < H) {
          f4 acc = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ka = 0; ka < 3; ++ka)
#pragma unroll
            for (int b = 0; b < 3; ++b)
              acc += (DIL == 1 ? win[ka][b] : col[((rr + ka * DIL) * WW + (b - 1) * DIL) * 8]) * wt[ka * 3 + b];      // dilation 2: taps straight from LDS
          *reinterpret_cast<f4*>(yout + (size_t)rr * W * y.cstride) = acc;
          if (a.part) {
            const f4 v = lhn_apply_xf(acc, yf);
#pragma unroll
            for (int rb = 0; rb < 3; ++rb)
              if (h >= rlo[rb] && h < rhi[rb]) rs[rb] += v;
          }
        }
      }
    }
    if (a.part) {
      __syncthreads();      // every tap has been read: the tile's head becomes the per-column sums
#pragma unroll
      for (int rb = 0; rb < 3; ++rb) tile[(pl * 3 + rb) * 8 + c4] = rs[rb];
      __syncthreads();
      if (tid < nb * nb * 8) {
        const int bin = tid >> 3, rb = bin / nb, cb = bin - rb * nb;
        const int lo = msrb_bin_lo(cb, W, nb) - tw * TW, hi = msrb_bin_hi(cb, W, nb) - tw * TW;      // (columns >= W hold zeros)
        f4 s = (f4){0.f, 0.f, 0.f, 0.f};
        for (int p = max(lo, 0); p < min(hi, TW); ++p) s += tile[(p * 3 + rb) * 8 + c4];
        const size_t slot = ((size_t)n * tiles_h * tiles_w + th * tiles_w + tw) * (nb * nb) + bin;
        *reinterpret_cast<f4*>(a.part + slot * y.C + cg * 32 + 4 * c4) = s;
      }
    }
  }
}

template <int NS>
__global__ void __launch_bounds__(256, 2) k_msrb_round_fwd(MsrbArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int cg = blockIdx.x % a.cgroups, hg = a.cgroups >> 1;      // grid % cgroups == 0 (host): fixed per block
  if (cg < hg) msrb_walk<1, NS>(a, a.x[0], a.ex[0], a.w[0], cg, cg, smem);
  else msrb_walk<2, NS>(a, a.x[1], a.ex[1], a.w[1], cg - hg, cg, smem);
}

// pooled[n, bin, c] = (sum of the image's item slots, in tile order) / |bin|
__global__ void __launch_bounds__(256) k_msrb_fold(const float* __restrict__ part, float* __restrict__ pooled, int ntl, int nb, int H,
                                                   int W, int C) {
  const int bins = nb * nb, n = blockIdx.x / bins, bin = blockIdx.x - n * bins, rb = bin / nb, cb = bin - rb * nb;
  const int cnt = (msrb_bin_hi(rb, H, nb) - msrb_bin_lo(rb, H, nb)) * (msrb_bin_hi(cb, W, nb) - msrb_bin_lo(cb, W, nb));
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float s = 0.f;
    for (int tl = 0; tl < ntl; ++tl) s += part[(((size_t)n * ntl + tl) * bins + bin) * C + c];
    pooled[((size_t)n * bins + bin) * C + c] = s / (float)cnt;
  }
}

static inline bool msrb_half_ok(int c) { return c == 32 || c == 64 || c == 128; }
static inline bool msrb_overlap(const lhn_view* a, const lhn_view* b) {
  return a->data == b->data && a->coff < b->coff + b->C && b->coff < a->coff + a->C;
}

extern "C" int64_t lhn_msrb_round_scratch_bytes(int N, int H, int W, int C) {
  if (N <= 0 || H <= 0 || W <= 0 || C % 2 || !msrb_half_ok(C / 2)) return 0;
  return (int64_t)N * ((H + 7) / 8) * ((W + 31) / 32) * 9 * C * 4;
}

extern "C" int lhn_msrb_round_fwd(const lhn_view x[2], const lhn_view* extra, const float* coef2, const float* w_d1, const float* w_d2,
                                  const lhn_view* y, float* pooled, int OH, int OW, void* scratch, void* stream) {
  LHN_CHECK_ARG(x && lhn_view_ok(&x[0]) && lhn_view_ok(&x[1]) && lhn_view_ok(y) && w_d1 && w_d2, "lhn_msrb_round_fwd: bad view / null pointer");
  LHN_CHECK_ARG(!extra || (lhn_view_ok(&extra[0]) && lhn_view_ok(&extra[1]) && coef2), "lhn_msrb_round_fwd: bad extra view / no coefficients");
  LHN_CHECK_ARG(lhn_no_pend(&x[0]) && lhn_no_pend(&x[1]) && lhn_no_pend(y) && (!extra || (lhn_no_pend(&extra[0]) && lhn_no_pend(&extra[1]))),
                "lhn_msrb_round_fwd: lhn_view.pend is reserved (NULL)");
  const int h = x[0].C;
  LHN_CHECK_ARG(msrb_half_ok(h) && x[1].C == h && y->C == 2 * h,
                "lhn_msrb_round_fwd: unsupported shape: halves of %d and %d channels into %d (built for 32, 64, 128 per half)", x[0].C, x[1].C, y->C);
  for (int k = 0; k < 2; ++k) {
    LHN_CHECK_ARG(x[k].N == y->N && x[k].H == y->H && x[k].W == y->W, "lhn_msrb_round_fwd: same-size output");
    LHN_CHECK_ARG(!msrb_overlap(y, &x[k]), "lhn_msrb_round_fwd: unsupported shape: y overlaps x[%d] in the same buffer", k);
    if (extra) {
      LHN_CHECK_ARG(extra[k].C == h && extra[k].N == y->N && extra[k].H == y->H && extra[k].W == y->W, "lhn_msrb_round_fwd: extra source geometry");
      LHN_CHECK_ARG(!msrb_overlap(y, &extra[k]), "lhn_msrb_round_fwd: unsupported shape: y overlaps extra[%d] in the same buffer", k);
    }
  }
  LHN_CHECK_ARG(!pooled || (OH == OW && (OH == 1 || OH == 3)), "lhn_msrb_round_fwd: unsupported shape: pooling to %dx%d (built for 1x1 and 3x3)", OH, OW);
  LHN_CHECK_ARG(!pooled || scratch, "lhn_msrb_round_fwd: unsupported shape: pooling needs the scratch of lhn_msrb_round_scratch_bytes");
  MsrbArgs a;
  memset(&a, 0, sizeof(a));
  for (int k = 0; k < 2; ++k) {
    a.x[k] = x[k];
    a.ex[k] = extra ? extra[k] : x[k];
  }
  a.y = *y;
  a.w[0] = w_d1;
  a.w[1] = w_d2;
  a.coef[0] = extra ? coef2[0] : 1.f;
  a.coef[1] = extra ? coef2[1] : 0.f;
  a.part = pooled ? static_cast<float*>(scratch) : nullptr;
  a.nb = pooled ? OH : 0;
  a.tiles_h = (y->H + 7) / 8;
  a.tiles_w = (y->W + 31) / 32;
  a.cgroups = 2 * h / 32;
  const int64_t ntile64 = (int64_t)y->N * a.tiles_h * a.tiles_w * a.cgroups;
  LHN_CHECK_ARG(ntile64 < (1ll << 30), "lhn_msrb_round_fwd: unsupported shape: too many tiles");
  const int ntile = (int)ntile64;
  const size_t lds = (size_t)(8 + 4) * (32 + 4) * 8 * 16;      // the dilation-2 halo tile; the dilation-1 blocks use its first 10 x 34 pixels
  hipStream_t s = (hipStream_t)stream;
  static LhnKernelCfg cfg1, cfg2;
  int per_cu = 1;
  const bool ok = extra ? lhn_kernel_cfg(cfg2, &k_msrb_round_fwd<2>, lds, 4, &per_cu) : lhn_kernel_cfg(cfg1, &k_msrb_round_fwd<1>, lds, 4, &per_cu);
  LHN_CHECK_ARG(ok, "lhn_msrb_round_fwd: %zu bytes of LDS refused", lds);
  int grid = lhn_num_cus() * per_cu * 2;      // persistent grid, two items per resident block and round (launch_dwk_fwd's measured choice)
  grid -= grid % a.cgroups;
  if (grid > ntile) grid = ntile;             // ntile is a multiple of cgroups
  if (grid < a.cgroups) grid = a.cgroups;
  if (extra) hipLaunchKernelGGL((k_msrb_round_fwd<2>), dim3(grid), dim3(256), lds, s, a);
  else hipLaunchKernelGGL((k_msrb_round_fwd<1>), dim3(grid), dim3(256), lds, s, a);
  LHN_CHECK_LAUNCH("lhn_msrb_round_fwd");
  if (pooled) {
    hipLaunchKernelGGL(k_msrb_fold, dim3(y->N * OH * OH), dim3(256), 0, s, a.part, pooled, a.tiles_h * a.tiles_w, OH, y->H, y->W, y->C);
    LHN_CHECK_LAUNCH("lhn_msrb_round_fwd (fold)");
  }
  return 0;
}
